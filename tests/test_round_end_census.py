"""tests/round_end_census.py on hand-built logs (one case per kind) and on a recorded game whose counts are read off by hand."""
import json
import os

import pytest

from tests import round_end_census as rc

HERE = os.path.dirname(os.path.abspath(__file__))
TEHAIS = [["1m", "2m", "3m", "4p", "5p", "6p", "7s", "8s", "9s", "E", "E", "S", "S"],
          ["1p", "1p", "1p", "2p", "3p", "4p", "5m", "6m", "7m", "8m", "9m", "W", "W"],
          ["2s", "3s", "4s", "5s", "6s", "7s", "1m", "1m", "1m", "C", "C", "N", "N"],
          ["3m", "3m", "4m", "5m", "6m", "7p", "8p", "9p", "2s", "2s", "P", "P", "F"]]


def kyoku(oya=0, honba=0, kyotaku=0, bakaze="E", scores=None, np_=4):
    scores = scores or ([26000, 25000, 25000, 24000] if np_ == 4 else [36000, 35000, 34000])   # one top score unless a case says so
    return {"type": "start_kyoku", "bakaze": bakaze, "dora_marker": "9m", "kyoku": oya + 1, "honba": honba,
            "kyotaku": kyotaku, "oya": oya, "scores": scores, "tehais": TEHAIS[:np_]}


def tsumo_win(actor, deltas, pai="S"):
    return [{"type": "tsumo", "actor": actor, "pai": pai}, {"type": "hora", "actor": actor, "target": actor, "deltas": deltas, "ura_markers": []}]


def ron(actor, target, deltas):
    return {"type": "hora", "actor": actor, "target": target, "deltas": deltas, "ura_markers": []}


def discard(actor, pai="S"):
    return [{"type": "tsumo", "actor": actor, "pai": pai}, {"type": "dahai", "actor": actor, "pai": pai, "tsumogiri": True}]


def draw(deltas, reason="exhaustive_draw"):
    return {"type": "ryukyoku", "deltas": deltas, "reason": reason}


def game(*rounds):
    """rounds: lists of events starting with their start_kyoku; end_kyoku between them, end_game after the last"""
    log = [{"type": "start_game"}]
    for r in rounds:
        log += r + [{"type": "end_kyoku"}]
    return log + [{"type": "end_game"}]


def only(c, **want):
    got = {k: v for k, v in c.items() if v}
    assert got == want, got


def test_wins():
    only(rc.census([game([kyoku(oya=1)] + tsumo_win(1, [-4000, 12000, -4000, -4000]))]), tsumo_dealer=1, game_end=1)
    only(rc.census([game([kyoku(oya=0, honba=2)] + tsumo_win(2, [-2200, -1200, 4600, -1200]))]), tsumo_nondealer=1, win_honba=1,
         tsumo_nondealer_honba=1, game_end=1)
    only(rc.census([game([kyoku()] + discard(0) + [ron(1, 0, [-1000, 1000, 0, 0])])]), ron_single=1, game_end=1)
    only(rc.census([game([kyoku(kyotaku=1)] + discard(0) + [ron(1, 0, [-1000, 2000, 0, 0]), ron(2, 0, [-3000, 0, 3000, 0])])]),
         ron_double=1, win_kyotaku=1, ron_double_kyotaku=1, game_end=1)
    only(rc.census([game([kyoku()] + discard(0) + [ron(s, 0, [-2000 * s] + [2000 * s if i == s else 0 for i in (1, 2, 3)]) for s in (1, 2, 3)])]),
         ron_triple=1, game_end=1)
    # riichi sticks: one on the table at the deal, or a declaration accepted in the round
    reach = [{"type": "reach", "actor": 3}, {"type": "dahai", "actor": 3, "pai": "F", "tsumogiri": False},
             {"type": "reach_accepted", "actor": 3}]
    only(rc.census([game([kyoku()] + [{"type": "tsumo", "actor": 3, "pai": "F"}] + reach + tsumo_win(2, [-1000, -1000, 4000, -1000]))]),
         tsumo_nondealer=1, win_kyotaku=1, game_end=1)


def test_pao():
    # a yakuman Tsumo paid by the responsible seat alone, and a Ron split between the discarder and it
    only(rc.census([game([kyoku()] + tsumo_win(1, [0, 8000, 0, -8000]))]), tsumo_nondealer=1, pao=1, game_end=1)
    only(rc.census([game([kyoku()] + discard(0) + [ron(1, 0, [-16000, 32000, 0, -16000])])]), ron_single=1, pao=1, game_end=1)


def test_kan_and_last_tile_wins():
    # rinshan: a Tsumo on the replacement draw of a concealed kan
    k = [kyoku(), {"type": "tsumo", "actor": 0, "pai": "E"}, {"type": "ankan", "actor": 0, "consumed": ["E", "E", "E", "E"]},
         {"type": "dora", "dora_marker": "1p"}] + tsumo_win(0, [48000, -16000, -16000, -16000])
    c = rc.census([game(k)])
    assert c["rinshan"] == 1 and c["haitei"] == 0 and c["tsumo_dealer"] == 1
    # chankan: a Ron on the tile of an added kan
    k = [kyoku(), {"type": "tsumo", "actor": 3, "pai": "P"}, {"type": "dahai", "actor": 3, "pai": "F", "tsumogiri": False},
         {"type": "pon", "actor": 0, "target": 3, "pai": "F", "consumed": ["F", "F"]},
         {"type": "dahai", "actor": 0, "pai": "S", "tsumogiri": False}, {"type": "tsumo", "actor": 1, "pai": "F"},
         {"type": "dahai", "actor": 1, "pai": "F", "tsumogiri": True}, {"type": "tsumo", "actor": 0, "pai": "F"},
         {"type": "kakan", "actor": 0, "pai": "F", "consumed": ["F", "F", "F"]}, ron(3, 0, [-1000, 0, 0, 1000])]
    c = rc.census([game(k)])
    assert c["chankan"] == 1 and c["ron_single"] == 1
    # haitei and houtei: the wall's 70 draws taken, then a Tsumo on the last one / a Ron on its discard
    walk = [e for i in range(69) for e in discard(i % 4, "N")]
    c = rc.census([game([kyoku()] + walk + tsumo_win(1, [-1000, 3000, -1000, -1000]))])
    assert c["haitei"] == 1 and c["houtei"] == 0
    c = rc.census([game([kyoku()] + walk + discard(1, "N") + [ron(2, 1, [0, -1000, 1000, 0])])])
    assert c["houtei"] == 1 and c["haitei"] == 0


def test_draws_and_transitions():
    k0 = [kyoku(oya=0, kyotaku=1), {"type": "tsumo", "actor": 1, "pai": "F"}, draw([1000, 1000, 1000, -3000])]
    k1 = [kyoku(oya=0, honba=1, kyotaku=1), draw([0, 0, 0, 0])]                 # no payment and the dealer deals again: all tenpai
    k2 = [kyoku(oya=0, honba=2, kyotaku=1), draw([0, 0, 0, 0])]                 # no payment and the deal moves on: nobody tenpai
    k3 = [kyoku(oya=1, honba=3, kyotaku=1), draw([-1000, -1000, 3000, -1000])]
    k4 = [kyoku(oya=2, honba=4, kyotaku=1)] + discard(2) + [ron(3, 2, [0, 0, -2000, 3200])]
    k5 = [kyoku(oya=3)] + tsumo_win(3, [-2000, -2000, -2000, 6000])
    k6 = [kyoku(oya=3, honba=1)] + tsumo_win(0, [3000, -1000, -1000, -1000])     # the game ends after it
    only(rc.census([game(k0, k1, k2, k3, k4, k5, k6)]), draw_tenpai_3=1, draw_tenpai_4=1, draw_tenpai_0=1, draw_tenpai_1=1,
         renchan_tenpai_draw=2, kyotaku_carried=4, rotation=3, ron_single=1, win_kyotaku=1, win_honba=2, tsumo_dealer=1,
         renchan_win=1, tsumo_nondealer=1, tsumo_nondealer_honba=1, game_end=1)
    # no payment at the last round of the game: nothing tells nobody from everybody
    only(rc.census([game([kyoku(oya=3), draw([0, 0, 0, 0])])]), draw_tenpai_0_or_all=1, game_end=1)
    # 3P: three seats, two tenpai
    only(rc.census([game([kyoku(oya=0, np_=3), draw([1000, 1000, -2000])])]), draw_tenpai_2=1, game_end=1)


@pytest.mark.parametrize("reason", ["nagashimangan", "kyushu_kyuhai", "sufuurenta", "suukansansen", "suucha_riichi", "sanchaho"])
def test_abortive_reasons(reason):
    only(rc.census([game([kyoku(), draw([0, 0, 0, 0], reason)])]), **{"ryukyoku_" + reason: 1, "game_end": 1})


def test_illegal_action():
    only(rc.census([game([kyoku(), draw([4000, 2000, 2000, -8000], "Error: Illegal Action by Player 3")])]), ryukyoku_illegal_action=1,
         game_end=1)


def test_game_ends():
    # a bust: the riichi deposit takes the last 1 000 points before the payment
    k = [kyoku(oya=0, scores=[1000, 25000, 25000, 49000]), {"type": "tsumo", "actor": 0, "pai": "F"}, {"type": "reach", "actor": 0},
         {"type": "dahai", "actor": 0, "pai": "F", "tsumogiri": True}, {"type": "reach_accepted", "actor": 0},
         draw([-1000, -1000, -1000, 3000])]
    only(rc.census([game(k)]), draw_tenpai_1=1, bust=1)
    # into the South round, and into the West round ended with two seats on the top score
    only(rc.census([game([kyoku(oya=3, bakaze="E"), draw([0, 0, 0, 0])], [kyoku(oya=0, bakaze="S", honba=1), draw([-1000, 3000, -1000, -1000])])]),
         draw_tenpai_0=1, draw_tenpai_1=1, rotation=1, south_entry=1, game_end=1)
    s = [kyoku(oya=3, bakaze="S"), draw([0, 0, 0, 0])]
    w = [kyoku(oya=0, bakaze="W", honba=1, scores=[26000, 26000, 24000, 24000]), draw([0, 0, 0, 0])]
    only(rc.census([game(s, w)]), draw_tenpai_0=1, draw_tenpai_0_or_all=1, rotation=1, west_entry=1, game_end=1, tied_top=1)
    # a slot's stream across a restart: two games
    c = rc.census([game([kyoku()] + tsumo_win(1, [-1000, 3000, -1000, -1000])) + game([kyoku(oya=2)] + tsumo_win(2, [-4000, -4000, 12000, -4000]))])
    assert c["game_end"] == 2 and c["tsumo_nondealer"] == 1 and c["tsumo_dealer"] == 1 and c["rotation"] == 0


def test_recorded_game():
    """tests/golden/126_204_0_mjai.jsonl, a half game (its draws carry no reason), read off by hand:
    E1 tsumo by 3 (sticks of two riichi) - E2 Ron 2 <- 3 (sticks) - E3 dealer tsumo - E3-1 dealer tsumo (sticks) - E3-2 tsumo by 3
    (sticks) - E4 dealer Ron 3 <- 1 - E4-1 draw, three tenpai, the dealer noten - S1-2 tsumo by 3 (the stick carried over) - S2 draw, two
    tenpai, the dealer among them - S2-1 Ron 0 <- 3 - S3 draw, three tenpai, the dealer noten - S4-1 Ron 2 <- 0 (the stick carried
    over), end of the game with nobody below 0 and one top score"""
    with open(os.path.join(HERE, "golden", "126_204_0_mjai.jsonl")) as f:
        log = [json.loads(line) for line in f]
    only(rc.census([log]), tsumo_dealer=2, tsumo_nondealer=3, ron_single=4, win_kyotaku=6, win_honba=5, tsumo_nondealer_honba=2,
         draw_tenpai_3=2, draw_tenpai_2=1, renchan_win=3, renchan_tenpai_draw=1, rotation=7, kyotaku_carried=2, south_entry=1,
         game_end=1)
