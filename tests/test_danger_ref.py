"""The yardstick of the deal-in danger targets (tests/danger_ref.py) against the oracle's own settlement: no GPU.

A value says what an opponent would win by ron on a discard.  So the test makes the discard: the position is poked into a second
oracle.Game, the current player discards the tile, exactly that opponent calls Ron, the others pass, and the scores say what moved."""
import numpy as np
import pytest

from oracle import oracle
from riichienv_amd import abi
from riichienv_amd.abi import DISCARD, PASS, RON, WAIT_ACT, WAIT_RESPONSE, pack_action, unpack_action
from tests import danger_ref as D
from tests import scenarios as SC

def settle(view, mode, discarder, tile, winner, rule_bits=abi.RULE_TENHOU):
    """`discarder` discards `tile` in the position `view`, `winner` rons, everyone else passes: (winner's gain, discarder's loss, what
    the remaining seats lost: a pao payer's share) from a second oracle game; None when the winner is not offered the Ron"""
    np_ = 3 if mode >= 3 else 4
    g = oracle.Game(game_mode=mode, rule_bits=rule_bits)
    g.reset()
    g.poke(view)
    before = [int(view.players[p].score) for p in range(4)]
    a = SC.find(g.legal(discarder), DISCARD, tile)
    assert a is not None, ("the discard is not legal", discarder, tile)
    g.step({discarder: a})
    active, phase, done = g.status()
    if done or phase != WAIT_RESPONSE or not (active >> winner) & 1:
        return None
    ron = SC.find(g.legal(winner), RON)
    if ron is None:
        return None
    g.step({p: (ron if p == winner else pack_action(PASS)) for p in range(np_) if (active >> p) & 1})
    after = [int(p.score) for p in g.peek().players]
    third = sum(before[p] - after[p] for p in range(np_) if p not in (winner, discarder))
    return after[winner] - before[winner], before[discarder] - after[discarder], third


# ---------------------------------------------------------------- the yardstick on positions of whole games
@pytest.mark.parametrize("mode", [2, 5])
def test_yardstick_equals_the_settlement_on_rolled_games(mode):
    np_ = 3 if mode >= 3 else 4
    compared, riichi_winners, with_pao = 0, 0, 0
    for gi in range(16):
        game = oracle.Game(game_mode=mode, seed=4300 + 53 * mode + gi)
        game.reset()
        for _ in range(6000):
            active, phase, done = game.status()
            if done:
                break
            view = game.peek()
            if phase == WAIT_ACT and view.pending_kan_dora_count == 0:
                cur = int(view.current_player)
                rows = {}
                seen = set()
                for a in game.legal(cur):
                    ty, tile, _ = unpack_action(a)
                    if ty != DISCARD or tile is None:
                        continue
                    k = D.kind_of_tile(tile)
                    if k in seen:
                        continue
                    seen.add(k)
                    for r in range(np_ - 1):
                        s = (cur + 1 + r) % np_
                        if mode >= 3 and view.players[s].riichi_declared:
                            continue   # a 3P view cannot carry the ura indicators the settlement counts
                        if s not in rows:
                            rows[s] = D.opp_danger(view, s, np_, ura=mode < 3)
                        value = int(rows[s][k])
                        if value == 0:
                            continue
                        got = settle(view, mode, cur, tile, s)
                        assert got is not None, ("the yardstick values a tile the opponent cannot ron", gi, int(game.step_count), cur, tile, s, value)
                        gain, loss, third = got
                        sticks = 1000 * int(view.riichi_sticks)
                        assert gain - sticks == value, (gi, int(game.step_count), cur, tile, s, gain, sticks, value)
                        assert loss + third == value and third >= 0, (gi, int(game.step_count), cur, tile, s, loss, third, value)
                        if third:     # a pao payer took a share: only then may the discarder lose less than the value
                            p = view.players[s]
                            assert p.pao_daisangen >= 0 or p.pao_daisuushi >= 0, (gi, int(game.step_count), s)
                            with_pao += 1
                        compared += 1
                        riichi_winners += bool(view.players[s].riichi_declared)
            game.step([int(x) for x in game.greedy_actions(61, gi, 64)])
    print(f"mode {mode}: {compared} positions compared, {riichi_winners} riichi winners, {with_pao} with a pao payer")
    assert compared >= (100 if mode == 2 else 50), compared


# ---------------------------------------------------------------- built positions
def _position(hand, waits_on, mode=2, melds=None, mutate=None, discarder=0, winner=1, oya=0, rule_bits=abi.RULE_TENHOU):
    """A WaitAct position: `winner` holds `hand` (13 tiles counting melds), `discarder` holds a 14-tile hand that contains the tiles
    `waits_on` (136-ids) and is to act.  Returns the view."""
    g = oracle.Game(game_mode=mode, rule_bits=rule_bits)
    np_ = 3 if mode >= 3 else 4
    used = set(hand) | set(waits_on) | {t for m in (melds or []) for t in m[1]}
    filler = [t for t in (4 * ty + c for ty in (27, 28, 29, 30, 31, 32, 33, 8, 9) for c in (3, 2)) if t not in used]   # honors, 9m, 1p: two of a type at the most
    mine = sorted(list(waits_on) + filler[: 14 - len(waits_on)])
    hands = [None] * 4
    hands[discarder], hands[winner] = mine[:13], list(hand)
    ml = [None] * 4
    ml[winner] = melds

    def mut(v):
        v.pending_kan_dora_count = 0
        v.n_dora = 1
        v.dora[0] = 4 * 31 + 3   # haku as the indicator: hatsu is dora, held by nobody here unless the position says so
        if mutate:
            mutate(v)

    SC.setup(g, hands=hands, melds=ml, current_player=discarder, drawn_tile=mine[13], oya=oya, mutate=mut)
    assert g.status()[1] == WAIT_ACT
    return g.peek(), np_


def _check(view, mode, np_, tile, expect_zero=False, discarder=0, winner=1, rule_bits=abi.RULE_TENHOU, ura=None):
    """the yardstick's value of `tile` against the settlement of the same position; returns (value, gain, loss, the oracle's evaluation)"""
    ura = mode < 3 if ura is None else ura
    value = int(D.opp_danger(view, winner, np_, ura, rule_bits)[D.kind_of_tile(tile)])
    got = settle(view, mode, discarder, tile, winner, rule_bits)
    if expect_zero:
        assert value == 0 and got is None, (value, got)
        return 0, 0, 0, None
    assert got is not None and value > 0, (value, got)
    gain, loss, third = got
    assert gain - 1000 * int(view.riichi_sticks) == value and loss + third == value, (gain, loss, third, value)
    res = D.ron_result(view, winner, np_, D.kind_of_tile(tile), ura)
    return value, gain, loss, dict(yaku=list(res.yaku[: res.n_yaku]), han=int(res.han), fu=int(res.fu))


def test_riichi_ippatsu():
    def mut(v):
        p = v.players[1]
        p.riichi_declared, p.ippatsu_cycle = 1, 1
        v.riichi_sticks = 1
    hand = SC.tiles("234m456p23478s11z")
    view, np_ = _position(hand, [4 * 26 + 1], mutate=mut)      # 9s
    value, gain, loss, res = _check(view, 2, np_, 4 * 26 + 1)
    assert 2 in res["yaku"] and 30 in res["yaku"] and loss == value and gain == value + 1000


def test_open_yakuhai():
    melds = [(abi.MELD_PON, [4 * 31, 4 * 31 + 1, 4 * 31 + 2], True, 0, 4 * 31)]
    hand = SC.tiles("234m45699p78s")
    view, np_ = _position(hand, [4 * 26 + 1, 4 * 23 + 1], melds=melds, mutate=lambda v: v.dora.__setitem__(0, 4 * 27))
    v9, _, loss, res = _check(view, 2, np_, 4 * 26 + 1)
    v6, _, _, _ = _check(view, 2, np_, 4 * 23 + 1)
    assert 7 in res["yaku"] and loss == v9 == v6 == 1000


def test_tenpai_without_yaku_is_zero_with_a_win_shape():
    hand = SC.tiles("234m456p23478s11z")
    view, np_ = _position(hand, [4 * 26 + 1])
    _check(view, 2, np_, 4 * 26 + 1, expect_zero=True)
    hc = D._case(view.players[1], False)
    hc.win_tile = 4 * 26 + 1
    res = oracle.eval_hands([hc])[0]
    assert res.has_win_shape and not res.is_win and (int(res.waits) >> 26) & 1


@pytest.mark.parametrize("how", ["own_discard", "missed_agari_doujun", "missed_agari_riichi"])
def test_furiten_is_zero(how):
    def mut(v):
        p = v.players[1]
        p.riichi_declared = 1
        if how == "own_discard":
            p.n_discards = 1
            p.discards[0] = 4 * 23 + 2    # 6s: the other side of the 6-9s wait
        else:
            setattr(p, how, 1)
    hand = SC.tiles("234m456p23478s11z")
    view, np_ = _position(hand, [4 * 26 + 1, 4 * 23 + 1], mutate=mut)
    _check(view, 2, np_, 4 * 26 + 1, expect_zero=True)
    _check(view, 2, np_, 4 * 23 + 1, expect_zero=True)
    live, _ = _position(hand, [4 * 26 + 1], mutate=lambda v: setattr(v.players[1], "riichi_declared", 1))
    assert int(D.opp_danger(live, 1, 4, True)[26]) > 0, "the same hand without the furiten is live"


def test_houtei_only():
    def mut(v):
        v.drawable_count = 0
        v.wall_len = 14
    hand = SC.tiles("234m456p23478s11z")
    view, np_ = _position(hand, [4 * 26 + 1], mutate=mut)
    value, _, loss, res = _check(view, 2, np_, 4 * 26 + 1)
    assert res["yaku"] == [6] and loss == value


def test_the_red_five_is_worth_one_han_more():
    hand = SC.tiles("234m46p234678s55z")       # kanchan 5p, haku pair: riichi gives the yaku
    view, np_ = _position(hand, [52, 53], mutate=lambda v: setattr(v.players[1], "riichi_declared", 1))
    plain, _, _, res_p = _check(view, 2, np_, 53)
    red, _, _, res_r = _check(view, 2, np_, 52)
    assert res_r["han"] == res_p["han"] + 1 and red > plain
    row = D.opp_danger(view, 1, 4, True)
    assert int(row[13]) == plain and int(row[35]) == red and int(row[34]) == 0 and int(row[36]) == 0


@pytest.mark.parametrize("rule_bits,units", [(abi.RULE_TENHOU, 1), (abi.RULE_MJSOUL, 2)])
def test_suuankou_tanki_under_both_rules(rule_bits, units):
    hand = SC.tiles("111m333p555s777s9s")
    view, np_ = _position(hand, [4 * 26 + 1], rule_bits=rule_bits)
    value, _, loss, res = _check(view, 2, np_, 4 * 26 + 1, rule_bits=rule_bits)
    assert 48 in res["yaku"] and value == 32000 * units == loss


def test_daisangen_with_pao_the_gain_is_the_value_the_loss_is_not():
    melds = [(abi.MELD_PON, [4 * 31, 4 * 31 + 1, 4 * 31 + 2], True, 2, 4 * 31), (abi.MELD_PON, [4 * 32, 4 * 32 + 1, 4 * 32 + 2], True, 2, 4 * 32),
             (abi.MELD_PON, [4 * 33, 4 * 33 + 1, 4 * 33 + 2], True, 2, 4 * 33)]
    hand = SC.tiles("23m99p")
    view, np_ = _position(hand, [4 * 0 + 1], melds=melds, mutate=lambda v: (setattr(v.players[1], "pao_daisangen", 2), v.dora.__setitem__(0, 100)))
    value, gain, loss, res = _check(view, 2, np_, 4 * 0 + 1)
    assert 37 in res["yaku"]
    assert gain == value == 32000 and loss == 16000


def test_honba_two():
    melds = [(abi.MELD_PON, [4 * 31, 4 * 31 + 1, 4 * 31 + 2], True, 0, 4 * 31)]
    hand = SC.tiles("234m45699p78s")
    view, np_ = _position(hand, [4 * 26 + 1], melds=melds, mutate=lambda v: (setattr(v, "honba", 2), v.dora.__setitem__(0, 4 * 27)))
    value, _, loss, _ = _check(view, 2, np_, 4 * 26 + 1)
    assert value == loss == 1000 + 600


def test_3p_two_kita_and_a_north_dora():
    def mut(v):
        p = v.players[1]
        p.n_kita = 2
        p.kita[0], p.kita[1] = 4 * 30, 4 * 30 + 1
        v.dora[0] = 4 * 29 + 3      # West indicates North
    melds = [(abi.MELD_PON, [4 * 31, 4 * 31 + 1, 4 * 31 + 2], True, 0, 4 * 31)]
    hand = SC.tiles("12345699p78s")
    view, np_ = _position(hand, [4 * 26 + 1], mode=5, melds=melds, mutate=mut)
    value, _, loss, res = _check(view, 5, np_, 4 * 26 + 1)
    # haku 1 + nukidora 2 + the two Norths as dora 2 = 5 han: mangan
    assert res["han"] == 5 and value == loss == 8000
    with pytest.raises(ValueError):
        D.opp_danger(_position(hand, [4 * 26 + 1], mode=5, melds=melds, mutate=lambda v: (mut(v), setattr(v.players[1], "riichi_declared", 1)))[0], 1, 3, True)


def test_rows_and_kinds():
    assert [D.kind_tile(k) for k in (0, 4, 33, 34, 35, 36)] == [1, 17, 133, 16, 52, 88]
    assert [D.kind_of_tile(t) for t in (16, 17, 52, 88, 0, 135)] == [34, 4, 35, 36, 0, 33]
    hand = SC.tiles("234m46p234678s55z")
    view, np_ = _position(hand, [52], mutate=lambda v: setattr(v.players[1], "riichi_declared", 1))
    row = D.danger_of_view(view, 0, 4, True)
    assert row.shape == (3, 37) and row.dtype == np.int32 and row[0, 35] > row[0, 13] > 0 and not row[1:].any()
    assert (D.danger_of_view(view, 3, 4, True)[1] == row[0]).all(), "seat 1 is toimen of seat 3"
    assert not D.danger_of_view(view, 3, 3, True).any()
    assert not D.opp_danger(view, 0, 4, True).any(), "a seat holding a drawn tile has no ron"
