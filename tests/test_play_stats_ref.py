"""CPU: the plain restatement of the play statistics (tests/play_stats_ref.py) against totals counted by hand on the golden log and on
hand-made logs, its two readings of a hora against each other, and riichienv_amd.stats.summarize on a hand-written table against rates
worked out by hand."""
import json
import math
import os
import re

import numpy as np

from riichienv_amd import abi, stats
from tests import play_stats_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "126_204_0_mjai.jsonl")


def _golden():
    with open(GOLDEN) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_the_columns_have_one_naming():
    assert list(stats.COLUMNS) == abi.PLAYSTAT_NAMES and len(stats.COLUMNS) == abi.PLAYSTAT_COLUMNS == 16
    for i, name in enumerate(stats.COLUMNS):
        assert getattr(abi, "PLAYSTAT_" + name) == i == getattr(R, name)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "..", "include", "riichi_mi355x.h")).read()
    for i, name in enumerate(stats.COLUMNS):
        assert re.search(rf"#define RMJ_PLAYSTAT_{name} +{i}\b", hdr), name
    assert "#define RMJ_PLAYSTAT_COLUMNS 16\n" in hdr


def test_golden_log_totals_and_both_readings_of_every_hora():
    log = _golden()
    rows = R.kyoku_rows(log, 4)
    assert rows.shape == (12, 4, 16)
    tot = rows.sum(axis=(0, 1))
    want = {"WIN": 9, "WIN_TSUMO": 5, "DEAL_IN": 4, "RIICHI": 10, "RIICHI_ACCEPTED": 9, "CHI": 9, "PON": 18, "KANS": 1, "DISCARDS": 659}
    assert {k: int(tot[getattr(R, k)]) for k in want} == want
    assert int(((rows[:, 0, R.END] & 2) != 0).sum()) == 3
    assert (rows[:, :, R.END] == rows[:, :1, R.END]).all() and (rows[:, :, R.DEALER].sum(axis=1) == 1).all()
    derived, by_target = R.derived_horas(log, 4), R.target_horas(log, 4)
    assert len(derived) == 9 and derived == by_target


def test_hand_made_logs_by_hand():
    for seats in (4, 3):
        logs = R.hand_made_logs(seats)
        for k in (0, 1, 63, 64, 65, 128, 129):
            assert len(logs[f"len{k}"]) == k
        t = {name: R.kyoku_rows(ev, seats) for name, ev in logs.items()}
        assert t["len0"].shape == (0, 4, 16) and t["len1"].shape == (1, 4, 16) and int(t["len1"].sum()) == 1        # the dealer flag alone
        assert int(t["len129"][0, :, R.DISCARDS].sum()) == 64
        assert logs["sk_lane63_lane0"][63]["type"] == logs["sk_lane63_lane0"][64]["type"] == "start_kyoku" and t["sk_lane63_lane0"].shape[0] == 3
        assert int(t["sk_lane63_lane0"][1].sum()) == 1 and t["sk_lane63_lane0"][2, 1, R.WIN] == 1                     # an empty kyoku between the two
        assert t["thirty_kyokus"].shape[0] == 30 and len(logs["thirty_kyokus"]) == 90 and (t["thirty_kyokus"][:, :, R.WIN_TSUMO].sum(axis=1) == 1).all()
        assert len(logs["hora_lane0"]) == 65 and t["hora_lane0"][0, 2, R.WIN] == 1 and t["hora_lane0"][0, :, R.DEAL_IN].sum() + t["hora_lane0"][0, 2, R.WIN_TSUMO] == 1
        assert len(logs["hora_two_passes_back"]) > 128 + 7 and t["hora_two_passes_back"][0, (9 // 2) % seats, R.DEAL_IN] == 1
        d = t["double_ron"][0]
        assert d[0, R.DEAL_IN] == 2 and d[1, R.WIN] == d[2, R.WIN] == 1 and d[:, R.WIN_TSUMO].sum() == 0 and (d[:seats, R.END] == 1).all()
        d = t["triple_hora"][0]
        assert d[1, R.DEAL_IN] == 3 and d[0, R.WIN] == 2 and d[2, R.WIN] == 1 and d[0, R.WIN_TURN] == 0
        d = t["reach_ronned"][0]
        assert d[0, R.RIICHI] == 1 and d[0, R.RIICHI_ACCEPTED] == 0 and d[0, R.RIICHI_TURN] == 2 and d[0, R.DEAL_IN] == 1 and d[1, R.WIN] == 1
        d = t["two_reaches"][0]
        assert d[2, R.RIICHI] == 2 and d[2, R.RIICHI_ACCEPTED] == 1 and d[2, R.RIICHI_TURN] == 1 and (d[:seats, R.END] == 2).all()
        d = t["chankan"][0]
        assert d[1, R.DEAL_IN] == 1 and d[1, R.KANS] == 1 and d[1, R.PON] == 1 and d[2, R.WIN] == 1 and d[2, R.WIN_TSUMO] == 0 and d[2, R.WIN_TURN] == 1
        d = t["hora_without_tile_event"][0]
        assert d[1, R.WIN] == 1 and d[:, R.WIN_TSUMO].sum() == 0 and d[:, R.DEAL_IN].sum() == 0 and d[0, R.RIICHI_TURN] == 1
        d = t["hora_after_own_dahai"][0]
        assert d[1, R.WIN] == 1 and d[1, R.WIN_TURN] == 1 and d[:, R.WIN_TSUMO].sum() == 0 and d[:, R.DEAL_IN].sum() == 0
        d = t["events_before_first_kyoku"]
        assert d.shape[0] == 1 and d[0, :, R.WIN].sum() == 0 and d[0, :, R.RIICHI].sum() == 0 and (d[0, :, R.END] == 0).all() and d[0, :, R.DISCARDS].sum() == 2
        d = t["actors_4_5"][0]
        assert d[:, R.WIN].sum() == 1 and d[0, R.DEAL_IN] == 1 and d[:, R.RIICHI].sum() == 0 and d[:, R.CALLS].sum() == 0 and (d[:seats, R.END] == 1).all()
        assert d[:, R.DISCARDS].sum() == 1 and d[:, R.KANS].sum() == 0
        d = t["kans_and_calls"][0]
        assert d[1, R.DEALER] == 1 and d[1, R.CHI] == 1 and d[2, R.KANS] == 2 and d[2, R.CALLS] == 1 and d[0, R.KANS] == 1 and d[0, R.CALLS] == 1
        assert d[0, R.WIN_TSUMO] == 1 and d[2, R.TSUMOGIRI] == 1
        if seats == 3:
            d = t["kita_and_seat3"][0]
            assert d[:, R.KITA].tolist() == [1, 1, 1, 0] and (d[3] == 0).all() and d[1, R.DEAL_IN] == 1 and d[2, R.WIN] == 2 and d[2, R.WIN_TSUMO] == 1
            assert d[2, R.DEALER] == 1 and d[0, R.DISCARDS] == 1
        for rows in t.values():
            assert (rows[:, seats:] == 0).all()


def test_the_soup_is_seeded_and_covers_the_lengths():
    a, b = R.soup_logs(400, 4, 7), R.soup_logs(400, 4, 7)
    assert a == b and a != R.soup_logs(400, 4, 8)
    lengths = [len(l) for l in a]
    assert min(lengths) <= 5 and max(lengths) > 350 and all(sum(1 for n in lengths if n == k) >= 5 for k in (63, 64, 65, 127, 128, 129, 191, 192, 193))
    types = {ev.get("type") for l in a for ev in l}
    assert set(R.TYPES) <= types and {None, "", "nukidora"} <= types
    assert {ev.get("actor") for l in a for ev in l} >= {0, 1, 2, 3, 4, 5}
    tab = R.table(a, 4)
    assert tab.shape[0] == R.kyoku_offsets(a)[-1] > 2000 and tab[:, :, R.DEAL_IN].sum() > 100 and tab[:, :, R.WIN_TSUMO].sum() > 20 and (tab >= 0).all()
    assert (R.table(a, 4, bad={3})[R.kyoku_offsets(a)[3]: R.kyoku_offsets(a)[4]] == -1).all()


# ------------------------------------------------------------------ summarize on a table written by hand
def _row(**kw):
    r = [0] * 16
    for k, v in kw.items():
        r[getattr(R, k)] = v
    return r


def _hand_table():
    k0 = [_row(WIN=1, WIN_TSUMO=1, RIICHI=1, RIICHI_ACCEPTED=1, RIICHI_TURN=6, DISCARDS=8, TSUMOGIRI=2, WIN_TURN=8, DEALER=1, END=1),
          _row(DISCARDS=8, TSUMOGIRI=4, CALLS=2, CHI=1, PON=1, END=1),
          _row(RIICHI=1, RIICHI_TURN=4, DISCARDS=7, TSUMOGIRI=1, END=1),
          _row(DISCARDS=7, END=1)]
    k1 = [_row(DISCARDS=18, TSUMOGIRI=3, END=2),
          _row(RIICHI=1, RIICHI_ACCEPTED=1, RIICHI_TURN=9, DISCARDS=17, TSUMOGIRI=9, DEALER=1, END=2),
          _row(DISCARDS=17, TSUMOGIRI=2, END=2),
          _row(CALLS=1, PON=1, DISCARDS=17, TSUMOGIRI=6, END=2)]
    rows = np.array([k0, k1, [[-1] * 16] * 4], dtype=np.int32)
    return {"rows": rows, "log_of": np.array([0, 0, 1]), "num_players": 4,
            "start_scores": np.array([[25000] * 4, [31000, 23000, 23000, 23000], [25000] * 4], np.int32),
            "end_scores": np.array([[31000, 23000, 23000, 23000], [30000, 24500, 22500, 23000], [0] * 4], np.int32),
            "rank": np.array([[0, 1, 3, 2], [0, 1, 3, 2], [255] * 4], np.uint8)}


def _same(got, want):
    assert list(got) == list(want), (list(got), list(want))
    for k, w in want.items():
        g = got[k]
        for a, b in zip(g if isinstance(g, list) else [g], w if isinstance(w, list) else [w]):
            assert isinstance(a, float) and ((math.isnan(a) and math.isnan(b)) or a == b), (k, g, w)


def test_summarize_against_rates_worked_out_by_hand():
    nan = float("nan")
    t = _hand_table()
    pooled = {"kyokus": 8.0, "win_rate": 1 / 8, "tsumo_share": 1.0, "deal_in_rate": 0.0, "riichi_rate": 3 / 8, "riichi_accept_share": 2 / 3, "call_rate": 2 / 8,
              "ryukyoku_rate": 4 / 8, "mean_riichi_turn": 19 / 3, "mean_win_turn": 8.0, "dealer_win_rate": 1 / 2, "tsumogiri_share": 27 / 99,
              "win_points_mean": 6000.0, "deal_in_points_mean": nan, "rank_mean": 1.5, "rank_rates": [0.25, 0.25, 0.25, 0.25]}
    _same(stats.summarize(t), pooled)
    # a bare table: the -1 row masks itself, no points, no ranks
    _same(stats.summarize(t["rows"]), {k: v for k, v in pooled.items() if k not in ("win_points_mean", "deal_in_points_mean", "rank_mean", "rank_rates")})
    # the hero of log 0 is seat 2, of the log that did not parse seat 0
    hero = {"kyokus": 2.0, "win_rate": 0.0, "tsumo_share": nan, "deal_in_rate": 0.0, "riichi_rate": 1 / 2, "riichi_accept_share": 0.0, "call_rate": 0.0,
            "ryukyoku_rate": 1 / 2, "mean_riichi_turn": 4.0, "mean_win_turn": nan, "dealer_win_rate": nan, "tsumogiri_share": 3 / 24,
            "win_points_mean": nan, "deal_in_points_mean": nan, "rank_mean": 3.0, "rank_rates": [0.0, 0.0, 0.0, 1.0]}
    _same(stats.summarize(t, hero=np.array([2, 0])), hero)
    # the dealer of kyoku 0 as hero: a deal-in made up in kyoku 1 to have its points
    t["rows"][1, 0, R.DEAL_IN] = 1
    got = stats.summarize(t, hero=[0, 0])
    assert got["kyokus"] == 2.0 and got["win_rate"] == 0.5 and got["deal_in_rate"] == 0.5 and got["win_points_mean"] == 6000.0 and got["deal_in_points_mean"] == 1000.0
    assert got["dealer_win_rate"] == 1.0 and got["rank_mean"] == 0.0 and got["mean_win_turn"] == 8.0
    # three players: seat 3 is no sample
    t3 = dict(t, num_players=3)
    assert stats.summarize(t3)["kyokus"] == 6.0 and stats.summarize(t3, hero=[3, 3])["kyokus"] == 0.0 and math.isnan(stats.summarize(t3, hero=[3, 3])["win_rate"])
    # nothing at all
    empty = stats.summarize(np.zeros((0, 4, 16), np.int32))
    assert empty["kyokus"] == 0.0 and all(math.isnan(v) for k, v in empty.items() if k != "kyokus")


def test_summarize_of_the_restated_golden_log():
    log = _golden()
    s = stats.summarize({"rows": R.kyoku_rows(log, 4), "log_of": np.zeros(12, np.int64), "num_players": 4})
    assert s["kyokus"] == 48.0 and s["win_rate"] == 9 / 48 and s["tsumo_share"] == 5 / 9 and s["deal_in_rate"] == 4 / 48 and s["ryukyoku_rate"] == 3 / 12
    assert s["riichi_rate"] == 10 / 48 and s["riichi_accept_share"] == 9 / 10
