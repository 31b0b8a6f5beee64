"""The plain restatement of the log validation (tests/log_check_ref.py) on its own, without a GPU: it finds nothing in the two golden
logs and in 32 logs per mode that the oracle wrote, and every mutation of them gives exactly the code it was made for, at an event
index not ahead of the mutation.  If the restatement flags an unmutated log, the definition is wrong: fix the definition, never the
corpus."""
import json
import os

import pytest

from tests import log_check_ref as R

GOLDEN = [os.path.join(os.path.dirname(__file__), "golden", n) for n in ("126_204_0_mjai.jsonl", "ui_example_after_injection.jsonl")]
MODES = {2: 4, 5: 3}     # game mode -> players
FULL = 8                 # logs per mode that get every mutation in all three kyokus; the others take one of the three in turn


def _golden():
    return [[json.loads(x) for x in open(p) if x.strip()] for p in GOLDEN]


def _assert_mutations(log, n, mode, positions, tag):
    muts = R.mutations(log, n, positions)
    for name, (events, code, point) in muts.items():
        got = R.check_log(events, n, mode)
        assert got[0] == code and got[1] >= point, (tag, name, R_NAMES[code], point, got)
    return muts


R_NAMES = ["OK", "PARSE", "NO_START_KYOKU", "AFTER_END", "UNFINISHED", "ACTOR", "DRAW_OUT_OF_TURN", "NOT_OFFERED", "TILE_NOT_HELD", "TILE_COUNT", "NO_LEGAL_MATCH",
           "SCORE_CONTINUITY", "SCORE_CONSERVATION"]


def test_the_names_are_the_librarys():
    from riichienv_amd import abi, logcheck

    assert R_NAMES == abi.LOGCHECK_NAMES == logcheck.NAMES and logcheck.CODES["SCORE_CONSERVATION"] == R.SCORE_CONSERVATION == 12


def test_golden_logs_are_clean_and_every_mutation_is_found():
    for i, log in enumerate(_golden()):
        assert R.check_log(log, 4, 2) == (R.OK, 0, 0, R.NO_SEAT), GOLDEN[i]
        muts = _assert_mutations(log, 4, 2, ("first", "mid", "last"), GOLDEN[i])
        assert R.kinds(muts) == set(range(2, 13)), sorted(R.kinds(muts))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_oracle_logs_are_clean_and_every_mutation_is_found(mode):
    n = MODES[mode]
    logs = R.oracle_logs(mode, 32)
    kinds, count = set(), 0
    for i, log in enumerate(logs):
        assert R.check_log(log, n, mode) == (R.OK, 0, 0, R.NO_SEAT), (mode, i)
        muts = _assert_mutations(log, n, mode, ("first", "mid", "last") if i < FULL else (("first", "mid", "last")[i % 3],), (mode, i))
        kinds |= R.kinds(muts)
        count += len(muts)
    print(f"mode {mode}: {len(logs)} clean logs, {count} mutated ones")
    assert kinds == set(range(2, 13)), sorted(kinds)


def test_findings_at_a_logs_first_and_last_event():
    log = R.oracle_logs(2, 32)[0]
    muts = R.mutations(log, 4, ("mid",))
    assert R.check_log(muts["no_start_kyoku_at_first_event"][0], 4, 2)[:2] == (R.NO_START_KYOKU, 0)
    events = muts["tsumo_after_the_end"][0]
    assert R.check_log(events, 4, 2)[:2] == (R.AFTER_END, len(events) - 1)
    events = muts["cut_mid_kyoku"][0]
    assert R.check_log(events, 4, 2)[:2] == (R.UNFINISHED, len(events))
    assert R.check_log([], 4, 2) == R.check_log([{"type": "start_game"}], 4, 2) == R.check_log([{"type": "start_game"}, {"type": "end_game"}], 4, 2) == (R.OK, 0, 0, R.NO_SEAT)


def test_both_readings_of_a_ryukyokus_deltas_pass_and_nothing_else():
    """converted Tenhou logs (the golden one) hold a ryukyoku's deltas without the riichi deposits, the oracle's logs with them; a kyoku
    that fits neither reading in some seat is SCORE_CONTINUITY"""
    log = _golden()[0]
    starts = [i for i, e in enumerate(log) if e["type"] == "start_kyoku"]
    at = [(i, {x["actor"] for x in log[max(k for k in starts if k < i): i] if x["type"] == "reach"}) for i, e in enumerate(log[: starts[-1]]) if e["type"] == "ryukyoku"]
    at = [(i, seats) for i, seats in at if seats]
    assert at, "the golden log holds a ryukyoku behind a riichi, ahead of its last kyoku"
    i, seats = at[0]
    with_deposit = list(log)
    with_deposit[i] = dict(log[i], deltas=[d - (1000 if s in seats else 0) for s, d in enumerate(log[i]["deltas"])])
    assert R.check_log(with_deposit, 4, 2)[0] == R.OK
    neither = list(log)
    neither[i] = dict(log[i], deltas=[d - (500 if s in seats else 0) for s, d in enumerate(log[i]["deltas"])])
    assert R.check_log(neither, 4, 2)[0] == R.SCORE_CONTINUITY
