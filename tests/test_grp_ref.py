"""CPU: the plain restatement of the GRP rows (tests/grp_ref.py) against the package's own host objects - the features
MjaiReplay.from_events(...).rounds[i].take_grp_features() gives, encoded the way GrpFeatureEncoder + GrpReplayDataset._encode_features
do - and against datasets' stable-argsort rank; and the proof that the sweep of the GPU test tells a float64 division from a float32
reciprocal multiply."""
import numpy as np
import pytest

from riichienv_amd import datasets
from riichienv_amd.replay import MjaiReplay
from tests import grp_ref as R


def _encoder_rows(log, n):
    """GrpFeatureEncoder(kyoku, n).encode() -> _encode_features for every kyoku and seat, with numpy as the dataset does it"""
    S = 35000.0 if n == 3 else 25000.0
    out = []
    for k in MjaiReplay.from_events(log).rounds:
        f = k.take_grp_features()
        scores = np.array([f["round_initial_scores"][i] / S for i in range(n)] + [f["round_end_scores"][i] / S for i in range(n)] +
                          [f["round_delta_scores"][i] / 12000.0 for i in range(n)], dtype=np.float32)
        meta = np.array([f["chang"] / 3.0, f["ju"] / 3.0, f["ben"] / 4.0, f["liqibang"] / 4.0], dtype=np.float32)
        seats = []
        for p in range(n):
            player = np.zeros(n, dtype=np.float32)
            player[p] = 1.0
            seats.append(np.concatenate([scores, meta, player]))
        out.append(np.stack(seats))
    return np.stack(out) if out else np.zeros((0, n, 4 * n + 4), np.float32)


@pytest.mark.parametrize("seats", [4, 3])
def test_rows_equal_the_feature_encoder_on_self_written_logs(seats):
    logs = R.random_logs(40, seats, seed=3 + seats)
    ref = R.logset_rows(logs, seats)
    want = np.concatenate([_encoder_rows(l, seats) for l in logs])
    assert ref["x"].shape == want.shape and want.shape[0] > 100
    assert np.array_equal(R.bits(ref["x"]), R.bits(want))
    start, end = datasets.kyoku_tables(logs, seats)
    assert np.array_equal(ref["start"], start) and np.array_equal(ref["end"], end)
    metas = [(k.chang, k.ju, k.ben, k.liqibang) for l in logs for k in MjaiReplay.from_events(l).rounds]
    assert ref["meta"].tolist() == [list(m) for m in metas]
    assert (ref["meta"][:, 1] == -1).any() and (ref["meta"][:, 3] == 300).any() and {0, 1, 2, 3} <= set(ref["meta"][:, 0].tolist())
    # the label: the seat's place in the log's last kyoku's end scores, on every kyoku of the log
    for l, log in enumerate(logs):
        rows = range(int(ref["kyoku_offsets"][l]), int(ref["kyoku_offsets"][l + 1]))
        final = datasets.compute_rank(end[rows[-1]][None], seats)[0]
        for r in rows:
            assert ref["rank"][r].tolist() == final.tolist() and ref["log_of"][r] == l


def test_ranks_equal_the_stable_argsort_on_tie_heavy_scores():
    rng = np.random.default_rng(9)
    for n in (3, 4):
        vecs = [[25000] * 4, [0, 0, -100, -100], [-5, 7, 7, -5], [1, 2, 3, 4], [4, 3, 2, 1]] + rng.integers(-3, 3, size=(400, 4)).tolist()
        want = datasets.compute_rank(np.array(vecs), n)
        for v, w in zip(vecs, want):
            assert R.ranks(v, n) == w.tolist(), v


@pytest.mark.parametrize("n", [4, 3])
def test_the_sweep_tells_the_division_from_a_reciprocal_multiply(n):
    init, delta, meta = R.sweep_case()
    end = [[a + b for a, b in zip(i, d)] for i, d in zip(init, delta)]
    good, wrong = R.rows(init, end, meta, n), R.rows_reciprocal(init, end, meta, n)
    k = len(R.SWEEP)
    differ = int((R.bits(good[:k, 0, 0]) != R.bits(wrong[:k, 0, 0])).sum())        # seat 0's init / S over the sweep
    print(f"n={n}: init / S differs from the reciprocal form in {differ} of {k} values")
    assert differ > 0
    if n == 4:
        assert differ == 614
    assert (R.bits(good[:k, 0, 2 * n + 1]) != R.bits(wrong[:k, 0, 2 * n + 1])).sum() > 0   # seat 1's delta / 12000
    v = 2 ** 24 + 1                      # the first integer float32 cannot hold is among the rows
    assert int(np.float32(v)) != v
    assert any(v in r for r in init)


def test_a_log_without_a_kyoku_and_a_last_kyoku_without_end_scores():
    empty = [{"type": "start_game"}, {"type": "end_game"}]
    open_end = R.hand_made_log([(dict(scores=[30000, 20000, 25000, 25000]), ("hora", 0, 1, [1000, -1000, 0, 0])),
                                (dict(scores=[31000, 19000, 25000, 25000], kyoku=2), None)], end_game=False)
    ref = R.logset_rows([empty, open_end], 4)
    assert ref["kyoku_offsets"].tolist() == [0, 0, 2] and ref["end"].tolist() == [[31000, 19000, 25000, 25000]] * 2
    assert ref["rank"].tolist() == [[0, 3, 1, 2]] * 2
