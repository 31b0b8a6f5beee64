"""The restatement of the PPO worker's bookkeeping (tests/ppo_collect_ref.py) on cases worked by hand: the GPU tests
(tests/test_gpu_ppo_collect.py) hold the collector's kernels to it."""
import numpy as np

from tests import ppo_collect_ref as R

A = 6


def _row(v, legal=(0, 2, 3), logits=None):
    mask = np.zeros(A, np.uint8)
    mask[list(legal)] = 1
    lg = np.zeros(A, np.float32) if logits is None else np.asarray(logits, np.float32)
    return ("f", mask, lg, np.float32(v))


def _ids(n, acting):
    ids = np.full((n, 4), -1, np.int32)
    for g, p, a in acting:
        ids[g, p] = a
    return ids


def test_single_step_advantage_is_reward_minus_value():
    p = R.PoolRef(1, 8, 0.99, 0.95, [2])
    p.record(_ids(1, [(0, 2, 3)]), lambda g: _row(0.25))
    p.close([1], [1.5])
    e = p.emit()
    assert e["advantage"].tolist() == [np.float32(1.5 - 0.25)] and e["return"].tolist() == [np.float32(1.5)]
    assert p.counts() == {"fill": 1, "valid": 1, "dropped": 0, "overflowed": 0, "segments": 1, "open": 0}


def test_gamma_lambda_one_returns_the_reward_everywhere():
    vals = [0.5, -0.25, 0.125, 2.0]
    p = R.PoolRef(1, 8, 1.0, 1.0, [0])
    for v in vals:
        p.record(_ids(1, [(0, 0, 0)]), lambda g, v=v: _row(v))
        p.close([0], [0.0])
    p.close([1], [3.0])
    e = p.emit()
    assert e["return"].tolist() == [3.0] * 4                      # (dyadic values: every sum is exact)
    assert e["advantage"].tolist() == [3.0 - v for v in vals]


def test_gae_by_hand_two_steps():
    g, lam, r, v0, v1 = 0.5, 0.5, 1.0, 0.25, 0.5
    adv, ret = R.gae_ref([np.float32(v0), np.float32(v1)], np.float32(r), g, lam)
    a1 = r - v1
    a0 = (g * v1 - v0) + g * lam * a1
    assert adv == [a0, a1] and ret == [a0 + v0, a1 + v1]


def test_only_the_hero_seat_records_and_order_is_by_game():
    p = R.PoolRef(3, 8, 0.9, 0.9, [1, 255, 0])
    wrote = p.record(_ids(3, [(0, 0, 2), (0, 1, 3), (1, 0, 0), (2, 0, 2)]), lambda g: _row(g))
    assert wrote == [(0, 0), (2, 1)]                              # game 1 has no hero; game 0 records seat 1 only
    assert [s["action"] for s in p.slots] == [3, 2]
    wrote = p.record(_ids(3, [(2, 0, 0), (0, 1, 0)]), lambda g: _row(g))
    assert wrote == [(0, 2), (2, 3)] and [s["prev"] for s in p.slots] == [-1, -1, 0, 1] and [s["t"] for s in p.slots] == [0, 0, 1, 1]


def test_renchan_under_both_boundary_rules():
    """three rounds of one game: east 1, east 1 again (renchan: kyoku_idx stays 0), east 2.  The round rule closes three trajectories, the
    worker's kyoku_idx rule two - the renchan extends the first, and its reward is the score change over both rounds"""
    round_ended, kidx, delta = [0, 1, 0, 1, 0, 1], [0, 0, 0, 1, 1, 2], [0, 1000, 0, -3000, 0, 500]
    a = R.PoolRef(1, 16, 0.99, 0.95, [0])
    b = R.PoolRef(1, 16, 0.99, 0.95, [0])
    prev, acc = np.zeros(1, np.int64), 0
    for s in range(6):
        for p in (a, b):
            p.record(_ids(1, [(0, 0, 0)]), lambda g: _row(0.0))
        a.close([round_ended[s]], [delta[s] / 1000.0])
        acc += delta[s]
        done, prev = R.boundary_kyoku_idx([round_ended[s]], [kidx[s]], prev, b.open_len())
        b.close(done, [acc / 1000.0])
        if done[0]:
            acc = 0
    assert [(len(t), r) for _, _, t, r in a.completed] == [(2, 1.0), (2, -3.0), (2, 0.5)]
    assert [(len(t), r) for _, _, t, r in b.completed] == [(4, -2.0), (2, 0.5)]
    assert [s for _, s, _, _ in a.completed] == [0, 1, 2] and a.counts()["valid"] == b.counts()["valid"] == 6


def test_overflow_breaks_the_trajectory_and_is_counted():
    p = R.PoolRef(2, 3, 0.99, 0.95, [0, 0])
    both = _ids(2, [(0, 0, 0), (1, 0, 0)])
    assert p.record(both, lambda g: _row(1.0)) == [(0, 0), (1, 1)]
    assert p.record(both, lambda g: _row(1.0)) == [(0, 2)]        # game 1 finds the pool full
    p.close([1, 1], [1.0, 1.0])
    c = p.counts()
    assert c == {"fill": 3, "valid": 2, "dropped": 1, "overflowed": 1, "segments": 1, "open": 0}
    assert p.emit()["slot"].tolist() == [0, 2]                    # game 1's trajectory has a hole: not emitted
    assert p.record(both, lambda g: _row(1.0)) == [] and p.counts()["overflowed"] == 3


def test_open_trajectory_at_the_end_is_left_out():
    p = R.PoolRef(2, 8, 0.99, 0.95, [0, 1])
    p.record(_ids(2, [(0, 0, 0), (1, 1, 2)]), lambda g: _row(0.5))
    p.close([1, 0], [2.0, 9.0])
    assert p.counts() == {"fill": 2, "valid": 1, "dropped": 0, "overflowed": 0, "segments": 1, "open": 1}
    assert p.emit()["slot"].tolist() == [0]
    p.close([1, 1], [0.0, 1.0])                                   # game 0: empty trajectory, skipped
    assert p.counts()["segments"] == 2 and p.serial == [1, 1]


def test_argmax_rules():
    m = [1, 0, 1, 1, 0, 1]
    nan, inf = float("nan"), float("inf")
    assert R.argmax_ref(m, [0, 9, 1, 1, 9, 0]) == 2               # ties to the lowest id, masked ids never
    assert R.argmax_ref(m, [nan, 9, -inf, -5, 9, nan]) == 3       # NaN and -inf lose to a finite logit
    assert R.argmax_ref(m, [nan, 9, -inf, -inf, 9, nan]) == 0     # nothing else: the lowest legal id
    assert R.argmax_ref(m, [1, 9, inf, inf, 9, 3]) == 2
    assert R.argmax_ref(m, None) == 0 and R.argmax_ref([0] * 6, None) == -1
    ids = R.select_ref([[4, 5, -1, -1]], [1], [[True, True, False, False]], [[m, m, m, m]], [[[0, 0, 3, 0, 0, 0]] * 4])
    assert ids.tolist() == [[2, 5, -1, -1]]
    assert R.select_ref([[4, 5, -1, -1]], [255], [[True, True, False, False]], [[m, m, m, m]], None).tolist() == [[0, 0, -1, -1]]


def test_log_prob_matches_torch_float64():
    import torch

    rng = np.random.default_rng(0)
    lg = (rng.standard_normal((500, 82)) * 3).astype(np.float32)
    mk = (rng.random((500, 82)) < 0.15).astype(np.uint8)
    mk[:, 7] = 1
    act = np.array([np.flatnonzero(r)[0] for r in mk])
    want = torch.log_softmax(torch.from_numpy(lg).double().masked_fill(~torch.from_numpy(mk).bool(), -1e9), -1).gather(1, torch.from_numpy(act)[:, None])[:, 0]
    assert np.abs(R.log_prob_ref(mk, lg, act) - want.numpy()).max() < 1e-12


def test_argmax_rows_is_argmax_ref():
    rng = np.random.default_rng(3)
    lg = np.round(rng.standard_normal((4000, 12)) * 2).astype(np.float32)      # (rounded: many ties)
    sp = rng.random(lg.shape)
    lg[sp < 0.1] = np.nan
    lg[(sp >= 0.1) & (sp < 0.2)] = -np.inf
    lg[(sp >= 0.2) & (sp < 0.25)] = np.inf
    mk = (rng.random(lg.shape) < 0.3).astype(np.uint8)
    got = R.argmax_rows(mk, lg)
    assert got.tolist() == [R.argmax_ref(m, r) for m, r in zip(mk, lg)]
    assert (got < 0).any() and (got >= 0).any()
