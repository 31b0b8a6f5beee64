"""The float64 restatement of the device sampler (tests/sampler_ref.py) on its own: the published splitmix64 vectors, the hash -> u
mapping over every 24-bit value, and the draw rules the GPU tests (tests/test_gpu_sampler.py) hold the kernel to."""
import math

import numpy as np

from tests import sampler_ref as R


def test_sm64_published_vectors():
    # splitmix64 seeded with 1234567: the first two outputs (the generator adds the golden gamma before mixing)
    assert int(R.sm64(1234567)) == 6457827717110365317
    assert int(R.sm64(1234567 + 0x9E3779B97F4A7C15)) == 3203168211198807973
    v = R.sm64(np.array([1234567, (1234567 + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    assert v.dtype == np.uint64 and [int(x) for x in v] == [6457827717110365317, 3203168211198807973]


def test_u_mapping_exhaustive():
    x = np.arange(1 << 24, dtype=np.uint32)
    u = R.hash_to_u(x)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    assert (np.diff(u.astype(np.float64)) >= 0).all()
    # (x + 0.5f) * 2^-24 rounded once to float32, as IEEE single precision does it - except the top value, which rounds to 1
    exact = ((x.astype(np.float64) + 0.5) / 16777216.0).astype(np.float32)
    differ = np.flatnonzero(u != exact)
    assert differ.tolist() == [R.TOP24] and exact[R.TOP24] == np.float32(1.0)
    assert u[R.TOP24] == R.U_MAX == np.float32(1.0 - 2.0 ** -24)
    assert u[0] == np.float32(2.0 ** -25)
    g = R.gumbel(u)
    assert np.isfinite(g).all()
    assert g.max() == R.gumbel(R.U_MAX) and 16.0 < g.max() < 17.0 and -3.0 < g.min() < -2.5
    for lg in (-1e4, -80.0, 0.0, 80.0, 1e4):
        assert np.isfinite(np.float64(np.float32(lg)) + g).all()


def _snap(n, mode=2, status=None, nlegal=None, mask=None, step_counts=None, game_offset=0):
    return {
        "status": np.full(n, 0x1, np.int64) if status is None else np.asarray(status, np.int64),
        "nlegal": np.full((n, 4), 5, np.uint8) if nlegal is None else np.asarray(nlegal, np.uint8),
        "mask": mask,
        "step_counts": np.zeros(n, np.uint64) if step_counts is None else np.asarray(step_counts, np.uint64),
        "game_offset": game_offset,
        "game_mode": mode,
    }


def _mask(n, ids):
    m = np.zeros((n, 4, 82), np.uint8)
    for s in range(4):
        m[:, s, ids] = 1
    return m


def test_draw_rules():
    n, legal = 2000, [3, 7, 11, 40, 81]
    snap = _snap(n, mask=_mask(n, legal), status=np.full(n, 0xF))
    ids, top, second = R.sample_ref(snap, seed=9)
    assert np.isin(ids, legal).all() and np.isfinite(top).all() and (top >= second).all()
    # cells that are never read: padding, illegal ids, nothing else depends on them
    lg = np.full((n, 4, 96), np.nan, np.float32)
    lg[:, :, legal] = 0.0
    assert (R.sample_ref(snap, 9, lg)[0] == ids).all()
    # -inf and NaN are never drawn while a finite logit is legal, and NaN draws what -inf draws
    lg[:, :, 81] = -np.inf
    lg[:, :, 7] = np.nan
    a = R.sample_ref(snap, 9, lg)[0]
    assert np.isin(a, [3, 11, 40]).all()
    lg[:, :, 7] = -np.inf
    assert (R.sample_ref(snap, 9, lg)[0] == a).all()
    # every legal id -inf or NaN: the lowest legal id
    lg[:, :, legal] = -np.inf
    lg[:, 1, 3] = np.nan
    assert (R.sample_ref(snap, 9, lg)[0] == 3).all()
    # several +inf: the lowest of them
    lg[:, :, legal] = 0.0
    lg[:, :, 40] = np.inf
    lg[:, :, 11] = np.inf
    assert (R.sample_ref(snap, 9, lg)[0] == 11).all()
    # 3P: ids >= 60 are not candidates even with their mask byte set
    s3 = _snap(n, mode=5, mask=_mask(n, legal), status=np.full(n, 0xF))
    assert np.isin(R.sample_ref(s3, 9)[0], [3, 7, 11, 40]).all()
    # the game index, the step count, the seat and the seed all move the draw; the global index is game_offset + g
    other = R.sample_ref(_snap(n, mask=_mask(n, legal), status=np.full(n, 0xF), step_counts=np.ones(n)), 9)[0]
    assert (other != ids).any() and (R.sample_ref(snap, 10)[0] != ids).any() and (ids[:, 0] != ids[:, 1]).any()
    shifted = _snap(n - 500, mask=_mask(n - 500, legal), status=np.full(n - 500, 0xF), game_offset=500)
    assert (R.sample_ref(shifted, 9)[0] == ids[500:]).all()


def test_who_draws():
    n = 8
    status = np.array([0x1, 0x2, 0xF, 0x0, 0x10001, 0x3, 0x8, 0x4], np.int64)   # game 4 is done
    nlegal = np.full((n, 4), 3, np.uint8)
    nlegal[5, 1] = 0                                                            # acting, nothing legal (3P riichi + kita)
    snap = _snap(n, status=status, nlegal=nlegal, mask=_mask(n, [1, 2, 3]))
    ids = R.sample_ref(snap, 1)[0]
    want = np.zeros((n, 4), bool)
    for g, s in [(0, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3), (5, 0), (6, 3), (7, 2)]:
        want[g, s] = True
    assert ((ids >= 0) == want).all() and ((ids == -1) | want).all()
    assert (R.acting(snap) == want).all()


def test_restatement_follows_softmax():
    # the restatement itself is a draw from softmax(logits) over the legal ids: 200 000 games at one position
    n, legal = 200_000, np.array([0, 5, 9, 13, 20, 33, 50, 61, 70])
    lg = np.zeros((n, 4, 82), np.float32)
    z = np.array([0.0, 1.0, -1.0, 2.5, -3.0, 0.5, -np.inf, 4.0, -8.0], np.float32)
    lg[:, :, legal] = z
    snap = _snap(n, mask=_mask(n, legal))
    ids = R.sample_ref(snap, 4242, lg)[0][:, 0]
    p = R.softmax_legal(lg[0, 0], legal)
    assert p[6] == 0.0 and not (ids == 50).any()
    obs = np.array([(ids == i).sum() for i in legal])
    stat, df, pv = R.chi_square(obs[p > 0], p[p > 0] * n)
    assert df >= 6 and pv > 1e-6, (obs, p * n, stat, pv)
    # and the test has power: the same counts against a uniform law fail
    assert R.chi_square(obs[p > 0], np.full(8, n / 8))[2] < 1e-6


def test_close_rows():
    top = np.array([1.0, 1.0, np.inf, -np.inf, 100.0, np.nan, 5.0])
    sec = np.array([1.0 - 5e-5, 1.0 - 3e-4, np.inf, -np.inf, 100.0 - 5e-3, np.nan, -np.inf])
    assert R.close_rows(top, sec).tolist() == [True, False, False, False, True, False, False]


def test_chi_square_helpers():
    for x in (0.1, 1.0, 3.0, 10.0, 40.0, 80.0):
        assert math.isclose(R.chi2_sf(x, 2), math.exp(-x / 2), rel_tol=1e-10)
        assert math.isclose(R.chi2_sf(x, 4), math.exp(-x / 2) * (1 + x / 2), rel_tol=1e-10)
    assert math.isclose(R.chi2_sf(3.841458820694124, 1), 0.05, rel_tol=1e-9)
    assert math.isclose(R.chi2_sf(18.307038053275146, 10), 0.05, rel_tol=1e-9)
    # bins below 5 expected draws are merged, smallest first: (1 + 2 + 47) and (50)
    stat, df, _ = R.chi_square([1, 2, 50, 47], [1.0, 2.0, 50.0, 47.0])
    assert stat == 0.0 and df == 1
    assert R.chi_square([3, 0, 10, 10, 10], [1.0, 2.0, 10.0, 10.0, 10.0])[1] == 2
    assert R.softmax_legal(None, [1, 2, 3, 4]).tolist() == [0.25] * 4
