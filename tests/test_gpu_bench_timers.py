"""The three event-timed launch loops of the C ABI - rmj_bench_encode, rmj_bench_encode_compact, rmj_bench_hand_kernel - share one
host helper (a warm-up launch, `reps` launches between two events, the average in ms).  Each returns 0 and a positive average, and the
encoder timers leave in the caller's buffers exactly what the `_device` entry point they repeat leaves there on the same state.  The
hand-kernel timer hands nothing back but the time (its outputs live in a buffer of the call), so it is held to its return code, its
argument checks and the time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_GAMES, N_HANDS, REPS = 64, 256, 2


def _env(mode):
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(N_GAMES, game_mode=mode, seed=5, event_ring=64)
    env.reset()
    env.step_random(9, 40, auto_reset=False)     # mid-hand states: discards, melds, claims to answer
    return env


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("extended", [False, True])
def test_bench_encode_leaves_the_device_entry_points_tensor(mode, extended):
    import torch

    from riichienv_amd import vecenv

    env = _env(mode)
    w, ch = (27 if mode >= 3 else 34), (215 if extended else 74)
    want = torch.full((N_GAMES, 4, ch, w), -7.0, dtype=torch.float32, device="cuda:0")
    got = torch.full((N_GAMES, 4, ch, w), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()      # torch's stream is not the handle's stream
    twin = env.L.rmj_encode_extended_device if extended else env.L.rmj_encode_device
    vecenv._chk(twin(env.h, 2, C.c_void_p(want.data_ptr())))
    ms = env.bench_encode(got.data_ptr(), REPS, extended=extended, only_active=2)
    env.L.rmj_sync(env.h)
    assert ms > 0.0
    assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    assert float(want.max().item()) > 0.0      # (some seat acts: the comparison is not of two untouched buffers)
    bad = C.c_double()
    assert env.L.rmj_bench_encode(env.h, int(extended), 2, C.c_void_p(got.data_ptr()), 0, C.byref(bad)) != 0     # reps = 0 is refused


@pytest.mark.parametrize("mode", [2, 5])
def test_bench_encode_compact_leaves_the_device_entry_points_batch(mode):
    import torch

    env = _env(mode)
    w, cap = (27 if mode >= 3 else 34), N_GAMES * 2
    bufs = []
    for _ in range(2):
        bufs.append((torch.full((cap, 74, w), -7.0, dtype=torch.float32, device="cuda:0"), torch.full((cap,), -1, dtype=torch.int32, device="cuda:0"),
                     torch.zeros((1,), dtype=torch.int32, device="cuda:0")))
    torch.cuda.synchronize()
    (wo, wi, wc), (go, gi, gc) = bufs
    env.encode_compact_device(wo.data_ptr(), wi.data_ptr(), cap, wc.data_ptr())
    ms = env.bench_encode_compact(go.data_ptr(), gi.data_ptr(), cap, gc.data_ptr(), REPS)
    env.L.rmj_sync(env.h)
    assert ms > 0.0
    k = int(wc.item())
    assert 0 < k <= cap and int(gc.item()) == k
    assert torch.equal(wi, gi) and torch.equal(wo.view(torch.int32), go.view(torch.int32))


def _hand_inputs(which, rng):
    from riichienv_amd import abi

    counts = np.zeros((N_HANDS, 34), np.uint8)
    for row in counts:      # 14 tiles of at most four a type
        for t in rng.permutation(np.repeat(np.arange(34), 4))[:14]:
            row[t] += 1
    if which == 0:
        cases = (abi.HandCase * N_HANDS)()
        for i, hc in enumerate(cases):     # 123m 456m 789m 123p + a pair of a number of souzu, won by tsumo on the pair
            pair = 72 + 4 * (i % 9)
            tiles = [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, pair, pair + 1]
            hc.n_tiles = 14
            for j, t in enumerate(tiles):
                hc.tiles[j] = t
            hc.win_tile, hc.tsumo, hc.player_wind, hc.round_wind = pair + 1, 1, i % 4, 0
        return cases, None
    if which in (1, 2, 3):
        return counts, None
    if which == 4:
        return counts, np.minimum(counts + rng.integers(0, 2, counts.shape, dtype=np.uint8), 4).astype(np.uint8)
    five = np.stack([rng.integers(1, 14, N_HANDS), rng.choice([20, 25, 30, 40, 50], N_HANDS), rng.integers(0, 2, N_HANDS), rng.integers(0, 2, N_HANDS),
                     rng.choice([3, 4], N_HANDS)]).astype(np.uint8)      # han, fu, oya, tsumo, num_players: five byte arrays one after the other
    return np.ascontiguousarray(five), rng.integers(0, 5, N_HANDS).astype(np.uint32)


@pytest.mark.parametrize("which", range(6))
def test_bench_hand_kernel_times_every_kernel(which):
    from riichienv_amd import vecenv

    L = vecenv.load_lib()
    a, b = _hand_inputs(which, np.random.default_rng(which))
    pa = C.cast(a, C.c_void_p) if which == 0 else C.c_void_p(a.ctypes.data)
    pb = C.c_void_p(b.ctypes.data) if b is not None else None
    ms = C.c_double(-1.0)
    vecenv._chk(L.rmj_bench_hand_kernel(0, which, pa, pb, N_HANDS, 0, REPS, C.byref(ms)))
    assert ms.value > 0.0
    assert L.rmj_bench_hand_kernel(0, which, pa, pb, N_HANDS, 0, 0, C.byref(ms)) != 0      # reps = 0
    assert L.rmj_bench_hand_kernel(0, 6, pa, pb, N_HANDS, 0, REPS, C.byref(ms)) != 0          # no such kernel
