"""GPU: MJAI text formatted on the device (rmj_drain_text / rmj_format_events_device, VecRiichiEnv.drain_text, TorchVecEnv.drain_text)
against the host formatter (rmj_drain_format / rmj_format_events, which stay the definition) and the oracle's logs: the same bytes and
offsets, the same cursors and loss counters."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from riichienv_amd import abi, vecenv
from riichienv_amd.shard import game_seed

pytestmark = pytest.mark.gpu


def _host(env, cur, seat=-1):
    """rmj_drain_format's text under the cursors `cur`, as a peek"""
    buf, toffs = env.drain_logs(seat=seat, cursor=cur.copy(), raw=True, peek=True)
    return bytes(buf[: int(toffs[-1])]), toffs.copy()


def _device_bytes(v):
    """a device-delivered RmjTextView, copied down through torch"""
    import torch

    from riichienv_amd.torch_env import _CudaArray

    offs = torch.as_tensor(_CudaArray(v.text_offsets, (v.n_games + 1,), "<i8", None), device="cuda").cpu().numpy().astype(np.uint64)
    text = torch.as_tensor(_CudaArray(v.text, (int(v.bytes),), "|u1", None), device="cuda").cpu().numpy().tobytes() if v.bytes else b""
    return text, offs


def _check_all_paths(env, cur, seat):
    want, woffs = _host(env, cur, seat)
    c0 = cur.copy()
    text, offs = env.drain_text(seat=seat, cursor=cur, peek=True)
    assert (cur == c0).all()
    assert text.tobytes() == want, seat
    assert (offs == woffs).all(), seat
    v = env._text_call(seat, cur, True, True)
    dtext, doffs = _device_bytes(v)
    assert dtext == want and (doffs == woffs).all(), seat
    return want


@pytest.mark.parametrize("mode", [0, 2, 3, 5])
def test_device_text_equals_the_host_formatter_for_every_seat(mode):
    n, npl = 192, 3 if mode >= 3 else 4
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=101 + mode, event_ring=1024)
    env.reset()
    env._log_cursor()
    restarts = 0
    for k in (150, 250, 500):
        env.step_random(7, k, auto_reset=True)
        cur = env._cursor.copy()
        whole = None
        for seat in range(-1, npl + 1):
            t = _check_all_paths(env, cur, seat)
            if seat == -1:
                whole = t
        restarts += whole.count(b'"type":"start_game"')
        env.drain_text()
    assert restarts > n   # the windows crossed auto-reset restarts (n start_game records open the first window)
    assert int(env.events_lost().sum()) == 0
    env.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_device_text_equals_the_oracle(mode):
    from oracle import oracle

    n, seed, pseed, steps = 64, 41 + mode, 13, 220
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, event_ring=4096)
    env.reset()
    env.step_random(pseed, steps, auto_reset=False)
    logs = env.drain_text(cursor=env.log_positions()[0].copy(), peek=True, split=True)
    for g in (0, 7, n - 1):
        o = oracle.Game(game_mode=mode, seed=game_seed(seed, g))
        o.reset()
        for _ in range(steps):
            if o.status()[2]:
                break
            o.step(o.random_actions(pseed, g))
        assert logs[g] == o.log(), g
    env.close()


def test_incremental_text_drains_concatenate_to_the_whole_log():
    n, pseed = 300, 5
    env = vecenv.VecRiichiEnv(n, game_mode=2, seed=9, event_ring=4096)
    env.reset()
    parts = [[] for _ in range(n)]
    for k in (1, 40, 7, 150):
        env.step_random(pseed, k, auto_reset=False)
        t = []
        for g, chunk in enumerate(env.drain_text(timings=t, split=True)):
            parts[g] += chunk
        assert len(t) == 3 and t[2] >= t[0]
    assert parts == env.mjai_logs()
    text, offs = env.drain_text()
    assert text.size == 0 and int(offs[-1]) == 0        # nothing new
    env.close()


def _twins(n, mode, seed, ring):
    envs = []
    for _ in range(2):
        e = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, event_ring=ring)
        e.reset()
        e._log_cursor()
        envs.append(e)
    return envs


@pytest.mark.parametrize("mode", [2, 5])
def test_cursors_and_losses_follow_drain_logs(mode):
    """one environment drains with drain_text, its twin (same seeds, same steps) with drain_logs: after every drain the texts, the
    cursors and the loss counters agree - through auto-reset restarts, late drains of a lapped ring, and windows starting in a triple"""
    a, b = _twins(512, mode, 17, 64)
    lapped_in_triple = False

    def tehai_heads():
        ev, eoffs = a.drain_events(cursor=a._cursor.copy(), peek=True)
        heads = eoffs[:-1][eoffs[:-1] < eoffs[1:]]
        return bool((ev[heads, 0] == abi.EV_TEHAI).any())

    for k in (30, 400, 12, 250):
        a.step_random(3, k, auto_reset=True)
        b.step_random(3, k, auto_reset=True)
        if k > 64:   # lapped: go on one step at a time until some game's window starts inside a start_kyoku triple
            for _ in range(300):
                if tehai_heads():
                    break
                a.step_random(3, 1, auto_reset=True)
                b.step_random(3, 1, auto_reset=True)
        lapped_in_triple |= tehai_heads()
        # PEEK changes nothing
        c0, l0, p0 = a._cursor.copy(), a.events_lost().copy(), a.log_positions()
        a.drain_text(peek=True)
        a._text_call(-1, a._cursor, True, True)
        assert (a._cursor == c0).all() and (a.events_lost() == l0).all()
        assert all((x == y).all() for x, y in zip(a.log_positions(), p0))
        text, offs = a.drain_text()
        buf, toffs = b.drain_logs(raw=True)
        assert text.tobytes() == bytes(buf[: int(toffs[-1])]) and (offs == toffs).all()
        assert (a._cursor == b._cursor).all()
        assert (a.events_lost() == b.events_lost()).all()
        assert a.last_drain_events == b.last_drain_events
    assert int(a.events_lost().sum()) > 0
    assert lapped_in_triple
    a.close()
    b.close()


def test_illegal_action_ryukyoku_text():
    n, seed, pseed = 64, 4242, 99
    env = vecenv.VecRiichiEnv(n, game_mode=2, seed=seed, event_ring=8192)
    env.reset()
    base = env.log_positions()[0].copy()
    rng = np.random.default_rng(seed)
    for _ in range(700):
        acts = env.random_actions(pseed)
        _, _, done = env.status()
        for g in range(n):
            if done[g] or rng.random() > 0.02:
                continue
            acts[g, int(rng.integers(4))] = abi.pack_action(abi.DISCARD, int(rng.integers(136)))
        env.step(acts)
    want, _ = _host(env, base)
    assert b"Error: Illegal Action by Player" in want
    _check_all_paths(env, base, -1)
    _check_all_paths(env, base, 2)
    env.close()


def _random_records(rng, n_games, big):
    sizes = rng.integers(0, 220, n_games)
    sizes[5] = 0
    sizes[big] = 5000
    total = int(sizes.sum())
    ev = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    r = rng.random(total)
    t = rng.integers(1, 18, total).astype(np.uint8)          # 1 .. 17: formatted types
    t[r < 0.08] = 2                                          # START_KYOKU (a head when two TEHAI follow)
    t[(r >= 0.08) & (r < 0.10)] = 18                         # stray TEHAI
    t[(r >= 0.10) & (r < 0.1008)] = rng.integers(19, 256)    # unknown: the log stops
    t[(r >= 0.1008) & (r < 0.1010)] = 0
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    lo, hi = int(offs[big]), int(offs[big + 1])
    t[lo:hi] = rng.integers(3, 18, hi - lo)                  # the long game never stops
    heads = np.nonzero(t == 2)[0]
    heads = heads[rng.random(heads.size) < 0.95]
    for d in (1, 2):
        idx = heads + d
        t[idx[idx < total]] = 18
    ev[:, 0] = t
    ev[:, 31] = np.where(rng.random(total) < 0.9, rng.integers(3, 5, total), ev[:, 31]).astype(np.uint8)
    return ev, offs


def test_format_events_device_fuzz_equals_the_host_formatter():
    import torch

    env = vecenv.VecRiichiEnv(64, game_mode=2, seed=1, event_ring=64)
    L = env.L
    rng = np.random.default_rng(2026)
    n_games, big = 1001, 17                                  # not a multiple of 4 or 64; game 5 holds no record
    ev, offs = _random_records(rng, n_games, big)
    assert len(ev) >= 100_000
    d_ev = torch.from_numpy(ev).cuda()
    d_offs = torch.from_numpy(offs.view(np.int32)).cuda()
    torch.cuda.synchronize()
    for seat in (-1, 0, 3, 5):
        toffs = np.zeros(n_games + 1, np.uint64)
        need = C.c_uint64()
        L.rmj_format_events(ev.ctypes.data, offs.ctypes.data, n_games, seat, None, 0, toffs.ctypes.data, C.byref(need))
        buf = np.zeros(max(int(need.value), 1), np.uint8)
        vecenv._chk(L.rmj_format_events(ev.ctypes.data, offs.ctypes.data, n_games, seat, buf.ctypes.data, int(need.value), toffs.ctypes.data,
                                        C.byref(need)))
        want = buf[: int(need.value)].tobytes()
        assert int(toffs[big + 1] - toffs[big]) > 64 * 1024 and toffs[5] == toffs[6]
        v = env.format_events_device(d_ev.data_ptr(), d_offs.data_ptr(), n_games, seat=seat)
        assert v.n_events == len(ev) and v.n_games == n_games
        text, hoffs = env._host_text(v)
        assert text.tobytes() == want and (hoffs == toffs).all(), seat
        dtext, doffs = _device_bytes(env.format_events_device(d_ev.data_ptr(), d_offs.data_ptr(), n_games, seat=seat, on_device=True))
        assert dtext == want and (doffs == toffs).all(), seat
    # no games at all
    v = env.format_events_device(d_ev.data_ptr(), d_offs.data_ptr(), 0)
    assert v.bytes == 0 and v.n_games == 0 and env._host_text(v)[1].tolist() == [0]
    env.close()


def test_torch_view_is_readable_on_the_current_stream():
    import torch

    from riichienv_amd.torch_env import TorchVecEnv

    tenv = TorchVecEnv(256, game_mode=2, seed=5, skip_mjai_logging=False, event_ring=1024)
    base = tenv.env.log_positions()[0].copy()
    tenv.env.step_random(9, 120, auto_reset=True)
    text, offs = tenv.drain_text(cursor=base.copy(), peek=True)
    assert text.dtype == torch.uint8 and offs.dtype == torch.int64 and text.is_cuda and offs.is_cuda
    nl = int((text == 10).sum())                              # read on torch's current stream right after the call
    host = text.cpu().numpy().tobytes()
    want, woffs = _host(tenv.env, base)
    assert host == want and nl == want.count(b"\n")
    assert (offs.cpu().numpy().astype(np.uint64) == woffs).all()
    tenv.env.close()


def test_full_size_drain_digest():
    n = 65536
    env = vecenv.VecRiichiEnv(n, game_mode=2, seed=0, rule_bits=abi.RULE_TENHOU, event_ring=512)
    env.reset()
    env._log_cursor()
    env.step_random(0xC0FFEE, 100, auto_reset=True)
    cur = env._cursor.copy()
    want, woffs = _host(env, cur)
    text, offs = env.drain_text(cursor=cur, peek=True)
    assert hashlib.sha256(text.tobytes()).hexdigest() == hashlib.sha256(want).hexdigest()
    assert (offs == woffs).all()
    dtext, doffs = _device_bytes(env._text_call(-1, cur, True, True))
    assert hashlib.sha256(dtext).hexdigest() == hashlib.sha256(want).hexdigest() and (doffs == woffs).all()
    env.close()
