"""The pools of the C boundary's host code as their `*_views` show them (csrc/rmj_api.hip: rmj_ppo_create, rmj_logreplay_create,
rmj_logcheck_create, laid out by rmjh::DevLayout): on one 4P and one 3P handle of 5 games (no multiple of the 4 slots per block) a PPO
collector of capacity 7, a log sample builder of capacity 7 with and without RMJ_LOGREPLAY_HIDDEN, and a checker with
RMJ_LOGCHECK_GUARDS at 1 and 5 slots.  Every exposed pointer lies a multiple of 256 bytes behind the first, the pointers ascend in the
pool's declared order, and no two arrays overlap at their documented sizes.  Each object is then run end to end, destroyed, made again
and run again from the same state of the handle: the second run's outputs equal the first's byte for byte."""
import ctypes as C

import numpy as np
import pytest

from riichienv_amd import abi
from tests import log_check_ref

pytestmark = pytest.mark.gpu
N, CAP = 5, 7

# the exposed arrays in the order their pool declares them: (field of the views struct, bytes) given the sizes in `d`
PPO_ORDER = [("features", lambda d: d["cap"] * d["stride"] * 4), ("action", lambda d: d["cap"] * 4), ("value", lambda d: d["cap"] * 4),
             ("log_prob", lambda d: d["cap"] * 4), ("advantage", lambda d: d["cap"] * 4), ("ret", lambda d: d["cap"] * 4), ("game", lambda d: d["cap"] * 4),
             ("serial", lambda d: d["cap"] * 4), ("t", lambda d: d["cap"] * 4), ("prev", lambda d: d["cap"] * 4), ("seg_len", lambda d: d["cap"] * 4),
             ("seg_reward", lambda d: d["cap"] * 4), ("open_len", lambda d: d["n"] * 4), ("counters", lambda d: 5 * 4), ("mask", lambda d: d["cap"] * d["A"]),
             ("valid", lambda d: d["cap"])]
LOG_ORDER = [("features", lambda d: d["cap"] * d["stride"] * 4), ("packed", lambda d: d["cap"] * 8), ("ret64", lambda d: d["cap"] * 8),
             ("action", lambda d: d["cap"] * 4), ("log", lambda d: d["cap"] * 4), ("kyoku", lambda d: d["cap"] * 4), ("seat", lambda d: d["cap"] * 4),
             ("t", lambda d: d["cap"] * 4), ("ret", lambda d: d["cap"] * 4), ("rank", lambda d: d["cap"] * 4), ("traj_len", lambda d: d["K"] * 16),
             ("counters", lambda d: 6 * 4), ("mask", lambda d: d["cap"] * d["A"]), ("log_status", lambda d: d["M"]), ("traj_broken", lambda d: d["K"] * 4)]
CHECK_ORDER = [("code", lambda d: d["M"]), ("seat", lambda d: d["M"]), ("kyoku", lambda d: d["M"] * 4), ("event", lambda d: d["M"] * 4),
               ("detail", lambda d: d["M"] * 4), ("counts", lambda d: abi.LOGCHECK_COUNTERS * 4)]


class Handle:
    """the handle of one game mode, a copy of its first state, and the log set the replays read"""

    def __init__(self, mode):
        import torch

        from riichienv_amd import vecenv
        from riichienv_amd.logset import LogSet
        from riichienv_amd.torch_env import TorchVecEnv

        self.torch, self.mode, self.np = torch, mode, 3 if mode >= 3 else 4
        self.tenv = TorchVecEnv(N, game_mode=mode, seed=31, features="base")
        self.env, self.L, self.chk = self.tenv.env, self.tenv.env.L, vecenv._chk
        self.first = self.env.clone()
        self.set = LogSet.from_logs(log_check_ref.oracle_logs(mode, 16)[:6], num_players=self.np)
        assert self.set.M == 6 and self.set.device_index == 0
        self.A = abi.ACTION_SPACE_3P if mode >= 3 else abi.ACTION_SPACE_4P
        self.feat = self.tenv.channels * self.tenv.width

    def restore(self):
        """the games as they were when the handle was made, the round tracker's baseline taken there"""
        self.env.copy_games(np.arange(N), self.first, np.arange(N))
        self.chk(self.L.rmj_round_track_reset(self.env.h))

    def close(self):
        self.set.close()
        self.first.close()
        self.tenv.env.close()

    def bytes_at(self, ptr, size):
        return abi.device_tensor(self.torch, self, self.tenv.device, ptr, (size,), "|u1").cpu().numpy().tobytes() if size else b""


@pytest.fixture(scope="module", params=[2, 5], ids=["mode2", "mode5"])
def handle(request):
    """one handle per game mode for the module's tests, closed (with its copy and its log set) when they are done"""
    H = Handle(request.param)
    yield H
    H.close()


def _fields(views, order, d):
    return [(k, getattr(views, k), size(d)) for k, size in order]


def _assert_layout(fields, tag):
    first = fields[0][1]
    for i, (k, ptr, size) in enumerate(fields):
        assert ptr, (tag, k)
        assert (ptr - first) % 256 == 0, (tag, k, ptr - first)
        if i + 1 < len(fields):
            assert ptr + size <= fields[i + 1][1], (tag, k, "reaches", fields[i + 1][0], ptr - first, size, fields[i + 1][1] - first)


def _dump(H, fields, rows=None):
    """the arrays' bytes; feature rows: the `rows` that were filled, without the floats that pad a row"""
    out = {}
    for k, ptr, size in fields:
        if k == "features":
            stride = size // (4 * CAP)
            a = np.frombuffer(H.bytes_at(ptr, size), np.uint8).reshape(CAP, stride * 4)
            out[k] = a[:CAP if rows is None else rows, : H.feat * 4].tobytes()
        else:
            out[k] = H.bytes_at(ptr, size)
    return out


class Models:
    """policy(obs) = (logits, values), baseline(obs) = logits from one seeded device generator (what is drawn depends on the rows only)"""

    def __init__(self, H):
        self.t, self.A, self.dev = H.torch, H.A, H.tenv.device
        self.gen = H.torch.Generator(device=self.dev).manual_seed(99)

    def policy(self, obs):
        k = obs.shape[0]
        return self.t.randn((k, self.A), generator=self.gen, device=self.dev) * 3.0, self.t.randn((k,), generator=self.gen, device=self.dev)

    def baseline(self, obs):
        return self.t.round(self.t.randn((obs.shape[0], self.A), generator=self.gen, device=self.dev) * 2.0)


def _ppo_once(H):
    from riichienv_amd.ppo import PPOCollector

    H.restore()
    hero = H.torch.tensor([g % H.np for g in range(N)], dtype=H.torch.uint8)
    col = PPOCollector(H.tenv, CAP, hero=hero, seed=3)
    try:
        v = abi.PpoViews()
        H.chk(H.L.rmj_ppo_views(col.h, C.byref(v)))
        assert (v.capacity, v.action_space) == (CAP, H.A)
        fields = _fields(v, PPO_ORDER, dict(cap=CAP, stride=v.row_stride, A=H.A, n=N))
        _assert_layout(fields, "ppo")
        m = Models(H)
        col.collect(m.policy, m.baseline, 40)
        counts = col.counts()
        assert counts["fill"] == CAP and counts["overflowed"] > 0, counts   # (the pool is far too small on purpose: its last slot is used)
        out = _dump(H, fields, counts["fill"])
        out["counts"] = repr(sorted(counts.items())).encode()
        out.update({"emit_" + k: x.cpu().numpy().tobytes() for k, x in col.transitions().items()})
        return [(k, p - fields[0][1]) for k, p, _ in fields], out
    finally:
        col.close()


def _builder_once(H, hidden):
    torch, L, s = H.torch, H.L, H.set
    H.restore()
    flags = abi.LOGREPLAY_INCLUDE_PASS | (abi.LOGREPLAY_HIDDEN if hidden else 0)
    cfg = abi.LogReplayConfig(abi.FEATURES["base"], CAP, flags, 0, 0.99, None)
    h, left = C.c_void_p(), C.c_uint32()
    H.chk(L.rmj_logreplay_create(H.env.h, s.handle, C.byref(cfg), C.byref(h)))
    try:
        v = abi.LogReplayViews()
        H.chk(L.rmj_logreplay_views(h, C.byref(v)))
        K = int(s.n_kyokus)
        assert (v.capacity, v.action_space) == (CAP, H.A) and v.steps > 0 and K > 0
        fields = _fields(v, LOG_ORDER, dict(cap=CAP, stride=v.row_stride, A=H.A, M=s.M, K=K))
        _assert_layout(fields, "builder")
        H.chk(L.rmj_logreplay_run_device(h, 0, C.byref(left)))
        assert left.value == 0
        reward = torch.as_tensor((s.end_scores.astype(np.float64) - s.start_scores.astype(np.float64)) * 1e-3).reshape(K, 4).to(H.tenv.device).contiguous()
        ends = torch.as_tensor(s.end_scores, dtype=torch.int32).reshape(K, 4).to(H.tenv.device).contiguous()
        H.chk(L.rmj_logreplay_finalize_device(h, C.c_void_p(reward.data_ptr()), C.c_void_p(ends.data_ptr())))
        c = abi.LogReplayCounts()
        H.chk(L.rmj_logreplay_counts(h, C.byref(c)))
        counts = {k: int(getattr(c, k)) for k, _ in abi.LogReplayCounts._fields_}
        assert counts["fill"] == CAP and counts["overflowed"] > 0 and counts["failed_logs"] == 0 and counts["complete_logs"] == s.M, counts
        out = _dump(H, fields)
        out["counts"] = repr(sorted(counts.items())).encode()
        dev = H.tenv.device
        rows = {"features": torch.zeros((CAP, H.feat), dtype=torch.float32, device=dev), "mask": torch.zeros((CAP, H.A), dtype=torch.uint8, device=dev),
                "action": torch.zeros(CAP, dtype=torch.int64, device=dev), "packed": torch.zeros(CAP, dtype=torch.int64, device=dev),
                "ret": torch.zeros(CAP, dtype=torch.float32, device=dev), "ret64": torch.zeros(CAP, dtype=torch.float64, device=dev),
                "rank": torch.zeros(CAP, dtype=torch.int64, device=dev)}
        rows.update({k: torch.zeros(CAP, dtype=torch.int32, device=dev) for k in ("log", "kyoku", "seat", "t")})
        cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        b = abi.LogBatch(*[rows[k].data_ptr() for k in ("features", "mask", "action", "packed", "ret", "ret64", "rank", "log", "kyoku", "seat", "t")],
                         cnt.data_ptr(), CAP, 0)
        H.chk(L.rmj_logreplay_emit_device(h, C.byref(b)))
        hv = abi.LogHiddenViews()
        H.chk(L.rmj_logreplay_hidden_views(h, C.byref(hv)))
        assert bool(hv.records) == hidden
        if hidden:
            assert hv.capacity == CAP
            out["hidden"] = H.bytes_at(hv.records, CAP * hv.record_bytes)
            hid = {"opp_hand": torch.zeros((CAP, 3, 34), dtype=torch.uint8, device=dev), "opp_shanten": torch.zeros((CAP, 3), dtype=torch.int8, device=dev),
                   "opp_waits": torch.zeros((CAP, 3), dtype=torch.int64, device=dev), "opp_flags": torch.zeros((CAP, 3), dtype=torch.uint8, device=dev),
                   "event": torch.zeros(CAP, dtype=torch.int32, device=dev)}
            hb = abi.LogHiddenBatch(*[hid[k].data_ptr() for k in ("opp_hand", "opp_shanten", "opp_waits", "opp_flags", "event")], CAP, 0)
            H.chk(L.rmj_logreplay_emit_hidden_device(h, C.byref(hb)))
            rows.update(hid)
        H.env.sync()
        out["emit_count"] = cnt.cpu().numpy().tobytes()
        out.update({"emit_" + k: x.cpu().numpy().tobytes() for k, x in rows.items()})
        return [(k, p - fields[0][1]) for k, p, _ in fields], out
    finally:
        L.rmj_logreplay_destroy(h)


def _checker_once(H, n_slots):
    L, s = H.L, H.set
    H.restore()
    h, left, v = C.c_void_p(), C.c_uint32(), abi.LogCheckViews()
    H.chk(L.rmj_logcheck_create(H.env.h, s.handle, n_slots, abi.LOGCHECK_GUARDS, C.byref(h)))
    try:
        H.chk(L.rmj_logcheck_views(h, C.byref(v)))
        assert v.n_logs == s.M and v.steps > 0
        fields = _fields(v, CHECK_ORDER, dict(M=s.M))
        _assert_layout(fields, "checker")
        H.chk(L.rmj_logcheck_run_device(h, 0, C.byref(left)))
        H.env.sync()
        assert left.value == 0
        out = _dump(H, fields)
        assert out["code"] == bytes(s.M), list(out["code"])   # (complete games written by the oracle: every log is OK)
        out["steps"] = repr(int(v.steps)).encode()
        return [(k, p - fields[0][1]) for k, p, _ in fields], out
    finally:
        L.rmj_logcheck_destroy(h)


OBJECTS = {"ppo": _ppo_once, "builder": lambda H: _builder_once(H, False), "builder_hidden": lambda H: _builder_once(H, True),
           "checker_1": lambda H: _checker_once(H, 1), "checker_5": lambda H: _checker_once(H, 5)}


@pytest.mark.parametrize("what", sorted(OBJECTS))
def test_pool_layout_and_a_second_object_repeats_the_first(handle, what):
    H, mode = handle, handle.mode
    offs_a, a = OBJECTS[what](H)
    offs_b, b = OBJECTS[what](H)
    assert offs_a == offs_b
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], (what, mode, k, len(a[k]))
    assert any(any(x) for x in a.values())
