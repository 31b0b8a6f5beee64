"""What the row targets share, on the GPU: every host entry (rmj_hidden_targets, rmj_danger_targets, rmj_discard_table,
rmj_determinize_ex) against its `_device` form on the same state, a sample builder that keeps all three extra records against the
builders that keep one or none, and the refusals of the emit entries.  Each target's own values are held to its restatement in the
target's own test file; here only the shared wiring is under test.  64 games per mode after 40 steps of the device policy that plays
to win."""
import ctypes as C
import functools

import numpy as np
import pytest

from riichienv_amd import abi

pytestmark = pytest.mark.gpu

N, STEPS = 64, 40
MODES = [2, 5]
ROWS = [0, 1, 4, 5, 257]   # the grid of a row kernel is (rows + 3) / 4 blocks, the claim kernel of determinize takes 256 rows a block
FILL = 0x5A                # what an array holds before a call: a byte no call may leave where it writes nothing


@functools.lru_cache(maxsize=None)
def _env(mode):
    """the batch (never stepped or determinized again) and one acting row (game * 4 + seat) of every game that has one"""
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(N, game_mode=mode, seed=77, share_stream=False)
    env.env.step_greedy(3, STEPS, auto_reset=False, call_rate_256=64)
    idx = env.env.legal_compact()[0].astype(np.int32)
    acting = np.array([idx[idx >> 2 == g][0] for g in sorted(set((idx >> 2).tolist()))], np.int32)
    assert acting.size > N // 2
    return env, acting


def _index(rows):
    """seat 3 of a game (absent in 3P), an index < 0, one >= 4 n, then the seats in order"""
    return np.concatenate([[7, -1, 4 * N, 9, 130], np.arange(4 * N)]).astype(np.int32)[:rows]


def _filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


ENTRIES = {"hidden": ("rmj_hidden_targets", ()), "danger": ("rmj_danger_targets", (abi.DANGER_URA,)), "discard_table": ("rmj_discard_table", (0,))}


def _both_forms(env, target, idx, without=()):
    """({field: bytes} of the host entry, the same of the device form) over arrays that held FILL; `without`: fields passed as NULL"""
    import torch

    from riichienv_amd import vecenv

    name, flags = ENTRIES[target]
    L, h, k = env.env.L, env.env.h, len(idx)
    host = {f.name: _filled((max(k, 1),) + f.shape, f.dtype) for f in abi.ROW_TARGETS[target].fields}   # (a pointer even for no rows)
    dev = {f: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(env.device) for f, v in host.items()}
    hidx = np.concatenate([idx, [0]]).astype(np.int32)
    didx = torch.from_numpy(hidx).to(env.device)
    hb, db = abi.row_struct(target, host), abi.row_struct(target, dev)
    for f in without:
        setattr(hb, f, None)
        setattr(db, f, None)
    torch.cuda.synchronize()
    vecenv._chk(getattr(L, name)(h, hidx.ctypes.data, k, *flags, C.byref(hb)))
    vecenv._chk(getattr(L, name + "_device")(h, C.c_void_p(didx.data_ptr()), k, None, *flags, C.byref(db)))
    env.sync()
    torch.cuda.synchronize()
    return {f: v.tobytes() for f, v in host.items()}, {f: v.cpu().numpy().tobytes() for f, v in dev.items()}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("target", list(ENTRIES))
@pytest.mark.parametrize("mode", MODES)
def test_host_entry_equals_device_form(mode, target, rows):
    env, _ = _env(mode)
    host, dev = _both_forms(env, target, _index(rows))
    for f in host:
        assert host[f] == dev[f], f
        assert (host[f] == bytes([FILL]) * len(host[f])) == (rows == 0), f"{f}: no rows write nothing, any row writes something"
    if target == "discard_table":   # the optional array left out: the others as before, the array itself untouched
        h3, d3 = _both_forms(env, target, _index(rows), without=("mask",))
        for f in host:
            assert h3[f] == d3[f] == (bytes([FILL]) * len(host[f]) if f == "mask" else host[f]), f


def _determinize_forms(mode, rows, tenpai, with_hold, with_status):
    """(status or None, {game: view bytes}) of the host entry and of the device form, each on a clone of the batch"""
    import torch

    from riichienv_amd import vecenv
    from tests.parity_util import view_bytes

    env, acting = _env(mode)
    # one row per game (the host entry refuses two), seat 3 (absent in 3P) for the last of them; the rest of a long index names no game at all
    idx = np.concatenate([acting[:3], [acting[-1] | 3, -1, 4 * N], acting[3:-1], 4 * N + 1 + np.arange(rows)]).astype(np.int32)[:rows]
    hold = (np.arange(rows) % 8).astype(np.uint8)
    flags = abi.DETF_RIICHI_TENPAI if tenpai else 0
    games = sorted({int(i) >> 2 for i in idx if 0 <= i < 4 * N})
    hidx, h_hold, h_st = np.concatenate([idx, [0]]).astype(np.int32), np.concatenate([hold, [0]]).astype(np.uint8), _filled(rows + 1, np.uint8)
    d_idx, d_hold, d_st = (torch.from_numpy(a.copy()).to(env.device) for a in (hidx, h_hold, h_st))
    out = []
    for device_form in (False, True):
        w = env.env.clone()
        if device_form:
            d = abi.Determinize(21, d_hold.data_ptr() if with_hold else None, d_st.data_ptr() if with_status else None)
            torch.cuda.synchronize()
            vecenv._chk(w.L.rmj_determinize_ex_device(w.h, C.c_void_p(d_idx.data_ptr()), rows, None, C.byref(d), flags))
            w.sync()
            st = d_st.cpu().numpy()
        else:
            d = abi.Determinize(21, h_hold.ctypes.data if with_hold else None, h_st.ctypes.data if with_status else None)
            vecenv._chk(w.L.rmj_determinize_ex(w.h, hidx.ctypes.data, rows, C.byref(d), flags))
            st = h_st
        out.append((st.tobytes(), {g: view_bytes(w.peek(g)) for g in games}))
        w.close()
    before = {g: view_bytes(env.env.peek(g)) for g in games}
    return out[0], out[1], before


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("tenpai", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_determinize_host_entry_equals_device_form(mode, tenpai, rows):
    (h_st, h_views), (d_st, d_views), before = _determinize_forms(mode, rows, tenpai, True, True)
    assert h_st == d_st and h_views == d_views
    assert h_st[rows:] == bytes([FILL]) and (rows == 0) == (h_st[:rows] == bytes([FILL]) * rows)
    if rows >= 4:
        assert any(h_views[g] != before[g] for g in h_views), "no game was re-dealt"
        # without the optional arrays: every opponent re-dealt, no status written, the same worlds from both forms
        (h_st, h_views), (d_st, d_views), _ = _determinize_forms(mode, rows, tenpai, False, False)
        assert h_st == d_st == bytes([FILL]) * (rows + 1) and h_views == d_views


# ---------------------------------------------------------------- the builder: all extras at once against each alone
PLAIN = ["features", "mask", "action", "packed", "return", "return64", "rank", "log", "kyoku", "seat", "t"]
EXTRA = {"hidden": ["opp_hand", "opp_shanten", "opp_waits", "opp_flags", "event"], "danger": ["danger"], "efficiency": ["dt_shanten", "dt_accept", "dt_ukeire"]}


def _samples(b):
    return {k: v.cpu().numpy() for k, v in b.samples().items()}


@functools.lru_cache(maxsize=None)
def _built(mode, small):
    """{settings: (samples, counts)} of the builder with all three extras, each alone and none, over 8 self-played logs in 3 slots; small:
    a pool of half the samples.  The builder of all three also runs a second time after clear()."""
    from riichienv_amd.datasets import LogSampleBuilder
    from tests import log_check_ref

    logs = log_check_ref.oracle_logs(mode, 8)
    cap = _built(mode, False)[()][1]["fill"] // 2 if small else None
    out = {}
    for on in [tuple(EXTRA), *((k,) for k in EXTRA), ()]:
        b = LogSampleBuilder(logs, game_mode=mode, n_slots=3, capacity=cap, **{k: True for k in on})
        b.run()
        out[on] = (_samples(b), b.counts())
        if len(on) == 3:
            b.clear()
            assert b.counts()["fill"] == 0
            b.run()
            out["again"] = (_samples(b), b.counts())
        b.close()
    return out


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_all_extras_in_one_builder_equal_each_alone(mode, small):
    built = _built(mode, small)
    every, counts = built[tuple(EXTRA)]
    assert list(every) == PLAIN + [c for k in EXTRA for c in EXTRA[k]]
    assert counts["failed_logs"] == 0 and counts["steps_left"] == 0 and counts["complete_logs"] == 8, counts
    assert (counts["overflowed"] > 0) == small and 0 < every["action"].shape[0] <= counts["fill"], counts
    assert small or every["action"].shape[0] == counts["fill"] == counts["decisions"]
    for on, (s, cn) in built.items():
        if on == "again":
            assert list(s) == list(every)
        else:
            assert list(s) == PLAIN + [c for k in on for c in EXTRA[k]], on
        assert cn == counts, on
        rows = np.stack([every[k] for k in ("log", "kyoku", "seat", "t")], 1)
        assert np.array_equal(rows, np.stack([s[k] for k in ("log", "kyoku", "seat", "t")], 1)), f"{on}: other samples survived"
        for k in s:
            assert s[k].dtype == every[k].dtype and s[k].shape == every[k].shape and s[k].tobytes() == every[k].tobytes(), (on, k)
    assert every["danger"].any() and every["opp_hand"].any() and (every["dt_shanten"] != abi.DTAB_NONE).any()


def test_emit_refusals():
    import torch

    from riichienv_amd import vecenv
    from riichienv_amd.datasets import LogSampleBuilder
    from tests import apply_events_util as U
    from tests import log_check_ref

    L = vecenv.load_lib()
    b = LogSampleBuilder(log_check_ref.oracle_logs(2, 8)[:2], game_mode=2)
    b.run()
    buf = torch.zeros(8 * 3 * 37 * 4, dtype=torch.uint8, device=b.device)   # room for a row of any batch
    p = buf.data_ptr()
    torch.cuda.synchronize()
    for entry, batch, flag in [("rmj_logreplay_emit_hidden_device", abi.LogHiddenBatch(p, p, p, p, p, 1, 0), "RMJ_LOGREPLAY_HIDDEN"),
                               ("rmj_logreplay_emit_danger_device", abi.LogDangerBatch(p, 1, 0), "RMJ_LOGREPLAY_DANGER"),
                               ("rmj_logreplay_emit_dtable_device", abi.LogDtableBatch(p, p, p, 1, 0), "RMJ_LOGREPLAY_DTABLE")]:
        assert getattr(L, entry)(b.h, C.byref(batch)) == -1   # RMJ_ERR_ARG
        assert L.rmj_last_error() == f"{entry}: the builder was made without {flag}".encode()
        assert getattr(L, entry)(None, C.byref(batch)) == -1 and L.rmj_last_error() == b"null argument"
        assert getattr(L, entry)(b.h, None) == -1 and L.rmj_last_error() == b"null argument"
        # the flag is asked for before the arrays are
        assert getattr(L, entry)(b.h, C.byref(type(batch)())) == -1 and L.rmj_last_error().endswith(flag.encode())
    b.close()
    b = LogSampleBuilder(log_check_ref.oracle_logs(2, 8)[:2], game_mode=2, hidden=True, danger=True, efficiency=True)
    for entry, batch in [("rmj_logreplay_emit_hidden_device", abi.LogHiddenBatch(p, p, p, p, None, 1, 0)), ("rmj_logreplay_emit_danger_device", abi.LogDangerBatch(None, 1, 0)),
                         ("rmj_logreplay_emit_dtable_device", abi.LogDtableBatch(p, None, p, 1, 0))]:
        assert getattr(L, entry)(b.h, C.byref(batch)) == -1 and L.rmj_last_error() == b"null argument", entry   # rows without an array
    b.close()
    texts = {"hidden": "hidden=True over a log set made with masked_ok=True: the masked seats' tiles are unknown, so are their hands, shanten and waits",
             "danger": "danger=True over a log set made with masked_ok=True: the masked seats' tiles are unknown, so is what they would win",
             "efficiency": "efficiency=True over a log set made with masked_ok=True: the set does not tell which seats' tiles are masked, and a "
                           "masked deciding seat has no hand to tabulate"}
    for setting, text in texts.items():
        with pytest.raises(ValueError) as e:
            LogSampleBuilder([U.furiten_log(False)], game_mode=2, masked_ok=True, **{setting: True})
        assert str(e.value) == text
