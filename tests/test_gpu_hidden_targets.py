"""Hidden-hand targets (csrc/rmj_hidden.hip.h: rmj_hidden_targets_device, LogSampleBuilder(hidden=True)) against the host yardstick
tests/hidden_targets_ref.py, which computes the four fields from a StateView with the oracle's hand mathematics: the live entry against
the device's own state, the builder's rows against an oracle replay of the same logs, bit for bit and with nothing left out."""
import json
import os

import numpy as np
import pytest

from riichienv_amd import abi
from tests import apply_events_util as U
from tests import hidden_targets_ref as H
from tests import log_check_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "126_204_0_mjai.jsonl")
M2, M3 = 1 << 1, 1 << 2
HIDDEN_KEYS = H.FIELDS + ("event",)
_CACHE = {}


def _logs(mode):
    logs = list(log_check_ref.oracle_logs(mode, 16))
    if mode == 2:
        with open(GOLDEN) as f:
            logs.append([json.loads(line) for line in f if line.strip()])
    return logs


def _build(logs, mode, **kw):
    """(samples as numpy arrays, counts) of one run of the builder"""
    from riichienv_amd.datasets import LogSampleBuilder

    b = LogSampleBuilder(logs, game_mode=mode, include_pass=True, **kw)
    b.run()
    counts = b.counts()
    s = {k: v.cpu().numpy() for k, v in b.samples().items()}
    b.close()
    return s, counts


def _built(mode):
    """the builder's run with hidden=True and with hidden=False over the logs of `mode`, and the yardstick's rows of every emitted
    (log, event, seat): made once, shared, never changed"""
    if mode not in _CACHE:
        logs = _logs(mode)
        hid, hid_counts = _build(logs, mode, hidden=True)
        plain, plain_counts = _build(logs, mode, hidden=False)
        keys = {}
        for lg, ev, st in zip(hid["log"].tolist(), hid["event"].tolist(), hid["seat"].tolist()):
            keys.setdefault(lg, set()).add((ev, st))
        ref = {}
        for lg, want in keys.items():
            for (ev, st), row in H.log_targets(logs[lg], mode, keys=want).items():
                ref[lg, ev, st] = row
        _CACHE[mode] = dict(logs=logs, hid=hid, hid_counts=hid_counts, plain=plain, plain_counts=plain_counts, ref=ref)
    return _CACHE[mode]


def _against_ref(s, ref):
    """every sample of `s` equals the yardstick's row of its (log, event, seat) in all four fields"""
    ks = list(zip(s["log"].tolist(), s["event"].tolist(), s["seat"].tolist()))
    assert len(set(ks)) == len(ks), "two samples of one (log, event, seat)"
    missing = [k for k in ks if k not in ref]
    assert not missing, missing[:4]
    want = H.stack([ref[k] for k in ks])
    for f in H.FIELDS:
        bad = np.flatnonzero((s[f] != want[f]).reshape(len(ks), -1).any(axis=1))
        assert bad.size == 0, (f, bad.size, [(ks[i], s[f][i].tolist(), want[f][i].tolist()) for i in bad[:3]])


# ---------------------------------------------------------------- 1. the live entry against the device's own state
@pytest.mark.parametrize("policy", ["greedy", "random"])
@pytest.mark.parametrize("mode", [2, 5])
def test_live_entry_equals_the_yardstick_on_the_devices_state(mode, policy):
    from riichienv_amd import vecenv

    n, np_ = 32, 3 if mode >= 3 else 4     # 32 games per policy: 64 per mode
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=77 + mode, event_ring=4096)
    env.reset()
    index = np.arange(4 * n, dtype=np.int32)
    at = 0
    for stop in (40, 120, 300):
        if policy == "greedy":
            env.step_greedy(5, stop - at, auto_reset=False, call_rate_256=64)
        else:
            env.step_random(5, stop - at, auto_reset=False)
        at = stop
        got = env.hidden_targets(index)
        want = H.stack([H.targets_of_view(view, seat, np_) for view in (env.peek(g) for g in range(n)) for seat in range(4)])
        present = (got["opp_flags"] & abi.HIDDEN_PRESENT) != 0
        print(f"mode {mode} {policy} step {stop}: tenpai rows {int(((got['opp_flags'] & abi.HIDDEN_TENPAI) != 0).sum())}, "
              f"rows with melds {int(((got['opp_flags'] >> 4) > 0).sum())}, furiten {int(((got['opp_flags'] & abi.HIDDEN_FURITEN) != 0).sum())}")
        assert int(present.sum()) == n * np_ * (np_ - 1)
        for f in H.FIELDS:
            assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
            bad = np.flatnonzero((got[f] != want[f]).reshape(4 * n, -1).any(axis=1))
            assert bad.size == 0, (f, stop, bad[:4].tolist(), got[f][bad[:2]].tolist(), want[f][bad[:2]].tolist())
    env.close()


# ---------------------------------------------------------------- 2. missed-win furiten
def test_missed_win_furiten_of_both_kinds():
    from riichienv_amd import vecenv

    logs = [U.furiten_log(False), U.furiten_log(True)]
    ends = [next(i for i, e in enumerate(l) if e["type"] == "ryukyoku") for l in logs]
    env = vecenv.VecRiichiEnv(2, game_mode=2, seed=1)
    env.reset()
    for i in range(max(ends)):
        env.apply_events([l[i] if i < end else None for l, end in zip(logs, ends)], replay=True)
    got = env.hidden_targets(np.arange(8, dtype=np.int32))
    for g, riichi in enumerate((False, True)):
        want = abi.HIDDEN_PRESENT | abi.HIDDEN_TENPAI | abi.HIDDEN_FURITEN | (abi.HIDDEN_RIICHI if riichi else 0)
        for hero, r in ((0, 0), (3, 1), (2, 2)):   # seat 1 as shimocha, toimen, kamicha
            row = g * 4 + hero
            assert int(got["opp_flags"][row, r]) == want, (g, hero, int(got["opp_flags"][row, r]))
            assert int(got["opp_waits"][row, r]) == M2 | M3 and int(got["opp_shanten"][row, r]) == 0
        view = env.peek(g)
        for hero in range(4):
            ref = H.targets_of_view(view, hero, 4)
            assert all((got[f][g * 4 + hero] == ref[f]).all() for f in H.FIELDS), (g, hero)
    env.close()


# ---------------------------------------------------------------- 3. the builder against the oracle replay
def _history(log, n):
    """{event index: (concealed kans, kitas, discarded types as a bit mask) per seat, of the kyoku so far} before every event"""
    out, ankan, kita, disc = {}, [0] * 4, [0] * 4, [0] * 4
    for i, e in enumerate(log):
        out[i] = (tuple(ankan), tuple(kita), tuple(disc))
        ty = e["type"]
        if ty == "start_kyoku":
            ankan, kita, disc = [0] * 4, [0] * 4, [0] * 4
        elif ty == "ankan":
            ankan[e["actor"]] += 1
        elif ty == "kita":
            kita[e["actor"]] += 1
        elif ty == "dahai":
            disc[e["actor"]] |= 1 << (log_check_ref.tid(e["pai"]) >> 2)
    return out


@pytest.mark.parametrize("mode", [2, 5])
def test_builder_rows_equal_the_oracle_replay(mode):
    c = _built(mode)
    s, np_ = c["hid"], 3 if mode >= 3 else 4
    cn = c["hid_counts"]
    assert cn["failed_logs"] == 0 and cn["overflowed"] == 0 and cn["steps_left"] == 0 and cn["complete_logs"] == len(c["logs"]), cn
    assert s["action"].shape[0] == cn["fill"] == cn["decisions"] > 0, "no sample may be left out"
    _against_ref(s, c["ref"])
    # what the compared opponent rows cover
    flags, melds = s["opp_flags"], s["opp_flags"] >> 4
    present = (flags & abi.HIDDEN_PRESENT) != 0
    assert (present.sum(axis=1) == np_ - 1).all()
    assert ((s["opp_hand"].sum(axis=-1).astype(np.int64) + 3 * melds)[present] == 13).all(), "an opponent of a deciding seat holds 13 tiles counting melds"
    hist = {lg: _history(log, np_) for lg, log in enumerate(c["logs"])}
    cover = {"ankan": 0, "kita": 0, "furiten_own_closed": 0}
    for i, (lg, ev, st) in enumerate(zip(s["log"].tolist(), s["event"].tolist(), s["seat"].tolist())):
        ankan, kita, disc = hist[lg][ev]
        for r in range(np_ - 1):
            o = (st + 1 + r) % np_
            cover["ankan"] += ankan[o] > 0
            cover["kita"] += kita[o] > 0
            cover["furiten_own_closed"] += bool(flags[i, r] & abi.HIDDEN_FURITEN) and melds[i, r] == 0 and (int(s["opp_waits"][i, r]) & disc[o]) != 0
    cover["melds"] = sorted(set(melds[present].tolist()))
    cover["riichi"] = int(((flags & abi.HIDDEN_RIICHI) != 0).sum())
    cover["shanten0"] = int(((s["opp_shanten"] == 0) & present).sum())
    cover["rows"] = int(present.sum())
    print(f"mode {mode}: {s['action'].shape[0]} samples, coverage {cover}")
    assert set(cover["melds"]) >= ({0, 1, 2, 3, 4} if mode == 2 else {0, 1, 2, 3}), cover
    assert cover["ankan"] > 0 and cover["riichi"] > 0 and cover["shanten0"] > 0 and cover["furiten_own_closed"] > 0, cover
    if mode == 5:
        assert cover["kita"] > 0, cover


# ---------------------------------------------------------------- 4. nothing else moves
@pytest.mark.parametrize("mode", [2, 5])
def test_hidden_changes_no_other_column(mode):
    c = _built(mode)
    today = ["features", "mask", "action", "packed", "return", "return64", "rank", "log", "kyoku", "seat", "t"]
    assert list(c["plain"]) == today
    assert list(c["hid"]) == today + list(HIDDEN_KEYS)
    assert c["plain_counts"] == c["hid_counts"]
    for k in today:
        assert c["plain"][k].dtype == c["hid"][k].dtype and c["plain"][k].tobytes() == c["hid"][k].tobytes(), k
    assert c["hid"]["opp_hand"].dtype == np.uint8 and c["hid"]["opp_shanten"].dtype == np.int8 and c["hid"]["opp_waits"].dtype == np.int64
    assert c["hid"]["opp_flags"].dtype == np.uint8 and c["hid"]["event"].dtype == np.int32


# ---------------------------------------------------------------- 5. consistency
@pytest.mark.parametrize("mode", [2, 5])
def test_two_samples_of_one_moment_agree_on_a_seat(mode):
    s, np_ = _built(mode)["hid"], 3 if mode >= 3 else 4
    seen, shared = {}, 0
    for i, (lg, ev, st) in enumerate(zip(s["log"].tolist(), s["event"].tolist(), s["seat"].tolist())):
        for r in range(np_ - 1):
            k = (lg, ev, (st + 1 + r) % np_)
            v = (s["opp_hand"][i, r].tobytes(), int(s["opp_shanten"][i, r]), int(s["opp_waits"][i, r]), int(s["opp_flags"][i, r]))
            if k in seen:
                shared += 1
                assert seen[k] == v, (k, seen[k], v)
            seen[k] = v
    assert shared > 0, "no two samples at one (log, event): nothing was compared"


# ---------------------------------------------------------------- 6. edges
def test_a_pool_too_small_keeps_the_columns_in_step():
    c = _built(2)
    logs = c["logs"][:4]
    s, counts = _build(logs, 2, hidden=True, capacity=600)
    _, plain_counts = _build(logs, 2, hidden=False, capacity=600)
    assert counts["overflowed"] > 0 and counts == plain_counts
    k = s["action"].shape[0]
    assert 0 < k <= 600 and all(s[f].shape[0] == k for f in HIDDEN_KEYS)
    _against_ref(s, c["ref"])      # (the logs are the first four of the shared run: the same log numbers)


@pytest.mark.parametrize("mode", [2, 5])
def test_slots_that_replay_several_logs(mode):
    c = _built(mode)
    s, counts = _build(c["logs"], mode, hidden=True, n_slots=3)
    assert counts["overflowed"] == 0 and counts["failed_logs"] == 0 and s["action"].shape[0] == c["hid"]["action"].shape[0]
    _against_ref(s, c["ref"])


def test_hidden_over_a_masked_set_is_refused():
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.logset import LogSet

    log = U.furiten_log(False)
    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder([log], game_mode=2, masked_ok=True, hidden=True)
    text = "\n".join(json.dumps(e) for e in log_check_ref.oracle_logs(2, 16)[0]).encode()
    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder.from_text([text], game_mode=2, masked_ok=True, hidden=True)
    ls = LogSet.from_logs([log], 4, masked_ok=True)
    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder.from_logset(ls, game_mode=2, hidden=True)
    LogSampleBuilder.from_logset(ls, game_mode=2, hidden=False).close()   # the plain builder takes it as before
    ls.close()


def test_an_empty_log_set():
    from riichienv_amd.datasets import LogSampleBuilder

    b = LogSampleBuilder([], game_mode=2, hidden=True)
    assert b.run() == 0
    s = b.samples()
    assert s["opp_hand"].shape == (0, 3, 34) and s["opp_waits"].shape == (0, 3) and s["event"].shape == (0,) and s["action"].shape == (0,)
    b.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_hidden_compact_stops_at_the_device_count(mode):
    import torch

    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(67, game_mode=mode, seed=5)      # 67: the last block of four rows is not full
    env.env.step_random(3, 90, auto_reset=True)
    _, index = env.obs_compact()
    k = int(index.shape[0])
    assert k > 32
    full = env.hidden_compact(index)
    host = env.env.hidden_targets(index.cpu().numpy())
    for f in H.FIELDS:
        assert (full[f].cpu().numpy() == host[f]).all(), f
    assert int(((full["opp_flags"] & abi.HIDDEN_PRESENT) != 0).sum()) == k * (2 if mode >= 3 else 3)
    cut = k // 2 + 1
    out = {f: torch.full_like(v, 0x5A) for f, v in full.items()}
    count = torch.tensor([cut], dtype=torch.int32, device=index.device)
    assert env.hidden_compact(index, count=count, out=out) is out
    torch.cuda.synchronize()
    for f in H.FIELDS:
        assert (out[f][:cut] == full[f][:cut]).all(), f
        assert (out[f][cut:] == 0x5A).all(), f"{f}: a row behind the count was written"
    env.env.close()


def test_a_bad_index_gives_an_absent_row():
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(4, game_mode=2, seed=2)
    env.reset()
    got = env.hidden_targets(np.array([0, 16, -1, 1 << 30, 15], dtype=np.int32))
    assert got["opp_flags"][0].all() and got["opp_flags"][4].all()
    for f in H.FIELDS:
        assert not got[f][1:4].any(), f
    env.close()


# ---------------------------------------------------------------- 7. the example
def test_the_example_runs():
    import importlib.util

    spec = importlib.util.spec_from_file_location("hidden_targets_example", os.path.join(ROOT, "examples", "hidden_targets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(games=8, steps=20000)
    assert out["logs"] == 8 and out["samples"] > 1000 and out["overflowed"] == 0
    assert len(out["tenpai_rate"]) == 3 and all(0.0 < x < 1.0 for x in out["tenpai_rate"]) and all(0.0 < x < 6.0 for x in out["mean_shanten"])
    assert 0.0 <= out["dealt_into_waits"] < 0.5 and out["discards"] > 0
