"""Deal-in danger targets (csrc/rmj_danger.hip.h: rmj_danger_targets_device, LogSampleBuilder(danger=True)) against the host yardstick
tests/danger_ref.py, which restates the definition with the oracle's evaluator, and against the device's own settlement: the live entry
on the device's state, a discard and a Ron stepped in a clone, the builder's rows against an oracle replay of the same logs."""
import json
import os

import numpy as np
import pytest

from riichienv_amd import abi
from tests import danger_ref as D
from tests import hidden_targets_ref as H
from tests import log_check_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "126_204_0_mjai.jsonl")
TODAY = ["features", "mask", "action", "packed", "return", "return64", "rank", "log", "kyoku", "seat", "t"]
HIDDEN_KEYS = list(H.FIELDS) + ["event"]
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
    """the builder's runs over the logs of `mode` - plain, danger, hidden, hidden + danger - and the yardstick's row of every emitted
    (log, event, seat): made once, shared, never changed"""
    if mode not in _CACHE:
        logs = _logs(mode)
        c = dict(logs=logs)
        for name, kw in (("plain", {}), ("danger", dict(danger=True)), ("hidden", dict(hidden=True)), ("both", dict(hidden=True, danger=True))):
            c[name], c[name + "_counts"] = _build(logs, mode, **kw)
        keys = {}
        for lg, ev, st in zip(c["both"]["log"].tolist(), c["both"]["event"].tolist(), c["both"]["seat"].tolist()):
            keys.setdefault(lg, set()).add((ev, st))
        ref = {}
        for lg, want in keys.items():
            for (ev, st), row in D.log_danger(logs[lg], mode, keys=want).items():
                ref[lg, ev, st] = row
        c["ref"] = ref
        _CACHE[mode] = c
    return _CACHE[mode]


def _against_ref(s, ref):
    """every sample of `s` (a run with hidden=True: it has the event column) equals the yardstick's row of its (log, event, seat)"""
    ks = list(zip(s["log"].tolist(), s["event"].tolist(), s["seat"].tolist()))
    assert len(set(ks)) == len(ks), "two samples of one (log, event, seat)"
    missing = [k for k in ks if k not in ref]
    assert not missing, missing[:4]
    want = np.stack([ref[k] for k in ks]) if ks else np.zeros((0, 3, 37), np.int32)
    assert s["danger"].dtype == np.int32 and s["danger"].shape == want.shape
    bad = np.flatnonzero((s["danger"] != want).reshape(len(ks), -1).any(axis=1))
    assert bad.size == 0, (bad.size, [(ks[i], np.argwhere(s["danger"][i] != want[i]).tolist(), s["danger"][i][s["danger"][i] != want[i]].tolist(),
                                       want[i][s["danger"][i] != want[i]].tolist()) for i in bad[:3]])


# ---------------------------------------------------------------- 1. the live entry against the yardstick
CLASSES = ("nonzero", "riichi", "open_hand", "furiten_zeroed", "no_yaku_zeroed", "red_differs", "ippatsu")


def _coverage(cover, view, got, g, np_):
    """what the rows of game g cover, by (row, opponent) pair"""
    for seat in range(np_):
        for r in range(np_ - 1):
            p = view.players[(seat + 1 + r) % np_]
            row = got[g * 4 + seat, r]
            _, _, waits, flags = H.seat_fields(p, np_ == 3)
            if row.any():
                cover["nonzero"] += 1
                cover["riichi"] += bool(p.riichi_declared)
                cover["open_hand"] += any(p.melds[i].opened for i in range(p.n_melds))
                cover["ippatsu"] += bool(p.riichi_declared and p.ippatsu_cycle)
                cover["red_differs"] += any(row[34 + i] > 0 and row[34 + i] != row[4 + 9 * i] for i in range(3))
            if flags & H.TENPAI and flags & H.FURITEN:
                cover["furiten_zeroed"] += 1
                assert not row.any(), "a furiten opponent costs nothing"
            elif flags & H.TENPAI:
                cover["no_yaku_zeroed"] += any((waits >> t) & 1 and row[t] == 0 for t in range(34))


@pytest.mark.parametrize("policy", ["greedy", "random"])
@pytest.mark.parametrize("mode", [2, 5])
def test_live_entry_equals_the_yardstick_on_the_devices_state(mode, policy):
    from riichienv_amd import vecenv

    n, np_ = 32, 3 if mode >= 3 else 4
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=77 + mode, event_ring=4096)
    env.reset()
    index = np.arange(4 * n, dtype=np.int32)
    cover = dict.fromkeys(CLASSES, 0)
    at = 0
    for stop in (range(20, 301, 20) if policy == "greedy" else (40, 120, 300)):
        if policy == "greedy":
            env.step_greedy(5, stop - at, auto_reset=False, call_rate_256=64)
        else:
            env.step_random(5, stop - at, auto_reset=False)
        at = stop
        views = [env.peek(g) for g in range(n)]
        for ura in ((False, True) if mode < 3 else (False,)):
            got = env.danger_targets(index, ura=ura)
            want = np.stack([D.danger_of_view(view, seat, np_, ura) for view in views for seat in range(4)])
            assert got.dtype == want.dtype and got.shape == want.shape == (4 * n, 3, 37)
            bad = np.flatnonzero((got != want).reshape(4 * n, -1).any(axis=1))
            assert bad.size == 0, (stop, ura, bad[:4].tolist(), [np.argwhere(got[i] != want[i]).tolist() for i in bad[:2]],
                                   [got[i][got[i] != want[i]].tolist() for i in bad[:2]], [want[i][got[i] != want[i]].tolist() for i in bad[:2]])
            if not ura:
                assert (got % 100 == 0).all() and (got >= 0).all()
                for g in range(n):
                    _coverage(cover, views[g], got, g, np_)
    env.close()
    print(f"mode {mode} {policy}: (row, opponent) pairs by class {cover}")
    if policy == "greedy":
        assert cover["nonzero"] >= 50, cover
        thin = [c for c in CLASSES if cover[c] == 0]
        assert not thin, f"classes never met: {thin} in {cover}"


# ---------------------------------------------------------------- 2. the device against its own settlement (3P ura included)
@pytest.mark.parametrize("mode", [2, 5])
def test_the_value_is_what_the_devices_settlement_pays(mode):
    from riichienv_amd import vecenv

    n, np_ = 256, 3 if mode >= 3 else 4
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=31 + mode, event_ring=4096)
    env.reset()
    compared, riichi_winners, at = 0, 0, 0
    for stop in (70, 150, 230):
        env.step_greedy(9, stop - at, auto_reset=False, call_rate_256=64)
        at = stop
        active, phase, done = env.status()
        legal, cnt = env.legal()
        before = env.scores()
        chosen = {}       # game -> (current player, discard action, winner seat, value, sticks, the winner is in riichi)
        cands = {}        # game -> (current player, view) of the games whose current player is to discard
        for g in range(n):
            if done[g] or phase[g] != abi.WAIT_ACT:
                continue
            view = env.peek(g)
            cur = int(view.current_player)
            if not view.pending_kan_dora_count and (active[g] >> cur) & 1:
                cands[g] = (cur, view)
        rows = env.danger_targets(np.array([g * 4 + cur for g, (cur, _) in cands.items()], np.int32), ura=True)
        for row, (g, (cur, view)) in zip(rows, cands.items()):
            for a in (int(x) for x in legal[g, cur, : cnt[g, cur]]):
                ty, tile, _ = abi.unpack_action(a)
                if ty != abi.DISCARD or tile is None or not row[:, D.kind_of_tile(tile)].any():
                    continue
                r = int(np.flatnonzero(row[:, D.kind_of_tile(tile)])[0])
                s = (cur + 1 + r) % np_
                chosen[g] = (cur, a, s, int(row[r, D.kind_of_tile(tile)]), 1000 * int(view.riichi_sticks), bool(view.players[s].riichi_declared))
                break
        if not chosen:
            continue
        fork = env.clone()
        acts = fork.random_actions(3)
        for g, (cur, a, *_rest) in chosen.items():
            acts[g] = abi.NO_ACTION
            acts[g, cur] = a
        fork.step(acts)
        f_active, f_phase, f_done = fork.status()
        f_legal, f_cnt = fork.legal()
        acts = fork.random_actions(4)
        for g, (cur, a, s, value, sticks, riichi) in chosen.items():
            assert not f_done[g] and f_phase[g] == abi.WAIT_RESPONSE and (f_active[g] >> s) & 1, (g, cur, s, "the valued tile is not offered as a Ron")
            ron = [int(x) for x in f_legal[g, s, : f_cnt[g, s]] if abi.unpack_action(int(x))[0] == abi.RON]
            assert ron, (g, cur, s, value)
            acts[g] = abi.NO_ACTION
            for p in range(np_):
                if (f_active[g] >> p) & 1:
                    acts[g, p] = ron[0] if p == s else abi.pack_action(abi.PASS)
        fork.step(acts)
        after = fork.scores()
        for g, (cur, a, s, value, sticks, riichi) in chosen.items():
            gain = int(after[g, s]) - int(before[g, s])
            assert gain - sticks == value, (mode, stop, g, cur, s, gain, sticks, value)
            compared += 1
            riichi_winners += riichi
        fork.close()
    env.close()
    print(f"mode {mode}: {compared} games compared, {riichi_winners} riichi winners")
    assert compared >= 20, compared
    if mode >= 3:
        assert riichi_winners > 0, "no riichi winner: the 3P ura indicators were not exercised"


# ---------------------------------------------------------------- 3. the builder against the oracle replay
@pytest.mark.parametrize("mode", [2, 5])
def test_builder_rows_equal_the_oracle_replay(mode):
    c = _built(mode)
    s, cn = c["both"], c["both_counts"]
    assert cn["failed_logs"] == 0 and cn["overflowed"] == 0 and cn["steps_left"] == 0 and cn["complete_logs"] == len(c["logs"]), cn
    assert s["action"].shape[0] == cn["fill"] == cn["decisions"] > 0, "no sample may be left out"
    _against_ref(s, c["ref"])
    nz = s["danger"].reshape(len(s["danger"]), 3, -1).any(axis=2)
    print(f"mode {mode}: {s['action'].shape[0]} samples, {int(nz.sum())} (sample, opponent) pairs with a nonzero value, largest {int(s['danger'].max())}")
    assert nz.sum() > 100


# ---------------------------------------------------------------- 4. nothing else moves
@pytest.mark.parametrize("mode", [2, 5])
def test_danger_changes_no_other_column(mode):
    c = _built(mode)
    assert list(c["plain"]) == TODAY and list(c["danger"]) == TODAY + ["danger"]
    assert list(c["hidden"]) == TODAY + HIDDEN_KEYS and list(c["both"]) == TODAY + HIDDEN_KEYS + ["danger"]
    assert c["plain_counts"] == c["danger_counts"] == c["hidden_counts"] == c["both_counts"]
    for a, b, keys in (("plain", "danger", TODAY), ("hidden", "both", TODAY + HIDDEN_KEYS), ("danger", "both", TODAY + ["danger"])):
        for k in keys:
            assert c[a][k].dtype == c[b][k].dtype and c[a][k].tobytes() == c[b][k].tobytes(), (a, b, k)
    s = c["both"]
    assert s["danger"].dtype == np.int32 and s["danger"].shape[1:] == (3, 37)
    # a value implies the wait and excludes furiten
    types = np.array([D.kind_type(k) for k in range(37)])
    bit = ((s["opp_waits"][:, :, None] >> types[None, None, :]) & 1) != 0
    live = s["danger"] > 0
    assert (bit | ~live).all(), "a value on a tile that is no wait"
    assert not (live.any(axis=2) & ((s["opp_flags"] & abi.HIDDEN_FURITEN) != 0)).any(), "a value against a furiten opponent"


# ---------------------------------------------------------------- 5. edges
def test_a_pool_too_small_keeps_the_columns_in_step():
    c = _built(2)
    logs = c["logs"][:4]
    s, counts = _build(logs, 2, hidden=True, danger=True, capacity=600)
    _, plain_counts = _build(logs, 2, capacity=600)
    assert counts["overflowed"] > 0 and counts == plain_counts
    k = s["action"].shape[0]
    assert 0 < k <= 600 and s["danger"].shape[0] == k
    _against_ref(s, c["ref"])      # (the logs are the first four of the shared run: the same log numbers)


@pytest.mark.parametrize("mode", [2, 5])
def test_slots_that_replay_several_logs(mode):
    c = _built(mode)
    s, counts = _build(c["logs"], mode, hidden=True, danger=True, n_slots=3)
    assert counts["overflowed"] == 0 and counts["failed_logs"] == 0 and s["action"].shape[0] == c["both"]["action"].shape[0]
    _against_ref(s, c["ref"])


def test_danger_over_a_masked_set_is_refused():
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.logset import LogSet
    from tests import apply_events_util as U

    log = U.furiten_log(False)
    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder([log], game_mode=2, masked_ok=True, danger=True)
    ls = LogSet.from_logs([log], 4, masked_ok=True)
    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder.from_logset(ls, game_mode=2, danger=True)
    LogSampleBuilder.from_logset(ls, game_mode=2).close()   # the plain builder takes it as before
    ls.close()


def test_an_empty_log_set():
    from riichienv_amd.datasets import LogSampleBuilder

    b = LogSampleBuilder([], game_mode=2, danger=True)
    assert b.run() == 0
    s = b.samples()
    assert s["danger"].shape == (0, 3, 37) and s["action"].shape == (0,) and "opp_hand" not in s
    b.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_danger_compact_stops_at_the_device_count(mode):
    import torch

    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(67, game_mode=mode, seed=5)      # 67: the last block of four rows is not full
    env.env.step_greedy(3, 150, auto_reset=True)
    _, index = env.obs_compact()
    k = int(index.shape[0])
    assert k > 32
    for ura in (False, True):
        full = env.danger_compact(index, ura=ura)
        assert full.dtype == torch.int32 and tuple(full.shape) == (k, 3, 37)
        assert (full.cpu().numpy() == env.env.danger_targets(index.cpu().numpy(), ura=ura)).all()
    cut = k // 2 + 1
    out = torch.full_like(full, 0x5A5A5A5A)
    count = torch.tensor([cut], dtype=torch.int32, device=index.device)
    assert env.danger_compact(index, count=count, ura=True, out=out) is out
    torch.cuda.synchronize()
    assert (out[:cut] == full[:cut]).all()
    assert (out[cut:] == 0x5A5A5A5A).all(), "a row behind the count was written"
    env.env.close()


def test_a_bad_index_gives_a_zero_row():
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(4, game_mode=2, seed=2)
    env.reset()
    v = env.peek(0)     # seat 1 waits on 6p-9p in riichi: every row of game 0 but its own has a value
    p = v.players[1]
    hand = [4 * t + 2 for t in (1, 2, 3, 18, 19, 20, 21, 22, 23, 15, 16)] + [4 * 27, 4 * 27 + 1]   # 234m 123s 456s 78p EE
    p.hand_len = 13
    for i, t in enumerate(sorted(hand)):
        p.hand[i] = t
    p.riichi_declared = 1
    env.poke(0, v)
    got = env.danger_targets(np.array([0, 16, -1, 1 << 30, 2, 4 * 4 - 1], dtype=np.int32))
    assert got[0, 0, 14] > 0 and got[0, 0, 17] > 0 and got[4, 2, 14] == got[0, 0, 14], got[0, 0].tolist()
    assert (got[0] == D.danger_of_view(env.peek(0), 0, 4)).all()
    assert not got[1:4].any()
    import ctypes as C

    one, idx = np.zeros((1, 3, 37), np.int32), np.zeros(1, np.int32)
    assert env.L.rmj_danger_targets(env.h, idx.ctypes.data, 1, 2, C.byref(abi.DangerOut(one.ctypes.data))) != 0, "an unknown flag is refused"
    assert env.L.rmj_danger_targets(env.h, idx.ctypes.data, 1, 0, C.byref(abi.DangerOut(None))) != 0, "a null array is refused"
    env.close()


def test_the_pool_record_holds_more_than_65535_points():
    """the pool stores hundreds of points in 16 bits: a dealer's double yakuman, 96 000 points, comes back whole"""
    tehais = [["1m", "1m", "1m", "3p", "3p", "3p", "5s", "5s", "5s", "7s", "7s", "7s", "9s"],
              ["2m", "3m", "4m", "5m", "6m", "7m", "8m", "9m", "1p", "2p", "4p", "5p", "6p"],
              ["1z", "2z", "3z", "4z", "5z", "6z", "7z", "7p", "8p", "9p", "2s", "8s", "1s"],
              ["4s", "6s", "8s", "4m", "5m", "6m", "7m", "8m", "9m", "1z", "2z", "3z", "4z"]]
    log = [{"type": "start_game"},
           {"type": "start_kyoku", "bakaze": "E", "kyoku": 1, "honba": 0, "kyoutaku": 0, "oya": 0, "scores": [25000] * 4, "dora_marker": "1z", "tehais": tehais},
           {"type": "tsumo", "actor": 0, "pai": "6z"}, {"type": "dahai", "actor": 0, "pai": "6z", "tsumogiri": True},
           {"type": "tsumo", "actor": 1, "pai": "7z"}, {"type": "dahai", "actor": 1, "pai": "7z", "tsumogiri": True},
           {"type": "ryukyoku", "reason": "yao9"}, {"type": "end_kyoku"}, {"type": "end_game"}]
    for rule, bits, want in (("mjsoul", abi.RULE_MJSOUL, 96000), ("tenhou", abi.RULE_TENHOU, 48000)):
        s, counts = _build([log], 2, hidden=True, danger=True, rule=rule)
        assert counts["failed_logs"] == 0 and counts["complete_logs"] == 1
        i = [j for j, (st, ev) in enumerate(zip(s["seat"].tolist(), s["event"].tolist())) if st == 1 and ev == 5]
        assert len(i) == 1, (s["seat"].tolist(), s["event"].tolist())
        row = s["danger"][i[0]]
        assert int(row[2, 26]) == want and 0 < int(row[2, 25]) < want and not row[:2].any(), (rule, row[2].tolist())   # (8s completes 789s with a 7s pair: no yakuman)
        ref = D.log_danger(log, 2, keys={(5, 1)}, rule_bits=bits)[5, 1]
        assert (row == ref).all()


# ---------------------------------------------------------------- 6. the example
def test_the_example_runs():
    import importlib.util

    spec = importlib.util.spec_from_file_location("danger_targets_example", os.path.join(ROOT, "examples", "danger_targets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(games=8, steps=20000)
    assert out["logs"] == 8 and out["samples"] > 1000 and out["overflowed"] == 0 and out["discards"] > 0
    assert 0.0 < out["dealt_in"] < 0.05 and out["horas"] > 0 and out["winner_label_zero"] == 0
    assert 1000 <= out["mean_danger_dealt_in"] <= 48000 and 0.0 <= out["mean_danger_safe"] < out["mean_danger_dealt_in"]
    assert 0.0 < out["wait_bits_costing_nothing"] < 1.0 and out["wait_bits"] > 0
