"""The log sample builder (riichienv_amd.datasets.LogSampleBuilder, rmj_logreplay_*) against its checkers: ReplayBatch.samples() /
Kyoku.steps' order on logs the library wrote itself (greedy and random rollouts, 4p-red-half and 3p-red-half, N_GAMES complete games
per mode), the oracle on the real log, and Python restatements of the returns and ranks."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

from riichienv_amd import abi, mjai

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(__file__), "golden", "126_204_0_mjai.jsonl")
N_GAMES = 1024      # complete games per mode
CHUNK = 128         # logs per ReplayBatch of the checker (the host path holds every game's dense tensor)
_LOGS = {}


def _rollout_logs(mode):
    """N_GAMES complete games of `mode` as MJAI event lists: half played by step_greedy(call_rate_256=64), half by step_random"""
    if mode not in _LOGS:
        from riichienv_amd import vecenv

        logs = []
        for policy, seed in (("greedy", 101 + mode), ("random", 202 + mode)):
            n = N_GAMES // 2
            env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, event_ring=8192)
            env.reset()
            for _ in range(40):
                if policy == "greedy":
                    env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
                else:
                    env.step_random(7, 500, auto_reset=False)
                if env.status()[2].all():
                    break
            assert env.status()[2].all(), "a rollout game did not finish"
            assert int(env.events_lost().sum()) == 0
            logs += [[json.loads(s) for s in g] for g in env.mjai_logs()]
            env.close()
        _LOGS[mode] = logs
    return _LOGS[mode]


def _row_key(row_bytes):
    return zlib.crc32(row_bytes), len(row_bytes)


def _checker_samples(logs, mode, extended, include_pass, skip_single, first_log=0):
    """{(log, kyoku, seat, t): (action_id, packed, mask bytes, row key)} from ReplayBatch.samples(), with kyoku = the start_kyoku events
    before the event index and t counted per (log, kyoku, seat) in Kyoku.steps' order (passes first, highest seat first)"""
    from riichienv_amd import replay

    out = {}
    kyoku_at = [np.cumsum([e.get("type") == "start_kyoku" for e in l]) for l in logs]
    tcount = {}
    rb = replay.ReplayBatch(logs, game_mode=mode, extended=extended, include_pass=include_pass)
    for smp in rb.samples():
        k = smp["index"]
        is_pass = [abi.unpack_action(int(a))[0] == abi.PASS for a in smp["action"]]
        order = sorted((j for j in range(len(is_pass)) if is_pass[j]), key=lambda j: -int(smp["seat"][j])) + [j for j in range(len(is_pass)) if not is_pass[j]]
        for j in order:
            if skip_single and len(smp["legal"][j]) <= 1:
                continue
            g, s = int(smp["game"][j]), int(smp["seat"][j])
            ky = int(kyoku_at[g][k - 1]) if k else 0
            t = tcount.get((g, ky, s), 0)
            tcount[(g, ky, s)] = t + 1
            out[(g + first_log, ky, s, t)] = (int(smp["action_id"][j]), int(smp["action"][j]), smp["mask"][j].tobytes(), _row_key(smp["obs"][j].tobytes()))
    rb.env.close()
    return out


def _builder_samples(b, rows=True):
    s = {k: v.cpu().numpy() for k, v in b.samples().items() if rows or k != "features"}
    out = {}
    for i in range(len(s["action"])):
        key = (int(s["log"][i]), int(s["kyoku"][i]), int(s["seat"][i]), int(s["t"][i]))
        assert key not in out, key
        out[key] = (int(s["action"][i]), int(s["packed"][i]) & 0xFFFFFFFFFFFFFFFF, s["mask"][i].tobytes(), _row_key(s["features"][i].tobytes()) if rows else None)
    return out, s


def _clean(b):
    c = b.counts()
    assert c["failed_logs"] == 0 and c["overflowed"] == 0 and c["steps_left"] == 0 and c["complete_logs"] == b.M, c
    return c


def test_the_rollouts_hold_every_kind_of_decision():
    want = {2: ("reach", "chi", "pon", "daiminkan", "ankan", "kakan", "hora", "ryukyoku"), 5: ("reach", "pon", "daiminkan", "ankan", "kakan", "kita", "hora", "ryukyoku")}
    for mode, kinds in want.items():
        seen = {}
        for l in _rollout_logs(mode):
            for e in l:
                seen[e["type"]] = seen.get(e["type"], 0) + 1
        for k in kinds:
            assert seen.get(k, 0) > 0, (mode, k, seen)


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("features", ["base", "extended"])
@pytest.mark.parametrize("include_pass", [True, False])
def test_samples_equal_the_checker(mode, features, include_pass):
    """every (log, kyoku, seat, t) with its action id, packed action, mask and feature row, bit for bit; passes, kyushu kyuhai and the Ron
    on a robbed kan must be among them"""
    from riichienv_amd.datasets import LogSampleBuilder

    logs = _rollout_logs(mode)
    b = LogSampleBuilder(logs, game_mode=mode, features=features, include_pass=include_pass, skip_single_action=True)
    b.run()
    _clean(b)
    got, _ = _builder_samples(b)
    b.close()
    want = {}
    for at in range(0, len(logs), CHUNK):
        want.update(_checker_samples(logs[at: at + CHUNK], mode, features == "extended", include_pass, True, first_log=at))
    print(f"mode {mode} {features} include_pass={include_pass}: {len(got)} samples from the builder, {len(want)} from the checker")
    assert got.keys() == want.keys(), (len(got), len(want), sorted(got.keys() ^ want.keys())[:8])
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (len(bad), bad[:4], [tuple(a == c for a, c in zip(got[k], want[k])) for k in bad[:4]])
    types = {abi.unpack_action(v[1])[0] for v in got.values()}
    assert (abi.PASS in types) == include_pass and abi.KYUSHU in types and abi.RON in types and abi.TSUMO in types, types


def test_robbed_kan_rons_occur_and_are_samples():
    """the Ron on a robbed kakan / ankan is not in the published lists: the rollouts must hold some, and the builder must emit each"""
    from riichienv_amd.datasets import LogSampleBuilder

    for mode in (2, 5):
        logs = _rollout_logs(mode)
        robbed = []
        for i, l in enumerate(logs):
            ky = 0
            for k, e in enumerate(l):
                ky += e["type"] == "start_kyoku"
                if e["type"] == "hora" and e["actor"] != e["target"]:
                    j = k - 1
                    while l[j]["type"] == "dora":
                        j -= 1
                    if l[j]["type"] in ("kakan", "ankan") and l[j]["actor"] == e["target"]:
                        robbed.append((i, ky, int(e["actor"])))
        assert robbed, f"no robbed kan in {len(logs)} games of mode {mode}"
        b = LogSampleBuilder(logs, game_mode=mode, include_pass=False, skip_single_action=True, capacity=2_000_000)
        b.run()
        _clean(b)
        got, _ = _builder_samples(b, rows=False)
        b.close()
        ron = {(k[0], k[1], k[2]) for k, v in got.items() if abi.unpack_action(v[1])[0] == abi.RON}
        assert set(robbed) <= ron, sorted(set(robbed) - ron)[:4]


def _oracle_logs(mode):
    """logs the ORACLE played, not the library: the games of tests/test_gpu_replay.py in which a kakan is robbed (greedy policy, calls at
    160 / 256, seeds 5000 + g) and its games of winning play (seeds 1300 + g, calls at 96 / 64)"""
    from oracle import oracle

    logs = []
    for seed0, pseed, rate, picks in ((5000, 71, 160, (17, 22, 39) if mode == 2 else (5, 10, 17)), (1300, 53, 96 if mode == 2 else 64, range(8))):
        for g in picks:
            o = oracle.Game(game_mode=mode, seed=seed0 + g)
            o.reset()
            for _ in range(2500):
                if o.status()[2]:
                    break
                o.step([int(x) for x in o.greedy_actions(pseed, g, rate)])
            logs.append([json.loads(x) for x in o.log()])
    return logs


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("include_pass", [True, False])
def test_oracle_played_logs_equal_the_checker(mode, include_pass):
    """the same comparison on logs a different engine wrote: every log replays completely (failed_logs == 0), the samples equal
    ReplayBatch's bit for bit in base and extended features, and every robbed kakan of these games is a Ron sample whose mask holds
    two ids"""
    from riichienv_amd.datasets import LogSampleBuilder

    logs = _oracle_logs(mode)
    chankan = set()
    for i, l in enumerate(logs):
        ky = 0
        for k, e in enumerate(l):
            ky += e["type"] == "start_kyoku"
            if e["type"] == "hora" and e["actor"] != e["target"] and l[k - 1]["type"] != "hora" and [x for x in l[:k] if x["type"] != "dora"][-1]["type"] == "kakan":
                chankan.add((i, ky, int(e["actor"])))
    assert len({c[0] for c in chankan}) >= 3, chankan
    for features in ("base", "extended"):
        for skip in (True, False):
            b = LogSampleBuilder(logs, game_mode=mode, features=features, include_pass=include_pass, skip_single_action=skip, n_slots=5)
            b.run()
            _clean(b)
            got, _ = _builder_samples(b)
            b.close()
            want = _checker_samples(logs, mode, features == "extended", include_pass, skip)
            assert got.keys() == want.keys(), (features, skip, len(got), len(want), sorted(got.keys() ^ want.keys())[:8])
            bad = [k for k in want if got[k] != want[k]]
            assert not bad, (features, skip, len(bad), bad[:4])
            rons = {k[:3]: v for k, v in got.items() if abi.unpack_action(v[1])[0] == abi.RON}
            assert chankan <= rons.keys(), sorted(chankan - rons.keys())
            assert all(sum(rons[c][2]) == 2 for c in chankan)


def test_order_within_a_kyoku_is_that_of_kyoku_steps():
    """t and the pool order of one log's samples against Kyoku.steps(seat) / Kyoku.steps(None)"""
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.replay import MjaiReplay

    logs = _rollout_logs(2)[:4]
    b = LogSampleBuilder(logs, game_mode=2, n_slots=4)
    b.run()
    _clean(b)
    _, s = _builder_samples(b, rows=False)
    b.close()
    for li, log in enumerate(logs):
        for ki, ky in enumerate(MjaiReplay.from_events(log).take_kyokus(), start=1):
            sel = (s["log"] == li) & (s["kyoku"] == ki)
            every = [(seat, int(a.encode())) for seat, o, a in ky.steps()]
            assert [(int(x), int(y)) for x, y in zip(s["seat"][sel], s["action"][sel])] == every, (li, ki)
            for seat in range(4):
                mine = [int(a.encode()) for o, a in ky.steps(seat)]
                m = sel & (s["seat"] == seat)
                assert list(s["t"][m]) == list(range(len(mine))) and [int(x) for x in s["action"][m]] == mine, (li, ki, seat)


def test_discard_shanten_rows_and_its_refusal_in_3p():
    from riichienv_amd import vecenv
    from riichienv_amd.datasets import LogSampleBuilder

    logs = _rollout_logs(2)[:32]
    rows = {}
    for f in ("base", "discard_shanten", "extended"):
        b = LogSampleBuilder(logs, game_mode=2, features=f)
        b.run()
        _clean(b)
        rows[f] = b.samples()["features"].cpu().numpy()
        b.close()
    assert rows["discard_shanten"].shape[1:] == (94, 34) and len(rows["discard_shanten"]) == len(rows["extended"]) > 0
    # feat_v2 = encode()'s 74 channels + encode_extended()'s channels 74..93
    assert rows["discard_shanten"][:, :74].tobytes() == rows["base"].tobytes()
    assert rows["discard_shanten"][:, 74:].tobytes() == rows["extended"][:, 74:94].tobytes()
    with pytest.raises(vecenv.RmjError, match="4-player only"):
        LogSampleBuilder(_rollout_logs(5)[:4], game_mode=5, features="discard_shanten")


def test_the_golden_log_against_the_oracle():
    """sample for sample against oracle.Game driven over the real log, the way tests/test_gpu_replay.py drives it"""
    from oracle import oracle
    from riichienv_amd import replay
    from riichienv_amd.datasets import LogSampleBuilder

    events = replay.load_mjai_jsonl(LOG)
    b = LogSampleBuilder([events], game_mode=2, include_pass=False, skip_single_action=False)
    b.run()
    _clean(b)
    s = {k: v.cpu().numpy() for k, v in b.samples().items()}
    b.close()
    o = oracle.Game(game_mode=2, seed=1)
    o.reset()
    kinds = ("dahai", "pon", "chi", "reach", "hora", "ankan", "kakan", "daiminkan")
    i = ky = 0
    tc = {}
    for ev in events:
        ky += ev["type"] == "start_kyoku"
        if ev["type"] in kinds:
            seat = int(ev["actor"])
            v = o.peek()
            sel = mjai.select_action_from_mjai(o.legal(seat), ev, None if v.drawn_tile < 0 else int(v.drawn_tile), False)
            assert sel is not None, ev
            t = tc.get((ky, seat), 0)
            tc[(ky, seat)] = t + 1
            assert (int(s["log"][i]), int(s["kyoku"][i]), int(s["seat"][i]), int(s["t"][i])) == (0, ky, seat, t), (i, ev)
            assert int(s["packed"][i]) & 0xFFFFFFFFFFFFFFFF == sel, (i, ev)
            assert (s["mask"][i] == np.asarray(o.mask(seat))).all() and s["mask"][i][s["action"][i]] == 1
            assert s["features"][i].tobytes() == o.encode(seat, False).tobytes(), (i, ev)
            i += 1
        o.apply_event(ev, replay=True)
    assert i == len(s["action"]) == sum(e["type"] in kinds for e in events)


def test_slot_streaming_gives_the_same_samples_in_a_reproducible_order():
    from riichienv_amd.datasets import LogSampleBuilder

    logs = _rollout_logs(5)[:64] + _rollout_logs(5)[-64:]
    ref = None
    for n in (len(logs), len(logs) // 4, 3):
        runs = []
        for _ in range(2):
            b = LogSampleBuilder(logs, game_mode=5, n_slots=n)
            b.run()
            _clean(b)
            s = b.samples()
            runs.append({k: v.cpu().numpy() for k, v in s.items()})
            b.close()
        for k in runs[0]:
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), (n, k)     # the pool order of two identical runs
        keyed = {(int(a), int(c), int(d), int(e)): (int(x), int(p), m.tobytes(), f.tobytes(), float(r)) for a, c, d, e, x, p, m, f, r in
                 zip(runs[0]["log"], runs[0]["kyoku"], runs[0]["seat"], runs[0]["t"], runs[0]["action"], runs[0]["packed"], runs[0]["mask"], runs[0]["features"],
                     runs[0]["return64"])}
        assert len(keyed) == len(runs[0]["action"])
        if ref is None:
            ref = keyed
        assert keyed == ref, n


def _restate_returns(s, rewards, koff, gamma):
    T = {}
    for l, k, seat in zip(s["log"], s["kyoku"], s["seat"]):
        T[(l, k, seat)] = T.get((l, k, seat), 0) + 1
    out = []
    for l, k, seat, t in zip(s["log"], s["kyoku"], s["seat"], s["t"]):
        r = float(rewards[int(koff[l]) + k - 1][seat])
        out.append(r * (gamma ** (T[(l, k, seat)] - int(t) - 1)))
    return out


@pytest.mark.parametrize("mode", [2, 5])
def test_returns_and_ranks(mode):
    from riichienv_amd.datasets import LogSampleBuilder, compute_rank

    logs = [list(l) for l in _rollout_logs(mode)[:96]]
    np_ = 3 if mode >= 3 else 4
    # a kyoku whose end scores tie: the next round's start scores are the end scores (two seats made equal)
    sk = [i for i, e in enumerate(logs[0]) if e["type"] == "start_kyoku"]
    assert len(sk) >= 2
    tied = dict(logs[0][sk[1]])
    tied["scores"] = [tied["scores"][1]] + list(tied["scores"][1:])
    logs[0][sk[1]] = tied
    gamma = 0.99
    b = LogSampleBuilder(logs, game_mode=mode, gamma=gamma)
    b.run()
    _clean(b)
    assert (b.end_scores[0][0] == b.end_scores[0][1])
    rng = np.random.default_rng(5)
    for rewards in (None, rng.normal(size=(b.n_kyokus, 4)) * 3.0):
        b.finalize(rewards)
        s = {k: v.cpu().numpy() for k, v in b.samples().items()}
        table = b.default_rewards() if rewards is None else rewards
        want = _restate_returns(s, table, b.kyoku_offsets, gamma)
        assert s["return64"].tobytes() == struct.pack(f"<{len(want)}d", *want)
        assert s["return"].tobytes() == np.array(want, dtype=np.float64).astype(np.float32).tobytes()
        ranks = compute_rank(b.end_scores, np_)
        rows = b.kyoku_offsets[s["log"]].astype(np.int64) + s["kyoku"] - 1
        assert (s["rank"] == ranks[rows, s["seat"]]).all()
        assert len(set(s["rank"][rows == 0])) == len(set(s["seat"][rows == 0]))   # tied scores still rank apart
    b.close()


def test_a_tampered_log_fails_alone():
    from riichienv_amd.datasets import LogSampleBuilder

    logs = [list(l) for l in _rollout_logs(2)[:24]]
    good, _ = None, None
    b = LogSampleBuilder(logs, game_mode=2, n_slots=6)
    b.run()
    _clean(b)
    good, _ = _builder_samples(b)
    b.close()
    # a dahai of a tile that is not in the hand, mid-game
    victim = 7
    ks = [i for i, e in enumerate(logs[victim]) if e["type"] == "dahai"]
    k = ks[len(ks) // 2]
    ev = dict(logs[victim][k])
    hand = []
    for e in logs[victim][:k]:
        if e["type"] == "start_kyoku":
            hand = list(e["tehais"][ev["actor"]])
        elif e.get("actor") == ev["actor"]:
            if e["type"] == "tsumo":
                hand.append(e["pai"])
            elif e["type"] in ("dahai", "kakan"):
                hand.remove(e["pai"])
            elif e["type"] in ("chi", "pon", "daiminkan", "ankan"):
                for x in e["consumed"]:
                    hand.remove(x)
    ev["pai"] = next(t for t in [f"{i}{c}" for c in "mps" for i in range(1, 10)] + list("ESWNPFC") if t not in hand)
    ev["tsumogiri"] = False
    logs[victim][k] = ev
    b = LogSampleBuilder(logs, game_mode=2, n_slots=6)
    b.run()
    c = b.counts()
    assert c["failed_logs"] == 1 and c["overflowed"] == 0 and c["complete_logs"] == len(logs) - 1, c
    got, _ = _builder_samples(b)
    b.close()
    assert not [key for key in got if key[0] == victim]
    assert got == {key: v for key, v in good.items() if key[0] != victim}


def test_edges():
    import torch

    from riichienv_amd.datasets import LogSampleBuilder

    logs = _rollout_logs(2)[:16]
    full = LogSampleBuilder(logs, game_mode=2, n_slots=4, share_stream=False)     # the library's own stream: every call synchronises
    full.run()
    _clean(full)
    whole, sw = _builder_samples(full)
    # a short pool: counted, and nothing of a truncated trajectory is emitted
    cap = len(whole) // 2
    b = LogSampleBuilder(logs, game_mode=2, n_slots=4, capacity=cap)
    b.run()
    c = b.counts()
    assert c["overflowed"] == len(whole) - cap and c["fill"] == cap and c["failed_logs"] == 0, c
    part, sp = _builder_samples(b)
    assert 0 < len(part) < cap
    lens = {}
    for key in whole:
        lens[key[:3]] = lens.get(key[:3], 0) + 1
    mine = {}
    for key, v in part.items():
        assert whole[key] == v
        mine[key[:3]] = mine.get(key[:3], 0) + 1
    assert all(lens[k] == n for k, n in mine.items()), "a truncated trajectory was emitted"
    # clear(): the same pool again
    b.clear()
    assert b.counts()["fill"] == 0 and b.counts()["steps_done"] == 0
    b.run()
    again, _ = _builder_samples(b)
    assert again == part
    b.close()
    # runs in pieces
    left = 1
    full.clear()
    while left:
        left = full.run(97)
    assert _builder_samples(full)[0] == whole
    # batches(): every sample once per epoch, the same seed the same order
    n = len(whole)
    seen = []
    for f, a, g, m, r in full.batches(1000, shuffle=True, generator=torch.Generator().manual_seed(3)):
        assert f.shape[1:] == (74, 34) and m.shape[1] == 82 and a.dtype == torch.int64 and g.dtype == torch.float32 and r.dtype == torch.int64
        seen.append(torch.stack([a, r]).cpu())
    one = torch.cat(seen, dim=1)
    two = torch.cat([torch.stack([a, r]).cpu() for f, a, g, m, r in full.batches(1000, shuffle=True, generator=torch.Generator().manual_seed(3))], dim=1)
    assert one.shape[1] == n and torch.equal(one, two)
    assert sorted(one[0].tolist()) == sorted(int(x) for x in sw["action"])
    plain = torch.cat([a.cpu() for f, a, g, m, r in full.batches(512, shuffle=False)])
    assert plain.tolist() == [int(x) for x in sw["action"]]
    full.close()
    # an empty log set
    e = LogSampleBuilder([], game_mode=2)
    e.run()
    assert e.counts()["fill"] == 0 and e.samples()["features"].shape == (0, 74, 34) and list(e.batches(8)) == []


def test_the_example_runs():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "examples", "bc_from_logs.py"), "--batches", "4"], capture_output=True, text=True, cwd=root, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "loss" in p.stdout
