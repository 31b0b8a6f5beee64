"""LogSet.validate (rmj_logcheck_*, csrc/rmj_logcheck.hip.h) against its plain restatement (tests/log_check_ref.py): exact equality of
(code, event, kyoku, seat) on every log, for 4P and 3P, through from_logs and from_text - the golden log alone and in 64 copies, a mixed
set of clean self-written logs, every mutation and three empty shells, at every slot count; a kept log that does not parse; the verdict
arrays between guard words; the report's summary, good_ids and the forwards; and the sample builder untouched by a validation."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from riichienv_amd import abi
from tests import log_check_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "126_204_0_mjai.jsonl")
MODES = {2: 4, 5: 3}
_CACHE = {}


def _text(log):
    return "".join(json.dumps(e, separators=(",", ":")) + "\n" for e in log).encode()


def _golden():
    if "golden" not in _CACHE:
        log = [json.loads(x) for x in open(GOLDEN) if x.strip()]
        _CACHE["golden"] = (log, R.check_log(log, 4, 2))
    return _CACHE["golden"]


def _self_written(mode):
    """16 complete games (half step_greedy, half step_random) and 4 games still in progress, drained with drain_logs"""
    from riichienv_amd import vecenv

    logs = []
    for policy, seed, n, rounds in (("greedy", 311 + mode, 8, 40), ("random", 422 + mode, 8, 40), ("random", 533 + mode, 4, 1)):
        env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, event_ring=8192)
        env.reset()
        for _ in range(rounds):
            if policy == "greedy":
                env.step_greedy(7, 400, auto_reset=False, call_rate_256=64)
            else:
                env.step_random(7, 400, auto_reset=False)
            if env.status()[2].all():
                break
        assert rounds == 1 or env.status()[2].all(), "a rollout game did not finish"
        assert int(env.events_lost().sum()) == 0
        logs += [[json.loads(s) for s in g] for g in env.drain_logs()]
        env.close()
    return logs


def _mixed(mode):
    """(logs, the restatement's verdicts): every mutation of an oracle log, each followed by a clean complete log (with one slot every
    failed log is followed in its slot by a clean one), then the games in progress, a log of no events, of start_game only, and of
    start_game, end_game"""
    if mode not in _CACHE:
        n = MODES[mode]
        own = _self_written(mode)
        complete = [l for l in own if l and l[-1]["type"] == "end_game"]
        running = [l for l in own if not (l and l[-1]["type"] == "end_game")]
        assert len(complete) == 16 and len(running) == 4
        muts = R.mutations(R.oracle_logs(mode, 32)[1], n)
        assert R.kinds(muts) == set(range(2, 13))
        logs = []
        for i, (name, (events, _code, _point)) in enumerate(sorted(muts.items())):
            logs += [events, complete[i % len(complete)]]
        logs += running + [[], [{"type": "start_game"}], [{"type": "start_game"}, {"type": "end_game"}]]
        want = [R.check_log(l, n, mode) for l in logs]
        for i, (name, (_events, code, _point)) in enumerate(sorted(muts.items())):
            assert want[2 * i][0] == code and want[2 * i + 1][0] == R.OK, (name, want[2 * i], want[2 * i + 1])
        assert all(w[0] == R.UNFINISHED for w in want[2 * len(muts): 2 * len(muts) + 4])
        _CACHE[mode] = (logs, want)
    return _CACHE[mode]


def _make(source, logs, n, **kw):
    from riichienv_amd.logset import LogSet

    if source == "logs":
        return LogSet.from_logs(logs, num_players=n)
    return LogSet.from_text([_text(l) for l in logs], num_players=n, on_error="keep", **kw)


def _verdicts(rep):
    code, event, kyoku, seat = (x.cpu().numpy() for x in (rep.code, rep.event, rep.kyoku, rep.seat))
    return [(int(code[i]), int(event[i]), int(kyoku[i]), int(seat[i])) for i in range(len(code))]


def _assert_equal(got, want, tag):
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, (tag, len(got), len(want), bad[:6])


@pytest.mark.parametrize("source", ["logs", "text"])
def test_golden_log_alone_and_in_64_copies(source):
    from riichienv_amd.logset import LogSet

    log, want = _golden()
    assert want == (R.OK, 0, 0, R.NO_SEAT)
    s = _make(source, [log], 4)
    rep = s.validate(n_slots=1)
    _assert_equal(_verdicts(rep), [want], source)
    assert bool(rep.ok.all()) and rep.summary()["OK"] == 1 and rep.describe(0) == "log 0: OK"
    s.close()
    if source == "logs":
        s = LogSet.from_logs([log] * 64, num_players=4)
    else:   # one buffer, the 64 ranges in reverse order
        t = _text(log)
        rng = np.array([[k * len(t), (k + 1) * len(t)] for k in reversed(range(64))], dtype=np.uint64)
        s = LogSet.from_text(t * 64, rng, num_players=4)
    for n_slots in (None, 7):
        _assert_equal(_verdicts(s.validate(n_slots=n_slots)), [want] * 64, (source, n_slots))
    s.close()


@pytest.mark.parametrize("source", ["logs", "text"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_mixed_set_equals_the_restatement_at_every_slot_count(mode, source):
    logs, want = _mixed(mode)
    s = _make(source, logs, MODES[mode])
    assert s.M == len(logs)
    for n_slots in (1, 4, 5, len(logs)):
        rep = s.validate(game_mode=mode, n_slots=n_slots)
        got = _verdicts(rep)
        _assert_equal(got, want, (mode, source, n_slots))
        hist = np.bincount(rep.code.cpu().numpy(), minlength=len(rep.NAMES))
        assert rep.summary() == {name: int(hist[i]) for i, name in enumerate(rep.NAMES)}, (mode, source, n_slots)
        assert rep.good_ids().tolist() == [i for i, w in enumerate(want) if w[0] == R.OK]
    bad = next(i for i, w in enumerate(want) if w[0] == R.TILE_NOT_HELD)
    d = rep.describe(bad)
    assert d.startswith(f"log {bad}: TILE_NOT_HELD at event {want[bad][1]} (kyoku {want[bad][2]}, seat {want[bad][3]}, tile "), d
    s.close()


def test_a_kept_log_that_does_not_parse_is_PARSE_and_its_neighbours_are_not_touched():
    from riichienv_amd.logset import LogSet

    logs, want = _mixed(2)
    pick = [1, 3, 0, 5]      # clean, clean, a mutated one, clean
    texts = [_text(logs[i]) for i in pick]
    lines = texts[1].split(b"\n")
    lines[40] = b'{"type":"dahai","actor":1,"pai":'     # the log's 41st line is no JSON object
    texts[1] = b"\n".join(lines)
    s = LogSet.from_text(texts, num_players=4, on_error="keep")
    assert [d[0] for d in s.dropped] == [1] and s.dropped[0][1] == 41
    rep = s.validate(n_slots=2)
    _assert_equal(_verdicts(rep), [want[1], (R.PARSE, 41, 0, R.NO_SEAT), want[0], want[5]], "keep")
    assert rep.summary()["PARSE"] == 1 and rep.describe(1).startswith("log 1: PARSE at line 41 (")
    s.close()


def test_verdict_arrays_lie_between_intact_guard_words():
    """through the C entry points with RMJ_LOGCHECK_GUARDS: 64 guard words either side of every verdict array and of the counters"""
    import torch

    from riichienv_amd import vecenv
    from riichienv_amd.logset import LogSet

    logs, want = _mixed(2)
    s = LogSet.from_text([_text(l) for l in logs], num_players=4, on_error="keep")
    L, M, G = s.L, s.M, abi.LOGCHECK_GUARD_WORDS
    env = vecenv.VecRiichiEnv(5, game_mode=2, seed=0, skip_mjai_logging=True, device=s.device_index)
    h, left, v = C.c_void_p(), C.c_uint32(), abi.LogCheckViews()
    vecenv._chk(L.rmj_logcheck_create(env.h, s.handle, 5, abi.LOGCHECK_GUARDS, C.byref(h)))
    try:
        vecenv._chk(L.rmj_logcheck_views(h, C.byref(v)))
        arrays = [(v.code, M), (v.seat, M), (v.kyoku, 4 * M), (v.event, 4 * M), (v.detail, 4 * M), (v.counts, 4 * abi.LOGCHECK_COUNTERS)]

        def guards():
            out = []
            for ptr, size in arrays:
                end = ptr + (size + 255) // 256 * 256     # the array's 256-byte step: the bytes up to it are never written (zeros)
                out.append((abi.device_tensor(torch, s, s.device, ptr - 4 * G, (G,), "<i4").cpu().numpy().view(np.uint32),
                            abi.device_tensor(torch, s, s.device, end, (G,), "<i4").cpu().numpy().view(np.uint32),
                            abi.device_tensor(torch, s, s.device, ptr + size, (end - ptr - size,), "|u1").cpu().numpy() if end > ptr + size else np.zeros(0, np.uint8)))
            return out

        env.sync()
        for before, after, pad in guards():
            assert (before == abi.LOGCHECK_GUARD_WORD).all() and (after == abi.LOGCHECK_GUARD_WORD).all() and not pad.any()
        vecenv._chk(L.rmj_logcheck_run_device(h, 0, C.byref(left)))
        env.sync()
        assert left.value == 0
        for before, after, pad in guards():
            assert (before == abi.LOGCHECK_GUARD_WORD).all() and (after == abi.LOGCHECK_GUARD_WORD).all() and not pad.any()
        code = abi.device_tensor(torch, s, s.device, v.code, (M,), "|u1").cpu().numpy()
        assert code.tolist() == [w[0] for w in want]
        assert L.rmj_logcheck_name(int(code.max())).decode() == abi.LOGCHECK_NAMES[int(code.max())] and L.rmj_logcheck_name(13) is None
    finally:
        L.rmj_logcheck_destroy(h)
        env.close()
        s.close()


def test_good_ids_build_samples_without_a_failed_log_and_the_forwards_agree():
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.grp import GrpDataset

    logs, want = _mixed(2)
    texts = [_text(l) for l in logs]
    b = LogSampleBuilder.from_text(texts, game_mode=2, features="base")
    rep = b.validate()
    _assert_equal(_verdicts(rep), want, "builder")
    g = GrpDataset.from_logset(b.logset)
    _assert_equal(_verdicts(g.validate()), want, "grp")
    _assert_equal(_verdicts(g.validate(n_slots=3)), want, "grp, 3 slots")
    b.close()
    good = rep.good_ids()
    assert 0 < len(good) < len(texts)
    b = LogSampleBuilder.from_text([texts[i] for i in good], game_mode=2, features="base")
    b.run()
    c = b.counts()
    assert c["failed_logs"] == 0 and c["complete_logs"] == len(good) and c["overflowed"] == 0, c
    b.close()


def test_a_validation_leaves_the_sample_builder_as_it_was():
    import torch

    from riichienv_amd.datasets import LogSampleBuilder

    logs, want = _mixed(5)
    clean = [l for l, w in zip(logs, want) if w[0] == R.OK and len(l) > 2][:6]
    b = LogSampleBuilder(clean, game_mode=5, features="base", n_slots=3)
    b.run()
    before = {k: v.clone() for k, v in b.samples().items()}
    assert bool(b.validate().ok.all()) and bool(b.validate(n_slots=2).ok.all())
    b.clear()
    b.run()
    after = b.samples()
    assert before.keys() == after.keys() and int(before["action"].shape[0]) > 1000
    for k in before:
        assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    b.close()


def test_a_set_of_no_logs_gives_an_empty_report():
    from riichienv_amd.logset import LogSet

    for s in (LogSet.from_logs([], num_players=4), LogSet.from_text([], num_players=3)):
        rep = s.validate()
        assert len(rep) == 0 and rep.good_ids().size == 0 and set(rep.summary().values()) == {0} and rep.ok.shape == (0,)
        s.close()
