"""Host side of the log sample builder (riichienv_amd.datasets): the event stream, the slot assignment, the table of powers, the rank
restatement, the exported symbols and the argument errors - none of it needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from riichienv_amd import abi, datasets, replay, vecenv

LOG = os.path.join(os.path.dirname(__file__), "golden", "126_204_0_mjai.jsonl")
NEW = ["rmj_logset_create", "rmj_logset_destroy", "rmj_logset_info", "rmj_logreplay_assign", "rmj_logreplay_create", "rmj_logreplay_destroy",
       "rmj_logreplay_run_device", "rmj_logreplay_finalize_device", "rmj_logreplay_emit_device", "rmj_logreplay_views", "rmj_logreplay_counts",
       "rmj_logreplay_clear"]


def test_the_stream_is_the_existing_packing_event_by_event():
    events = replay.load_mjai_jsonl(LOG)
    logs = [events, events[:37], [], events[100:400]]
    recs, off = datasets.pack_logs(logs)
    assert off.tolist() == [0, len(events), len(events) + 37, len(events) + 37, len(events) + 337]
    size = abi.EVENT_SLOTS * C.sizeof(abi.Event)
    raw = bytes(recs)
    assert len(raw) == int(off[-1]) * size
    at = 0
    for log in logs:
        for ev in log:
            assert raw[at * size: (at + 1) * size] == bytes(abi.event_records_from_mjai(ev, 4)), (at, ev)
            at += 1
    # an MjaiReplay goes through the same door
    recs2, off2 = datasets.pack_logs([replay.MjaiReplay.from_events(events)])
    assert bytes(recs2) == raw[: len(events) * size] and off2.tolist() == [0, len(events)]


def _assign_restated(lengths, n):
    busy, lists = [0] * n, [[] for _ in range(n)]
    for i, ln in enumerate(lengths):
        s = min(range(n), key=lambda j: (busy[j], j))
        busy[s] += ln
        lists[s].append(i)
    return lists, max(busy) if busy else 0


def test_slot_assignment_is_a_function_of_the_lengths():
    rng = np.random.default_rng(1)
    for m, n in ((1, 1), (6, 3), (40, 40), (97, 8), (500, 3)):
        lengths = rng.integers(0, 2000, size=m)
        slot_of, lists, steps = datasets.assign_slots(lengths, n)
        want, want_steps = _assign_restated(lengths.tolist(), n)
        assert lists == want and steps == want_steps
        assert [int(slot_of[i]) for l in lists for i in l] == [s for s, l in enumerate(lists) for _ in l]
        assert sorted(i for l in lists for i in l) == list(range(m))
        assert datasets.assign_slots(lengths, n)[1] == lists
    assert datasets.assign_slots([5, 3, 9, 2, 2, 7], 3)[1:] == ([[0, 4], [1, 3, 5], [2]], 12)
    with pytest.raises(vecenv.RmjError, match="n_slots"):
        datasets.assign_slots([3, 4], 3)


def test_powers_and_ranks():
    p = datasets.gamma_powers(0.99, 300)
    assert p.dtype == np.float64 and all(float(p[k]) == 0.99 ** k for k in range(300))
    sc = [[25000, 25000, 30000, 20000], [0, 0, 0, 0], [100, 300, 200, 300], [35000, 35000, 35000, 0]]
    assert datasets.compute_rank(sc, 4).tolist() == [[1, 2, 0, 3], [0, 1, 2, 3], [3, 0, 2, 1], [0, 1, 2, 3]]
    assert datasets.compute_rank(sc, 3).tolist() == [[1, 2, 0], [0, 1, 2], [2, 0, 1], [0, 1, 2]]
    for row in sc:    # mjai_logs.py:14-17, restated
        s = np.array(row, dtype=np.float64)
        assert datasets.compute_rank([row], 4)[0].tolist() == (-s).argsort(kind="stable").argsort(kind="stable").tolist()


def test_kyoku_tables_of_the_real_log():
    events = replay.load_mjai_jsonl(LOG)
    start, end = datasets.kyoku_tables([events], 4)
    starts = [e["scores"] for e in events if e["type"] == "start_kyoku"]
    assert start.tolist() == starts and end[:-1].tolist() == starts[1:]


def test_new_symbols_are_in_the_library_and_the_package():
    lib = vecenv.load_lib()
    for sym in NEW:
        assert sym in vecenv.EXPORTS and getattr(lib, sym) is not None
    import riichienv_amd

    assert riichienv_amd.LogSampleBuilder is datasets.LogSampleBuilder


def test_argument_errors():
    events = replay.load_mjai_jsonl(LOG)
    with pytest.raises(ValueError, match="feature set"):
        datasets.LogSampleBuilder([events], features="nope")
    with pytest.raises(ValueError, match="capacity"):
        datasets.LogSampleBuilder([events], capacity=0)
    with pytest.raises(ValueError, match="n_slots"):
        datasets.LogSampleBuilder([events], n_slots=2)
    with pytest.raises(ValueError, match="rule"):
        datasets.LogSampleBuilder([events], rule="other")
