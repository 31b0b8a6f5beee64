"""CPU: the reference of the device text parser (tests/logtext_ref.py) on its own - expect() against datasets.pack_logs and
datasets.kyoku_tables on the golden logs, split_events against the line numbers the spoiled-log test of the device expects, and the seeded
walk soups through the host build of rmjp::KyokuWalk (tests/evparse/evparse_check.cpp feeds the walk every event, the device only a
filtered subset: tests/test_gpu_log_text_layouts.py compares the two through this reference)."""
import json
import random
import struct

import numpy as np

from riichienv_amd import datasets

from tests import logtext_ref as R


def _golden_forms():
    """[(text, events)]: both golden logs as stored, as json.dumps writes them, and reshuffled with junk keys and ragged ends"""
    rng = random.Random(17)
    out = []
    for path in R.GOLDEN:
        raw = open(path, "rb").read()
        evs = [json.loads(l) for l in R._lines(path)]
        out.append((raw, evs))
        out.append((R.jsonl(evs, b""), evs))
        for end in (b"\n", b"\r\n", b"\n\n  \n\t\r\n"):
            out.append((b"\r\n \n".join(R._shuffled(e, rng).encode() for e in evs) + end, evs))
    return out


def test_expect_equals_the_host_packing_on_the_golden_logs():
    forms = _golden_forms()
    texts, logs = [t for t, _ in forms], [e for _, e in forms]
    want = R.expect(texts, 4)
    recs, off = datasets.pack_logs(logs, 4)
    n = int(off[-1])
    assert want["offsets"] == off.tolist() and n > 1000
    assert bytes(want["events"]) == bytes(recs)[: n * 96]
    start, end = datasets.kyoku_tables(logs, 4)
    assert want["status"] == [R.OK] * len(logs) and want["error_line"] == [0] * len(logs)
    assert want["start_scores"].tolist() == start.tolist() and want["end_scores"].tolist() == end.tolist()
    assert want["kyoku_offsets"][-1] == len(start) and len(start) >= 2 * len(R.GOLDEN)
    assert want["decisions"] == [sum(e.get("type") in datasets._DECISION_TYPES for e in l) for l in logs]


def test_split_events_counts_blank_lines_and_keeps_odd_bytes():
    assert R.split_events(b"") == [] and R.split_events(b"\n \t\r\n\r") == []
    assert R.split_events(b"{}") == [(0, 2, 1)] and R.split_events(b"{}\n") == [(0, 2, 1)]
    assert R.split_events(b"\n\n  {}\r\n{} ") == [(4, 7, 3), (8, 11, 4)]
    assert R.split_events(b"\f\n\v") == [(0, 1, 1), (2, 3, 2)]                      # form feed and vertical tab are not blank: events (ERR_JSON)
    # the spoiled logs of tests/test_gpu_log_text_ingest.py: line sk + 1 as it stands, line ts + 3 behind two inserted blank lines
    lines = R._lines(R.GOLDEN[0])
    evs = [json.loads(l) for l in lines]
    sk = next(k for k, e in enumerate(evs) if e["type"] == "start_kyoku")
    ts = next(k for k, e in enumerate(evs) if e["type"] == "tsumo")
    assert R.split_events(b"\n".join(lines))[sk][2] == sk + 1
    spoiled = list(lines)
    spoiled[ts] = b"\n\n" + spoiled[ts]
    got = R.split_events(b"\n".join(spoiled))
    assert got[ts][2] == ts + 3 and got[ts - 1][2] == ts and len(got) == len(lines)
    text = b"\n".join(spoiled)
    assert [text[s:e] for s, e, _ in got] == lines


def test_expect_takes_a_bad_lines_status_from_the_table():
    table = R.status_table(4, False)
    assert len(table) > 400 and set(table.values()) == {R.UNSUPPORTED, R.ERR_JSON, R.ERR_KEY, R.ERR_TEHAI, R.ERR_TILE, R.ERR_VALUE}
    good = b'{"type":"dora","dora_marker":"1m"}'
    log = good + b"\n\n" + b'{"type":"dora"}' + b"\n" + b'{"type":"tsumo","actor":1,"pai":"8z"}' + b"\r\n" + good
    want = R.expect([log, good], 4, False, table)
    assert want["status"] == [R.ERR_KEY, R.OK] and want["error_line"] == [3, 0] and want["offsets"] == [0, 4, 5]
    assert not want["events"][1:3].any() and want["events"][0].any() and bytes(want["events"][0]) == bytes(want["events"][3])
    assert want["tables"][0] is None and want["kyoku_offsets"] is None
    try:
        R.expect([b'{"type":"dora"}'], 4)      # an unclassified bad line is the test's mistake, not a status
    except KeyError:
        pass
    else:
        raise AssertionError("an unclassified bad line went through")


def test_walk_soups_meet_their_conditions_and_the_host_walk_agrees(tmp_path):
    soups = R.walk_soups()
    texts = [R.jsonl(s) for s in soups]
    want = R.expect(texts, 4)
    assert len(soups) == R.N_SOUPS and all(5 <= len(s) <= 150 for s in soups) and max(len(s) for s in soups) > 128
    assert set(want["status"]) == {R.OK, R.ERR_REPLAY}
    assert want["status"].count(R.OK) * 5 >= len(soups) and want["status"].count(R.ERR_REPLAY) * 5 >= len(soups)
    assert sum(R.hora_then_dahai(s) for s in soups) >= 30
    assert sum(R.hora_then_dahai(s) and st == R.OK for s, st in zip(soups, want["status"])) >= 30
    # the unfiltered walk of the host build, every event fed
    entries = [(json.dumps(e).encode(), 4, False, i == 0) for s in soups for i, e in enumerate(s)]
    _, tables = R.run_harness(tmp_path, ["-O2"], entries)
    at = 0
    for i, tab in enumerate(want["tables"]):
        k, st = struct.unpack_from("<II", tables, at)
        rows = np.frombuffer(tables, dtype=np.int32, count=k * 8, offset=at + 8).reshape(k, 2, 4)
        at += 8 + 32 * k
        assert st == want["status"][i], (i, st, want["status"][i])
        if tab is not None:
            assert rows[:, 0].tolist() == tab[0].tolist() and rows[:, 1].tolist() == tab[1].tolist(), i
    assert at == len(tables)
