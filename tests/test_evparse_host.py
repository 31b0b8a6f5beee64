"""CPU: the per-line MJAI parser that the device parser runs (riichienv_amd/csrc/rmj_evparse.h) compiled as host C++ with g++ and held to
abi.event_records_from_mjai(json.loads(line)) record for record, and its kyoku walk to datasets.kyoku_tables - once plain and once under
AddressSanitizer + UBSan, every line in a heap block of exactly its size (tests/evparse/evparse_check.cpp).

The corpus: every line of the two golden logs in four forms (as stored, json.dumps default, compact with sorted keys, keys shuffled with
injected unknown keys), synthetic events of every type and alias, and a list of bad lines with the status each must get.  On the good
lines the share reported UNSUPPORTED or ERR must be 0; no line is left out of the comparison."""
import json
import struct

import numpy as np
import pytest

from riichienv_amd import abi, datasets

# the corpus and the harness live in tests/logtext_ref.py: the device tests (tests/test_gpu_log_text_layouts.py) run the same lines
from tests.logtext_ref import CLS, ERR_REPLAY, GOLDEN, OK, SAN, UNSUPPORTED, _lines, corpus as _corpus, run_harness as _run, walk_rule_logs


def _python_status(text, np_, masked):
    """what the host path does with the line: 'ok' or the exception"""
    try:
        abi.event_records_from_mjai(json.loads(text), np_, masked)
        return "ok"
    except Exception as e:  # noqa: BLE001
        return type(e).__name__


def _side(row):
    b = bytes(row[96:])
    scores, deltas = struct.unpack("<4i", b[:16]), struct.unpack("<4i", b[16:32])
    cls, flags, n_scores, n_deltas, status, actor = b[32:38]
    return dict(scores=list(scores), deltas=list(deltas), cls=cls, flags=flags, n_scores=n_scores, n_deltas=n_deltas, status=status, actor=actor)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_evparse_equals_the_packer(tmp_path, flags):
    good, bad = _corpus()
    entries = [(t, n, m, f) for t, n, m, _, f in good] + [(t, n, m, False) for t, n, m, _ in bad]
    raw, tables = _run(tmp_path, flags, entries)
    # ---- good lines: bit-equal records, the side struct, and not one UNSUPPORTED / ERR
    failed = 0
    for i, (text, np_, masked, ev, _) in enumerate(good):
        side = _side(raw[i])
        failed += side["status"] != OK
        assert side["status"] == OK, (i, text, side)
        want = bytes(abi.event_records_from_mjai(json.loads(text), np_, masked))
        assert bytes(raw[i, :96]) == want, (i, text)
        assert want == bytes(abi.event_records_from_mjai(ev, np_, masked))
        ty = ev.get("type")
        assert side["cls"] == (CLS.get(ty, 0) if isinstance(ty, str) else 0), (i, text, side)
        assert bool(side["flags"] & 4) == (ty in datasets._DECISION_TYPES), (i, text)
        assert bool(side["flags"] & 8) == (ev.get("actor") is None), (i, text)
        if ty in ("start_kyoku", "hora", "ryukyoku"):
            sc = ev.get("scores")
            assert bool(side["flags"] & 1) == (sc is not None), (i, text)
            if sc is not None:
                assert side["n_scores"] == len(sc) and side["scores"] == (list(sc) + [0] * 4)[:4], (i, text, side)
        if ty in ("hora", "ryukyoku") and ev.get("scores") is None:
            d = ev.get("deltas", ev.get("delta"))
            assert bool(side["flags"] & 2) == (d is not None), (i, text)
            if d is not None:
                assert side["n_deltas"] == min(len(d), 4) and side["deltas"] == (list(d) + [0] * 4)[:4], (i, text, side)
    assert failed == 0 and len(good) > 4 * 1000
    # ---- bad lines: the status each must get, NONE records, and the host path agrees on which side of the line they fall
    for j, (text, np_, masked, status) in enumerate(bad):
        row = raw[len(good) + j]
        side = _side(row)
        assert side["status"] == status, (text, side, status)
        assert not row[:96].any(), text
        py = _python_status(text, np_, masked)
        if status == UNSUPPORTED:
            assert py != "JSONDecodeError", (text, py)      # valid JSON that the parser declines
        else:
            assert py != "ok", (text, py)                    # the host path raises too
    # ---- the kyoku walk over every form of the golden logs = datasets.kyoku_tables
    at = 0
    for path in GOLDEN:
        evs = [json.loads(l) for l in _lines(path)]
        start, end = datasets.kyoku_tables([evs], 4)
        for _ in range(4):
            k, st = struct.unpack_from("<II", tables, at)
            rows = np.frombuffer(tables, dtype=np.int32, count=k * 8, offset=at + 8).reshape(k, 2, 4)
            at += 8 + 32 * k
            assert st == OK and k == len(start)
            assert rows[:, 0].tolist() == start.tolist() and rows[:, 1].tolist() == end.tolist()


def _walk(tmp_path, events, name):
    entries = [(json.dumps(e).encode(), 4, False, i == 0) for i, e in enumerate(events)]
    d = tmp_path / name
    d.mkdir()
    _, tables = _run(d, ["-O2"], entries)
    k, st = struct.unpack_from("<II", tables, 0)
    return st, np.frombuffer(tables, dtype=np.int32, count=k * 8, offset=8).reshape(k, 2, 4)


def test_kyoku_walk_rules(tmp_path):
    """deltas with the riichi sticks (reach_accepted for hora, reach for ryukyoku), consecutive horas, scores over deltas, events outside a kyoku"""
    logs, raising = walk_rule_logs()
    for name, evs in logs.items():
        st, rows = _walk(tmp_path, evs, name)
        start, end = datasets.kyoku_tables([evs], 4)
        assert st == OK, name
        assert rows[:, 0].tolist() == start.tolist() and rows[:, 1].tolist() == end.tolist(), (name, rows.tolist(), end.tolist())
    # where MjaiReplay.from_events raises, the walk reports it
    for name, evs in raising.items():
        with pytest.raises(Exception):  # noqa: B017
            datasets.kyoku_tables([evs], 4)
        assert _walk(tmp_path, evs, name)[0] == ERR_REPLAY, name
