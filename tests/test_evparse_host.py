"""CPU: the per-line MJAI parser that the device parser runs (riichienv_amd/csrc/rmj_evparse.h) compiled as host C++ with g++ and held to
abi.event_records_from_mjai(json.loads(line)) record for record, and its kyoku walk to datasets.kyoku_tables - once plain and once under
AddressSanitizer + UBSan, every line in a heap block of exactly its size (tests/evparse/evparse_check.cpp).

The corpus: every line of the two golden logs in four forms (as stored, json.dumps default, compact with sorted keys, keys shuffled with
injected unknown keys), synthetic events of every type and alias, and a list of bad lines with the status each must get.  On the good
lines the share reported UNSUPPORTED or ERR must be 0; no line is left out of the comparison."""
import ctypes as C
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from riichienv_amd import abi, datasets

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "evparse", "evparse_check.cpp")
GOLDEN = [os.path.join(HERE, "golden", n) for n in ("126_204_0_mjai.jsonl", "ui_example_after_injection.jsonl")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
OK, UNSUPPORTED, ERR_JSON, ERR_KEY, ERR_TEHAI, ERR_TILE, ERR_VALUE, ERR_REPLAY = range(8)
CLS = {"start_kyoku": 1, "hora": 2, "ryukyoku": 3, "reach": 4, "reach_accepted": 5, "end_kyoku": 6, "end_game": 6, "dahai": 7, "chi": 8, "pon": 8,
       "daiminkan": 8, "kan": 8}
JUNK = [("meta", {"a": [1, 2, {"b": None}], "c": "x"}), ("note", 'quote \" backslash \\ newline \n brace { bracket ]'), ("名前", "東風戦 ✓"),
        ("nested", [[[], {}], {"k": [True, False, None, -1.5e-3, 0]}]), ("num", -12.5), ("flag", True), ("nil", None), ("e", 1e300)]


def _lines(path):
    with open(path, "rb") as f:
        return [l.rstrip(b"\n") for l in f.read().split(b"\n") if l.strip()]


def _shuffled(ev, rng):
    items = list(ev.items()) + rng.sample(JUNK, 3)
    rng.shuffle(items)
    sep = rng.choice([(",", ":"), (", ", ": "), (" ,\t", " :  ")])
    return json.dumps(dict(items), separators=sep, ensure_ascii=False)   # UTF-8 names stay UTF-8: an escaped key is declined (UNSUPPORTED)


def _tehai(n=13):
    return ["1m", "2m", "3m", "4p", "5pr", "6p", "7s", "8s", "9s", "E", "S", "P", "C", "1z", "7z"][:n]


def _start_kyoku(**kw):
    ev = {"type": "start_kyoku", "bakaze": "S", "dora_marker": "5sr", "kyoku": 3, "honba": 2, "kyotaku": 1, "oya": 2, "scores": [25000, 24000, 26000, 25000],
          "tehais": [_tehai(), _tehai(), _tehai(), _tehai()]}
    ev.update(kw)
    return ev


def _synthetic():
    """(event, num_players, masked_ok) of every type, alias and optional-field form"""
    out = []
    add = lambda ev, np_=4, masked=False: out.append((ev, np_, masked))  # noqa: E731
    add({"type": "start_game"})
    add({"type": "start_game", "names": ["a", "b", "c", "d"], "kyoku_first": 0, "aka_flag": True})
    add(_start_kyoku())
    add(_start_kyoku(kyoutaku=300, kyotaku=2))
    k = _start_kyoku()
    del k["kyotaku"]
    add(k)
    add(_start_kyoku(scores=[35000, 35000, 35000], tehais=[_tehai(), _tehai(), _tehai()], bakaze="E"), 3)
    add(_start_kyoku(scores=[35000, 35000, 35000], tehais=[_tehai(), _tehai(), _tehai(), ["?"] * 2]), 3)   # a fourth entry is not looked at in 3P
    add(_start_kyoku(tehais=[_tehai(), ["?"] * 13, ["?"] * 13, ["?"] * 13]), 4, True)
    add(_start_kyoku(tehais=[_tehai(), _tehai()], scores=[-2147483648, 2147483647, 0, -1, 5]))
    add(_start_kyoku(bakaze="N", dora_marker="0m", kyoku=255, honba=255, kyotaku=65535, oya=0))
    for tile in ["1m", "5m", "5mr", "0p", "9s", "E", "C", "1z", "7z", "5sr", "1mX", "3pqq"]:
        add({"type": "tsumo", "actor": 1, "pai": tile})
    add({"type": "tsumo", "actor": 3, "pai": "?"}, 4, True)
    add({"type": "tsumo", "actor": 3, "pai": "8z"}, 4, True)
    add({"type": "tsumo", "pai": "2s"})
    add({"type": "tsumo", "actor": None, "pai": "2s"})
    add({"type": "tsumo", "actor": False, "pai": "2s"})
    add({"type": "dahai", "actor": 2, "pai": "N", "tsumogiri": True})
    add({"type": "dahai", "actor": 2, "pai": "N", "tsumogiri": False})
    add({"type": "dahai", "actor": 2, "pai": "N", "tsumogiri": None})
    add({"type": "dahai", "actor": 255, "pai": "N"})
    add({"type": "reach", "actor": 1})
    add({"type": "reach_accepted", "actor": 1, "deltas": [0, -1000, 0, 0], "scores": [1, 2, 3, 4]})
    add({"type": "pon", "actor": 0, "target": 2, "pai": "5p", "consumed": ["5pr", "5p"]})
    add({"type": "chi", "actor": 0, "target": 3, "pai": "4s", "consumed": ["5sr", "6s"]})
    add({"type": "chi", "actor": 0, "target": None, "pai": "4s", "consumed": []})
    add({"type": "pon", "actor": 0, "pai": "4s", "consumed": ["4s", "4s"]})
    add({"type": "daiminkan", "actor": 1, "target": 0, "pai": "P", "consumed": ["P", "P", "P"]})
    add({"type": "kan", "actor": 1, "target": 0, "pai": "P", "consumed": ["P", "P", "P"]})
    add({"type": "ankan", "actor": 1, "consumed": ["F", "F", "F", "F"]})
    add({"type": "ankan", "actor": 1, "consumed": ["F", "F", "F", "F", "1m", "2m"], "pai": 7})
    add({"type": "kakan", "actor": 1, "pai": "5mr", "consumed": ["5m", "5m", "5m"]})
    add({"type": "dora", "dora_marker": "3z"})
    add({"type": "kita", "actor": 2, "pai": "N"}, 3)
    add({"type": "hora", "actor": 1, "target": 2, "deltas": [0, 8000, -8000, 0], "ura_markers": ["1m"]})
    add({"type": "hora", "actor": 1, "target": 1, "delta": [-2000, 6000, -2000, -2000], "uradora_markers": []})
    add({"type": "hora", "actor": 1, "target": 1, "deltas": None, "delta": [1, 2, 3, 4]})
    add({"type": "hora", "actor": 1, "target": 2, "scores": [1, 2, 3, 4], "deltas": ["x"], "pai": 5, "han": 3, "fu": 30})
    add({"type": "hora", "actor": 1, "target": 2, "scores": None, "deltas": [1, 2, 3]})
    add({"type": "ryukyoku", "deltas": [1500, -1500, 1500, -1500], "reason": "exhaustive_draw"})
    add({"type": "ryukyoku", "actor": 2, "scores": [25000, 25000, 25000, 25000]})
    add({"type": "ryukyoku"})
    add({"type": "end_kyoku"})
    add({"type": "end_game", "scores": [1, 2, 3, 4]})
    add({"type": "none_of_these", "actor": 3, "pai": "zz", "tehais": [["q"]], "scores": "no", "consumed": 5})
    add({"actor": 2})
    add({})
    add({"type": None, "actor": 1})
    add({"type": 7})
    add({"type": "tsümo", "actor": 1, "pai": "1m"})
    return out


BAD = [  # (text, num_players, masked_ok, status)
    (json.dumps(_start_kyoku(tehais=[_tehai(), _tehai(12), _tehai(), _tehai()])), 4, False, ERR_TEHAI),
    (json.dumps(_start_kyoku(tehais=[_tehai(), _tehai(), _tehai(), _tehai(14)])), 4, False, ERR_TEHAI),
    (json.dumps(_start_kyoku(tehais=[_tehai(), _tehai(), _tehai(), _tehai(12)])), 4, True, ERR_TEHAI),
    (json.dumps(_start_kyoku(tehais=[_tehai(), _tehai(), _tehai(), ["?"] * 13])), 4, False, ERR_TILE),
    ('{"type":"tsumo","actor":1,"pai":"8z"}', 4, False, ERR_TILE),
    ('{"type":"tsumo","actor":1,"pai":"xx"}', 4, False, ERR_TILE),
    ('{"type":"pon","actor":1,"target":0,"pai":"1m","consumed":["1m","1x"]}', 4, False, ERR_TILE),
    ('{"type":"ankan","actor":1,"consumed":["1m","1m","1m","1m","zz"]}', 4, False, ERR_TILE),
    ('{"type":"tsumo","actor":1.5,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1.0,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1e0,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":256,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":-1,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":"1","pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":true,"pai":"1m"}', 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(kyoku=300)), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(kyotaku=65536)), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(scores=[25000, 2147483648, 0, 0])), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(scores=[25000.0, 1, 0, 0])), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(bakaze="X")), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(bakaze="ES")), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(bakaze="")), 4, False, UNSUPPORTED),
    (json.dumps(_start_kyoku(honba=None)), 4, False, ERR_VALUE),
    ('{"ty\\u0070e":"tsumo","actor":1,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1,"pai":"1m","x\\ny":1}', 4, False, UNSUPPORTED),
    ('{"type":"ts\\u0075mo","actor":1,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1,"pai":"1\\u006d"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1,"pai":"1m","pai":"2m"}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","type":"dahai","actor":1,"pai":"1m"}', 4, False, UNSUPPORTED),
    ('{"type":"dahai","actor":1,"pai":"1m","tsumogiri":1}', 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1,"pai":7}', 4, False, UNSUPPORTED),
    ('{"type":["tsumo"]}', 4, False, UNSUPPORTED),
    ('{"type":"hora","actor":1,"deltas":[1.5,0,0,0]}', 4, False, UNSUPPORTED),
    ('{"type":"x","k":' + "[" * 70 + "]" * 70 + "}", 4, False, UNSUPPORTED),
    ('{"type":"tsumo","actor":1}', 4, False, ERR_KEY),
    ('{"type":"dora"}', 4, False, ERR_KEY),
    ('{"type":"pon","actor":1,"pai":"1m"}', 4, False, ERR_KEY),
    (json.dumps({k: v for k, v in _start_kyoku().items() if k != "oya"}), 4, False, ERR_KEY),
    (json.dumps({k: v for k, v in _start_kyoku().items() if k != "tehais"}), 4, False, ERR_KEY),
    (json.dumps({k: v for k, v in _start_kyoku().items() if k != "bakaze"}), 4, False, ERR_KEY),
    ('{"type":"tsumo","actor":1,"pai":"1m"} x', 4, False, ERR_JSON),
    ('{"type":"tsumo","actor":1,"pai":"1m",}', 4, False, ERR_JSON),
    ('{"type":"tsumo","actor":01,"pai":"1m"}', 4, False, ERR_JSON),
    ('{"type":"tsumo" "actor":1}', 4, False, ERR_JSON),
    ("{'type':'tsumo'}", 4, False, ERR_JSON),
    ('{"type":"a\tb"}', 4, False, ERR_JSON),
    ('{"type":"a\\qb"}', 4, False, ERR_JSON),
    ('{"type":"a","u":"\\u12g4"}', 4, False, ERR_JSON),
    ('{"type":"a","u":[1,2}', 4, False, ERR_JSON),
    ('{"type":"a","u":{"k":1]}', 4, False, ERR_JSON),
    ('{"type":"a","u":tru}', 4, False, ERR_JSON),
    ('{"type":"a","u":-}', 4, False, ERR_JSON),
    ('{"type":"a","u":1.}', 4, False, ERR_JSON),
    ('{"type":"a","u":-NaN}', 4, False, ERR_JSON),
    ('["type"]', 4, False, ERR_JSON),
    ("17", 4, False, ERR_JSON),
    ("", 4, False, ERR_JSON),
    (b'{"type":"a","u":"\xff"}', 4, False, ERR_JSON),
    (b'{"type":"a","u":"\xe0\x80\x80"}', 4, False, ERR_JSON),
    (b'{"type":"a","u":"\xc3"}', 4, False, ERR_JSON),
]


def _truncations():
    out = []
    for text in (json.dumps(_start_kyoku()), '{"type":"pon","actor":0,"target":2,"pai":"5p","consumed":["5pr","5p"]}'):
        out += [(text[:k], 4, False, ERR_JSON) for k in range(len(text))]
    return out


def _python_status(text, np_, masked):
    """what the host path does with the line: 'ok' or the exception"""
    try:
        abi.event_records_from_mjai(json.loads(text), np_, masked)
        return "ok"
    except Exception as e:  # noqa: BLE001
        return type(e).__name__


def _corpus():
    """good: [(bytes, np, masked, event dict, first_of_log)], bad: [(bytes, np, masked, status)]"""
    rng = random.Random(5)
    good = []
    for path in GOLDEN:
        raw = _lines(path)
        evs = [json.loads(l) for l in raw]
        forms = [raw, [json.dumps(e).encode() for e in evs], [json.dumps(e, separators=(",", ":"), sort_keys=True).encode() for e in evs],
                 [_shuffled(e, rng).encode() for e in evs]]
        for form in forms:
            assert len(form) == len(evs)
            good += [(l, 4, False, e, i == 0) for i, (l, e) in enumerate(zip(form, evs))]
    for ev, np_, masked in _synthetic():
        dumps = lambda e, **kw: json.dumps(e, ensure_ascii=False, **kw)   # noqa: E731  (an escape inside a type string is declined, by design)
        for text in (dumps(ev), dumps(ev, separators=(",", ":"), sort_keys=True), _shuffled(ev, rng), "  \t" + dumps(ev) + " \r"):
            good.append((text.encode(), np_, masked, ev, True))   # every synthetic line is a log of its own for the walk
    bad = [(t if isinstance(t, bytes) else t.encode(), n, m, s) for t, n, m, s in BAD + _truncations()]
    return good, bad


def _run(tmp_path, flags, entries):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "evparse_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", exe], check=True)
    corpus, out = str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(entries)))
        for text, np_, masked, first in entries:
            f.write(struct.pack("<IBBBB", len(text), np_, 1 if masked else 0, 1 if first else 0, 0) + text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "evparse OK" in r.stdout
    raw = np.fromfile(out, dtype=np.uint8).reshape(len(entries), 136)
    with open(out + ".tables", "rb") as f:
        tables = f.read()
    return raw, tables


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
    sk = lambda **kw: _start_kyoku(**kw)  # noqa: E731
    logs = {
        "double_ron": [{"type": "start_game"}, {"type": "hora", "actor": 0, "deltas": [9, 9, 9, 9]}, sk(), {"type": "reach", "actor": 1},
                       {"type": "dahai", "actor": 1, "pai": "1m", "tsumogiri": False}, {"type": "reach_accepted", "actor": 1}, {"type": "reach", "actor": 3},
                       {"type": "hora", "actor": 0, "target": 1, "deltas": [3000, -2000, 0, 0]}, {"type": "hora", "actor": 2, "target": 1, "deltas": [0, -8000, 8000, 0]},
                       {"type": "end_kyoku"}, {"type": "hora", "actor": 0, "deltas": [1, 1, 1, 1]}],
        "draw": [sk(), {"type": "reach", "actor": 2}, {"type": "ryukyoku", "deltas": [1500, -1500, 1500, -1500]}, {"type": "end_kyoku"}, sk(scores=[1, 2, 3, 4]),
                 {"type": "hora", "actor": 1, "scores": [5, 6, 7, 8], "deltas": [1, 1, 1, 1]}, {"type": "dora", "dora_marker": "1m"},
                 {"type": "hora", "actor": 1, "delta": [10, 0, 0]}],
        "three": [sk(scores=[35000, 35000, 35000], tehais=[_tehai()] * 3), {"type": "reach_accepted", "actor": 0}, {"type": "hora", "actor": 0, "deltas": [100, 200]}],
        "none": [{"type": "start_game"}, {"type": "end_game"}],
    }
    for name, evs in logs.items():
        st, rows = _walk(tmp_path, evs, name)
        start, end = datasets.kyoku_tables([evs], 4)
        assert st == OK, name
        assert rows[:, 0].tolist() == start.tolist() and rows[:, 1].tolist() == end.tolist(), (name, rows.tolist(), end.tolist())
    # where MjaiReplay.from_events raises, the walk reports it
    for name, evs in {"no_actor": [sk(), {"type": "reach"}], "far_actor": [sk(), {"type": "dahai", "actor": 7, "pai": "1m"}],
                      "no_target": [sk(), {"type": "pon", "actor": 1, "pai": "1m", "consumed": ["1m", "1m"]}]}.items():
        with pytest.raises(Exception):  # noqa: B017
            datasets.kyoku_tables([evs], 4)
        assert _walk(tmp_path, evs, name)[0] == ERR_REPLAY, name
