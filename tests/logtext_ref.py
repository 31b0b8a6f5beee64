"""The plain reference of the device MJAI text parser (rmj_logset_create_from_text) and the corpus it shares with the host test of the
scalar parser (tests/test_evparse_host.py): what the device must return for a set of logs, stated with bytes.split, json.loads,
abi.event_records_from_mjai and datasets.kyoku_tables, nothing of the parser's own.  tests/test_logtext_ref.py checks this module on the
CPU; tests/test_gpu_log_text_layouts.py holds the kernels to it.

The status of a line that does not parse is never derived here: it comes from the hand-classified table (BAD, _truncations) that
tests/test_evparse_host.py pins on the CPU, handed to expect() as known_status."""
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


def corpus():
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


def run_harness(tmp_path, flags, entries):
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


def walk_rule_logs():
    """(logs the kyoku walk must accept, logs on which MjaiReplay.from_events raises): deltas with the riichi sticks (reach_accepted for
    hora, reach for ryukyoku), consecutive horas, scores over deltas, events outside a kyoku"""
    sk = lambda **kw: _start_kyoku(**kw)  # noqa: E731
    good = {
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
    bad = {"no_actor": [sk(), {"type": "reach"}], "far_actor": [sk(), {"type": "dahai", "actor": 7, "pai": "1m"}],
           "no_target": [sk(), {"type": "pon", "actor": 1, "pai": "1m", "consumed": ["1m", "1m"]}]}
    return good, bad


# ---------------------------------------------------------------- the reference
BLANK = b" \t\r"
NONE_RECORDS = bytes(96)


def split_events(log_bytes):
    """[(start, end, line_no)] of a log's events: the lines between b"\n" that hold a byte other than space, tab, "\r"; start is the first
    such byte, end the position of the line's "\n" (the end of the log for a last line without one), line_no counts every line from 1"""
    out, pos = [], 0
    for no, line in enumerate(bytes(log_bytes).split(b"\n"), 1):
        body = line.lstrip(BLANK)
        if body:
            out.append((pos + len(line) - len(body), pos + len(line), no))
        pos += len(line) + 1
    return out


def status_table(num_players=4, masked_ok=False):
    """{line bytes: status} of the hand-classified bad lines of one (num_players, masked_ok) group"""
    out = {}
    for t, n, m, s in BAD + _truncations():
        t = (t if isinstance(t, bytes) else t.encode()).strip(BLANK)
        if (n, m) == (num_players, masked_ok) and t:
            assert out.setdefault(t, s) == s, t
    return out


def _walk_is_declined(evs):
    """the walks the header lists as declined (UNSUPPORTED) rather than decided: an end-of-round `scores` of another length than the kyoku's"""
    n = None
    for ev in evs:
        ty = ev.get("type")
        if ty == "start_kyoku":
            n = min(len(ev["scores"]), 4)
        elif ty in ("end_kyoku", "end_game"):
            n = None
        elif n is not None and ty in ("hora", "ryukyoku") and ev.get("scores") is not None and min(len(ev["scores"]), 4) != n:
            return True
    return False


def expect(logs_bytes, num_players=4, masked_ok=False, known_status=None):
    """What rmj_logset_create_from_text must return for the logs: events [N, 3, 32] uint8, offsets [M + 1], decisions / status / error_line
    [M], tables [M]: (start, end) [k, 4] int32 of every log whose status is OK (None for the others), and - when every log is OK -
    kyoku_offsets / start_scores / end_scores of the whole set (None otherwise).
    A line found in known_status with a status other than OK gives three NONE records and that status; every other line must load and pack
    (an exception here is a line the test forgot to classify)."""
    known = known_status or {}
    recs, offsets, decisions, status, error_line, tables = [], [0], [], [], [], []
    for log in logs_bytes:
        log = bytes(log)
        evs, st, line, dec = [], OK, 0, 0
        for s, e, no in split_events(log):
            text = log[s:e].rstrip(BLANK)
            k = known.get(text, OK)
            if k != OK:
                recs.append(NONE_RECORDS)
                if st == OK:
                    st, line = k, no
                continue
            ev = json.loads(text)
            recs.append(bytes(abi.event_records_from_mjai(ev, num_players, masked_ok)))
            evs.append(ev)
            dec += ev.get("type") in datasets._DECISION_TYPES
        offsets.append(len(recs))
        decisions.append(dec)
        tab = None
        if st == OK:
            if _walk_is_declined(evs):
                raise NotImplementedError("the reference does not decide a walk that the parser declines")
            try:
                tab = datasets.kyoku_tables([evs], num_players)
            except OverflowError:
                raise NotImplementedError("the reference does not decide a walk whose scores leave int32") from None
            except Exception:  # noqa: BLE001  (MjaiReplay.from_events raises: IndexError, TypeError, KeyError)
                st = ERR_REPLAY
        status.append(st)
        error_line.append(line)
        tables.append(tab)
    out = dict(events=np.frombuffer(b"".join(recs), np.uint8).reshape(-1, 3, 32), offsets=offsets, decisions=decisions, status=status, error_line=error_line,
               tables=tables, kyoku_offsets=None, start_scores=None, end_scores=None)
    if all(s == OK for s in status):
        out["kyoku_offsets"] = [0] + np.cumsum([len(t[0]) for t in tables], dtype=np.int64).tolist()
        out["start_scores"] = np.concatenate([t[0] for t in tables] + [np.zeros((0, 4), np.int32)])
        out["end_scores"] = np.concatenate([t[1] for t in tables] + [np.zeros((0, 4), np.int32)])
    return out


def jsonl(events, end=b"\n"):
    return b"\n".join(json.dumps(e).encode() for e in events) + (end if events else b"")


# ---------------------------------------------------------------- seeded soups for the kyoku walk
SOUP_SEED, N_SOUPS = 20260, 512


def walk_soups(seed=SOUP_SEED, n=N_SOUPS):
    """n short logs (5 to 150 events) drawn from the event forms the walk reads - legal play is not the point: the walk's rules are (what
    opens and closes a kyoku, which actor is a seat, what ends a batch of horas, deltas against scores).  Two logs in five draw only forms
    the walk accepts in a four-seat kyoku, one in five keeps its actors inside the kyoku it is in, the rest draw everything."""
    rng = random.Random(seed)
    soups = []
    for _ in range(n):
        mode = rng.choice(["four", "four", "seats", "any", "any"])
        seats, evs = None, []   # seats of the open kyoku
        for _ in range(rng.randrange(5, 151)):
            form = rng.choices(["start_kyoku", "tsumo", "dahai", "reach", "reach_accepted", "pon", "dora", "hora", "ryukyoku", "end_kyoku", "end_game"],
                               [4, 14, 30, 4, 4, 5, 6, 22, 4, 5, 1])[0]
            live = seats if (seats and mode != "any") else 4
            actor = rng.randrange(live)
            if form == "start_kyoku":
                k = 4 if mode == "four" else rng.choice([3, 4])
                base = 35000 if k == 3 else 25000
                seats = k
                evs.append(_start_kyoku(scores=[base + 100 * rng.randrange(-50, 50) for _ in range(k)], tehais=[_tehai()] * k, kyoku=rng.randrange(1, 5)))
            elif form == "tsumo":
                evs.append({"type": "tsumo", "actor": actor, "pai": "3s"})
            elif form == "dahai":
                ev = {"type": "dahai", "actor": actor, "pai": "7z", "tsumogiri": bool(rng.randrange(2))}
                if mode == "any" and rng.random() < 0.02:
                    del ev["actor"]
                evs.append(ev)
            elif form in ("reach", "reach_accepted"):
                ev = {"type": form, "actor": actor}
                if mode == "any" and rng.random() < 0.05:
                    del ev["actor"]
                evs.append(ev)
            elif form == "pon":
                ev = {"type": "pon", "actor": actor, "target": rng.randrange(4), "pai": "5p", "consumed": ["5pr", "5p"]}
                if mode == "any" and rng.random() < 0.1:
                    del ev["target"]
                evs.append(ev)
            elif form == "dora":
                evs.append({"type": "dora", "dora_marker": "2p"})
            elif form == "hora":
                k = seats or 4
                ev = {"type": "hora", "actor": actor, "target": rng.randrange(4)}
                kind = rng.choice(["deltas", "deltas", "delta", "scores", "none"])
                if kind == "scores":
                    ev["scores"] = [100 * rng.randrange(0, 600) for _ in range(k)]
                elif kind != "none":
                    ev[kind] = [100 * rng.randrange(-80, 80) for _ in range(rng.choice([k, k, 4, 2]))]
                evs.append(ev)
            elif form == "ryukyoku":
                ev = {"type": "ryukyoku"}
                if rng.randrange(3):
                    ev["deltas"] = [rng.choice([-3000, -1500, 0, 1500, 3000]) for _ in range(seats or 4)]
                evs.append(ev)
            else:
                seats = None
                evs.append({"type": form})
        soups.append(evs)
    return soups


def hora_then_dahai(evs):
    return any(a.get("type") == "hora" and b.get("type") == "dahai" for a, b in zip(evs, evs[1:]))
