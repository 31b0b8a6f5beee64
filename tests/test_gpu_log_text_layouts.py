"""GPU: the device MJAI text parser (rmj_logset_create_from_text: k_lt_lines, k_lt_scan, k_lt_parse, k_lt_tables) on the layouts that
well-formed game logs never have, bit for bit against the plain reference tests/logtext_ref.py (expect(): bytes.split, json.loads,
abi.event_records_from_mjai, datasets.kyoku_tables; the status of a bad line from the hand-classified table the host test pins).

One test or parametrised group per mechanism, so that a failure names it: the host parser's corpus on the device (and more than 1 024
logs through k_lt_scan), the LDS and the global-memory side of k_lt_parse around LT_LDS_TEXT, the 1 024-byte tile seams of the line
census, the 64-event seams of the parse and the table walk, the walk's filtered feed, the first error across chunks, device-resident text
at an odd address.  Log bases at chosen offsets of a 16-byte line: the upload starts at the lowest range, so a one-byte log sits at 0."""
import json

import numpy as np
import pytest

from riichienv_amd import datasets

from tests import logtext_ref as R

pytestmark = pytest.mark.gpu
DORA = b'{"type":"dora","dora_marker":"1m"}'
ERR_TILE_LINE, ERR_KEY_LINE, ERR_JSON_LINE = b'{"type":"tsumo","actor":1,"pai":"8z"}', b'{"type":"dora"}', b'{"type":"a","u":[1,2}'
LT_LDS_TEXT = 16384
_CACHE = {}


def _golden_lines(i=0):
    if i not in _CACHE:
        _CACHE[i] = R._lines(R.GOLDEN[i])
    return _CACHE[i]


def _fetch(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _place(logs, bases):
    """(buffer, ranges): log i begins at an address that is bases[i] past a multiple of 16, bytes that are no log's in between"""
    assert bases[0] == 0 and len(bases) == len(logs)
    buf, ranges = bytearray(), []
    for log, b in zip(logs, bases):
        buf += b'"{\n'
        while len(buf) % 16 != b:
            buf += b"}"
        if not ranges:
            buf = bytearray()      # the first log is the base of the upload
        ranges.append((len(buf), len(buf) + len(log)))
        buf += log
    return bytes(buf) + b'\n{"', np.array(ranges, np.uint64)


def _parse(logs, num_players=4, masked_ok=False, bases=None):
    if bases is None:
        return _fetch(datasets.parse_logs_device(logs, num_players=num_players, masked_ok=masked_ok))
    buf, ranges = _place(logs, bases)
    for (b, e), log in zip(ranges.tolist(), logs):
        assert buf[b:e] == log
    return _fetch(datasets.parse_logs_device(buf, ranges, num_players=num_players, masked_ok=masked_ok))


def _same(got, want, what):
    """bit for bit: offsets, records, decisions, status, error_line of every log, the table rows of every log that is OK"""
    assert got["offsets"].tolist() == want["offsets"], what
    g, w = got["events"], want["events"]
    assert g.shape == w.shape, what
    if not (g == w).all():
        i = int(np.flatnonzero((g != w).any(axis=(1, 2)))[0])
        raise AssertionError(f"{what}: event {i}: {bytes(g[i]).hex()} != {bytes(w[i]).hex()}")
    for k in ("status", "error_line", "decisions"):
        if got[k].tolist() != want[k]:
            i = next(i for i, (a, b) in enumerate(zip(got[k].tolist(), want[k])) if a != b)
            raise AssertionError(f"{what}: {k} of log {i}: {got[k][i]} != {want[k][i]}")
    koff = got["kyoku_offsets"].tolist()
    assert koff[0] == 0 and koff[-1] == len(got["start_scores"]) == len(got["end_scores"]), what
    for l, tab in enumerate(want["tables"]):
        if tab is not None:
            assert got["start_scores"][koff[l]: koff[l + 1]].tolist() == tab[0].tolist(), (what, l, "start")
            assert got["end_scores"][koff[l]: koff[l + 1]].tolist() == tab[1].tolist(), (what, l, "end")
    if want["kyoku_offsets"] is not None:
        assert koff == want["kyoku_offsets"], what


def _check(logs, what, num_players=4, masked_ok=False, known=None, bases=None):
    want = R.expect(logs, num_players, masked_ok, known)
    got = _parse(logs, num_players, masked_ok, bases)
    _same(got, want, what)
    return got, want


# ---------------------------------------------------------------- a. the host parser's corpus on the device
GROUPS = [(4, False), (3, False), (4, True)]


def _group(num_players, masked_ok):
    good, bad = R.corpus()
    g = [(t, ev) for t, n, m, ev, _ in good if (n, m) == (num_players, masked_ok)]
    b = [(t, s) for t, n, m, s in bad if (n, m) == (num_players, masked_ok)]
    return g, b


@pytest.mark.parametrize("num_players,masked_ok", GROUPS)
def test_corpus_one_line_per_log(num_players, masked_ok):
    good, bad = _group(num_players, masked_ok)
    known = R.status_table(num_players, masked_ok)
    logs, kind = [b"", b" \n\t\r\n", b""], ["empty"] * 3
    for i, (t, tag) in enumerate([(t, "good") for t, _ in good] + [(t, s) for t, s in bad]):
        if i % 97 == 50:                       # empty logs and logs of blank lines between the full ones
            logs += [b"", b"\n\n \r\n"]
            kind += ["empty"] * 2
        logs.append(t + (b"\n" if i % 3 else b""))
        kind.append(tag)
    logs += [b"\r\n", b"", b""]
    kind += ["empty"] * 3
    if (num_players, masked_ok) == (4, False):
        assert len(logs) > 4 * 1024 and len(logs) % 1024, "k_lt_scan: several logs per thread and a ragged last thread"
    got, want = _check(logs, "one line per log", num_players, masked_ok, known)
    # what the reference said, spelled out
    off = want["offsets"]
    for l, tag in enumerate(kind):
        n = off[l + 1] - off[l]
        if tag == "empty" or not logs[l].strip(b" \t\r\n"):
            assert n == 0 and got["status"][l] == R.OK and got["error_line"][l] == 0, l      # BAD's empty string: no event at all
        elif tag == "good":
            assert n == 1 and got["status"][l] == R.OK and got["error_line"][l] == 0, (l, logs[l])
        else:
            assert n == 1 and got["status"][l] == tag and got["error_line"][l] == 1 and not got["events"][off[l]].any(), (l, logs[l])
    assert kind.count("good") == len(good) and len(kind) == len(logs)


@pytest.mark.parametrize("num_players,masked_ok", GROUPS)
def test_corpus_concatenated_200_lines_to_a_log(num_players, masked_ok):
    """the golden lines in the order of their logs; the synthetic lines - a soup no walk was ever pinned on - each closed by an end_kyoku, so
    that every start_kyoku gives a row and nothing else is inside a kyoku (the walk has its own tests below)"""
    good, _ = _group(num_players, masked_ok)
    n_golden = 4 * sum(len(_golden_lines(i)) for i in range(2)) if (num_players, masked_ok) == (4, False) else 0
    golden, synth = [t for t, _ in good[:n_golden]], [t for t, _ in good[n_golden:]]
    assert len(golden) + len(synth) == len(good) and len(synth) > 0
    logs = [b"\n".join(golden[i: i + 200]) + b"\n" for i in range(0, len(golden), 200)]
    logs += [b"".join(t + b'\n{"type":"end_kyoku"}\r\n' for t in synth[i: i + 200]) for i in range(0, len(synth), 200)]
    got, want = _check(logs, "200 lines to a log", num_players, masked_ok)
    assert want["status"] == [R.OK] * len(logs) and want["offsets"][-1] == len(golden) + 2 * len(synth)
    if golden:
        assert want["kyoku_offsets"][-1] > 8


# ---------------------------------------------------------------- b. the LDS side and the global side of k_lt_parse
def _inflated(lines, target, way, bad_at=None):
    """130 events whose first 64-event chunk spans exactly `target` bytes (first byte of event 0 to the newline of event 63)"""
    lines = list(lines[:130])
    if bad_at is not None:
        lines[bad_at] = ERR_KEY_LINE
    span = sum(len(l) for l in lines[:64]) + 63
    pad = target - span
    assert pad >= 16
    if way == "junk":
        assert lines[10].endswith(b"}")
        lines[10] = lines[10][:-1] + b',"zz":"' + b"a" * (pad - 8) + b'"}'
    else:
        lines[30] = lines[30] + b"\n" + (b" \r\n\t\n\n  \t" * (pad // 8 + 1))[: pad - 2] + b" "
    log = b"\n".join(lines) + b"\n"
    ev = R.split_events(log)
    assert len(ev) == 130 and ev[63][1] - ev[0][0] == target and ev[129][1] - ev[64][0] < 8192
    return log


@pytest.mark.parametrize("way", ["junk", "blank"])
def test_first_chunk_on_both_sides_of_the_lds_limit(way):
    lines = _golden_lines(0)
    plain = b"\n".join(lines[:130]) + b"\n"
    base_want = R.expect([plain], 4)
    assert base_want["status"] == [R.OK] and base_want["kyoku_offsets"][-1] >= 1
    logs, bases, bad = [b"\n"], [0], []
    for target in (LT_LDS_TEXT - 1, LT_LDS_TEXT, LT_LDS_TEXT + 1, 40000):
        for base in (0, 1, 7, 8, 15):
            logs.append(_inflated(lines, target, way))
            bases.append(base)
        for base in (0, 7):                     # one bad line inside the long chunk: behind the padding
            bad.append(len(logs))
            logs.append(_inflated(lines, target, way, bad_at=40))
            bases.append(base)
    got, want = _check(logs, "inflated " + way, 4, False, {ERR_KEY_LINE: R.ERR_KEY}, bases)
    off = got["offsets"].tolist()
    koff = got["kyoku_offsets"].tolist()
    for l in range(1, len(logs)):
        if l in bad:
            line = R.split_events(logs[l])[40][2]
            assert (got["status"][l], got["error_line"][l]) == (R.ERR_KEY, line) and (line == 41 if way == "junk" else line > 41), l
            continue
        # nothing of the padding shows: the uninflated log's records, tables and counts
        assert bytes(got["events"][off[l]: off[l + 1]]) == bytes(base_want["events"]), l
        assert got["start_scores"][koff[l]: koff[l + 1]].tolist() == base_want["start_scores"].tolist(), l
        assert got["end_scores"][koff[l]: koff[l + 1]].tolist() == base_want["end_scores"].tolist(), l
        assert got["decisions"][l] == base_want["decisions"][0] and got["status"][l] == R.OK and got["error_line"][l] == 0, l


# ---------------------------------------------------------------- c. the tile seams of the line census
def _newline_at(pos, junk):
    """a log whose first line ends with its newline at byte `pos`"""
    if junk:
        first = DORA[:-1] + b',"z":"' + b"b" * (pos - len(DORA) - 7) + b'"}'
    else:
        first = DORA + b" " * (pos - len(DORA))
    assert len(first) == pos
    return first + b"\n" + DORA + b"\n"


def _seam_logs():
    logs = []
    for pos in (1022, 1023, 1024, 1025):
        logs += [_newline_at(pos, False), _newline_at(pos, True), b"\n" * pos + DORA, DORA + b"\n" * (pos - len(DORA)) + b"\n" + DORA]
    for n in (1500, 3000):
        long = _newline_at(n, True)
        logs += [long, DORA + b"\n" + long, long[:-1]]
    logs.append(b"\n" * 2500 + DORA + b"\n")
    logs.append(b"\n" * 1024 + b"\n" * 1024)                                     # tiles of nothing but newlines, and no event at all
    logs.append(b"{}\n" * 1100)
    logs.append(b"{}\n" * 1100 + b" \r\n\n\t\n" * 200)                           # 3 300 bytes, then a blank run across the seam at 4 096
    logs.append(b"{}\n" * 1100 + b" \r\n\n\t\n" * 200 + DORA)
    logs.append(b"\r\n".join(_golden_lines(0)[:70]) + b"\r\n")                   # CRLF on every line
    logs.append(b"".join(l + b"\n \t\r\n\r\r\n\t\t  \n" for l in _golden_lines(0)[:70]))
    tail = DORA[:-1] + b',"z":"' + b"c" * (1024 - 20 * (len(DORA) + 1) - len(DORA) - 7) + b'"}'
    logs.append((DORA + b"\n") * 20 + tail)                                      # the last line has no newline and ends at byte 1 024
    assert len(logs[-1]) == 1024
    logs.append(DORA + b"\n\f\n" + DORA + b"\n\v \n")                            # form feed / vertical tab: events that fail
    return logs


def test_census_and_index_across_tile_seams():
    logs = [b"\n"] + _seam_logs()
    bases = [0] + [(5 * i) % 16 for i in range(len(logs) - 1)]
    got, want = _check(logs, "seams", 4, False, {b"\f": R.ERR_JSON, b"\v": R.ERR_JSON}, bases)
    assert want["status"][-1] == R.ERR_JSON and want["error_line"][-1] == 2 and want["status"][:-1] == [R.OK] * (len(logs) - 1)
    assert max(np.diff(want["offsets"])) == 1101
    got0, _ = _check(logs, "seams, every log at a 16-byte base", 4, False, {b"\f": R.ERR_JSON, b"\v": R.ERR_JSON}, [0] * len(logs))
    assert bytes(got0["events"]) == bytes(got["events"])


def test_short_logs_at_every_alignment():
    text = b'{}\n {"type":"dora","dora_marker":"1m"}\r\n\n{}'
    assert len(text) > 40
    # hand-classified: a proper prefix of a line that holds one object is not JSON
    known = {DORA[:k]: R.ERR_JSON for k in range(1, len(DORA))}
    known[b"{"] = R.ERR_JSON
    for t in known:
        with pytest.raises(json.JSONDecodeError):
            json.loads(t)
    logs, bases = [b"\n"], [0]
    for base in range(16):
        for n in range(41):
            logs.append(text[:n])
            bases.append(base)
    got, want = _check(logs, "short logs", 4, False, known, bases)
    assert sorted(set(want["status"])) == [R.OK, R.ERR_JSON] and set(want["error_line"]) == {0, 1, 2}
    # and cut from the front: the ragged head of the first tile with other bytes in front of it
    logs2, bases2 = [b"\n"], [0]
    for base in range(16):
        for n in (0, 3, 4):
            logs2.append(text[n:])
            bases2.append(base)
    _check(logs2, "short logs cut from the front", 4, False, known, bases2)


# ---------------------------------------------------------------- d. the 64-event seams of the parse and the walk
def _sk(**kw):
    return R._start_kyoku(**kw)


def _padded(prefix, index):
    """prefix, then dora events until the next event has log index `index`"""
    assert len(prefix) <= index
    return list(prefix) + [{"type": "dora", "dora_marker": "3z"}] * (index - len(prefix))


def _hora(actor, deltas, **kw):
    return dict({"type": "hora", "actor": actor, "target": 1, "deltas": deltas}, **kw)


def test_logs_that_end_at_a_chunk_seam():
    for i in range(2):
        lines = _golden_lines(i)
        logs = [b"\n".join(lines[:n]) + (b"\n" if n % 2 else b"") for n in (1, 63, 64, 65, 127, 128, 129)]
        got, want = _check(logs, f"golden {i} cut at the seams")
        assert np.diff(want["offsets"]).tolist() == [1, 63, 64, 65, 127, 128, 129] and want["status"] == [R.OK] * 7


@pytest.mark.parametrize("at", [62, 63, 64, 65, 127, 128])
def test_horas_at_a_tile_seam_of_the_walk(at):
    """`at` is the log index of the first hora (63: the last event of a tile; 64: the first of the next)"""
    opening = [{"type": "start_game"}, _sk(), {"type": "reach", "actor": 1}, {"type": "dahai", "actor": 1, "pai": "1m", "tsumogiri": False},
               {"type": "reach_accepted", "actor": 1}, {"type": "reach", "actor": 3}]
    h0, h1 = _hora(0, [3000, -2000, 0, 0]), _hora(2, [0, -8000, 8000, 0])
    dahai = {"type": "dahai", "actor": 0, "pai": "2m", "tsumogiri": True}
    rest = [{"type": "end_kyoku"}, _sk(scores=[1, 2, 3, 4]), _hora(1, [5, 5, 5, 5])]
    logs = {
        "a hora, then end_kyoku": _padded(opening, at) + [h0] + rest[:1],
        "a hora, the last event of the log": _padded(opening, at) + [h0],
        "a double ron": _padded(opening, at) + [h0, h1] + rest,
        "a double ron, the last kyoku": _padded(opening, at) + [h0, h1],
        "a hora, a dahai of seat 0, a hora": _padded(opening, at) + [h0, dahai, h1],
        "a hora, a dora, a hora": _padded(opening, at) + [h0, {"type": "dora", "dora_marker": "1m"}, h1] + rest,
        "start_kyoku at the seam": _padded([{"type": "start_game"}], at) + opening[1:] + [h0, h1],
        "start_kyoku behind a hora outside a kyoku": _padded([{"type": "start_game"}], at - 1) + [_hora(0, [9, 9, 9, 9])] + opening[1:] + [h0, dahai, h1],
    }
    names = list(logs)
    for n in names:
        assert logs[n][at]["type"] in ("hora", "start_kyoku")
    got, want = _check([R.jsonl(logs[n]) for n in names], f"horas at {at}")
    assert want["status"] == [R.OK] * len(names), dict(zip(names, want["status"]))
    ends = {n: want["tables"][i][1][0].tolist() for i, n in enumerate(names)}
    assert ends["a double ron, the last kyoku"] != ends["a hora, a dahai of seat 0, a hora"]      # the dahai between them decides


# ---------------------------------------------------------------- e. the walk on the device: the filtered feed against the whole feed
def test_walk_rule_logs():
    good, raising = R.walk_rule_logs()
    sk3 = _sk(scores=[35000, 35000, 35000], tehais=[R._tehai()] * 3)
    seat3 = {"type": "dahai", "actor": 3, "pai": "1m", "tsumogiri": False}
    seat2 = {"type": "dahai", "actor": 2, "pai": "1m", "tsumogiri": False}
    h = _hora(0, [1000, -1000, 0, 0])
    extra_ok = {
        "seat 3 discards where only three tehais are listed, four scores": [_sk(tehais=[R._tehai()] * 3), seat3, h],
        "a dahai right behind a hora": [_sk(), h, seat2, _hora(2, [0, -500, 500, 0]), {"type": "end_kyoku"}, seat3],
        "seat 2 discards in a kyoku of three": [sk3, seat2, _hora(0, [100, 200])],
    }
    extra_raising = {
        "seat 3 discards in a kyoku of three": [sk3, {"type": "tsumo", "actor": 0, "pai": "1m"}, seat3, h],
        "seat 3 discards in a kyoku of three, behind a hora": [sk3, _hora(0, [100, 200, 300]), seat3],
        "seat 2 discards in a kyoku of two": [_sk(scores=[1000, 2000], tehais=[R._tehai()] * 2), seat2],
        "seat 2 discards in a kyoku of two, the second of the log": [_sk(), seat2, {"type": "end_kyoku"}, _sk(scores=[1000, 2000], tehais=[R._tehai()] * 2), seat2],
        "a kyoku of two opens at a tile seam": _padded([_sk(), seat2], 63) + [_sk(scores=[1000, 2000])] + [seat2],
        "a kyoku of two stays open across a tile seam": _padded([_sk(scores=[1000, 2000])], 70) + [seat2],
        "seat 0 without actor": [_sk(), {"type": "dahai", "pai": "1m"}],
    }
    names = list(good) + list(extra_ok) + list(raising) + list(extra_raising)
    logs = [dict(good, **extra_ok, **raising, **extra_raising)[n] for n in names]
    n_ok = len(good) + len(extra_ok)
    got, want = _check([R.jsonl(l) for l in logs], "walk rules")
    assert want["status"] == [R.OK] * n_ok + [R.ERR_REPLAY] * (len(names) - n_ok), dict(zip(names, want["status"]))
    assert got["error_line"].tolist() == [0] * len(names)
    # the same in 3P parsing: the fourth tehai is not looked at, the walk goes by the scores
    _check([R.jsonl(l) for l in logs], "walk rules, num_players 3", num_players=3)


def test_walk_soups():
    soups = R.walk_soups()
    got, want = _check([R.jsonl(s) for s in soups], "soups")
    n = len(soups)
    ok, replay = want["status"].count(R.OK), want["status"].count(R.ERR_REPLAY)
    assert n == 512 and ok + replay == n and ok * 5 >= n and replay * 5 >= n, (ok, replay)
    assert sum(R.hora_then_dahai(s) for s in soups) >= 30
    assert got["error_line"].tolist() == [0] * n


# ---------------------------------------------------------------- f. the first error of a log
def test_first_error_across_chunks_and_against_the_walk():
    lines = _golden_lines(0)[:200]
    clean = b"\n".join(lines) + b"\n"
    known = {ERR_TILE_LINE: R.ERR_TILE, ERR_KEY_LINE: R.ERR_KEY, ERR_JSON_LINE: R.ERR_JSON}

    def spoil(edits):
        l = list(lines)
        for i, t in edits.items():
            l[i] = t
        return b"\n".join(l) + b"\n"

    no_actor = b'{"type":"reach"}'
    cases = [
        (spoil({150: ERR_TILE_LINE, 20: ERR_KEY_LINE}), R.ERR_KEY, 21),
        (spoil({150: ERR_KEY_LINE, 20: ERR_TILE_LINE, 199: ERR_JSON_LINE}), R.ERR_TILE, 21),
        (spoil({70: ERR_TILE_LINE, 100: ERR_JSON_LINE}), R.ERR_TILE, 71),               # two in one chunk
        (spoil({100: ERR_TILE_LINE, 70: ERR_JSON_LINE, 64: b"\n\n" + lines[64]}), R.ERR_JSON, 73),
        (spoil({63: ERR_KEY_LINE, 64: ERR_TILE_LINE}), R.ERR_KEY, 64),                  # either side of a chunk seam
        (spoil({180: ERR_TILE_LINE, 30: no_actor}), R.ERR_TILE, 181),                   # the parse error wins over the walk
        (spoil({30: no_actor}), R.ERR_REPLAY, 0),                                       # the walk alone: no line
    ]
    other = b"\n".join(_golden_lines(1)[:90]) + b"\n"
    logs = [clean]
    for i, (text, _, _) in enumerate(cases):
        logs += [text, other if i % 2 else clean]
    got, want = _check(logs, "first errors", 4, False, known)
    for i, (_, st, line) in enumerate(cases):
        assert (want["status"][1 + 2 * i], want["error_line"][1 + 2 * i]) == (st, line), i
        assert (got["status"][1 + 2 * i], got["error_line"][1 + 2 * i]) == (st, line), i
    # the neighbours of a failed log are what they are in a clean set
    ref = _parse([clean, other])
    off, koff, roff, rkoff = got["offsets"].tolist(), got["kyoku_offsets"].tolist(), ref["offsets"].tolist(), ref["kyoku_offsets"].tolist()
    for l in range(0, len(logs), 2):
        j = 0 if logs[l] is clean else 1
        assert bytes(got["events"][off[l]: off[l + 1]]) == bytes(ref["events"][roff[j]: roff[j + 1]]), l
        for k in ("start_scores", "end_scores"):
            assert got[k][koff[l]: koff[l + 1]].tolist() == ref[k][rkoff[j]: rkoff[j + 1]].tolist(), (l, k)
        assert (got["status"][l], got["error_line"][l], got["decisions"][l]) == (R.OK, 0, ref["decisions"][j]), l


# ---------------------------------------------------------------- g. device-resident text at an odd address
def test_device_text_at_an_odd_address():
    import torch

    logs = [R.jsonl(s) for s in R.walk_soups()[:40]] + [b"", b"\n" * 1030 + DORA, (DORA + b"\n") * 70] + [b"\n".join(_golden_lines(0)[:130])]
    want = _parse(logs)
    buf, ends = np.frombuffer(b"".join(logs), np.uint8), np.cumsum([len(l) for l in logs])
    ranges = np.stack([ends - [len(l) for l in logs], ends], axis=1)
    whole = torch.zeros(3 + buf.size, dtype=torch.uint8, device="cuda")
    whole[:3] = torch.tensor([ord("{"), ord('"'), 10], dtype=torch.uint8)
    whole[3:] = torch.from_numpy(buf.copy()).cuda()
    view = whole[3:]
    assert view.data_ptr() % 16 == 3
    got = _fetch(datasets.parse_logs_device(view, torch.from_numpy(ranges.astype(np.int64)).cuda(), num_players=4))
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k
    _same(got, R.expect(logs, 4), "device text")
