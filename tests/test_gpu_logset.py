"""GPU: logset.LogSet, the one Python owner of the device log set - every constructor against the plain reference tests/logtext_ref.py
(expect(): bytes.split, json.loads, abi.event_records_from_mjai, kyoku_tables) and the host packing, the three on_error modes, one set
feeding both LogSampleBuilder and GrpDataset, and the sets of no logs."""
import gzip
import json

import numpy as np
import pytest

from riichienv_amd import abi, datasets, vecenv
from riichienv_amd.datasets import LogSampleBuilder
from riichienv_amd.grp import GrpDataset
from riichienv_amd.logset import LogSet
from tests import logtext_ref as R

pytestmark = pytest.mark.gpu
DTYPES = {"events": np.uint8, "offsets": np.int64, "kyoku_offsets": np.int64, "start_scores": np.int32, "end_scores": np.int32, "status": np.uint8,
          "error_line": np.int64, "decisions": np.int64}
_CACHE = {}


def _games(mode):
    """12 (4P) / 8 (3P) complete self-played games as the device formatter's text, made as the other log tests make them"""
    if mode not in _CACHE:
        n = 12 if mode == 2 else 8
        env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=31 + mode, event_ring=8192)
        env.reset()
        for _ in range(40):
            env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
            if env.status()[2].all():
                break
        assert env.status()[2].all() and int(env.events_lost().sum()) == 0
        text, offs = env.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
        raw = text.tobytes()
        _CACHE[mode] = [raw[int(offs[g]): int(offs[g + 1])] for g in range(n)]
        env.close()
    return _CACHE[mode]


def _corpus(mode):
    """(texts, expectation): 8 games, an empty log, a log of start_game / end_game only (no kyoku) - and the two golden logs in 4P"""
    if ("corpus", mode) not in _CACHE:
        texts = ([open(p, "rb").read() for p in R.GOLDEN] if mode == 2 else []) + _games(mode)[:8]
        texts = texts[:3] + [b"", R.jsonl([{"type": "start_game"}, {"type": "end_game"}])] + texts[3:]
        _CACHE[("corpus", mode)] = (texts, R.expect(texts, 3 if mode >= 3 else 4))
    return _CACHE[("corpus", mode)]


def _dicts(texts):
    return [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in texts]


def _assert_tensors(got, want, what):
    """tensors() against expect(): byte for byte, in the documented dtypes; the table rows of the logs that parse when some do not"""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert sorted(g) == sorted(DTYPES) and all(v.is_cuda for v in got.values()), what
    for k, dt in DTYPES.items():
        assert g[k].dtype == dt, (what, k)
    assert g["events"].shape == want["events"].shape and g["events"].tobytes() == want["events"].tobytes(), what
    for k in ("offsets", "status", "error_line", "decisions"):
        assert g[k].tobytes() == np.asarray(want[k], DTYPES[k]).tobytes(), (what, k)
    koff = g["kyoku_offsets"].tolist()
    assert koff[0] == 0 and koff[-1] == len(g["start_scores"]) == len(g["end_scores"]) and g["start_scores"].shape[1:] == (4,), what
    if want["kyoku_offsets"] is not None:
        for k in ("kyoku_offsets", "start_scores", "end_scores"):
            assert g[k].tobytes() == np.asarray(want[k], DTYPES[k]).tobytes(), (what, k)
    for l, tab in enumerate(want["tables"]):
        if tab is not None:
            assert g["start_scores"][koff[l]: koff[l + 1]].tobytes() == tab[0].tobytes() and g["end_scores"][koff[l]: koff[l + 1]].tobytes() == tab[1].tobytes(), (what, l)


def _host_packing(texts, n):
    """(logs, offsets, start, end) of pack_logs / kyoku_tables over the logs as dicts, computed once per corpus"""
    key = ("host", n, hash(tuple(texts)))
    if key not in _CACHE:
        logs = _dicts(texts)
        _CACHE[key] = (logs, datasets.pack_logs(logs, n)[1]) + datasets.kyoku_tables(logs, n)
    return _CACHE[key]


def _assert_set(s, texts, want, what, text_set=True):
    """the set's attributes against the host packing of the same logs, its tensors() against the reference"""
    logs, off, start, end = _host_packing(texts, s.num_players)
    assert (s.M, s.n_events, s.n_kyokus, s.longest_log) == (len(logs), int(off[-1]), len(start), max(len(l) for l in logs)), what
    assert s.kyoku_offsets.dtype == np.uint32 and s.kyoku_offsets.tolist() == want["kyoku_offsets"], what
    assert s.lengths.dtype == np.int64 and s.lengths.tolist() == [len(l) for l in logs], what
    assert s.decisions.dtype == np.int64 and s.decisions.tolist() == [sum(e.get("type") in datasets._DECISION_TYPES for e in l) for l in logs], what
    assert s.log_ids.tolist() == list(range(len(logs))) and s.dropped == [] and s.owns_tables == text_set and (s.logs is None) == text_set, what
    assert s.start_scores.tolist() == start.tolist() and s.end_scores.tolist() == end.tolist() and s.end_scores.dtype == np.int32, what
    _assert_tensors(s.tensors(), want, what)
    s.close()
    assert s.handle is None


def _layout(texts, order):
    """(buffer, ranges [M, 2]): the logs laid out in `order` with bytes that are no log's between them"""
    buf, ranges = b'{"x\n', np.zeros((len(texts), 2), np.uint64)
    for i in order:
        ranges[i] = (len(buf), len(buf) + len(texts[i]))
        buf += texts[i] + b"\n}{" * (i % 3)
    return buf, ranges


# ------------------------------------------------------------------ ingest
@pytest.mark.parametrize("mode", [2, 5])
def test_every_constructor_holds_what_the_host_packing_holds(mode, tmp_path):
    import torch

    n = 3 if mode >= 3 else 4
    texts, want = _corpus(mode)
    assert want["status"] == [R.OK] * len(texts) and want["kyoku_offsets"][4] == want["kyoku_offsets"][5] and 0 in np.diff(want["offsets"])
    _assert_set(LogSet.from_logs(_host_packing(texts, n)[0], n), texts, want, "from_logs", text_set=False)
    _assert_set(LogSet.from_text(texts, num_players=n), texts, want, "from_text, a list")
    buf, ranges = _layout(texts, list(range(len(texts)))[::2] + list(range(len(texts)))[1::2])
    _assert_set(LogSet.from_text(np.frombuffer(buf, np.uint8), ranges, n), texts, want, "from_text, a buffer and ranges")
    _assert_set(LogSet.from_text(buf, ranges[::-1].copy(), n), texts[::-1], R.expect(texts[::-1], n), "from_text, the ranges in reverse order")
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / (f"g{i}.jsonl.gz" if i % 2 else f"g{i}.jsonl")))
        with open(paths[-1], "wb") as f:
            f.write(gzip.compress(t) if i % 2 else t)
    _assert_set(LogSet.from_jsonl(paths, num_players=n), texts, want, "from_jsonl")
    text = torch.frombuffer(bytearray(b"".join(texts)), dtype=torch.uint8).cuda()
    offs = torch.tensor([0] + np.cumsum([len(t) for t in texts]).tolist(), dtype=torch.int64, device="cuda")
    _assert_set(LogSet.from_device_text(text, offs, n), texts, want, "from_device_text")


# ------------------------------------------------------------------ on_error
def _spoiled():
    """the corpus of test_spoiled_logs_are_reported_and_dropped: 12 games - log 2: a truncated line; log 5: a 12-tile tehai; log 9: an
    unknown tile behind two blank lines.  (texts, the bad lines' statuses, the (log, line, status name) of the three)"""
    texts = list(_games(2))
    logs = _dicts(texts)
    lines = [t.split(b"\n") for t in texts]
    lines[2][10] = lines[2][10][: len(lines[2][10]) // 2]
    sk = next(k for k, e in enumerate(logs[5]) if e["type"] == "start_kyoku")
    ev = json.loads(lines[5][sk])
    ev["tehais"][1] = ev["tehais"][1][:12]
    lines[5][sk] = json.dumps(ev).encode()
    ts = next(k for k, e in enumerate(logs[9]) if e["type"] == "tsumo")
    ev = json.loads(lines[9][ts])
    ev["pai"] = "9z"
    tile_line = json.dumps(ev).encode()
    lines[9][ts] = b"\n\n" + tile_line
    known = {lines[2][10].strip(R.BLANK): R.ERR_JSON, lines[5][sk]: R.ERR_TEHAI, tile_line: R.ERR_TILE}
    for i in (2, 5, 9):
        texts[i] = b"\n".join(lines[i])
    return texts, known, [(2, 11, "ERR_JSON"), (5, sk + 1, "ERR_TEHAI"), (9, ts + 3, "ERR_TILE")]


def test_the_three_on_error_modes():
    texts, known, dropped = _spoiled()
    keep = [0, 1, 3, 4, 6, 7, 8, 10, 11]
    with pytest.raises(ValueError) as e:
        LogSet.from_text(texts, num_players=4)
    assert str(e.value) == "log 2: line 11: ERR_JSON (3 of 12 logs do not parse; on_error='drop' skips them)"
    s = LogSet.from_text(texts, num_players=4, on_error="drop")
    assert s.log_ids.tolist() == keep and s.dropped == dropped and s.M == 9 and len(s.kyoku_offsets) == 10 and len(s.lengths) == 9
    _assert_tensors(s.tensors(), R.expect([texts[i] for i in keep], 4), "drop")
    s.close()
    s = LogSet.from_text(texts, num_players=4, on_error="keep")
    want = R.expect(texts, 4, known_status=known)
    assert s.M == 12 and s.log_ids.tolist() == list(range(12)) and s.dropped == dropped
    assert [(i, want["error_line"][i], abi.LOGTEXT_STATUS_NAMES[want["status"][i]]) for i in range(12) if want["status"][i]] == dropped
    _assert_tensors(s.tensors(), want, "keep")
    s.close()


# ------------------------------------------------------------------ one parse, both stages
def _bytes(tensors):
    return {k: (str(v.dtype), tuple(v.shape), v.cpu().numpy().tobytes()) for k, v in tensors.items()}


@pytest.mark.parametrize("mode", [2, 5])
def test_one_set_feeds_the_builder_and_the_grp_dataset(mode):
    n = 3 if mode >= 3 else 4
    texts = _games(mode)[:8]
    s = LogSet.from_text(texts, num_players=n)
    b = LogSampleBuilder.from_logset(s, game_mode=mode, n_slots=4, features="base")
    g = GrpDataset.from_logset(s)
    b2 = LogSampleBuilder.from_text(texts, game_mode=mode, n_slots=4, features="base")
    g2 = GrpDataset.from_text(texts, game_mode=mode)
    assert b.logset is s and g.logset is s and b2.logset is not s and b.capacity == b2.capacity and g.n_kyokus == g2.n_kyokus == s.n_kyokus
    b.run()
    b2.run()
    got, want = _bytes(b.samples()), _bytes(b2.samples())
    assert b.counts() == b2.counts() and b.counts()["fill"] > 100 and b.counts()["failed_logs"] == 0
    assert sorted(got) == sorted(want) and all(got[k] == want[k] for k in want), [k for k in want if got[k] != want[k]]
    got, want = _bytes(g.tensors()), _bytes(g2.tensors())
    assert want["x"][1] == (s.n_kyokus * n, 4 * n + 4) and all(got[k] == want[k] for k in want), [k for k in want if got[k] != want[k]]
    for c in (b, g, b2, g2):
        c.close()
    assert b2.logset.handle is None and g2.logset.handle is None and s.handle          # a consumer closes the set it made, not the one it was handed
    _assert_tensors(s.tensors(), R.expect(texts, n), "after the consumers closed")
    s.close()
    s.close()
    assert s.handle is None


# ------------------------------------------------------------------ sets of no logs
def test_empty_sets_through_every_constructor(tmp_path):
    import torch

    no_text, no_offs = torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    made = {"from_logs": lambda c, **kw: c([], **kw) if c is not LogSet else c.from_logs([], **kw), "from_text, a list": lambda c, **kw: c.from_text([], **kw),
            "from_text, ranges": lambda c, **kw: c.from_text(b"", np.zeros((0, 2), np.uint64), **kw), "from_jsonl": lambda c, **kw: c.from_jsonl([], **kw),
            "from_device_text": lambda c, **kw: c.from_device_text(no_text, no_offs, **kw),
            "every log dropped": lambda c, **kw: c.from_text([b'{"type":"dora"}', b'{"type":"a","u":[1,2}\n'], on_error="drop", **kw)}
    shapes = {"events": (0, 3, 32), "offsets": (1,), "kyoku_offsets": (1,), "start_scores": (0, 4), "end_scores": (0, 4), "status": (0,), "error_line": (0,),
              "decisions": (0,)}
    for what, make in made.items():
        s = make(LogSet, num_players=3)
        assert (s.M, s.n_events, s.n_kyokus, s.longest_log, s.handle) == (0, 0, 0, 0, None), what
        assert s.kyoku_offsets.tolist() == [0] and s.lengths.shape == (0,) and s.decisions.shape == (0,) and s.start_scores.shape == (0, 4), what
        assert len(s.dropped) == (2 if what == "every log dropped" else 0) and s.log_ids.shape == (0,), what
        t = s.tensors()
        for k, shape in shapes.items():
            assert tuple(t[k].shape) == shape and t[k].cpu().numpy().dtype == DTYPES[k] and t[k].is_cuda and not t[k].cpu().numpy().any(), (what, k)
        r = s.grp_rows()
        assert tuple(r["x"].shape) == (0, 3, 16) and tuple(r["meta"].shape) == (0, 4) and tuple(r["rank"].shape) == (0, 3) and tuple(r["log_of"].shape) == (0,), what
        assert r["kyoku_offsets"].cpu().tolist() == [0] and r["rank"].dtype == torch.uint8 and r["x"].dtype == torch.float32, what
        b = LogSampleBuilder.from_logset(s, game_mode=5)
        assert b.run() == 0 and tuple(b.samples()["features"].shape) == (0, 74, 27) and b.samples()["action"].dtype == torch.int64 and b.counts()["fill"] == 0, what
        b.close()
        s.close()
        if what == "every log dropped":
            continue                       # GrpDataset keeps what does not parse: its set is not empty
        b, g = make(LogSampleBuilder, game_mode=5), make(GrpDataset, game_mode=5)
        assert b.M == 0 and b.run() == 0 and int(b.samples()["action"].shape[0]) == 0 and list(b.batches(8)) == [] and b.capacity == 64, what
        assert g.M == 0 and tuple(g.grp_rows()["x"].shape) == (0, 3, 16) and tuple(g.tensors()["y"].shape) == (0, 3) and list(g.batches(8)) == [], what
        b.close()
        g.close()
