"""GPU: MJAI text parsed on the device (rmj_logset_create_from_text, LogSampleBuilder.from_text / from_jsonl / from_device_text,
datasets.parse_logs_device) against the host path that stays the definition: pack_logs + rmj_logset_create for the records,
datasets.kyoku_tables for the score tables, LogSampleBuilder(dict logs) for the samples.  (tests/test_gpu_log_text.py is the test of the
opposite direction, records -> text.)"""
import ctypes as C
import gzip
import json
import os
import random

import numpy as np
import pytest

from riichienv_amd import abi, datasets, vecenv
from riichienv_amd.logset import LogSet

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = [os.path.join(HERE, "golden", n) for n in ("126_204_0_mjai.jsonl", "ui_example_after_injection.jsonl")]
N_GAMES = 1024
FIELDS = ("features", "mask", "action", "packed", "return", "return64", "rank", "log", "kyoku", "seat", "t")
JUNK = [("meta", {"a": [1, 2, {"b": None}], "c": "x"}), ("note", 'quote \" backslash \\ newline \n brace { bracket ]'), ("名前", "東風戦 ✓"),
        ("nested", [[[], {}], {"k": [True, False, None, -1.5e-3, 0]}]), ("num", -12.5), ("flag", True), ("nil", None)]
_TEXT = {}


def _game_texts(mode, n=N_GAMES):
    """n complete self-written games of `mode` as the device formatter's own text: a list of per-log byte strings"""
    if (mode, n) not in _TEXT:
        env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=31 + mode, event_ring=8192)
        env.reset()
        for _ in range(40):
            env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
            if env.status()[2].all():
                break
        assert env.status()[2].all(), "a rollout game did not finish"
        assert int(env.events_lost().sum()) == 0
        text, offs = env.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
        raw = text.tobytes()
        _TEXT[(mode, n)] = [raw[int(offs[g]): int(offs[g + 1])] for g in range(n)]
        env.close()
    return _TEXT[(mode, n)]


def _dicts(texts):
    return [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in texts]


def _shuffled_text(logs, seed):
    rng = random.Random(seed)
    out = []
    for log in logs:
        lines = []
        for ev in log:
            items = list(ev.items()) + rng.sample(JUNK, 2)
            rng.shuffle(items)
            lines.append(json.dumps(dict(items), separators=rng.choice([(",", ":"), (", ", ": "), (" ,\t", " :  ")]), ensure_ascii=False))
        out.append(("\n".join(lines) + rng.choice(["\n", "", "\r\n", "\n\n  \n"])).encode())
    return out


def _reference_set(logs, n_players):
    """what pack_logs + rmj_logset_create hold for the dict logs: events bytes, offsets, kyoku_offsets, n_kyokus, longest_log"""
    recs, off = datasets.pack_logs(logs, n_players)
    s = LogSet.from_logs(logs, n_players)
    v = abi.LogsetViews()
    vecenv._chk(vecenv.load_lib().rmj_logset_views(s.handle, C.byref(v)))
    assert not v.start_scores and not v.end_scores and not v.status and not v.error_line and not v.decisions and v.events and v.offsets
    s.close()
    n = int(off[-1])
    assert (s.M, s.n_events) == (len(logs), n)
    return np.frombuffer(bytes(recs), dtype=np.uint8)[: n * 96].reshape(n, 3, 32), off.astype(np.int64), s.kyoku_offsets.astype(np.int64), s.n_kyokus, s.longest_log


def _check_parse(texts, logs, n_players, what):
    ev, off, koff, K, longest = _reference_set(logs, n_players)
    start, end = datasets.kyoku_tables(logs, n_players)
    dec = [sum(1 for e in l if e.get("type") in datasets._DECISION_TYPES) for l in logs]
    got = datasets.parse_logs_device(texts, num_players=n_players)
    assert got["status"].cpu().tolist() == [0] * len(logs), what
    assert got["error_line"].cpu().tolist() == [0] * len(logs), what
    assert got["offsets"].cpu().tolist() == off.tolist(), what
    assert got["kyoku_offsets"].cpu().tolist() == koff.tolist(), what
    g = got["events"].cpu().numpy()
    assert g.shape == ev.shape, what
    if not (g == ev).all():
        i = int(np.flatnonzero((g != ev).any(axis=(1, 2)))[0])
        raise AssertionError(f"{what}: event {i}: {bytes(g[i]).hex()} != {bytes(ev[i]).hex()}")
    assert got["start_scores"].cpu().numpy().tolist() == start.tolist(), what
    assert got["end_scores"].cpu().numpy().tolist() == end.tolist(), what
    assert got["decisions"].cpu().tolist() == dec, what
    # n_kyokus and longest_log of the set itself
    s = LogSet.from_text(texts, num_players=n_players)
    s.close()
    assert (s.M, s.n_events, s.n_kyokus, s.longest_log) == (len(logs), int(off[-1]), K, longest), what


@pytest.mark.parametrize("mode", [2, 5])
def test_records_equal_the_host_packing(mode):
    n_players = 3 if mode >= 3 else 4
    texts = _game_texts(mode)
    logs = _dicts(texts)
    assert len(logs) == N_GAMES and min(len(l) for l in logs) > 50
    _check_parse(texts, logs, n_players, "device formatter text")
    _check_parse([("\n".join(json.dumps(e) for e in l) + "\n").encode() for l in logs], logs, n_players, "json.dumps default")
    _check_parse(_shuffled_text(logs, 7 + mode), logs, n_players, "shuffled with junk keys")


def test_records_of_the_golden_logs():
    texts = [open(p, "rb").read() for p in GOLDEN]
    logs = _dicts(texts)
    _check_parse(texts, logs, 4, "golden")
    _check_parse(_shuffled_text(logs, 3), logs, 4, "golden shuffled")
    # an empty log, a log of blank lines only, and a last line without its newline
    t2 = [b"", b"\n  \n\t\r\n", texts[0].rstrip(b"\n")]
    _check_parse(t2, [[], [], logs[0]], 4, "empty logs")


def _assert_same_samples(a, b, what):
    import torch

    sa, sb = a.samples(), b.samples()
    assert a.counts() == b.counts(), what
    assert int(sa["action"].shape[0]) > 0, what
    for f in FIELDS:
        assert sa[f].shape == sb[f].shape and sa[f].dtype == sb[f].dtype, (what, f)
        assert torch.equal(sa[f].view(torch.uint8) if sa[f].is_floating_point() else sa[f], sb[f].view(torch.uint8) if sb[f].is_floating_point() else sb[f]), (what, f)


@pytest.mark.parametrize("mode,features,n", [(2, "base", 256), (5, "base", 256), (2, "extended", 48), (5, "extended", 48)])
def test_samples_equal_the_dict_builder(mode, features, n):
    texts = _game_texts(mode)[:n]
    logs = _dicts(texts)
    a = datasets.LogSampleBuilder.from_text(texts, game_mode=mode, features=features, n_slots=n // 2)
    b = datasets.LogSampleBuilder(logs, game_mode=mode, features=features, n_slots=n // 2)
    assert "ingest" in a.host_seconds and a.capacity == b.capacity and a.n_kyokus == b.n_kyokus
    assert a.kyoku_offsets.tolist() == b.kyoku_offsets.tolist() and a.lengths.tolist() == b.lengths.tolist()
    a.run()
    b.run()
    assert a.default_rewards().is_cuda                      # no host round trip
    assert np.array_equal(a.default_rewards().cpu().numpy(), b.default_rewards())
    _assert_same_samples(a, b, (mode, features))
    assert a.logset._h_end is None                           # finalize() took the device table
    assert a.start_scores.tolist() == b.start_scores.tolist() and a.end_scores.tolist() == b.end_scores.tolist()
    a.close()
    b.close()


def test_from_jsonl_reads_plain_and_gzip_files(tmp_path):
    texts = _game_texts(2)[:8]
    paths = []
    for i, t in enumerate(texts):
        p = tmp_path / (f"g{i}.jsonl.gz" if i % 2 else f"g{i}.jsonl")
        p.write_bytes(gzip.compress(t) if i % 2 else t)
        paths.append(str(p))
    a = datasets.LogSampleBuilder.from_jsonl(paths, game_mode=2)
    b = datasets.LogSampleBuilder(_dicts(texts), game_mode=2)
    a.run()
    b.run()
    _assert_same_samples(a, b, "jsonl")
    a.close()
    b.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_device_text_to_samples_without_the_host(mode):
    from riichienv_amd.torch_env import TorchVecEnv

    n = 128
    tenv = TorchVecEnv(n, game_mode=mode, seed=77, skip_mjai_logging=False, event_ring=8192)
    env = tenv.env
    env.reset()
    for _ in range(40):
        env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
        if env.status()[2].all():
            break
    assert env.status()[2].all() and int(env.events_lost().sum()) == 0
    text, offs = tenv.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
    assert text.is_cuda and offs.is_cuda
    a = datasets.LogSampleBuilder.from_device_text(text, offs, game_mode=mode, n_slots=n // 2)
    raw, o = text.cpu().numpy().tobytes(), offs.cpu().tolist()
    b = datasets.LogSampleBuilder.from_text([raw[o[g]: o[g + 1]] for g in range(n)], game_mode=mode, n_slots=n // 2)
    a.run()
    b.run()
    _assert_same_samples(a, b, ("device text", mode))
    a.close()
    b.close()
    env.close()


def test_spoiled_logs_are_reported_and_dropped():
    texts = list(_game_texts(2)[:12])
    logs = _dicts(texts)

    def lines(i):
        return texts[i].split(b"\n")

    # log 2: a truncated line; log 5: a 12-tile tehai; log 9: an unknown tile
    l2 = lines(2)
    l2[10] = l2[10][: len(l2[10]) // 2]
    sk = next(k for k, e in enumerate(logs[5]) if e["type"] == "start_kyoku")
    ev = json.loads(lines(5)[sk])
    ev["tehais"][1] = ev["tehais"][1][:12]
    l5 = lines(5)
    l5[sk] = json.dumps(ev).encode()
    ts = next(k for k, e in enumerate(logs[9]) if e["type"] == "tsumo")
    ev = json.loads(lines(9)[ts])
    ev["pai"] = "9z"
    l9 = lines(9)
    l9[ts] = b"\n\n" + json.dumps(ev).encode()        # two blank lines in front: the line number counts them
    spoiled = list(texts)
    spoiled[2], spoiled[5], spoiled[9] = b"\n".join(l2), b"\n".join(l5), b"\n".join(l9)
    got = datasets.parse_logs_device(spoiled)
    want_status = [0] * 12
    want_line = [0] * 12
    want_status[2], want_line[2] = abi.LOGTEXT_ERR_JSON, 11
    want_status[5], want_line[5] = abi.LOGTEXT_ERR_TEHAI, sk + 1
    want_status[9], want_line[9] = abi.LOGTEXT_ERR_TILE, ts + 3
    assert got["status"].cpu().tolist() == want_status and got["error_line"].cpu().tolist() == want_line
    with pytest.raises(ValueError, match=r"log 2: line 11: ERR_JSON"):
        datasets.LogSampleBuilder.from_text(spoiled, game_mode=2)
    a = datasets.LogSampleBuilder.from_text(spoiled, game_mode=2, on_error="drop")
    keep = [i for i in range(12) if i not in (2, 5, 9)]
    assert a.log_ids.tolist() == keep
    assert a.dropped == [(2, 11, "ERR_JSON"), (5, sk + 1, "ERR_TEHAI"), (9, ts + 3, "ERR_TILE")]
    b = datasets.LogSampleBuilder([logs[i] for i in keep], game_mode=2)
    a.run()
    b.run()
    _assert_same_samples(a, b, "drop")
    a.close()
    b.close()


def test_ranges_in_any_order_and_with_gaps():
    texts = _game_texts(5)[:16]
    logs = _dicts(texts)
    rng = random.Random(11)
    order = list(range(16))
    rng.shuffle(order)
    buf, ranges, at = b"", np.zeros((16, 2), np.uint64), 0
    for i in order:                       # the logs laid out in shuffled order with junk between them
        gap = b"x{\n" * rng.randrange(0, 5) + b"\0" * rng.randrange(0, 17)
        buf += gap
        ranges[i] = (len(buf), len(buf) + len(texts[i]))
        buf += texts[i]
    want = datasets.parse_logs_device(texts, num_players=3)
    got = datasets.parse_logs_device(np.frombuffer(buf, np.uint8), ranges, num_players=3)
    rev = datasets.parse_logs_device(buf, ranges[::-1].copy(), num_players=3)
    ev, off = want["events"].cpu().numpy(), want["offsets"].cpu().tolist()
    roff = rev["offsets"].cpu().tolist()
    for k in ("events", "offsets", "kyoku_offsets", "start_scores", "end_scores", "status", "decisions"):
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k
    assert want["status"].cpu().tolist() == [0] * 16 and len(logs) == 16
    for i in range(16):                   # reversed ranges: log i of the reversed set is log 15 - i
        j = 15 - i
        assert np.array_equal(rev["events"].cpu().numpy()[roff[i]: roff[i + 1]], ev[off[j]: off[j + 1]]), i
    # dropping a log = leaving its range out
    sub = datasets.parse_logs_device(buf, ranges[[0, 3, 4]], num_players=3)
    so = sub["offsets"].cpu().tolist()
    for i, j in enumerate([0, 3, 4]):
        assert np.array_equal(sub["events"].cpu().numpy()[so[i]: so[i + 1]], ev[off[j]: off[j + 1]])


def test_argument_errors():
    L = vecenv.load_lib()
    h = C.c_void_p()
    rng = np.array([[5, 2]], np.uint64)
    buf = np.zeros(16, np.uint8)
    assert L.rmj_logset_create_from_text(0, buf.ctypes.data, rng.ctypes.data, 1, 4, 0, C.byref(h)) == -1       # end < begin
    assert L.rmj_logset_create_from_text(0, buf.ctypes.data, rng.ctypes.data, 1, 5, 0, C.byref(h)) == -1       # num_players
    assert L.rmj_logset_create_from_text(0, buf.ctypes.data, rng.ctypes.data, 1, 4, 8, C.byref(h)) == -1       # unknown flag
    with pytest.raises(ValueError, match="on_error"):
        datasets.LogSampleBuilder.from_text([b"{}\n"], on_error="ignore")
    with pytest.raises(ValueError, match="behind the text"):
        datasets.LogSampleBuilder.from_text(b"{}\n", ranges=[[0, 9]])
    e = datasets.LogSampleBuilder.from_text([], game_mode=2)
    assert e.M == 0 and e.run() == 0 and int(e.samples()["action"].shape[0]) == 0
