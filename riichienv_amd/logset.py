"""The device log set's one Python owner.  A LogSet holds an rmj_logset handle - the packed event records of M MJAI logs, resident on the
device - and everything the library tells about it; LogSampleBuilder (datasets.py) replays it into BC/CQL samples, GrpDataset and
grp_rows (grp.py) turn it into the rank model's rows, and one set may feed both.  Nothing else in the package calls rmj_logset_*.

Two kinds of set.  from_logs packs event dicts on the host (abi.event_records_from_mjai, rmj_logset_create); its kyoku score tables are
host arrays (kyoku_tables) that finalize() and grp_rows() upload.  from_text / from_jsonl / from_device_text parse MJAI JSONL bytes on the
device (rmj_logset_create_from_text: no Python work per event); such a set holds its own tables on the device (`owns_tables`) and a
status per log."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import abi, vecenv
from .streams import stream_ptr

_DECISION_TYPES = ("dahai", "chi", "pon", "daiminkan", "kan", "ankan", "kakan", "reach", "hora", "kita", "ryukyoku")


def _events_of(log):
    """a log as a list of MJAI event dicts: a list, an MjaiReplay (its events) or an MjSoulReplay (to_mjai())"""
    if hasattr(log, "to_mjai"):
        return log.to_mjai()
    if hasattr(log, "events"):
        return list(log.events)
    return list(log)


def pack_logs(logs, num_players=4, masked_ok=False):
    """The event stream of a log set: (records, offsets) - records a ctypes array of abi.Event, abi.EVENT_SLOTS per MJAI event in log
    order (abi.event_records_from_mjai of every event, as rmj_apply_events takes them), offsets [M + 1] int64-safe uint32: log i is
    events offsets[i] .. offsets[i + 1]."""
    logs = [_events_of(l) for l in logs]
    offsets = np.zeros(len(logs) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(l) for l in logs], dtype=np.int64)
    total = int(offsets[-1])
    recs = (abi.Event * (abi.EVENT_SLOTS * max(total, 1)))()
    step = abi.EVENT_SLOTS * C.sizeof(abi.Event)
    base, at = C.addressof(recs), 0
    for log in logs:
        for ev in log:
            r = abi.event_records_from_mjai(ev, num_players, masked_ok)
            C.memmove(base + at * step, C.addressof(r), step)
            at += 1
    return recs, offsets


def kyoku_tables(logs, n_players):
    """[K, 4] int32 start and end scores of every kyoku of every log, in (log, kyoku) order - the rows of the reward table"""
    from .replay import MjaiReplay

    start, end = [], []
    for log in logs:
        for k in MjaiReplay.from_events(_events_of(log)).rounds:
            s = (list(k.scores) + [0] * 4)[:4]
            e = (list(k.end_scores if k.end_scores else k.scores) + [0] * 4)[:4]
            start.append(s)
            end.append(e)
    return np.array(start, dtype=np.int32).reshape(-1, 4), np.array(end, dtype=np.int32).reshape(-1, 4)


def kyoku_own_end_scores(logs, n_players):
    """[K, 8] int32: the end scores every kyoku's own hora / ryukyoku events give - kyoku_tables' end column before MjaiReplay replaces it,
    for every kyoku but a log's last, with the next start_kyoku's scores - in two readings: [:, :4] as Kyoku computes them (a ryukyoku's
    deltas without the riichi deposits, as converted Tenhou logs hold them), [:, 4:] with a ryukyoku's deltas read as already holding the
    deposits (as this engine writes them).  validate() compares them with the next kyoku's start scores."""
    from .replay import Kyoku

    rows = []

    def close(k, alt):
        rows.append((list(k.end_scores) + [0] * 4)[:4] + (list(alt) + [0] * 4)[:4])

    for log in logs:
        cur = alt = None
        for ev in _events_of(log):
            ty = ev.get("type")
            if ty == "start_kyoku" or ty in ("end_kyoku", "end_game"):
                if cur is not None:
                    close(cur, alt)
                cur = Kyoku(ev) if ty == "start_kyoku" else None
                alt = list(cur.scores) if cur is not None else None
            elif cur is not None:
                cur._feed(ev)
                deltas = ev.get("deltas", ev.get("delta"))
                if ty == "ryukyoku" and ev.get("scores") is None and deltas is not None:
                    alt = [s + d for s, d in zip(cur.scores, deltas)] + list(cur.scores[len(deltas):])
                elif ty in ("hora", "ryukyoku"):
                    alt = list(cur.end_scores)
        if cur is not None:
            close(cur, alt)
    return np.array(rows, dtype=np.int32).reshape(-1, 8)


def _text_and_ranges(text, ranges):
    """(uint8 array, [M, 2] uint64 ranges) of from_text's two input forms"""
    if ranges is None:
        parts = [bytes(t) for t in text]
        ends = np.cumsum([len(p) for p in parts], dtype=np.uint64) if parts else np.zeros(0, np.uint64)
        rng = np.zeros((len(parts), 2), dtype=np.uint64)
        rng[:, 1] = ends
        rng[1:, 0] = ends[:-1]
        text = b"".join(parts)
    else:
        rng = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    if len(rng) and int(rng[:, 1].max()) > buf.size:
        raise ValueError("a range ends behind the text")
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)
    return buf, rng


def _read_log_file(path):
    import gzip

    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def check_on_error(on_error, modes=("raise", "drop", "keep")):
    if on_error not in modes:
        raise ValueError("on_error is " + ", ".join(repr(m) for m in modes[:-1]) + " or " + repr(modes[-1]))


def _host_table(name, i):
    """start_scores / end_scores: the host array [K, 4] int32 - kept for a set packed from dicts, a copy made when first read for a set that
    owns its tables"""
    def get(self):
        if getattr(self, name) is None and self.owns_tables:
            setattr(self, name, self.device_scores()[i].cpu().numpy())
        return getattr(self, name)

    return property(get, lambda self, v: setattr(self, name, v))


class LogSet:
    """s = LogSet.from_text(texts, num_players=4); s.tensors(); s.grp_rows(); s.close()

    from_logs(logs)                    lists of MJAI event dicts, MjaiReplay or MjSoulReplay objects, packed on the host
    from_text(text, ranges)            bytes / bytearray / numpy uint8 with ranges [M, 2] (begin, end) byte ranges of the logs (any order,
                                       gaps allowed) - or, with ranges=None, a list of per-log byte strings
    from_jsonl(paths)                  from_text over files read on the host: one log per path, gzip detected by its magic bytes and
                                       decompressed with Python's gzip (as MjaiReplay.from_jsonl does)
    from_device_text(text, offsets)    text that already lies in device memory: the (text uint8, offsets int64 [M + 1]) tensors of
                                       TorchVecEnv.drain_text - log i is text[offsets[i]:offsets[i + 1]] - or offsets as [M, 2] ranges

    on_error (text): "raise" - a ValueError naming the first log that does not parse, its line and status; "drop" - the set is rebuilt
    from the good logs: `log_ids[i]` is the caller's index of set log i; "keep" - the set keeps the failed logs with their status (no
    kyoku of theirs gets a rank).  `dropped` lists (log, line, status) of the failed logs in both.

    Holds: handle (None once closed, and for a set of no logs), device, num_players, M, n_events, n_kyokus, longest_log, kyoku_offsets
    [M + 1] uint32, lengths / decisions [M] int64 (events and decision events per log), log_ids, dropped, logs (from_logs: the event
    lists), host_seconds, and the kyoku score tables: start_scores / end_scores are host arrays [K, 4] int32 - a copy made when first
    read if the set owns its tables, whose device views are device_scores()."""

    def __init__(self, device, num_players, owns_tables, n_logs):
        import torch

        self.torch, self.L, self.handle = torch, vecenv.load_lib(), None
        self.device_index, self.device, self.num_players = int(device), torch.device("cuda", int(device)), int(num_players)
        self.owns_tables = bool(owns_tables)      # parsed from text: the score tables and the per-log status live in the set
        self.masked_ok = False                    # made with masked_ok=True: "?" tiles were read as tile 0 - the hidden seats' state is then garbage
        self.logs, self.log_ids, self.dropped = None, np.arange(n_logs, dtype=np.int64), []
        self.M, self.n_events, self.n_kyokus, self.longest_log = int(n_logs), 0, 0, 0
        self.kyoku_offsets = np.zeros(self.M + 1, dtype=np.uint32)
        self._h_start = self._h_end = self._d_scores = self._decisions = self._lengths = None

    def _adopt(self, handle):
        """the handle over the logs `log_ids`, and what rmj_logset_info tells about it"""
        info, self.kyoku_offsets = abi.LogsetInfo(), np.zeros(len(self.log_ids) + 1, dtype=np.uint32)
        vecenv._chk(self.L.rmj_logset_info(handle, C.byref(info), self.kyoku_offsets.ctypes.data))
        self.handle = handle
        self.M, self.n_events, self.n_kyokus, self.longest_log = int(info.n_logs), int(info.n_events), int(info.n_kyokus), int(info.longest_log)

    # ---- constructors
    @classmethod
    def from_logs(cls, logs, num_players=4, masked_ok=False, device=0):
        t0 = time.perf_counter()
        logs = [_events_of(l) for l in logs]
        self = cls(device, num_players, False, len(logs))
        self.logs, self.masked_ok = logs, bool(masked_ok)
        t1 = time.perf_counter()
        self.start_scores, self.end_scores = kyoku_tables(logs, self.num_players)
        self.host_seconds = {"kyoku_tables": time.perf_counter() - t1}   # the one-off host work of the constructor, for cost reports
        self._lengths = np.array([len(l) for l in logs], dtype=np.int64)
        if logs:
            t1 = time.perf_counter()
            recs, offsets = pack_logs(logs, self.num_players, masked_ok)
            self.host_seconds["pack_logs"] = time.perf_counter() - t1
            h = C.c_void_p()
            vecenv._chk(self.L.rmj_logset_create(self.device_index, C.addressof(recs), offsets.ctypes.data, len(logs), C.byref(h)))
            self._adopt(h)
            assert self.n_kyokus == len(self.end_scores), "the stream's start_kyoku records and the parsed rounds disagree"
        self.host_seconds["ingest"] = time.perf_counter() - t0
        return self

    @classmethod
    def from_text(cls, text, ranges=None, num_players=4, masked_ok=False, device=0, on_error="raise"):
        t0 = time.perf_counter()
        check_on_error(on_error)
        return cls._parse(*_text_and_ranges(text, ranges), num_players, masked_ok, device, on_error, t0)

    @classmethod
    def from_jsonl(cls, paths, **kw):
        return cls.from_text([_read_log_file(p) for p in paths], **kw)

    @classmethod
    def from_device_text(cls, text, offsets, num_players=4, masked_ok=False, device=None, on_error="raise"):
        """The text is only read during this call (clone nothing).  Torch's current stream is synchronised before every create call: it
        runs on the library's own stream order."""
        import torch

        t0 = time.perf_counter()
        check_on_error(on_error)
        if not (text.is_cuda and offsets.is_cuda) or text.dtype != torch.uint8:
            raise ValueError("from_device_text takes a uint8 text tensor and an offsets tensor on the GPU")
        o = offsets.to(torch.int64)
        rng = o.contiguous() if o.dim() == 2 else torch.stack([o[:-1], o[1:]], dim=1).contiguous()
        return cls._parse(text.contiguous(), rng, num_players, masked_ok, text.device.index if device is None else device, on_error, t0)

    @classmethod
    def _parse(cls, text, rng, num_players, masked_ok, device, on_error, t0):
        """rmj_logset_create_from_text over (text, rng) - numpy arrays on the host or torch tensors on the device - then the one status read"""
        n_logs, host = len(rng), isinstance(rng, np.ndarray)
        self = cls(device, num_players, True, n_logs)
        self.masked_ok = bool(masked_ok)
        L, torch = self.L, self.torch
        flags = (abi.LOGTEXT_MASKED_OK if masked_ok else 0) | (0 if host else abi.LOGTEXT_ON_DEVICE)

        def create(keep):
            """a handle over the caller's logs `keep` (None: all of them)"""
            if host:
                r = rng if keep is None else np.ascontiguousarray(rng[keep])
                tp, rp = text.ctypes.data, r.ctypes.data
            else:
                r = rng if keep is None else rng[torch.as_tensor(keep, device=rng.device)].contiguous()
                torch.cuda.current_stream(text.device).synchronize()
                tp, rp = text.data_ptr() if text.numel() else 0, r.data_ptr() if r.numel() else 0
            h = C.c_void_p()
            vecenv._chk(L.rmj_logset_create_from_text(self.device_index, C.c_void_p(tp), C.c_void_p(rp), len(r), self.num_players, flags, C.byref(h)))
            return h

        self.handle = create(None)
        try:
            status, line = np.zeros(max(n_logs, 1), np.uint8), np.zeros(max(n_logs, 1), np.uint32)
            vecenv._chk(L.rmj_logset_status(self.handle, status.ctypes.data, line.ctypes.data, None, None))
            status = status[:n_logs]
            self.dropped = [(int(i), int(line[i]), abi.LOGTEXT_STATUS_NAMES[int(status[i])]) for i in np.flatnonzero(status)]
            if self.dropped and on_error != "keep":
                self.close()
                if on_error == "raise":
                    i, ln, st = self.dropped[0]
                    raise ValueError(f"log {i}: line {ln}: {st} ({len(self.dropped)} of {n_logs} logs do not parse; on_error='drop' skips them)")
                self.log_ids = np.flatnonzero(status == 0).astype(np.int64)
                self.handle = create(self.log_ids)    # one more create call over the ranges of the good logs
            self._adopt(self.handle)
        except Exception:
            self.close()
            raise
        if self.M == 0:
            self.close()
            self.start_scores = self.end_scores = np.zeros((0, 4), np.int32)
            self._decisions = self._lengths = np.zeros(0, np.int64)
        self.host_seconds = {"ingest": time.perf_counter() - t0}
        return self

    def close(self):
        """rmj_logset_destroy; the host attributes stay"""
        if getattr(self, "handle", None):
            self.L.rmj_logset_destroy(self.handle)
        self.handle = self._d_scores = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- what the set holds
    def _log_counts(self, name):
        """decisions / lengths, made when first asked for: counted over the dicts, or read from the device for a text set"""
        if getattr(self, name) is None and self.logs is not None:
            self._decisions = np.array([sum(1 for ev in l if ev.get("type") in _DECISION_TYPES) for l in self.logs], dtype=np.int64)
        elif getattr(self, name) is None:
            dec, off = np.zeros(self.M, np.uint32), np.zeros(self.M + 1, np.uint32)
            vecenv._chk(self.L.rmj_logset_status(self.handle, None, None, dec.ctypes.data, off.ctypes.data))
            self._decisions, self._lengths = dec.astype(np.int64), np.diff(off.astype(np.int64))
        return getattr(self, name)

    start_scores, end_scores = _host_table("_h_start", 0), _host_table("_h_end", 1)
    decisions = property(lambda self: self._log_counts("_decisions"))
    lengths = property(lambda self: self._log_counts("_lengths"))

    def _views(self):
        v = abi.LogsetViews()
        if self.handle:
            vecenv._chk(self.L.rmj_logset_views(self.handle, C.byref(v)))
        elif self.M:
            raise vecenv.RmjError("the log set is closed")
        return v

    def _wrap(self, ptr, shape, typestr):
        return abi.device_tensor(self.torch, self, self.device, ptr, shape, typestr)

    def device_scores(self):
        """(start, end) int32 [K, 4] device tensors: views into a set that owns its tables (None for a set packed from dicts)"""
        if self._d_scores is None and self.owns_tables:
            v, K = self._views(), self.n_kyokus
            self._d_scores = (self._wrap(v.start_scores, (K, 4), "<i4"), self._wrap(v.end_scores, (K, 4), "<i4")) if K else \
                (self.torch.zeros((0, 4), dtype=self.torch.int32, device=self.device),) * 2
        return self._d_scores

    def tensors(self):
        """The set as a dict of torch tensors on the GPU, clones: events [N, 3, 32] uint8 (abi.Event records, what pack_logs gives),
        offsets / kyoku_offsets [M + 1] int64, start_scores / end_scores [K, 4] int32, status [M] uint8 (abi.LOGTEXT_*), error_line /
        decisions [M] int64."""
        t, dev, m, n, k, v = self.torch, self.device, self.M, self.n_events, self.n_kyokus, self._views()

        def get(ptr, shape, ts):
            return self._wrap(ptr, shape, ts).clone() if ptr and int(np.prod(shape)) else t.zeros(shape, dtype=t.uint8, device=dev)
        out = {"events": get(v.events, (n, 3, 32), "|u1"), "offsets": get(v.offsets, (m + 1,), "<i4").to(t.int64),
               "kyoku_offsets": get(v.kyoku_offsets, (m + 1,), "<i4").to(t.int64), "start_scores": get(v.start_scores, (k, 4), "<i4").to(t.int32),
               "end_scores": get(v.end_scores, (k, 4), "<i4").to(t.int32), "status": get(v.status, (m,), "|u1"),
               "error_line": get(v.error_line, (m,), "<i4").to(t.int64), "decisions": get(v.decisions, (m,), "<i4").to(t.int64)}
        if not self.owns_tables:
            out.update(start_scores=t.as_tensor(self.start_scores, device=dev), end_scores=t.as_tensor(self.end_scores, device=dev),
                       decisions=t.as_tensor(self.decisions, device=dev))
        t.cuda.synchronize(dev)
        return out

    def grp_rows(self, num_players=None):
        """The GRP rows of every kyoku as device tensors, in table order `kyoku_offsets[log] + kyoku - 1`:
          x [K, n, 4n + 4] f32, meta [K, 4] i32 (chang, ju, ben, liqibang), rank [K, n] u8 (the seat's place in its LOG'S final scores,
          GrpReplayDataset's label; 255 for the kyokus of a log that did not parse), log_of [K] i32, kyoku_offsets [M + 1] i64.
        num_players defaults to the set's.  Asynchronous on torch's current stream; nothing is read back."""
        torch, dev = self.torch, self.device
        n, K = int(self.num_players if num_players is None else num_players), self.n_kyokus
        out = {"x": torch.empty((K, n, 4 * n + 4), dtype=torch.float32, device=dev), "meta": torch.zeros((K, 4), dtype=torch.int32, device=dev),
               "rank": torch.full((K, n), 255, dtype=torch.uint8, device=dev), "log_of": torch.zeros((K,), dtype=torch.int32, device=dev),
               "kyoku_offsets": torch.as_tensor(np.asarray(self.kyoku_offsets, dtype=np.int64), device=dev)}
        if not K or not self.handle:
            return out
        self._grp_call(n, abi.GrpOut(out["meta"].data_ptr(), out["x"].data_ptr(), out["rank"].data_ptr(), out["log_of"].data_ptr()))
        return out

    def _grp_call(self, n, o):
        """rmj_logset_grp_device into the abi.GrpOut `o` on torch's current stream, over the set's own tables (NULL) or the host tables
        uploaded for the call"""
        torch, dev = self.torch, self.device
        tables = [] if self.owns_tables else [torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev) for a in (self.start_scores, self.end_scores)]
        stream = torch.cuda.current_stream(dev)
        vecenv._chk(self.L.rmj_logset_grp_device(self.handle, n, *([a.data_ptr() for a in tables] or [None, None]), C.byref(o), stream.cuda_stream))
        for a in tables:
            a.record_stream(stream)

    def final_ranks(self, num_players=None):
        """uint8 [K, n] device tensor: grp_rows()["rank"] alone - every seat's place (0 = first) in its log's final scores, repeated in
        each kyoku row of the log, 255 in the kyokus of a log that did not parse - through rmj_logset_grp_device with no other output (its
        walk of the records and the x kernel are not run).  Asynchronous on torch's current stream."""
        torch, dev = self.torch, self.device
        n, K = int(self.num_players if num_players is None else num_players), self.n_kyokus
        rank = torch.full((K, n), 255, dtype=torch.uint8, device=dev)
        if not K:
            return rank
        if not self.handle:
            raise vecenv.RmjError("the log set is closed")
        self._grp_call(n, abi.GrpOut(None, None, rank.data_ptr(), None))
        return rank

    def log_of(self):
        """int64 [K] device tensor: the log of every kyoku row (from the host's kyoku_offsets: an upload, nothing is read back)"""
        return self.torch.as_tensor(np.repeat(np.arange(self.M, dtype=np.int64), np.diff(self.kyoku_offsets.astype(np.int64))), device=self.device)

    def play_stats(self, num_players=None):
        """How every seat played every kyoku (rmj_logset_playstats_device; the columns are abi.PLAYSTAT_NAMES, riichienv_amd.stats summarises
        them), as device tensors in table order `kyoku_offsets[log] + kyoku - 1`:
          rows [K, 4, 16] i32 (seats >= num_players all zero; -1 everywhere in the kyokus of a log that did not parse), valid [K] bool (the
          kyoku's log parsed), log_of [K] i64, kyoku_offsets [M + 1] i64.
        num_players defaults to the set's.  Asynchronous on torch's current stream; nothing is read back."""
        torch, dev = self.torch, self.device
        n, K = int(self.num_players if num_players is None else num_players), self.n_kyokus
        if n not in (3, 4):
            raise ValueError("num_players is 3 or 4")
        if K and not self.handle:
            raise vecenv.RmjError("the log set is closed")
        log_of = self.log_of()
        out = {"rows": torch.empty((K, 4, abi.PLAYSTAT_COLUMNS), dtype=torch.int32, device=dev), "valid": torch.ones((K,), dtype=torch.bool, device=dev),
               "log_of": log_of, "kyoku_offsets": torch.as_tensor(np.asarray(self.kyoku_offsets, dtype=np.int64), device=dev), "num_players": n}
        if not K:
            return out
        if self.owns_tables:
            out["valid"] = self._wrap(self._views().status, (self.M,), "|u1")[log_of] == abi.LOGTEXT_OK
        vecenv._chk(self.L.rmj_logset_playstats_device(self.handle, n, out["rows"].data_ptr(), stream_ptr(torch, dev)))
        return out

    def validate(self, game_mode=None, rule=None, n_slots=None, share_stream=True):
        """A verdict for every log, by a checking replay on the device (rmj_logcheck_*): a logcheck.LogReport with the first finding of
        every log - code, event, kyoku, seat, detail - and summary() / good_ids() / describe(i).  riichienv_amd.logcheck lists the codes
        and the known limits (a later hora of a multiple ron is not checked against an offer, settlement amounts are not recomputed,
        feature encodings are not inspected, masked logs trip TILE_COUNT).  A set of no logs returns an empty report."""
        from . import logcheck

        return logcheck.validate(self, game_mode, rule, n_slots, share_stream)
