"""Behaviour-cloning / offline-RL samples from MJAI logs, built on the device: what riichienv-ml's MCDataset yields
(datasets/mjai_logs.py:62-129) - per decision `(features, action_id, G_t, mask, rank)` with G_t = reward * gamma ** (T - t - 1) over the
seat's decisions of the kyoku and rank the seat's place in the kyoku's end scores - for many logs at once.

The logs are packed once on the host into one array of event records (abi.event_records_from_mjai, unchanged) and uploaded; from there
on the replay is kernels of the library (rmj_logset_*, rmj_logreplay_*: csrc/rmj_logreplay.hip.h): the next event of every log is
matched against the published legal lists on the device, the deciding seats' rows are encoded straight into a pool, the event is
applied - no host work per event, no host synchronisation inside the replay.  ReplayBatch.samples() / Kyoku.steps() compute the same
samples through the host and stay as the checker.

M logs run in n_slots <= M games; a slot whose log ends takes its next one.  Which slot gets which logs is decided before the replay
(`assign_slots`): logs in order, each to the slot that is free first when every event takes one step, ties to the lowest slot - a pure
function of (M, n_slots, the logs' lengths), so two runs fill the pool in the same order.

What the records do not carry.  Matching follows the packed records, which hold less than the MJAI text: a dahai without a `tsumogiri`
field reads as tsumogiri = false (select_action_from_mjai skips the drawn-tile rule when the field is absent, so on third-party logs
without it the builder may pick the other tile of the same name), a kakan is matched by its tile name without `consumed`, and the seat
a robbed kan is taken from is the log's previous actor, not the hora's `target`.  On logs that a game produced these agree.  The only
failure detected is a decision that matches nothing in the list its actor is offered; an event that does not fit the state in another
way (a decision by a seat that is not to act) is applied like apply_events applies it and the log counts as complete.

Memory: the pool is capacity x (C x W x 4 + A + 52) bytes, and samples() holds a second copy of what it emits (fill x the same row) until
the next run() / finalize() / clear() - at the default capacity about three times the samples' own size in all.  What does not fit is counted (`counts()["overflowed"]`) and the trajectory that lost a
sample is not emitted; a log in which a decision matches no legal action is dropped whole (`counts()["failed_logs"]`), like a file whose
replay raises in MCDataset."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, vecenv

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


def assign_slots(lengths, n_slots):
    """(slot_of_log [M], lists: per slot the logs it replays in order, steps of the whole replay) - rmj_logreplay_assign, a host function
    of the library (no GPU needed)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    m = int(lengths.size)
    off = np.zeros(m + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lengths)
    slot_of = np.zeros(max(m, 1), dtype=np.uint32)
    order = np.zeros(max(m, 1), dtype=np.uint32)
    first = np.zeros(int(n_slots) + 1, dtype=np.uint32)
    steps = C.c_uint32()
    vecenv._chk(vecenv.load_lib().rmj_logreplay_assign(off.ctypes.data, m, int(n_slots), slot_of.ctypes.data, order.ctypes.data, first.ctypes.data, C.byref(steps)))
    return slot_of[:m].copy(), [order[first[s]: first[s + 1]].tolist() for s in range(int(n_slots))], int(steps.value)


def gamma_powers(gamma, n):
    """P[k] = gamma ** k for k < n in Python floats (the dataset's own arithmetic), float64"""
    g = float(gamma)
    return np.array([g ** k for k in range(int(n))], dtype=np.float64)


def compute_rank(end_scores, n_players):
    """_compute_rank (mjai_logs.py:14-17) of every seat: [K, 4] scores -> [K, n_players] ranks (0 = first; equal scores rank by seat)"""
    sc = np.asarray(end_scores, dtype=np.float64).reshape(-1, 4)[:, :n_players]
    return (-sc).argsort(axis=1, kind="stable").argsort(axis=1, kind="stable")


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


def parse_logs_device(text, ranges=None, num_players=4, masked_ok=False, device=0):
    """MJAI JSONL text -> the packed records, parsed on the device (rmj_logset_create_from_text), as a dict of torch tensors on the GPU:
    events [N, 3, 32] uint8 (abi.Event records, what pack_logs gives), offsets / kyoku_offsets [M + 1] int64, start_scores / end_scores
    [K, 4] int32, status [M] uint8 (abi.LOGTEXT_*), error_line / decisions [M] int64.  text / ranges as in LogSampleBuilder.from_text, or a
    uint8 tensor on the GPU with ranges an int64 [M, 2] tensor there."""
    import torch

    L = vecenv.load_lib()
    flags = abi.LOGTEXT_MASKED_OK if masked_ok else 0
    h = C.c_void_p()
    if isinstance(text, torch.Tensor) and text.is_cuda:
        text, rng = text.contiguous(), ranges.to(torch.int64).contiguous()
        device, m = text.device.index, int(rng.shape[0])
        torch.cuda.current_stream(text.device).synchronize()
        vecenv._chk(L.rmj_logset_create_from_text(device, C.c_void_p(text.data_ptr() if text.numel() else 0), C.c_void_p(rng.data_ptr() if m else 0), m,
                                                  int(num_players), flags | abi.LOGTEXT_ON_DEVICE, C.byref(h)))
    else:
        buf, rng = _text_and_ranges(text, ranges)
        m = len(rng)
        vecenv._chk(L.rmj_logset_create_from_text(int(device), buf.ctypes.data, rng.ctypes.data, m, int(num_players), flags, C.byref(h)))
    try:
        info, v = abi.LogsetInfo(), abi.LogsetViews()
        vecenv._chk(L.rmj_logset_info(h, C.byref(info), None))
        vecenv._chk(L.rmj_logset_views(h, C.byref(v)))
        from .torch_env import _CudaArray

        dev = torch.device("cuda", device)
        keep = object()
        get = lambda ptr, shape, ts: torch.as_tensor(_CudaArray(ptr, shape, ts, keep), device=dev).clone() if int(np.prod(shape)) else torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        n, k = int(info.n_events), int(info.n_kyokus)
        out = {"events": get(v.events, (n, 3, 32), "|u1"), "offsets": get(v.offsets, (m + 1,), "<i4").to(torch.int64),
               "kyoku_offsets": get(v.kyoku_offsets, (m + 1,), "<i4").to(torch.int64), "start_scores": get(v.start_scores, (k, 4), "<i4").to(torch.int32),
               "end_scores": get(v.end_scores, (k, 4), "<i4").to(torch.int32), "status": get(v.status, (m,), "|u1"),
               "error_line": get(v.error_line, (m,), "<i4").to(torch.int64), "decisions": get(v.decisions, (m,), "<i4").to(torch.int64)}
        torch.cuda.synchronize(dev)
    finally:
        L.rmj_logset_destroy(h)
    return out


class LogSampleBuilder:
    """b = LogSampleBuilder(logs, game_mode=2, features="base"); b.run(); s = b.samples()

    logs: lists of MJAI event dicts, MjaiReplay objects or MjSoulReplay objects (their to_mjai()).
    features: "base" (74 x W), "discard_shanten" (94 x 34, 4P only) or "extended" (215 x W).
    n_slots: games replayed at once (default and at most: the number of logs).  capacity: pool size in samples.  The default - twice the
    logs' decision events - is a heuristic, not a bound: a discard can add a Pass sample for up to three seats, and those are not
    counted.  Check counts()["overflowed"] after run(); it is 0 on every log set of the tests.  rule: "tenhou" (default) or "mjsoul".
    rewards: finalize(rewards) takes a float64 [K, 4] table by kyoku row (`kyoku_offsets[log] + kyoku - 1`; the GRP reward model's
    output) - default: the seat's score change of the kyoku times kyoku_scale."""

    def __init__(self, logs, game_mode=2, features="base", n_slots=None, capacity=None, gamma=0.99, include_pass=True, skip_single_action=True,
                 rule=None, device=0, share_stream=True, masked_ok=False, kyoku_scale=1.0 / 1000.0):
        self._check(features, rule)
        self.logs = [_events_of(l) for l in logs]
        self._configure(len(self.logs), game_mode, features, n_slots, gamma, include_pass, skip_single_action, rule, device, share_stream, kyoku_scale)
        if capacity is None:
            capacity = 2 * sum(1 for l in self.logs for ev in l if ev.get("type") in _DECISION_TYPES) + 64
        self._set_capacity(capacity)
        import time

        t0 = time.perf_counter()
        self.start_scores, self.end_scores = kyoku_tables(self.logs, self.n_players)
        self.host_seconds = {"kyoku_tables": time.perf_counter() - t0}   # the one-off host work of the constructor, for cost reports
        self.lengths = np.array([len(l) for l in self.logs], dtype=np.int64)
        if self.M == 0:
            self.kyoku_offsets = np.zeros(1, dtype=np.uint32)
            return
        t0 = time.perf_counter()
        recs, offsets = pack_logs(self.logs, self.n_players, masked_ok)
        self.host_seconds["pack_logs"] = time.perf_counter() - t0
        L = self.L = vecenv.load_lib()
        self.set = C.c_void_p()
        vecenv._chk(L.rmj_logset_create(device, C.addressof(recs), offsets.ctypes.data, self.M, C.byref(self.set)))
        self._attach()
        assert self.n_kyokus == len(self.end_scores), "the stream's start_kyoku records and the parsed rounds disagree"

    @staticmethod
    def _check(features, rule):
        if features not in abi.FEATURES:
            raise ValueError(f"unknown feature set {features!r}: one of {sorted(abi.FEATURES)}")
        if rule not in (None, "tenhou", "mjsoul"):
            raise ValueError(f"Unknown rule: '{rule}'. Expected 'tenhou' or 'mjsoul'")

    def _configure(self, n_logs, game_mode, features, n_slots, gamma, include_pass, skip_single_action, rule, device, share_stream, kyoku_scale):
        """the settings every constructor shares (no device work)"""
        import torch

        self.torch = torch
        self.M = int(n_logs)
        self.rule, self._device_index = rule, int(device)
        self._d_start = self._d_end = None    # device score tables (sets parsed from text)
        self._h_start = self._h_end = None
        self.game_mode = vecenv._mode_id(game_mode)
        self.sanma = self.game_mode >= 3
        self.n_players = 3 if self.sanma else 4
        self.features, self._feat = features, abi.FEATURES[features]
        self.channels, self.width = abi.FEATURE_CHANNELS[self._feat], 27 if self.sanma else 34
        self.A = abi.ACTION_SPACE_3P if self.sanma else abi.ACTION_SPACE_4P
        self.n_slots = self.M if n_slots is None else int(n_slots)
        if self.n_slots > self.M or (self.M and self.n_slots < 1):
            raise ValueError(f"n_slots must be between 1 and the number of logs ({self.M})")
        self.gamma, self.kyoku_scale = float(gamma), float(kyoku_scale)
        self.include_pass, self.skip_single_action = bool(include_pass), bool(skip_single_action)
        self.device = torch.device("cuda", device)
        self.shared = bool(share_stream)
        self._finalized = False
        self._emitted = None    # what samples() returned last, until run() / finalize() / clear()
        self.h = self.set = self.env = None

    def _set_capacity(self, capacity):
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("capacity must be positive (samples)")

    # the kyoku score tables: host arrays for dict logs; for a set parsed from text they stay on the device and a host copy is made only
    # when the attribute is read
    @property
    def start_scores(self):
        if self._h_start is None and self._d_start is not None:
            self._h_start = self._d_start.cpu().numpy()
        return self._h_start

    @start_scores.setter
    def start_scores(self, v):
        self._h_start = v

    @property
    def end_scores(self):
        if self._h_end is None and self._d_end is not None:
            self._h_end = self._d_end.cpu().numpy()
        return self._h_end

    @end_scores.setter
    def end_scores(self, v):
        self._h_end = v

    def _attach(self):
        """the environment, the replay and the pool views over self.set (whichever call made it)"""
        from .torch_env import _CudaArray

        torch, L, device, rule = self.torch, self.L, self._device_index, self.rule
        info = abi.LogsetInfo()
        self.kyoku_offsets = np.zeros(self.M + 1, dtype=np.uint32)
        vecenv._chk(L.rmj_logset_info(self.set, C.byref(info), self.kyoku_offsets.ctypes.data))
        self.n_kyokus = int(info.n_kyokus)
        bits = abi.RULE_MJSOUL if rule == "mjsoul" else abi.RULE_TENHOU
        self.env = vecenv.VecRiichiEnv(self.n_slots, game_mode=self.game_mode, seed=0, rule_bits=bits, device=device, skip_mjai_logging=True)
        if self.shared:
            vecenv._chk(L.rmj_set_stream(self.env.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), 0))
        self._powers = gamma_powers(self.gamma, int(info.longest_log) + 1)
        flags = (abi.LOGREPLAY_INCLUDE_PASS if self.include_pass else 0) | (abi.LOGREPLAY_SKIP_SINGLE_ACTION if self.skip_single_action else 0)
        cfg = abi.LogReplayConfig(self._feat, self.capacity, flags, len(self._powers), self.gamma, self._powers.ctypes.data)
        self.h = C.c_void_p()
        try:
            vecenv._chk(L.rmj_logreplay_create(self.env.h, self.set, C.byref(cfg), C.byref(self.h)))
        except vecenv.RmjError:
            self.h = None
            self.close()
            raise
        v = abi.LogReplayViews()
        vecenv._chk(L.rmj_logreplay_views(self.h, C.byref(v)))
        self.steps = int(v.steps)
        wrap = lambda ptr, shape, ts: torch.as_tensor(_CudaArray(ptr, shape, ts, self), device=self.device)  # noqa: E731
        cap, fl, K = self.capacity, self.channels * self.width, max(self.n_kyokus, 1)
        rows = wrap(v.features, (cap, v.row_stride), "<f4")
        self.pool = {"features": rows[:, :fl].unflatten(-1, (self.channels, self.width)), "mask": wrap(v.mask, (cap, self.A), "|u1"),
                     "action": wrap(v.action, (cap,), "<i4"), "packed": wrap(v.packed, (cap,), "<i8"), "return": wrap(v.ret, (cap,), "<f4"),
                     "return64": wrap(v.ret64, (cap,), "<f8"), "rank": wrap(v.rank, (cap,), "<i4"), "log": wrap(v.log, (cap,), "<i4"),
                     "kyoku": wrap(v.kyoku, (cap,), "<i4"), "seat": wrap(v.seat, (cap,), "<i4"), "t": wrap(v.t, (cap,), "<i4"),
                     "log_status": wrap(v.log_status, (self.M,), "|u1"), "traj_len": wrap(v.traj_len, (K, 4), "<i4"),
                     "traj_broken": wrap(v.traj_broken, (K, 4), "|u1"), "counters": wrap(v.counters, (6,), "<i4")}
        self._sync()

    # ---- log sets parsed from MJAI text on the device (rmj_logset_create_from_text)
    @classmethod
    def _from_set(cls, make_set, n_logs, game_mode, features, n_slots, capacity, gamma, include_pass, skip_single_action, rule, device, share_stream,
                  kyoku_scale, on_error, ingest_seconds):
        """make_set(keep) -> rmj_logset handle over the caller's logs `keep` (None: all of them)"""
        import time

        if on_error not in ("raise", "drop"):
            raise ValueError("on_error is 'raise' or 'drop'")
        cls._check(features, rule)
        self = cls.__new__(cls)
        self.logs = None
        L = self.L = vecenv.load_lib()
        t0 = time.perf_counter()
        handle = make_set(None)
        status = np.zeros(max(n_logs, 1), np.uint8)
        line = np.zeros(max(n_logs, 1), np.uint32)
        vecenv._chk(L.rmj_logset_status(handle, status.ctypes.data, line.ctypes.data, None, None))
        bad = np.flatnonzero(status[:n_logs])
        self.log_ids, self.dropped = np.arange(n_logs, dtype=np.int64), []
        if bad.size:
            self.dropped = [(int(i), int(line[i]), abi.LOGTEXT_STATUS_NAMES[int(status[i])]) for i in bad]
            L.rmj_logset_destroy(handle)
            if on_error == "raise":
                i, ln, st = self.dropped[0]
                raise ValueError(f"log {i}: line {ln}: {st} ({len(self.dropped)} of {n_logs} logs do not parse; on_error='drop' skips them)")
            self.log_ids = np.flatnonzero(status[:n_logs] == 0).astype(np.int64)
            handle = make_set(self.log_ids)    # one more create call over the ranges of the good logs
        try:
            self._configure(len(self.log_ids), game_mode, features, n_slots, gamma, include_pass, skip_single_action, rule, device, share_stream, kyoku_scale)
        except Exception:
            L.rmj_logset_destroy(handle)
            raise
        self.set = handle
        self.host_seconds = {"ingest": ingest_seconds + time.perf_counter() - t0}
        try:
            if self.M == 0:
                self.kyoku_offsets, self.lengths = np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.int64)
                self._h_start = self._h_end = np.zeros((0, 4), np.int32)
                self._set_capacity(64 if capacity is None else capacity)
                L.rmj_logset_destroy(self.set)
                self.set = None
                return self
            dec = np.zeros(self.M, np.uint32)
            off = np.zeros(self.M + 1, np.uint32)
            vecenv._chk(L.rmj_logset_status(self.set, None, None, dec.ctypes.data, off.ctypes.data))
            self.lengths = np.diff(off.astype(np.int64))
            self._set_capacity(2 * int(dec.sum(dtype=np.int64)) + 64 if capacity is None else capacity)
            self._attach()
            v = abi.LogsetViews()
            vecenv._chk(L.rmj_logset_views(self.set, C.byref(v)))
            from .torch_env import _CudaArray

            K = self.n_kyokus
            wrap = lambda ptr: self.torch.as_tensor(_CudaArray(ptr, (K, 4), "<i4", self), device=self.device)  # noqa: E731
            if K:
                self._d_start, self._d_end = wrap(v.start_scores), wrap(v.end_scores)
            else:
                self._d_start = self._d_end = self.torch.zeros((0, 4), dtype=self.torch.int32, device=self.device)
        except Exception:
            self.close()
            raise
        return self

    @classmethod
    def from_text(cls, text, ranges=None, game_mode=2, features="base", n_slots=None, capacity=None, gamma=0.99, include_pass=True, skip_single_action=True,
                  rule=None, device=0, share_stream=True, masked_ok=False, kyoku_scale=1.0 / 1000.0, on_error="raise"):
        """The builder over MJAI JSONL text parsed on the device (no Python work per event).  text: bytes / bytearray / numpy uint8 with
        ranges [M, 2] (begin, end) byte ranges of the logs (any order, gaps allowed) - or, with ranges=None, a list of per-log byte strings.
        on_error: "raise" - a ValueError naming the first log that does not parse, its line and status; "drop" - the set is rebuilt from
        the good logs: `log_ids[i]` is the caller's index of set log i (the `log` field of the samples counts set logs) and `dropped`
        lists (log, line, status) of the others.  The other arguments and every method are LogSampleBuilder's."""
        import time

        t0 = time.perf_counter()
        buf, rng = _text_and_ranges(text, ranges)
        n_players = 3 if vecenv._mode_id(game_mode) >= 3 else 4
        flags = abi.LOGTEXT_MASKED_OK if masked_ok else 0

        def make_set(keep):
            r = rng if keep is None else np.ascontiguousarray(rng[keep])
            h = C.c_void_p()
            vecenv._chk(vecenv.load_lib().rmj_logset_create_from_text(int(device), buf.ctypes.data, r.ctypes.data, len(r), n_players, flags, C.byref(h)))
            return h

        return cls._from_set(make_set, len(rng), game_mode, features, n_slots, capacity, gamma, include_pass, skip_single_action, rule, device, share_stream,
                             kyoku_scale, on_error, time.perf_counter() - t0)

    @classmethod
    def from_jsonl(cls, paths, **kw):
        """from_text over JSONL files read on the host: one log per path; gzip is detected by its magic bytes and decompressed with Python's
        gzip (as MjaiReplay.from_jsonl does)."""
        return cls.from_text([_read_log_file(p) for p in paths], **kw)

    @classmethod
    def from_device_text(cls, text, offsets, game_mode=2, features="base", n_slots=None, capacity=None, gamma=0.99, include_pass=True, skip_single_action=True,
                         rule=None, device=None, share_stream=True, masked_ok=False, kyoku_scale=1.0 / 1000.0, on_error="raise"):
        """The builder over text that already lies in device memory: the (text uint8, offsets int64 [M + 1]) tensors of
        TorchVecEnv.drain_text - log i is text[offsets[i]:offsets[i + 1]].  The text is only read during this call (clone nothing).  Torch's
        current stream is synchronised first: the create call runs on the library's own stream order."""
        import time

        import torch

        t0 = time.perf_counter()
        if not (text.is_cuda and offsets.is_cuda) or text.dtype != torch.uint8:
            raise ValueError("from_device_text takes a uint8 text tensor and an offsets tensor on the GPU")
        dev = text.device.index if device is None else int(device)
        text = text.contiguous()
        o = offsets.to(torch.int64)
        rng = torch.stack([o[:-1], o[1:]], dim=1).contiguous().view(torch.int64)
        n_players = 3 if vecenv._mode_id(game_mode) >= 3 else 4
        flags = abi.LOGTEXT_ON_DEVICE | (abi.LOGTEXT_MASKED_OK if masked_ok else 0)

        def make_set(keep):
            r = rng if keep is None else rng[torch.as_tensor(keep, device=rng.device)].contiguous()
            torch.cuda.current_stream(text.device).synchronize()
            h = C.c_void_p()
            vecenv._chk(vecenv.load_lib().rmj_logset_create_from_text(dev, C.c_void_p(text.data_ptr() if text.numel() else 0), C.c_void_p(r.data_ptr() if r.numel() else 0),
                                                                      int(r.shape[0]), n_players, flags, C.byref(h)))
            return h

        return cls._from_set(make_set, int(rng.shape[0]), game_mode, features, n_slots, capacity, gamma, include_pass, skip_single_action, rule, dev, share_stream,
                             kyoku_scale, on_error, time.perf_counter() - t0)

    # ---- stream order (a builder that keeps the library's own stream synchronises around every call)
    def _pre(self):
        if not self.shared:
            self.torch.cuda.current_stream(self.device).synchronize()

    def _sync(self):
        if not self.shared and self.env is not None:
            self.env.sync()

    def close(self):
        """rmj_logreplay_destroy, the environment, rmj_logset_destroy"""
        if getattr(self, "h", None) and self.env is not None and getattr(self.env, "h", None):
            self.L.rmj_logreplay_destroy(self.h)
        self.h = None
        if getattr(self, "env", None) is not None:
            self.env.close()
            self.env = None
        if getattr(self, "set", None):
            self.L.rmj_logset_destroy(self.set)
        self.set = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the library calls
    def run(self, n_steps=0):
        """n_steps steps of the replay (0: to the end), asynchronous on a shared stream; returns the steps that remain"""
        if self.M == 0:
            return 0
        left = C.c_uint32()
        self._pre()
        vecenv._chk(self.L.rmj_logreplay_run_device(self.h, int(n_steps), C.byref(left)))
        self._sync()
        self._finalized, self._emitted = False, None
        return int(left.value)

    def default_rewards(self):
        """[K, 4] float64: the seats' score change of every kyoku times kyoku_scale (a device tensor, computed there, when the set was parsed
        from text: no host round trip)"""
        if self._d_end is not None:
            t = self.torch
            return (self._d_end.to(t.float64) - self._d_start.to(t.float64)) * self.kyoku_scale
        return (self.end_scores.astype(np.float64) - self.start_scores.astype(np.float64)) * self.kyoku_scale

    def grp_rows(self, num_players=None):
        """riichienv_amd.grp.grp_rows(self): the GRP rank model's rows x, labels rank, meta, log_of of every kyoku, on the device - with a
        model, grp.DeviceRewardPredictor(model, pts_weight).kyoku_rewards(self) is the table finalize() takes"""
        from .grp import grp_rows

        return grp_rows(self, num_players)

    def finalize(self, rewards=None):
        """returns and ranks of the pool's samples (rmj_logreplay_finalize_device); rewards: [K, 4] float64 (numpy or torch) by kyoku
        row, default default_rewards()"""
        if self.M == 0:
            return self
        t = self.torch
        if rewards is None:
            rewards = self.default_rewards()
        rw = t.as_tensor(rewards, dtype=t.float64).reshape(-1, 4).to(self.device).contiguous()
        assert rw.shape[0] == self.n_kyokus, f"the reward table needs one row per kyoku ({self.n_kyokus})"
        if rw.shape[0] == 0:
            rw = t.zeros((1, 4), dtype=t.float64, device=self.device)
        if self._d_end is not None:
            es = self._d_end if self.n_kyokus else t.zeros((1, 4), dtype=t.int32, device=self.device)
        else:
            es = t.as_tensor(self.end_scores if len(self.end_scores) else np.zeros((1, 4), np.int32), dtype=t.int32).to(self.device).contiguous()
        self._pre()
        vecenv._chk(self.L.rmj_logreplay_finalize_device(self.h, C.c_void_p(rw.data_ptr()), C.c_void_p(es.data_ptr())))
        self._sync()
        if self.shared:
            rw.record_stream(t.cuda.current_stream(self.device))
            es.record_stream(t.cuda.current_stream(self.device))
        self._finalized, self._emitted = True, None
        return self

    def counts(self):
        """fill, overflowed (samples that found no pool slot), failed_logs, complete_logs, decisions, events, steps_done, steps_left (waits)"""
        if self.M == 0:
            return {k: 0 for k, _ in abi.LogReplayCounts._fields_}
        c = abi.LogReplayCounts()
        vecenv._chk(self.L.rmj_logreplay_counts(self.h, C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in abi.LogReplayCounts._fields_}

    def clear(self):
        """empty the pool and rewind every slot to its first log (rmj_logreplay_clear)"""
        if self.M:
            vecenv._chk(self.L.rmj_logreplay_clear(self.h))
            self._sync()
        self._finalized, self._emitted = False, None

    def _empty(self, k):
        t, d = self.torch, self.device
        return {"features": t.empty((k, self.channels, self.width), dtype=t.float32, device=d), "mask": t.empty((k, self.A), dtype=t.uint8, device=d),
                "action": t.empty((k,), dtype=t.int64, device=d), "packed": t.empty((k,), dtype=t.int64, device=d),
                "return": t.empty((k,), dtype=t.float32, device=d), "return64": t.empty((k,), dtype=t.float64, device=d),
                "rank": t.empty((k,), dtype=t.int64, device=d), "log": t.empty((k,), dtype=t.int32, device=d), "kyoku": t.empty((k,), dtype=t.int32, device=d),
                "seat": t.empty((k,), dtype=t.int32, device=d), "t": t.empty((k,), dtype=t.int32, device=d)}

    def samples(self):
        """The dataset: {"features" [N, C, W] f32, "action" [N] i64, "return" [N] f32, "return64" [N] f64, "mask" [N, A] u8, "rank" [N] i64,
        "packed" [N] i64 (the packed action's bits), "log", "kyoku", "seat", "t" [N] i32} on the device, in pool order - the samples of the
        logs replayed to their end, without the trajectories that lost a sample to a full pool (rmj_logreplay_emit_device).  Finalizes with
        the default rewards if finalize() was not called since the last run.  Reads the pool's fill on the host to size the tensors.  The
        result is kept (and returned again, the same tensors) until run(), finalize() or clear()."""
        if self.M == 0:
            return self._empty(0)
        if not self._finalized:
            self.finalize()
        if self._emitted is not None:
            return self._emitted
        t = self.torch
        rows = self.counts()["fill"]
        out = self._empty(rows)
        cnt = t.zeros((2,), dtype=t.int32, device=self.device)
        b = abi.LogBatch(out["features"].data_ptr(), out["mask"].data_ptr(), out["action"].data_ptr(), out["packed"].data_ptr(), out["return"].data_ptr(),
                         out["return64"].data_ptr(), out["rank"].data_ptr(), out["log"].data_ptr(), out["kyoku"].data_ptr(), out["seat"].data_ptr(),
                         out["t"].data_ptr(), cnt.data_ptr(), rows, 0)
        self._pre()
        vecenv._chk(self.L.rmj_logreplay_emit_device(self.h, C.byref(b)))
        self._sync()
        k = int(cnt[0])
        self._emitted = {name: v[:k] for name, v in out.items()}
        return self._emitted

    def batches(self, batch_size, shuffle=True, generator=None):
        """One epoch over samples() as `(features, actions, targets, masks, ranks)` tuples - MCDataset's order of fields - of batch_size rows
        (the last one shorter).  shuffle draws one permutation from `generator` (a torch.Generator on the CPU; None: torch's global one)."""
        t = self.torch
        s = self.samples()
        n = int(s["action"].shape[0])
        order = (t.randperm(n, generator=generator) if shuffle else t.arange(n)).to(self.device)
        for i in range(0, n, int(batch_size)):
            idx = order[i: i + int(batch_size)]
            yield s["features"][idx], s["action"][idx], s["return"][idx], s["mask"][idx], s["rank"][idx]
