"""Behaviour-cloning / offline-RL samples from MJAI logs, built on the device: what riichienv-ml's MCDataset yields
(datasets/mjai_logs.py:62-129) - per decision `(features, action_id, G_t, mask, rank)` with G_t = reward * gamma ** (T - t - 1) over the
seat's decisions of the kyoku and rank the seat's place in the kyoku's end scores - for many logs at once.

The logs become one device log set (logset.LogSet, the one owner of the library's log set: event dicts packed on the host with
abi.event_records_from_mjai and uploaded, or MJAI text parsed on the device); from there on the replay is kernels of the library
(rmj_logreplay_*: csrc/rmj_logreplay.hip.h): the next event of every log is matched against the published legal lists on the device,
the deciding seats' rows are encoded straight into a pool, the event is applied - no host work per event, no host synchronisation
inside the replay.  ReplayBatch.samples() / Kyoku.steps() compute the same samples through the host and stay as the checker.

M logs run in n_slots <= M games; a slot whose log ends takes its next one.  Which slot gets which logs is decided before the replay
(`assign_slots`): logs in order, each to the slot that is free first when every event takes one step, ties to the lowest slot - a pure
function of (M, n_slots, the logs' lengths), so two runs fill the pool in the same order.

What the records do not carry.  Matching follows the packed records, which hold less than the MJAI text: a dahai without a `tsumogiri`
field reads as tsumogiri = false (select_action_from_mjai skips the drawn-tile rule when the field is absent, so on third-party logs
without it the builder may pick the other tile of the same name), a kakan is matched by its tile name without `consumed`, and the seat
a robbed kan is taken from is the log's previous actor, not the hora's `target`.  On logs that a game produced these agree.  The only
failure the builder detects is a decision that matches nothing in the list its actor is offered; an event that does not fit the state in
another way (a decision by a seat that is not to act) is applied like apply_events applies it and the log counts as complete.  For logs
of unknown quality call validate() first (LogSet.validate, logcheck.py): a checking replay that gives every log a verdict.

Memory: the pool is capacity x (C x W x 4 + A + 52) bytes (+ 152 with hidden=True), and samples() holds a second copy of what it emits (fill x the same row) until
the next run() / finalize() / clear() - at the default capacity about three times the samples' own size in all.  What does not fit is counted (`counts()["overflowed"]`) and the trajectory that lost a
sample is not emitted; a log in which a decision matches no legal action is dropped whole (`counts()["failed_logs"]`), like a file whose
replay raises in MCDataset."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import abi, vecenv
from .logset import _DECISION_TYPES, LogSet, check_on_error, kyoku_tables, pack_logs  # noqa: F401  (re-exported: callers know them by this module)
from .streams import StreamLink


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


def parse_logs_device(text, ranges=None, num_players=4, masked_ok=False, device=0):
    """MJAI JSONL text -> the packed records, parsed on the device, as a dict of torch tensors on the GPU: LogSet.tensors() of a set that
    keeps the logs that do not parse (their status says so).  text / ranges as in LogSet.from_text, or a uint8 tensor on the GPU with
    ranges an int64 [M, 2] tensor there."""
    if getattr(text, "is_cuda", False):
        s = LogSet.from_device_text(text, ranges, num_players, masked_ok, on_error="keep")
    else:
        s = LogSet.from_text(text, ranges, num_players, masked_ok, device, on_error="keep")
    try:
        return s.tensors()
    finally:
        s.close()


# The extra columns a builder can keep beside the plain ones, in the order the library records them: the setting that asks for them, its
# RMJ_LOGREPLAY_* flag, the row target whose fields they are (abi.ROW_TARGETS) - under `prefix` + the field's name, without the fields
# in `skip` (the pool does not keep them) - columns of their own, the batch struct (the columns in this order, then rows and a reserved
# word) with its emit entry, and why a log set with masked tiles is refused.
_Extra = collections.namedtuple("_Extra", "setting flag target prefix skip more batch emit masked")
_EXTRAS = (
    _Extra("hidden", abi.LOGREPLAY_HIDDEN, "hidden", "", (), (abi.RowField("event", "int32", (), 0),), abi.LogHiddenBatch, "rmj_logreplay_emit_hidden_device",
           "the masked seats' tiles are unknown, so are their hands, shanten and waits"),
    _Extra("danger", abi.LOGREPLAY_DANGER, "danger", "", (), (), abi.LogDangerBatch, "rmj_logreplay_emit_danger_device",
           "the masked seats' tiles are unknown, so is what they would win"),
    _Extra("efficiency", abi.LOGREPLAY_DTABLE, "discard_table", "dt_", ("mask",), (), abi.LogDtableBatch, "rmj_logreplay_emit_dtable_device",
           "the set does not tell which seats' tiles are masked, and a masked deciding seat has no hand to tabulate"),
)


def _extra_columns(x):
    """[(sample key, abi.RowField)] of an extra, in the order of its batch struct"""
    return [(x.prefix + f.name, f) for f in abi.ROW_TARGETS[x.target].fields if f.name not in x.skip] + [(f.name, f) for f in x.more]


class LogSampleBuilder:
    """b = LogSampleBuilder(logs, game_mode=2, features="base"); b.run(); s = b.samples()

    logs: lists of MJAI event dicts, MjaiReplay objects or MjSoulReplay objects (their to_mjai()).  from_text / from_jsonl /
    from_device_text take what LogSet's constructors of those names take; from_logset replays a LogSet the caller made (and keeps).
    The settings, by keyword, of every constructor:
    features="base": "base" (74 x W), "discard_shanten" (94 x 34, 4P only) or "extended" (215 x W).
    n_slots=None: games replayed at once (default and at most: the number of logs).  capacity=None: pool size in samples.  The default -
    twice the logs' decision events - is a heuristic, not a bound: a discard can add a Pass sample for up to three seats, and those are
    not counted.  Check counts()["overflowed"] after run(); it is 0 on every log set of the tests.  rule=None: "tenhou" (default) or
    "mjsoul".  gamma=0.99, include_pass=True, skip_single_action=True, share_stream=True, kyoku_scale=1 / 1000.
    hidden=False: with True every sample also carries what its seat could not see - samples() gains "opp_hand" [N, 3, 34] u8, "opp_shanten"
    [N, 3] i8, "opp_waits" [N, 3] i64, "opp_flags" [N, 3] u8 (the rows of TorchVecEnv.hidden_compact: the opponents (seat + 1 + r) mod NP
    at the moment of the decision) and "event" [N] i32, the index in the log of the event the decision precedes; 152 more bytes per pool
    slot.  ValueError over a log set made with masked_ok=True: "?" tiles make those targets meaningless.
    danger=False: with True samples() gains "danger" [N, 3, 37] i32 - the points opponent (seat + 1 + r) mod NP would win by ron if the
    deciding seat discarded a tile of kind c at the moment of the decision (the rows of TorchVecEnv.danger_compact without ura: logs
    carry no wall); 224 more bytes per pool slot.  Independent of hidden, combinable with it, refused over masked sets like it.
    efficiency=False: with True samples() gains "dt_shanten" [N, 35] i8, "dt_accept" [N, 35] u8, "dt_ukeire" [N, 35] u8 - the discard efficiency
    table of the deciding seat at the moment of the decision (the rows of TorchVecEnv.discard_table_compact without the masks: column t <
    34 the shanten after discarding type t, abi.DTAB_NONE where there is no such discard, the types that then lower it and their live
    tiles; column 34 the hand itself); 112 more bytes per pool slot.  Independent of hidden and danger, combinable with them.  The table
    needs only the deciding seat's own hand, but a set made with masked_ok=True does not say per sample whether that seat's tiles were
    masked, so it is refused over such sets like danger.
    rewards: finalize(rewards) takes a float64 [K, 4] table by kyoku row (`kyoku_offsets[log] + kyoku - 1`; the GRP reward model's
    output) - default: the seat's score change of the kyoku times kyoku_scale.
    on_error (text): "raise" or "drop" as LogSet takes them; after a drop the `log` field of the samples counts set logs (`log_ids`)."""

    def __init__(self, logs, game_mode=2, *, device=0, masked_ok=False, **settings):
        logs = list(logs)
        self._settings(game_mode, **settings)._slots(len(logs))
        self._attach(LogSet.from_logs(logs, self.n_players, masked_ok, device), True)

    @classmethod
    def from_logset(cls, logset, game_mode=2, **settings):
        """The builder over a LogSet the caller made: close() leaves the set open, for the caller to close after the builder."""
        return cls.__new__(cls)._settings(game_mode, **settings)._attach(logset, False)

    @classmethod
    def from_text(cls, text, ranges=None, game_mode=2, *, device=0, masked_ok=False, on_error="raise", **settings):
        """The builder over MJAI JSONL text parsed on the device (no Python work per event): LogSet.from_text"""
        self = cls.__new__(cls)._settings(game_mode, on_error, **settings)
        return self._attach(LogSet.from_text(text, ranges, self.n_players, masked_ok, device, on_error), True)

    @classmethod
    def from_jsonl(cls, paths, game_mode=2, *, device=0, masked_ok=False, on_error="raise", **settings):
        """from_text over JSONL files read on the host, one log per path: LogSet.from_jsonl"""
        self = cls.__new__(cls)._settings(game_mode, on_error, **settings)
        return self._attach(LogSet.from_jsonl(paths, num_players=self.n_players, masked_ok=masked_ok, device=device, on_error=on_error), True)

    @classmethod
    def from_device_text(cls, text, offsets, game_mode=2, *, device=None, masked_ok=False, on_error="raise", **settings):
        """The builder over text that already lies in device memory (TorchVecEnv.drain_text), which is only read during this call:
        LogSet.from_device_text"""
        self = cls.__new__(cls)._settings(game_mode, on_error, **settings)
        return self._attach(LogSet.from_device_text(text, offsets, self.n_players, masked_ok, device, on_error), True)

    def _settings(self, game_mode, on_error="raise", features="base", n_slots=None, capacity=None, gamma=0.99, include_pass=True, skip_single_action=True,
                  rule=None, share_stream=True, kyoku_scale=1.0 / 1000.0, hidden=False, danger=False, efficiency=False):
        """validates and stores what every constructor shares (no device work)"""
        import torch

        check_on_error(on_error, ("raise", "drop"))
        if features not in abi.FEATURES:
            raise ValueError(f"unknown feature set {features!r}: one of {sorted(abi.FEATURES)}")
        if rule not in (None, "tenhou", "mjsoul"):
            raise ValueError(f"Unknown rule: '{rule}'. Expected 'tenhou' or 'mjsoul'")
        if capacity is not None and int(capacity) <= 0:
            raise ValueError("capacity must be positive (samples)")
        self.torch, self.L, self.rule = torch, vecenv.load_lib(), rule
        self.game_mode = vecenv._mode_id(game_mode)
        self.sanma = self.game_mode >= 3
        self.n_players = 3 if self.sanma else 4
        self.features, self._feat = features, abi.FEATURES[features]
        self.channels, self.width = abi.FEATURE_CHANNELS[self._feat], 27 if self.sanma else 34
        self.A = abi.ACTION_SPACE_3P if self.sanma else abi.ACTION_SPACE_4P
        self.n_slots, self.capacity = n_slots, capacity
        self.gamma, self.kyoku_scale = float(gamma), float(kyoku_scale)
        self.include_pass, self.skip_single_action = bool(include_pass), bool(skip_single_action)
        self.shared, self.hidden, self.danger, self.efficiency = bool(share_stream), bool(hidden), bool(danger), bool(efficiency)
        self._finalized = False
        self._emitted = None    # what samples() returned last, until run() / finalize() / clear()
        self.h = self.env = self.logset = None
        return self

    def _slots(self, m):
        """n_slots for m logs"""
        n = m if self.n_slots is None else int(self.n_slots)
        if n > m or (m and n < 1):
            raise ValueError(f"n_slots must be between 1 and the number of logs ({m})")
        return n

    # the kyoku score tables are the log set's: host arrays for dict logs; for a set parsed from text they stay on the device and a host
    # copy is made only when the attribute is read
    start_scores = property(lambda self: self.logset.start_scores, lambda self, v: setattr(self.logset, "start_scores", v))
    end_scores = property(lambda self: self.logset.end_scores, lambda self, v: setattr(self.logset, "end_scores", v))

    def _attach(self, logset, owned):
        """the environment, the replay and the pool views over the log set; `owned`: close() closes the set too"""
        self.logset, self._owned = logset, owned
        try:
            assert self.n_players == logset.num_players, "the log set was made for another number of players"
            self._extras = [x for x in _EXTRAS if getattr(self, x.setting)]
            for x in self._extras:
                if getattr(logset, "masked_ok", False):
                    raise ValueError(f"{x.setting}=True over a log set made with masked_ok=True: {x.masked}")
            for k in ("logs", "M", "device", "kyoku_offsets", "n_kyokus", "log_ids", "dropped", "lengths"):
                setattr(self, k, getattr(logset, k))
            self.host_seconds = dict(logset.host_seconds)
            self.n_slots = self._slots(self.M)
            self.capacity = int(2 * int(logset.decisions.sum()) + 64 if self.capacity is None else self.capacity)
            if self.M == 0:
                return self
            torch, L = self.torch, self.L
            bits = abi.RULE_MJSOUL if self.rule == "mjsoul" else abi.RULE_TENHOU
            self.env = vecenv.VecRiichiEnv(self.n_slots, game_mode=self.game_mode, seed=0, rule_bits=bits, device=logset.device_index, skip_mjai_logging=True)
            self.link = StreamLink(torch, self.device, self.env, owner=self)   # stream order and pointer passing of every call: streams.py
            if self.shared:
                self.link.bind()
            self._powers = gamma_powers(self.gamma, logset.longest_log + 1)
            flags = (abi.LOGREPLAY_INCLUDE_PASS if self.include_pass else 0) | (abi.LOGREPLAY_SKIP_SINGLE_ACTION if self.skip_single_action else 0) | \
                sum(x.flag for x in self._extras)
            cfg = abi.LogReplayConfig(self._feat, self.capacity, flags, len(self._powers), self.gamma, self._powers.ctypes.data)
            h = C.c_void_p()
            self.link.call(L.rmj_logreplay_create, self.env.h, logset.handle, C.byref(cfg), C.byref(h))
            self.h = h
            v = abi.LogReplayViews()
            vecenv._chk(L.rmj_logreplay_views(self.h, C.byref(v)))
            self.steps = int(v.steps)
            wrap = self.link.wrap
            cap, fl, K = self.capacity, self.channels * self.width, max(self.n_kyokus, 1)
            rows = wrap(v.features, (cap, v.row_stride), "<f4")
            self.pool = {"features": rows[:, :fl].unflatten(-1, (self.channels, self.width)), "mask": wrap(v.mask, (cap, self.A), "|u1"),
                         "action": wrap(v.action, (cap,), "<i4"), "packed": wrap(v.packed, (cap,), "<i8"), "return": wrap(v.ret, (cap,), "<f4"),
                         "return64": wrap(v.ret64, (cap,), "<f8"), "rank": wrap(v.rank, (cap,), "<i4"), "log": wrap(v.log, (cap,), "<i4"),
                         "kyoku": wrap(v.kyoku, (cap,), "<i4"), "seat": wrap(v.seat, (cap,), "<i4"), "t": wrap(v.t, (cap,), "<i4"),
                         "log_status": wrap(v.log_status, (self.M,), "|u1"), "traj_len": wrap(v.traj_len, (K, 4), "<i4"),
                         "traj_broken": wrap(v.traj_broken, (K, 4), "|u1"), "counters": wrap(v.counters, (6,), "<i4")}
            if self.hidden:   # the records as they lie: [capacity, 152] bytes (header: RmjLogHiddenViews)
                hv = abi.LogHiddenViews()
                vecenv._chk(L.rmj_logreplay_hidden_views(self.h, C.byref(hv)))
                self.pool["hidden"] = wrap(hv.records, (cap, hv.record_bytes), "|u1")
        except Exception:
            self.close()
            raise
        return self

    def close(self):
        """rmj_logreplay_destroy, the environment, and the log set if the builder made it"""
        if getattr(self, "h", None) and self.env is not None and getattr(self.env, "h", None):
            self.L.rmj_logreplay_destroy(self.h)
        self.h = None
        if getattr(self, "env", None) is not None:
            self.env.close()
            self.env = None
        if getattr(self, "_owned", False):
            self.logset.close()

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
        self.link.call(self.L.rmj_logreplay_run_device, self.h, int(n_steps), C.byref(left))
        self._finalized, self._emitted = False, None
        return int(left.value)

    def default_rewards(self):
        """[K, 4] float64: the seats' score change of every kyoku times kyoku_scale (a device tensor, computed there, when the set was parsed
        from text: no host round trip)"""
        if self.logset.owns_tables:
            t, (start, end) = self.torch, self.logset.device_scores()
            return (end.to(t.float64) - start.to(t.float64)) * self.kyoku_scale
        return (self.end_scores.astype(np.float64) - self.start_scores.astype(np.float64)) * self.kyoku_scale

    def grp_rows(self, num_players=None):
        """LogSet.grp_rows of the builder's set: the GRP rank model's rows x, labels rank, meta, log_of of every kyoku, on the device - with a
        model, grp.DeviceRewardPredictor(model, pts_weight).kyoku_rewards(self) is the table finalize() takes"""
        return self.logset.grp_rows(num_players)

    def play_stats(self, num_players=None):
        """LogSet.play_stats of the builder's set: how every seat played every kyoku, on the device (riichienv_amd.stats summarises it)"""
        return self.logset.play_stats(num_players)

    def validate(self, n_slots=None):
        """LogSet.validate of the builder's set, with the builder's game mode and rule: a verdict for every log (logcheck.LogReport), by a
        checking replay of its own - the builder's pool and slots are not touched"""
        return self.logset.validate(self.game_mode, self.rule, n_slots, self.shared)

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
        if self.logset.owns_tables:
            es = self.logset.device_scores()[1] if self.n_kyokus else t.zeros((1, 4), dtype=t.int32, device=self.device)
        else:
            es = t.as_tensor(self.end_scores if len(self.end_scores) else np.zeros((1, 4), np.int32), dtype=t.int32).to(self.device).contiguous()
        self.link.call(self.L.rmj_logreplay_finalize_device, self.h, rw, es)
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
            self.link.call(self.L.rmj_logreplay_clear, self.h)
        self._finalized, self._emitted = False, None

    def _empty(self, k):
        t = self.torch
        extra = {key: t.empty((k,) + f.shape, dtype=abi.torch_dtype(t, f.dtype), device=self.device) for x in self._extras for key, f in _extra_columns(x)}
        return {**self._empty_plain(k), **extra}

    def _empty_plain(self, k):
        t, d = self.torch, self.device
        return {"features": t.empty((k, self.channels, self.width), dtype=t.float32, device=d), "mask": t.empty((k, self.A), dtype=t.uint8, device=d),
                "action": t.empty((k,), dtype=t.int64, device=d), "packed": t.empty((k,), dtype=t.int64, device=d),
                "return": t.empty((k,), dtype=t.float32, device=d), "return64": t.empty((k,), dtype=t.float64, device=d),
                "rank": t.empty((k,), dtype=t.int64, device=d), "log": t.empty((k,), dtype=t.int32, device=d), "kyoku": t.empty((k,), dtype=t.int32, device=d),
                "seat": t.empty((k,), dtype=t.int32, device=d), "t": t.empty((k,), dtype=t.int32, device=d)}

    def samples(self):
        """The dataset: {"features" [N, C, W] f32, "action" [N] i64, "return" [N] f32, "return64" [N] f64, "mask" [N, A] u8, "rank" [N] i64,
        "packed" [N] i64 (the packed action's bits), "log", "kyoku", "seat", "t" [N] i32} - with hidden=True also "opp_hand", "opp_shanten",
        "opp_waits", "opp_flags" and "event", with danger=True "danger", with efficiency=True "dt_shanten", "dt_accept", "dt_ukeire" (class docstring), same rows, same order - on the device, in pool order - the samples of the
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
        self.link.call(self.L.rmj_logreplay_emit_device, self.h, C.byref(b))
        for x in self._extras:
            xb = x.batch(*(out[key].data_ptr() for key, _ in _extra_columns(x)), rows, 0)
            self.link.call(getattr(self.L, x.emit), self.h, C.byref(xb))
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
