"""The GRP rank model's data on the device: what riichienv-ml's GRP stage computes on the host from every log
(datasets/grp_dataset.py GrpReplayDataset, models/grp_model.py RewardPredictor.calc_all_player_rewards, trainers/_ppo_worker.py:100-116).

The row of (kyoku, seat p), n players, is 4n + 4 float32
    init[0..n) / S, end[0..n) / S, delta[0..n) / 12000, chang / 3, ju / 3, ben / 4, liqibang / 4, onehot(p)[0..n)
with S = 25000 (4P) / 35000 (3P) - bit-equal to the reference's rows (every quotient is a float64 division rounded once to float32).
The rows come from the records and score tables a log set already holds on the device (rmj_logset_grp_device), or from the round
tracker's tensors of live games (rmj_grp_rows_device): csrc/rmj_grp.hip.h.  Torch is used for the model, for device memory and for
the element-wise ops around the two calls.

    grp_rows(source)                    x, rank, meta, log_of, kyoku_offsets of every kyoku of a LogSet (logset.py: the one owner of the
                                        device log set), or of the set of a LogSampleBuilder / GrpDataset
    GrpDataset                          GrpReplayDataset's (x, one-hot rank) stream from logs, text, JSONL files or device text
    DeviceRewardPredictor               the [K, 4] reward table LogSampleBuilder.finalize takes, and PPOCollector's reward_fn"""
from __future__ import annotations

import time

import numpy as np

from . import vecenv
from .logset import LogSet, check_on_error
from .streams import stream_ptr

_BUILDER_ONLY = ("features", "n_slots", "capacity", "gamma", "include_pass", "skip_single_action", "rule", "share_stream", "kyoku_scale")
_KEEP = {"raise": "raise", "drop": "keep"}    # GrpDataset's "drop" keeps the log in the set: its kyokus get rank 255 and tensors() filters them


def _players(game_mode, kw, on_error="raise"):
    """the arguments of GrpDataset's constructors, checked before any device work; returns the number of players"""
    unknown = set(kw) - set(_BUILDER_ONLY)
    if unknown:
        raise TypeError(f"unexpected arguments {sorted(unknown)}")
    check_on_error(on_error, ("raise", "drop"))
    return 3 if vecenv._mode_id(game_mode) >= 3 else 4


def live_rows(init, delta, meta, num_players, out=None):
    """rmj_grp_rows_device: init, delta, meta int32 [rows, 4] device tensors -> x [rows, n, 4n + 4] float32 (end = init + delta; meta =
    (chang, ju, ben, liqibang) as TorchVecEnv.round_track gives it).  Asynchronous on torch's current stream."""
    import torch

    n = int(num_players)
    init, delta, meta = (t.to(torch.int32).contiguous() for t in (init, delta, meta))
    rows = int(init.shape[0])
    assert init.is_cuda and tuple(init.shape) == tuple(delta.shape) == tuple(meta.shape) == (rows, 4)
    x = torch.empty((rows, n, 4 * n + 4), dtype=torch.float32, device=init.device) if out is None else out
    assert x.is_contiguous() and tuple(x.shape) == (rows, n, 4 * n + 4) and x.dtype == torch.float32
    vecenv._chk(vecenv.load_lib().rmj_grp_rows_device(init.device.index, init.data_ptr(), delta.data_ptr(), meta.data_ptr(), rows, n, x.data_ptr(),
                                                      stream_ptr(torch, init.device)))
    return x


def grp_rows(source, num_players=None):
    """LogSet.grp_rows of `source` - a LogSet, or the set of a LogSampleBuilder or a GrpDataset: the GRP rows of every kyoku as device
    tensors.  num_players defaults to the set's.  Asynchronous on torch's current stream; nothing is read back."""
    return (source if isinstance(source, LogSet) else source.logset).grp_rows(num_players)


class GrpDataset:
    """ds = GrpDataset(logs, game_mode=2); for x, y in ds.batches(256): ...

    GrpReplayDataset's stream - for every kyoku of every log and every seat, x [4n + 4] and y = the one-hot of the seat's final rank in
    the log - built on the device, without its file shuffling: batches() draws one permutation over all rows.  logs: lists of MJAI event
    dicts, MjaiReplay or MjSoulReplay objects; from_text / from_jsonl / from_device_text parse MJAI JSONL text on the device and take the
    arguments of LogSampleBuilder's constructors of those names (the replay-only ones - features, capacity, gamma, ... - are accepted
    and unused: no game is replayed); from_logset takes a LogSet the caller made (and keeps).  on_error: "raise" - a ValueError naming the
    first log that does not parse; "drop" - its rows are left out (`dropped` lists (log, line, status); the `log` field of tensors()
    keeps the caller's numbering)."""

    def __init__(self, logs, game_mode=2, device=0, masked_ok=False, **kw):
        self._adopt(LogSet.from_logs(logs, _players(game_mode, kw), masked_ok, device), True, game_mode)

    @classmethod
    def from_logset(cls, logset, **kw):
        """over a LogSet the caller made: close() leaves the set open"""
        _players(2, kw)
        return cls.__new__(cls)._adopt(logset, False)

    @classmethod
    def from_text(cls, text, ranges=None, game_mode=2, device=0, masked_ok=False, on_error="raise", **kw):
        """MJAI JSONL text parsed on the device: text / ranges as LogSet.from_text takes them"""
        n = _players(game_mode, kw, on_error)
        return cls.__new__(cls)._adopt(LogSet.from_text(text, ranges, n, masked_ok, device, _KEEP[on_error]), True, game_mode)

    @classmethod
    def from_jsonl(cls, paths, game_mode=2, device=0, masked_ok=False, on_error="raise", **kw):
        """from_text over JSONL files read on the host: one log per path, gzip detected by its magic bytes"""
        n = _players(game_mode, kw, on_error)
        return cls.__new__(cls)._adopt(LogSet.from_jsonl(paths, num_players=n, masked_ok=masked_ok, device=device, on_error=_KEEP[on_error]), True, game_mode)

    @classmethod
    def from_device_text(cls, text, offsets, game_mode=2, device=None, masked_ok=False, on_error="raise", **kw):
        """over the (text uint8, offsets int64 [M + 1]) device tensors of TorchVecEnv.drain_text; the text is only read during this call"""
        n = _players(game_mode, kw, on_error)
        return cls.__new__(cls)._adopt(LogSet.from_device_text(text, offsets, n, masked_ok, device, _KEEP[on_error]), True, game_mode)

    def _adopt(self, logset, owned, game_mode=None):
        self.logset, self._owned, self.torch = logset, owned, logset.torch
        self.game_mode, self.n_players = None if game_mode is None else vecenv._mode_id(game_mode), logset.num_players
        self.M, self.device, self.kyoku_offsets, self.n_kyokus, self.dropped = logset.M, logset.device, logset.kyoku_offsets, logset.n_kyokus, logset.dropped
        self.host_seconds = dict(logset.host_seconds)
        self._rows = self._tensors = None
        return self

    start_scores = property(lambda self: self.logset.start_scores)
    end_scores = property(lambda self: self.logset.end_scores)

    def close(self):
        if self._owned:
            self.logset.close()

    def grp_rows(self):
        """the set's grp_rows(), computed once"""
        if self._rows is None:
            self._rows = self.logset.grp_rows()
        return self._rows

    def play_stats(self, num_players=None):
        """LogSet.play_stats of the set: how every seat played every kyoku, on the device (riichienv_amd.stats summarises it)"""
        return self.logset.play_stats(num_players)

    def validate(self, rule=None, n_slots=None):
        """LogSet.validate of the set, in the dataset's game mode: a verdict for every log (logcheck.LogReport) - a log that did not parse,
        which this dataset keeps out of its rows, is PARSE there"""
        return self.logset.validate(self.game_mode, rule, n_slots)

    def tensors(self):
        """Every (kyoku, seat) row of the good logs at once, in (log, kyoku, seat) order: {"x" [R, 4n + 4] f32, "y" [R, n] f32 (one-hot of
        rank), "rank" [R] i64, "log", "kyoku" (the table row), "seat" [R] i32} on the device.  Reads the row count on the host once."""
        if self._tensors is not None:
            return self._tensors
        t, n = self.torch, self.n_players
        t0 = time.perf_counter()
        r = self.grp_rows()
        K = int(r["x"].shape[0])
        rank = r["rank"].reshape(K * n)
        rows = t.arange(K * n, device=self.device, dtype=t.int32)
        kyoku, seat = t.div(rows, n, rounding_mode="floor"), rows % n
        log = r["log_of"].repeat_interleave(n)
        x = r["x"].reshape(K * n, 4 * n + 4)
        if self.dropped:
            keep = rank != 255
            x, rank, kyoku, seat, log = x[keep], rank[keep], kyoku[keep], seat[keep], log[keep]
        rank = rank.to(t.int64)
        y = t.zeros((rank.shape[0], n), dtype=t.float32, device=self.device)
        y.scatter_(1, rank[:, None], 1.0)
        self._tensors = {"x": x, "y": y, "rank": rank, "log": log, "kyoku": kyoku, "seat": seat}
        t.cuda.current_stream(self.device).synchronize()
        self.host_seconds["rows"] = time.perf_counter() - t0
        return self._tensors

    def batches(self, batch_size, generator=None, shuffle=True):
        """One epoch of `(x [B, 4n + 4] f32, y [B, n] f32)` batches (the last one shorter); shuffle draws one permutation from `generator`
        (a torch.Generator on the CPU; None: torch's global one)."""
        t = self.torch
        s = self.tensors()
        rows = int(s["x"].shape[0])
        order = (t.randperm(rows, generator=generator) if shuffle else t.arange(rows)).to(self.device)
        for i in range(0, rows, int(batch_size)):
            idx = order[i: i + int(batch_size)]
            yield s["x"][idx], s["y"][idx]


class DeviceRewardPredictor:
    """RewardPredictor (models/grp_model.py) on the device: reward = softmax(model(x), 1) @ pts_weight.float() - float(np.mean(pts_weight)),
    evaluated in float32 under inference_mode.  model: any torch module mapping [*, 4n + 4] -> [*, n], already on the device with its
    weights loaded (riichienv-ml's RankPredictor is Linear 4n+4 -> 128 -> 64 -> n with ReLU between)."""

    def __init__(self, model, pts_weight, num_players=4):
        import torch

        self.torch, self.model, self.n = torch, model.eval(), int(num_players)
        self.pts_weight = [float(v) for v in pts_weight]
        assert len(self.pts_weight) == self.n, "one weight per rank"
        self.mean_pts = float(np.mean(self.pts_weight))
        self._pts = {}

    def _rewards(self, x):
        """[R, 4n + 4] -> [R] float32"""
        t = self.torch
        with t.inference_mode():
            if x.device not in self._pts:
                self._pts[x.device] = t.tensor(self.pts_weight, device=x.device).float()
            return t.softmax(self.model(x), dim=1) @ self._pts[x.device] - self.mean_pts

    def kyoku_rewards(self, builder):
        """[K, 4] float64 device tensor by kyoku row, what LogSampleBuilder.finalize(rewards) takes: every seat's reward of every kyoku of
        the builder (or GrpDataset); seat 3 is 0 in 3P."""
        t, n = self.torch, self.n
        x = grp_rows(builder, n)["x"]
        K = int(x.shape[0])
        out = t.zeros((K, 4), dtype=t.float64, device=x.device)
        if K:
            out[:, :n] = self._rewards(x.reshape(K * n, 4 * n + 4)).reshape(K, n).to(t.float64)
        return out

    def reward_fn(self, tenv):
        """A callable with the signature of PPOCollector.collect's `reward_fn` - (delta [n, 4] i32, meta [n, 4] i32, ended [n] u8,
        hero [n] u8) -> [n] float32: the hero's reward for the games that close a trajectory in this step, 0 elsewhere (a hero of 255: 0).

        reward_fn is handed score changes but no scores, and the environment's own scores may already be the next game's when a game
        ends, so the adapter keeps the scores at the opening of every game's current trajectory itself: taken from `tenv.scores()`
        here (create it where the collector's trajectories open: before the first collect, or right after a reset), moved by `delta`
        where a round ends, and set to the mode's starting scores (25000 / 35000) where the game ends - what an auto-reset deals.
        `.rebase()` of the returned callable re-reads the environment's scores (after a reset with other scores).  No host
        synchronisation per call.

        Boundary modes: PPOCollector(boundary="round") only - there `ended` is 1 at a round end and 2 at the game's end.  Under
        boundary="kyoku_idx" the collector passes ended = 0 / 1 and swallows game ends that close nothing, so the opening scores
        cannot be followed from the arguments; do not use it there."""
        return _LiveReward(self, tenv)


class _LiveReward:
    def __init__(self, predictor, tenv):
        self.p, self.tenv, self.t = predictor, tenv, predictor.torch
        n_players = 3 if tenv.sanma else 4
        assert n_players == predictor.n, "the predictor's num_players and the environment's game mode disagree"
        t = self.t
        self.fresh = t.zeros((tenv.n, 4), dtype=t.int32, device=tenv.device)
        self.fresh[:, :n_players] = 35000 if tenv.sanma else 25000
        self.rebase()

    def rebase(self):
        """the opening scores of every game's current trajectory = the environment's scores now"""
        self.open = self.tenv.scores().to(self.t.int32).clone()

    def __call__(self, delta, meta, ended, hero):
        t, n = self.t, self.p.n
        x = live_rows(self.open, delta, meta, n)                              # [games, n, 4n + 4]
        h = hero.to(t.int64)
        seat = h.clamp(max=n - 1)
        hx = x[t.arange(x.shape[0], device=x.device), seat]
        r = self.p._rewards(hx)
        closes = (ended != 0) & (h < n)
        reward = t.where(closes, r, t.zeros_like(r))
        self.open = t.where((ended == 2)[:, None], self.fresh, t.where((ended == 1)[:, None], self.open + delta, self.open))
        return reward
