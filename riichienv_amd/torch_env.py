"""Trainer-side batched environment: a Gym-style loop over all games of a shard with the policy
on the same GPU.  Observations are encoded straight into torch tensors (rmj_encode_device / rmj_encode_extended_device),
masks / legal lists / status are zero-copy views of the library's device slabs, actions are the policy's categorical
ids (rmj_step_ids_device = Observation.find_action + RiichiEnv.step), rewards come from scores()/ranks()
(riichienv-python/src/env.rs:401-404, 673-727).  Replaces the per-game Python loop of
riichienv-ml trainers/_ppo_worker.py:113-466.

torch is used for device memory and streams only; all game logic runs in the HIP library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, vecenv
from .streams import StreamLink
from .abi import _CudaArray  # noqa: F401  (imported from here by tests and scripts)


class TorchVecEnv:
    """`n_games` games on one GPU driven by a torch policy.

    obs(), mask, status … describe the state AFTER the last step; step(action_ids) takes an int32 tensor [n, 4] on the
    same device (-1 for seats that do not act)."""

    def __init__(self, n_games, game_mode=2, seed=0, device=0, extended=False, skip_mjai_logging=True, share_stream=True, pad_rows=True,
                 features=None, **kw):
        """share_stream: issue the library's kernels on torch's current stream of `device` (rmj_set_stream): policy and
        environment are then ordered by the stream, without host synchronisation between them.  With False the library keeps
        its own stream and every call synchronises.
        features: the observation every obs / step_obs / compact call returns - "base" (Observation.encode(), 74 x W),
        "discard_shanten" (riichienv-ml feat_v2: encode() + discard decay + shanten efficiency, 94 x 34, 4P only) or "extended"
        (Observation.encode_extended(), 215 x W); extended=True is a synonym for features="extended"."""
        import torch

        if features is None:
            features = "extended" if extended else "base"
        if features not in abi.FEATURES:
            raise ValueError(f"unknown feature set {features!r} (one of {', '.join(abi.FEATURES)})")
        if extended and features != "extended":
            raise ValueError(f"extended=True conflicts with features={features!r}")
        if features == "discard_shanten" and vecenv._mode_id(game_mode) >= 3:
            raise ValueError("the discard_shanten feature set (riichienv-ml feat_v2) is 4-player only")

        self.torch = torch
        self.device = torch.device("cuda", device)
        self.env = vecenv.VecRiichiEnv(n_games, game_mode=game_mode, seed=seed, device=device,
                                       skip_mjai_logging=skip_mjai_logging, **kw)
        L = self.env.L
        self.n = int(n_games)
        self.sanma = self.env.game_mode >= 3
        self.features = features
        self._feat = abi.FEATURES[features]
        self.extended = features == "extended"
        self.channels = abi.FEATURE_CHANNELS[self._feat]
        self.width = 27 if self.sanma else 34
        self.link = StreamLink(torch, self.device, self.env, owner=self)   # stream order and pointer passing of every call: streams.py
        v = abi.DeviceViews()
        vecenv._chk(L.rmj_device_views(self.env.h, C.byref(v)))
        wrap = self.link.wrap
        self.status_raw = wrap(v.status, (self.n,), "<u4") if hasattr(torch, "uint32") else wrap(v.status, (self.n,), "<i4")
        self.nlegal = wrap(v.nlegal, (self.n, 4), "|u1")
        self.mask = wrap(v.mask, (self.n, 4, abi.ACTION_SPACE_4P), "|u1")      # zero-copy, rewritten by every step
        self.legal = wrap(v.legal, (self.n, 4, abi.MAX_LEGAL), "<i8")          # packed actions (bit pattern of the u64)
        self.waits = wrap(v.waits, (self.n, 4), "<i8")
        # pad_rows (the default since round 5): every (game, seat) row of the 74-channel tensor padded to a multiple of 256 B
        # (rmj_set_encode_row_stride): the acting seats' rows are written 1.3-1.4 x faster (trainer loop 260 -> 274 M env.step/s); obs() then
        # returns a strided view [n, 4, 74, W] of the padded buffer (same values, same indexing; .contiguous() copies).  pad_rows=False: dense
        self.pad_rows = bool(pad_rows) and features == "base"
        if self.pad_rows:
            self.row_stride = self.env.padded_row_stride()
            self.env.set_encode_row_stride(self.row_stride)
            self._obs_buf = torch.zeros((self.n, 4, self.row_stride), dtype=torch.float32, device=self.device)
            self._obs = self._obs_buf[:, :, : 74 * self.width].unflatten(-1, (74, self.width))
        else:
            self.row_stride = self.channels * self.width
            self._obs_buf = torch.zeros((self.n, 4, self.channels, self.width), dtype=torch.float32, device=self.device)
            self._obs = self._obs_buf
        # row stride of the batch entries (rmj_encode_batch_device): the padded rows of the base set, else C x W (0: 215 x 27 is odd)
        self._batch_stride = self.row_stride if self.pad_rows else 0
        self._scores = torch.zeros((self.n, 4), dtype=torch.int32, device=self.device)
        if share_stream:
            self.link.bind()
        self.env.reset()

    shared = property(lambda self: self.link.shared)   # the library issues on torch's stream (share_stream, or after bind_stream)

    def _batch(self, compact):
        """the RmjObsBatch of the resident tensor, or of the compact buffers, by reference"""
        if compact:
            return C.byref(self.env.obs_batch(self._feat, self._cobs_buf.data_ptr(), True, self._cidx.data_ptr(), self._cap, self._ccnt.data_ptr(),
                                              self._batch_stride))
        return C.byref(self.env.obs_batch(self._feat, self._obs_buf.data_ptr(), row_stride=self._batch_stride))

    # ---- status helpers (views, no copies beyond the arithmetic)
    def _status(self):
        s = self.status_raw.to(self.torch.int64) & 0xFFFFFFFF
        return s & 0xFF, (s >> 8) & 0xFF, ((s >> 16) & 0xFF).bool()

    def active(self):
        """bool [n, 4]: seats that must act now"""
        a, _, done = self._status()
        seats = self.torch.arange(4, device=self.device)
        return (((a[:, None] >> seats[None, :]) & 1) == 1) & ~done[:, None]

    def done(self):
        return self._status()[2]

    def obs(self, only_active=True):
        """encode() / the feature set's encoder into a resident tensor [n, 4, C, W].  only_active=True refreshes only the rows
        of the seats that must act (rows of the other seats keep their previous contents: mask them with active()).  The
        discard_shanten set encodes acting seats only (rmj_encode_batch_device, dense)."""
        L = self.env.L
        if self.features == "discard_shanten":
            if not only_active:
                raise ValueError("the discard_shanten feature set encodes the acting seats only: obs(only_active=True)")
            self.link.call(L.rmj_encode_batch_device, self.env.h, self._batch(False))
        else:
            fn = L.rmj_encode_extended_device if self.extended else L.rmj_encode_device
            self.link.call(fn, self.env.h, 2 if only_active else 0, self._obs_buf)
        return self._obs

    def _compact_buffers(self, capacity=None):
        """the compact batch's buffers, at least `capacity` rows (default n + n // 2 + 1, or what an earlier call grew to)"""
        t = self.torch
        cap = int(capacity or getattr(self, "_cap", 0) or (self.n + self.n // 2 + 1))
        if getattr(self, "_cobs", None) is None or self._cobs.shape[0] < cap:
            ch = self.channels
            self._cobs_buf = t.zeros((cap, self._batch_stride or ch * self.width), dtype=t.float32, device=self.device)
            self._cobs = self._cobs_buf[:, : ch * self.width].unflatten(-1, (ch, self.width))
            self._cidx = t.zeros((cap,), dtype=t.int32, device=self.device)
            self._ccnt = t.zeros((1,), dtype=t.int32, device=self.device)
            self._cap = cap

    def _compact_result(self, sync_count):
        """(obs [k, C, W], index [k]) after an encode into the compact buffers; the buffers grow (and the same state is encoded
        again, without stepping) when the state had more acting seats than rows"""
        if not sync_count:
            return self._cobs, self._cidx, self._ccnt
        k = int(self._ccnt.item())
        if k > self._cap:                                          # more claimants than rows: grow once and encode again
            self._cobs = None
            self._compact_buffers(k + k // 8)
            self.link.call(self.env.L.rmj_encode_batch_device, self.env.h, self._batch(True))
        return self._cobs[:k], self._cidx[:k]

    def obs_compact(self, capacity=None, sync_count=True):
        """The batch a policy consumes: the acting seats' observations only, dense, in (game, seat) order
        (rmj_encode_compact_device for the base set, rmj_encode_batch_device for the others).  Returns (obs [k, C, W], index [k]
        int32 = game * 4 + seat); with sync_count=False the full-capacity buffers and the device count tensor are returned instead
        (no host round trip: rows behind the count hold old data).  capacity defaults to n + n // 2 rows and grows on demand."""
        self._compact_buffers(capacity)
        if self.features == "base":
            self.link.call(self.env.L.rmj_encode_compact_device, self.env.h, self._cobs_buf, self._cidx, self._cap, self._ccnt)
        else:
            self.link.call(self.env.L.rmj_encode_batch_device, self.env.h, self._batch(True))
        return self._compact_result(sync_count)

    def _row_index(self, index):
        """(index as int32 [k] on the device, k)"""
        idx = index.to(device=self.device, dtype=self.torch.int32).contiguous().reshape(-1)
        return idx, int(idx.shape[0])

    def _row_target(self, target, fn, index, count, out, *flags):
        """the tensors of abi.ROW_TARGETS[target] for the rows `index`, allocated unless `out` brings them, filled by the entry `fn`"""
        t, fields = self.torch, abi.ROW_TARGETS[target].fields
        idx, k = self._row_index(index)
        if out is None:
            out = {f.name: t.full((k,) + f.shape, f.fill, dtype=abi.torch_dtype(t, f.dtype), device=self.device) for f in fields}
        assert all(out[f.name].shape[0] >= k and out[f.name].is_contiguous() for f in fields), "out is too small for the index"
        if k:
            self.link.call(fn, self.env.h, idx, k, count, *flags, C.byref(abi.row_struct(target, out)))
        return out

    def hidden_compact(self, index, count=None, out=None):
        """What the observation hides from the rows of a compact batch: index [k] int32 = game * 4 + seat as obs_compact returns it (or
        any other seats, acting or not) -> {"opp_hand" uint8 [k, 3, 34], "opp_shanten" int8 [k, 3], "opp_waits" int64 [k, 3] (bit t =
        tile type t), "opp_flags" uint8 [k, 3] (abi.HIDDEN_* bits, n_melds << 4)} on the device, for the opponents (seat + 1 + r) mod NP
        (rmj_hidden_targets_device; 3P: the third opponent is zeros).  count: the device count tensor of obs_compact(sync_count=False) -
        rows at or behind it are left as they were; out: the dict of an earlier call to write into (no allocation)."""
        return self._row_target("hidden", self.env.L.rmj_hidden_targets_device, index, count, out)

    def danger_compact(self, index, count=None, ura=False, out=None):
        """Deal-in danger of the rows of a compact batch: index [k] int32 = game * 4 + seat -> int32 [k, 3, 37] on the device, the points
        opponent (seat + 1 + r) mod NP would win by ron if the seat discarded a tile of kind c now (kinds 0..33 tile types, 34..36 copy 0
        of the fives; rmj_danger_targets_device).  count: the device count tensor of obs_compact(sync_count=False) - rows at or behind it
        are left as they were; ura: opponents in riichi count their ura indicators; out: the tensor of an earlier call to write into."""
        assert out is None or out.dtype == self.torch.int32, "out is too small for the index"
        return self._row_target("danger", self.env.L.rmj_danger_targets_device, index, count, None if out is None else {"danger": out},
                                abi.DANGER_URA if ura else 0)["danger"]

    def discard_table_compact(self, index, count=None, out=None):
        """Discard efficiency table of the rows of a compact batch: index [k] int32 = game * 4 + seat -> {"shanten" int8 [k, 35], "accept"
        uint8 [k, 35], "ukeire" uint8 [k, 35], "mask" int64 [k, 35] (bit t = tile type t)} on the device - column t < 34: the shanten
        after discarding type t (abi.DTAB_NONE: no such discard), the types that then lower it and their live tiles; column 34: the hand
        itself (rmj_discard_table_device).  count: the device count tensor of obs_compact(sync_count=False) - rows at or behind it are
        left as they were; out: the dict of an earlier call to write into (no allocation)."""
        return self._row_target("discard_table", self.env.L.rmj_discard_table_device, index, count, out, 0)

    def scores(self):
        self.link.call(self.env.L.rmj_scores_device, self.env.h, self._scores, None)
        return self._scores

    def points(self, rule_name="basic"):
        """RiichiEnv.points(rule_name) (env.rs:691-727) of every game as a float64 tensor [n, 4] on the device (rmj_points_device):
        the terminal reward of a trainer loop (riichienv-ml trainers/_ppo_worker.py reads env.points / env.ranks on the host)"""
        rules = vecenv.VecRiichiEnv.POINT_RULES
        if rule_name not in rules or (self.sanma and rule_name != "basic"):
            raise ValueError(f"Unknown preset rule{' for 3P' if self.sanma else ''}: {rule_name}")
        if not hasattr(self, "_points"):
            self._points = self.torch.zeros((self.n, 4), dtype=self.torch.float64, device=self.device)
        self.link.call(self.env.L.rmj_points_device, self.env.h, rules[rule_name], self._points)
        return self._points

    def ranks(self):
        """ranks() of env.rs:673-689 (1 = first; ties broken by seat) computed on the device from scores()"""
        sc = self.scores().to(self.torch.int64)
        np_ = 3 if self.sanma else 4
        key = sc[:, :np_] * 8 - self.torch.arange(np_, device=self.device)[None, :]
        r = (key[:, None, :] > key[:, :, None]).sum(-1) + 1
        out = self.torch.zeros((self.n, 4), dtype=self.torch.int64, device=self.device)
        out[:, :np_] = r
        return out

    def step(self, action_ids, auto_reset=True):
        self.link.call(self.env.L.rmj_step_ids_device, self.env.h, self._ids_in(action_ids), int(auto_reset))

    # ---- rewards (rmj_round_track_device): what riichienv-ml's PPO worker derives between steps on the host
    def round_track(self):
        """Call once after every step: (ended [n] u8, delta [n, 4] i32, meta [n, 4] i32, kyoku_idx [n] u8) - ended 1: a round ended in
        the last step and the next one was dealt, 2: the round and the game ended; delta = the seats' score change over that round,
        meta = (round_wind, oya, honba, riichi_sticks) when it was dealt (the GRP features chang / ju / ben / liqibang of
        trainers/_ppo_worker.py:100-116).  The first call only takes the baseline.  Resident tensors, rewritten by every call."""
        t = self.torch
        if not hasattr(self, "_rt"):
            self._rt = (t.zeros((self.n,), dtype=t.uint8, device=self.device), t.zeros((self.n, 4), dtype=t.int32, device=self.device),
                        t.zeros((self.n, 4), dtype=t.int32, device=self.device), t.zeros((self.n,), dtype=t.uint8, device=self.device))
        self.link.call(self.env.L.rmj_round_track_device, self.env.h, *self._rt)
        return self._rt

    RANK_REWARDS_4P = (10.0, 4.0, -4.0, -10.0)   # trainers/_ppo_worker.py:283-291
    RANK_REWARDS_3P = (10.0, 0.0, -10.0)

    def step_rl(self, action_ids, auto_reset=True, kyoku_scale=1.0 / 1000.0, rank_rewards=None, with_obs=True):
        """One Gym-style transition of every game: (obs, reward, terminated, info).
        reward [n, 4] f32 per seat = kyoku_scale x the seat's score change over a round, paid in the step that ends the round
        (the worker's reward at a kyoku boundary, _ppo_worker.py:240-266, with the identity in place of its learned GRP model: the
        model's inputs are in info), plus the rank reward of _ppo_worker.py:283-291 in the step that ends the game (rank_rewards:
        a per-rank tuple, default 10 / 4 / -4 / -10; () for none).  terminated [n] bool: the game ended in this step (with auto_reset
        it restarts at the next one).  info: ended, delta, meta, kyoku_idx (round_track), scores, ranks of the games that ended.
        obs: the resident feature tensor of the feature set (step_obs) - rows of the seats that act next; None with with_obs=False.
        The worker's full output - one hero's transitions cut per kyoku, with GAE - is riichienv_amd.ppo.PPOCollector."""
        t = self.torch
        if not hasattr(self, "_rt"):
            self.round_track()                       # baseline before the first transition
        if with_obs:
            obs = self.step_obs(action_ids, auto_reset=auto_reset)
        else:
            self.step(action_ids, auto_reset=auto_reset)
            obs = None
        ended, delta, meta, kidx = self.round_track()
        reward = delta.to(t.float32) * float(kyoku_scale)
        terminated = ended == 2
        rr = rank_rewards if rank_rewards is not None else (self.RANK_REWARDS_3P if self.sanma else self.RANK_REWARDS_4P)
        ranks = self.ranks()
        if len(rr):
            table = t.tensor([0.0] + list(rr) + [0.0] * (4 - len(rr)), dtype=t.float32, device=self.device)
            reward = reward + t.where(terminated[:, None], table[ranks], t.zeros_like(reward))
        info = {"ended": ended, "delta": delta, "meta": meta, "kyoku_idx": kidx, "scores": self.scores(), "ranks": ranks}
        return obs, reward, terminated, info

    def _ids_in(self, action_ids):
        t = self.torch
        ids = action_ids.to(device=self.device, dtype=t.int32).contiguous()
        assert ids.shape == (self.n, 4)
        return ids

    def _logits_in(self, logits):
        """(logits or None, their row stride), with the resident ids tensor made"""
        t = self.torch
        if not hasattr(self, "_ids"):
            self._ids = t.full((self.n, 4), -1, dtype=t.int32, device=self.device)
        if logits is None:
            return None, 0
        assert logits.dtype == t.float32 and logits.is_contiguous() and tuple(logits.shape[:2]) == (self.n, 4)
        return logits, int(logits.shape[2])

    def step_obs(self, action_ids, auto_reset=True):
        """step(action_ids) and obs(only_active=True): returns the resident tensor [n, 4, C, W] whose rows of the seats that are to act
        next have just been written.  Base set: ONE launch (rmj_step_ids_encode_device); the others: the step and the batch encoder
        on one stream (rmj_step_ids_encode_batch_device)."""
        ids = self._ids_in(action_ids)
        if self.features == "base":
            self.link.call(self.env.L.rmj_step_ids_encode_device, self.env.h, ids, int(auto_reset), self._obs_buf)
        else:
            self.link.call(self.env.L.rmj_step_ids_encode_batch_device, self.env.h, ids, int(auto_reset), self._batch(False))
        return self._obs

    def step_sample_obs(self, logits=None, seed=0, auto_reset=True):
        """sample_ids(logits, seed) + step_obs(ids): returns (ids [n, 4] int32 - the ids the two calls would have produced -, the resident
        tensor [n, 4, C, W] with the rows of the seats that act next).  logits: float32 [n, 4, A'] (A' >= 82; 60 in 3P) on this device, or
        None for the uniform policy.  Base set: ONE launch (rmj_step_sample_encode_device); the others: rmj_step_sample_encode_batch_device."""
        logits, stride = self._logits_in(logits)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self.features == "base":
            self.link.call(self.env.L.rmj_step_sample_encode_device, self.env.h, logits, stride, seed, int(auto_reset), self._ids, self._obs_buf)
        else:
            self.link.call(self.env.L.rmj_step_sample_encode_batch_device, self.env.h, logits, stride, seed, int(auto_reset), self._ids, self._batch(False))
        return self._ids, self._obs

    def step_obs_compact(self, action_ids, sync_count=True, auto_reset=True):
        """step(action_ids) + obs_compact(): the step and the compact batch of the feature set on one stream
        (rmj_step_ids_encode_batch_device).  Returns (obs [k, C, W], index [k]); with sync_count=False the full-capacity buffers and the
        device count (obs_compact's form: no host round trip, capturable in a HIP graph once the buffers exist)."""
        ids = self._ids_in(action_ids)
        self._compact_buffers()
        self.link.call(self.env.L.rmj_step_ids_encode_batch_device, self.env.h, ids, int(auto_reset), self._batch(True))
        return self._compact_result(sync_count)

    def step_sample_obs_compact(self, logits=None, seed=0, sync_count=True, auto_reset=True):
        """sample_ids(logits, seed) + step + obs_compact() (rmj_step_sample_encode_batch_device): returns (ids [n, 4], obs [k, C, W],
        index [k]), or (ids, obs, index, count) - the full-capacity buffers and the device count - with sync_count=False."""
        logits, stride = self._logits_in(logits)
        self._compact_buffers()
        self.link.call(self.env.L.rmj_step_sample_encode_batch_device, self.env.h, logits, stride, int(seed) & 0xFFFFFFFFFFFFFFFF, int(auto_reset),
                       self._ids, self._batch(True))
        return (self._ids,) + tuple(self._compact_result(sync_count))

    def bind_stream(self, stream=None):
        """Issue the library's further work on `stream` (a torch.cuda.Stream; default: torch's current stream of the device) -
        rmj_set_stream.  Work already issued is waited for first.  This is what puts the environment INSIDE a HIP graph: bind the
        side stream the graph will be captured on, run one warm-up iteration there, then capture `sample_ids` / `step_obs` /
        `step` / `obs` / `scores` / `points` together with the policy's kernels (`with torch.cuda.graph(g, stream=s): ...`) - these
        calls only launch kernels on the bound stream (no allocation, no host synchronisation), and the sampler's noise is keyed by
        every game's own step count, so each replay of the graph draws fresh actions.  `step_obs_compact(sync_count=False)` captures too
        (its buffers must exist before the capture); `obs_compact(sync_count=True)` reads a count on the host and cannot be captured."""
        return self.link.bind(stream)

    def sync(self):
        """own stream: wait for the library's work; shared stream: nothing to do, torch's stream orders it"""
        if not self.shared:
            self.env.sync()

    def drain_text(self, seat=-1, cursor=None, peek=False, timings=None):
        """The MJAI text every game logged since the last drain, formatted on the GPU and left there (rmj_drain_text with
        RMJ_TEXT_ON_DEVICE): (text torch.uint8 [bytes], offsets torch.int64 [n + 1]) on this device - game g's log is
        text[offsets[g]:offsets[g + 1]], its events each followed by a newline; the same bytes as VecRiichiEnv.drain_logs(raw=True).
        Both tensors are zero-copy views of the library's buffers: valid until the next drain_text on this environment (clone what must
        outlive it).  The call returns with the text complete, so any stream may read it at once.  Cursor, peek and timings as in
        VecRiichiEnv.drain_text.  Note: TorchVecEnv defaults to skip_mjai_logging=True, which logs nothing - the logs are then empty;
        create it with skip_mjai_logging=False to have them."""
        v = self.env._text_call(seat, cursor, peek, True)
        if timings is not None:
            timings[:] = [v.ms[0], v.ms[1], v.ms[2]]
        wrap = self.link.wrap
        text = wrap(v.text, (int(v.bytes),), "|u1") if v.bytes else self.torch.zeros(0, dtype=self.torch.uint8, device=self.device)
        return text, wrap(v.text_offsets, (v.n_games + 1,), "<i8")

    def copy_games(self, dst_idx, src_env, src_idx):
        """rmj_copy_games_device: the complete state of src_env's games `src_idx` into this environment's games `dst_idx` (int32 /
        int64 tensors on this device; src_env may be self when the two index sets are disjoint) - forks for a tree search that
        lives on the GPU, saved positions, refilling slots.  Asynchronous on a shared stream; with the library's own stream the call
        returns when the copy is done (the index tensors are temporaries of torch's allocator)."""
        t = self.torch
        a = dst_idx.to(device=self.device, dtype=t.int32).contiguous()
        b = src_idx.to(device=self.device, dtype=t.int32).contiguous()
        assert a.numel() == b.numel()
        # own stream: torch's caching allocator orders the reuse of `a` / `b` by torch's stream, not by the library's, so the
        # kernel must have read them before they are released - link.call returns after it (shared stream: torch's stream orders it)
        self.link.call(self.env.L.rmj_copy_games_device, self.env.h, a, src_env.env.h, b, int(a.numel()))

    def determinize(self, index, seed, count=None, hold=None, riichi_tenpai=False):
        """rmj_determinize_device: re-deal, in place, what the rows index [k] int32 = game * 4 + seat (as obs_compact returns them; the
        seat must be to act) cannot see - the opponents' concealed hands and the wall that can still be drawn or revealed - by the
        permutation the header defines for (seed, global game, seat), and republish lists, masks, waits and status.  count: the device
        count of obs_compact(sync_count=False) - rows at or behind it are left alone; hold: uint8 [k] (or one int for every row), bit r
        set = opponent (seat + 1 + r) mod NP keeps its hand.  Returns the status tensor uint8 [k] on the device (abi.DET_*; rows behind
        the count read 0).  Of several rows that name one game the lowest is carried out, the others read DET_DUPLICATE.
        riichi_tenpai: rmj_determinize_ex_device with abi.DETF_RIICHI_TENPAI - the re-dealt riichi hands walk to tenpai by seeded
        exchanges (header: the nearest tenpai hand by fewest exchanges from a uniform deal, not a posterior); abi.DET_SWAPPED marks the
        worlds in which a tile was exchanged.  Stream handling as in copy_games."""
        t = self.torch
        idx, k = self._row_index(index)
        st = t.zeros((k,), dtype=t.uint8, device=self.device)
        if not k:
            return st
        h = None
        if hold is not None:
            h = (hold.to(device=self.device, dtype=t.uint8) if t.is_tensor(hold) else t.as_tensor(hold, dtype=t.uint8, device=self.device)).expand(k).contiguous()
        d = abi.Determinize(int(seed) & 0xFFFFFFFFFFFFFFFF, None if h is None else h.data_ptr(), st.data_ptr())
        if riichi_tenpai:
            self.link.call(self.env.L.rmj_determinize_ex_device, self.env.h, idx, k, count, C.byref(d), abi.DETF_RIICHI_TENPAI)
        else:
            self.link.call(self.env.L.rmj_determinize_device, self.env.h, idx, k, count, C.byref(d))
        return st

    def sample_ids(self, logits=None, seed=0, index=None, count=None):
        """One id per acting seat drawn from softmax(logits) over the seat's legal ids, -1 elsewhere, by ONE kernel of the
        library (rmj_sample_ids_device: Gumbel-max on the resident mask slab) - no torch indexing / multinomial in the loop.
        logits: float32 [n, 4, A'] with A' >= 82 (60 in 3P) on this device, or None for the uniform policy; with `index`
        (the second result of obs_compact(): game * 4 + seat per row) logits are the compact rows [k, A'] a policy computed
        from the compact observation batch, scattered here into the [n, 4, A'] layout (rows of seats that do not act are never
        read by the sampler).  `count`: the device count tensor of obs_compact(sync_count=False) - rows of `index` behind it hold stale
        (game, seat) values that may repeat live ones, so they are sent to a sink row instead of racing with the live rows; without
        `count` every row of `index` must be live (the sync_count=True form).
        Non-finite logits: a -inf or NaN logit is never drawn while a finite one is legal; if every legal id is -inf or NaN the
        lowest legal id is drawn; among several +inf logits the lowest of them wins (step_sample_obs draws the same way)."""
        t = self.torch
        if logits is not None and index is not None:
            a = int(logits.shape[-1])
            if getattr(self, "_full_logits", None) is None or self._full_logits.shape[-1] != a:
                self._full_logits = t.zeros((self.n * 4 + 1, a), dtype=t.float32, device=self.device)   # (+ the sink row)
            k = int(index.shape[0])
            dst = index.to(t.int64)
            if count is not None:
                live = t.arange(k, device=self.device) < count.to(t.int64).reshape(-1)[0]
                dst = t.where(live, dst, t.full_like(dst, self.n * 4))
            elif k > self.n * 4:
                raise ValueError("sample_ids: more index rows than (game, seat) pairs - pass the device count of obs_compact(sync_count=False)")
            self._full_logits[dst] = logits.reshape(-1, a)[:k].to(t.float32)
            logits = self._full_logits[: self.n * 4].view(self.n, 4, a)
        logits, stride = self._logits_in(logits)
        self.link.call(self.env.L.rmj_sample_ids_device, self.env.h, logits, stride, int(seed) & 0xFFFFFFFFFFFFFFFF, self._ids)
        return self._ids

    def sample_random_ids(self, generator=None):
        """uniform choice among the legal ids of every acting seat (a masked categorical policy's baseline)"""
        t = self.torch
        m = self.mask.to(t.float32) * self.active()[:, :, None]
        has = m.sum(-1) > 0
        probs = t.where(has[:, :, None], m, t.ones_like(m))
        ids = t.multinomial(probs.view(-1, m.shape[-1]), 1, generator=generator).view(self.n, 4)
        return t.where(has, ids, t.full_like(ids, -1)).to(t.int32)


class ShardedTorchVecEnv:
    """`n_games` games as `parts` shards (by game index, like the ranks of a multi-GPU run) on `parts` torch streams of ONE
    GPU.  A step driven by an external policy ends with its slowest wave and the encoder is bound by its stores (DESIGN.md
    sections 4.6 / 4.7); with the shards on separate streams the tail of one shard's step and the encoder of another overlap
    (measured: 216 M -> 285 M env.step/s at 65 536 games with the fused sampler).  Results do not depend on the split: shard
    i holds the global games [i * n / parts, (i + 1) * n / parts) (game_offset), seeds and sampler noise are keyed by the
    global game index."""

    def __init__(self, n_games, parts=4, device=0, **kw):
        import torch

        if n_games % parts:
            raise ValueError("n_games must be a multiple of parts")
        self.torch = torch
        self.n, self.parts, self.per = int(n_games), int(parts), int(n_games) // int(parts)
        self.device = torch.device("cuda", device)
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.parts)]
        base = int(kw.pop("game_offset", 0))
        self.shards = []
        for i, st in enumerate(self.streams):
            with torch.cuda.stream(st):
                self.shards.append(TorchVecEnv(self.per, device=device, share_stream=True, game_offset=base + i * self.per, **kw))

    def for_each(self, fn):
        """fn(shard, i) for every shard under the shard's stream (everything fn enqueues is ordered with the shard's kernels);
        returns the list of results.  Nothing synchronises: call synchronize() before reading results on the host."""
        out = []
        for i, (e, st) in enumerate(zip(self.shards, self.streams)):
            with self.torch.cuda.stream(st):
                out.append(fn(e, i))
        return out

    def step_policy(self, policy, auto_reset=True, compact=True):
        """One step of every game: per shard, the observations of the acting seats (obs_compact: dense rows + index + device
        count, or the [n, 4] tensor with compact=False), `policy(shard, obs...) -> int32 ids [per, 4]` (-1 = no action), step."""
        def one(e, _i):
            ids = policy(e, *e.obs_compact(sync_count=False)) if compact else policy(e, e.obs(only_active=True))
            e.step(ids, auto_reset=auto_reset)
        self.for_each(one)

    def step_policy_one_launch(self, policy, auto_reset=True):
        """One step of every game with step + encode as ONE launch per shard (TorchVecEnv.step_obs): per shard,
        `policy(shard, obs [per, 4, 74, W]) -> int32 ids [per, 4]` on the observations the previous call left, then step_obs."""
        def one(e, _i):
            if getattr(e, "_cur_obs", None) is None:
                e._cur_obs = e.obs(only_active=True)
            e._cur_obs = e.step_obs(policy(e, e._cur_obs), auto_reset=auto_reset)
        self.for_each(one)

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def scores(self):
        self.synchronize()
        out = self.torch.cat(self.for_each(lambda e, _i: e.scores().clone()))
        self.synchronize()
        return out

    def step_counts(self):
        import numpy as np

        self.synchronize()
        return np.concatenate([e.env.step_counts() for e in self.shards])


class GymVectorAdapter:
    """A Gymnasium-VectorEnv-shaped face of TorchVecEnv for single-agent learners (the hero-versus-opponents set-up of
    riichienv-ml's PPO worker, trainers/_ppo_worker.py:113-466): env i exposes ONE seat, hero[i]; the other seats are played by
    `opponent(env, active_mask) -> ids [n, 4]` (default: the library's uniform sampler over the legal ids).  reset() / step(actions)
    return what gymnasium.vector.VectorEnv returns - (obs, info) and (obs, reward, terminated, truncated, info) - with torch tensors
    on the device; gymnasium itself is not needed (and not installed in this image).

    step(actions [n] int): the hero's action id for every env, then the environment advances - opponents' turns, claims, round ends -
    until the hero is to act again in every env or its game is over.  Envs that reach the hero's turn early wait: they send no action
    (-1) and stay where they are while the others catch up.  reward [n] = the hero's share of step_rl's rewards summed over the inner
    steps; terminated [n]: the game ended (it restarts with the next step: autoreset like gymnasium's NEXT_STEP mode).
    observation: {"features": [n, C, W] f32 (the hero's observation in env's feature set: C = env.channels), "mask": [n, A] bool}."""

    def __init__(self, env: TorchVecEnv, hero=0, opponent=None, max_inner=256):
        self.env, self.t = env, env.torch
        t = self.t
        self.num_envs = env.n
        self.hero = (t.full((env.n,), int(hero), dtype=t.int64, device=env.device) if isinstance(hero, int)
                     else hero.to(device=env.device, dtype=t.int64))
        self.opponent = opponent
        self.max_inner = int(max_inner)
        self.action_space_n = abi.ACTION_SPACE_3P if env.sanma else abi.ACTION_SPACE_4P
        self.single_observation_shape = {"features": (env.channels, env.width), "mask": (self.action_space_n,)}
        self.features = env.features
        self._seat = t.arange(4, device=env.device)[None, :]
        self._seed = 0

    def _hero_turn(self):
        return self.env.active().gather(1, self.hero[:, None])[:, 0]

    def _obs(self):
        e, t = self.env, self.t
        feats = e.obs(only_active=True)
        idx = self.hero[:, None, None, None].expand(-1, 1, feats.shape[2], feats.shape[3])
        mask = e.mask.gather(1, self.hero[:, None, None].expand(-1, 1, e.mask.shape[2]))[:, 0, : self.action_space_n] != 0
        return {"features": feats.gather(1, idx)[:, 0], "mask": mask & self._hero_turn()[:, None]}

    def _advance(self, hero_ids, reward, terminated):
        """inner steps until every env is at its hero's decision (or over); hero_ids [n]: the hero's id for the FIRST inner step, -1 = none"""
        e, t = self.env, self.t
        first = True
        for _ in range(self.max_inner):
            act = e.active()
            hero_now = act.gather(1, self.hero[:, None])[:, 0]
            over = e.done() | terminated
            wait = hero_now & ((hero_ids < 0) if first else t.ones_like(hero_now))   # at the hero's decision with nothing to send: stay
            if bool((wait | over).all()):
                break
            self._seed += 1
            ids = (self.opponent(e, act) if self.opponent is not None else e.sample_ids(None, seed=self._seed)).clone().to(t.int32)
            if first:
                ids = t.where(self._seat == self.hero[:, None], hero_ids.to(t.int32)[:, None].expand(-1, 4), ids)
            ids = t.where((wait | over)[:, None], t.full_like(ids, -1), ids)
            _o, r, term, _info = e.step_rl(ids, auto_reset=False, with_obs=False)
            reward += r.gather(1, self.hero[:, None])[:, 0]
            terminated |= term
            first = False
        return reward, terminated

    def reset(self, seed=None):
        e, t = self.env, self.t
        self._seed = int(seed or 0) * 1000003
        e.env.reset()
        if hasattr(e, "_rt"):
            e.link.call(e.env.L.rmj_round_track_reset, e.env.h)
        else:
            e.round_track()
        self._terminated = t.zeros((e.n,), dtype=t.bool, device=e.device)
        self._advance(t.full((e.n,), -1, dtype=t.int64, device=e.device), t.zeros((e.n,), dtype=t.float32, device=e.device),
                      t.zeros((e.n,), dtype=t.bool, device=e.device))
        return self._obs(), {}

    def step(self, actions):
        e, t = self.env, self.t
        if bool(self._terminated.any()):   # games that ended in the previous step restart now (their action is ignored)
            e.env.reset(select=self._terminated.to(t.uint8).cpu().numpy())
            e.link.call(e.env.L.rmj_round_track_device, e.env.h, None, None, None, None)   # re-opens the restarted games silently
            lead = self._terminated
            self._advance(t.full((e.n,), -1, dtype=t.int64, device=e.device), t.zeros((e.n,), dtype=t.float32, device=e.device), ~lead)
        acts = actions.to(device=e.device, dtype=t.int64)
        ids = t.where(self._terminated | ~self._hero_turn(), t.full_like(acts, -1), acts)
        reward = t.zeros((e.n,), dtype=t.float32, device=e.device)
        reward, terminated = self._advance(ids, reward, t.zeros((e.n,), dtype=t.bool, device=e.device))
        self._terminated = terminated
        info = {"scores": e.scores(), "ranks": e.ranks()}
        return self._obs(), reward, terminated, t.zeros_like(terminated), info
