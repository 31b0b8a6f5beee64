"""PPO transition collector on the device: what riichienv-ml's PPO worker returns (trainers/_ppo_worker.py:129-391
collect_episodes) - the transitions of one hero seat per game, one trajectory per kyoku, GAE run backwards over each kyoku with the
kyoku's reward on its last decision - and its evaluation loop (:393-466 evaluate_episodes), over a TorchVecEnv of any feature set.

The pool, the hero / opponent action selector, the log-probabilities, the kyoku segmentation and the GAE are kernels of the library
(rmj_select_ids_device, rmj_ppo_*: csrc/rmj_ppo.hip.h); torch is used for the policy, for device memory and for the few element-wise
ops between the calls (merging the two models' logits by hero, the reward).

Memory: capacity x (C x W x 4 + A + 45) bytes - 1 M transitions of 74 x 34 are 10 GB.  Capacity is the caller's decision; what does
not fit is counted (`counts()["overflowed"]`), and a trajectory that lost a transition is never emitted."""
from __future__ import annotations

import ctypes as C
import functools

from . import abi, vecenv

NO_HERO = 255   # hero value of a game in which every seat takes the arg-max and nothing is recorded (evaluate_episodes)


class PPOCollector:
    """collector = PPOCollector(tenv, capacity); collector.collect(policy, baseline, n_steps); batch = collector.transitions()

    hero: [n] uint8 tensor (seat per game; 255 = none), or None = drawn per game from a generator seeded with `seed`
    (_ppo_worker.py:134 `random.randint(0, n - 1)`).
    boundary: where a trajectory ends.
      "round"      rmj_round_track_device's `ended`: every round end, a renchan (the dealer repeats, kyoku_idx stays) included; the
                   reward is that round's score change.
      "kyoku_idx"  what the worker literally does (:240-266): when kyoku_idx changes or the game ends - a renchan EXTENDS the
                   trajectory, and the reward is the score change since the trajectory's first round was dealt.  A kyoku in which the
                   hero never decided closes nothing: its score change goes to the next trajectory (the worker keeps its start scores).
    The two rules hand different `ended` / `reward` tensors to the same kernel and differ exactly on renchan rounds."""

    def __init__(self, tenv, capacity, gamma=0.99, gae_lambda=0.95, hero=None, boundary="round", seed=0):
        if boundary not in ("round", "kyoku_idx"):
            raise ValueError("boundary is 'round' or 'kyoku_idx'")
        self.tenv, self.t, self.link = tenv, tenv.torch, tenv.link
        t, L = self.t, tenv.env.L
        self.L = L
        self.n, self.capacity, self.boundary = tenv.n, int(capacity), boundary
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.A = abi.ACTION_SPACE_3P if tenv.sanma else abi.ACTION_SPACE_4P
        self.n_players = 3 if tenv.sanma else 4
        dev = tenv.device
        if hero is None:
            gen = t.Generator().manual_seed(int(seed))
            hero = t.randint(0, self.n_players, (self.n,), generator=gen, dtype=t.uint8)
        self.hero = hero.to(device=dev, dtype=t.uint8).contiguous()
        assert self.hero.shape == (self.n,)
        self._hero64 = self.hero.to(t.int64).clamp(max=3)
        self._no_hero = t.full((self.n,), NO_HERO, dtype=t.uint8, device=dev)
        cfg = abi.PpoConfig(tenv._feat, self.capacity, self.gamma, self.gae_lambda)
        self.h = C.c_void_p()
        self.link.call(L.rmj_ppo_create, tenv.env.h, C.byref(cfg), C.byref(self.h))
        v = abi.PpoViews()
        vecenv._chk(L.rmj_ppo_views(self.h, C.byref(v)))
        wrap = functools.partial(self.link.wrap, owner=self)
        cap, fl = self.capacity, tenv.channels * tenv.width
        self._pool_rows = wrap(v.features, (cap, v.row_stride), "<f4")
        self.pool = {"features": self._pool_rows[:, :fl].unflatten(-1, (tenv.channels, tenv.width)), "mask": wrap(v.mask, (cap, self.A), "|u1"),
                     "action": wrap(v.action, (cap,), "<i4"), "value": wrap(v.value, (cap,), "<f4"), "log_prob": wrap(v.log_prob, (cap,), "<f4"),
                     "advantage": wrap(v.advantage, (cap,), "<f4"), "return": wrap(v.ret, (cap,), "<f4"), "valid": wrap(v.valid, (cap,), "|u1"),
                     "game": wrap(v.game, (cap,), "<i4"), "t": wrap(v.t, (cap,), "<i4"), "prev": wrap(v.prev, (cap,), "<i4"),
                     "seg_len": wrap(v.seg_len, (cap,), "<i4"), "serial": wrap(v.serial, (cap,), "<i4"), "seg_reward": wrap(v.seg_reward, (cap,), "<f4"),
                     "open_len": wrap(v.open_len, (self.n,), "<i4"), "counters": wrap(v.counters, (5,), "<i4")}
        self._ids = t.full((self.n, 4), -1, dtype=t.int32, device=dev)
        self._full = None
        self._seed = int(seed) * 1000003
        self._reset_boundary()

    def close(self):
        """rmj_ppo_destroy (the environment's close destroys its collectors too)"""
        if getattr(self, "h", None) and getattr(self.tenv.env, "h", None):
            self.L.rmj_ppo_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _reset_boundary(self):
        t, dev = self.t, self.tenv.device
        self._acc = t.zeros((self.n, 4), dtype=t.int32, device=dev)     # score change since the open trajectory's first round was dealt
        self._meta0 = t.zeros((self.n, 4), dtype=t.int32, device=dev)   # that round's (round_wind, oya, honba, riichi_sticks)
        self._fresh = t.ones((self.n,), dtype=t.bool, device=dev)
        self._prev_kidx = None

    # ---- the library calls
    def select_ids(self, logits, seed, hero="own"):
        """rmj_select_ids_device: logits float32 [n, 4, A'] (or None: all equal) -> ids [n, 4] int32 (resident).  The hero seat draws like
        TorchVecEnv.sample_ids, every other acting seat takes the arg-max over its legal ids (ties to the lowest id); hero=None: every
        seat draws; a hero tensor of 255s: every seat takes the arg-max."""
        t = self.t
        stride = 0
        if logits is not None:
            assert logits.dtype == t.float32 and logits.is_contiguous() and tuple(logits.shape[:2]) == (self.n, 4)
            stride = int(logits.shape[2])
        hp = self.hero if isinstance(hero, str) else hero
        self.link.call(self.L.rmj_select_ids_device, self.tenv.env.h, logits, stride, int(seed) & 0xFFFFFFFFFFFFFFFF, hp, self._ids)
        return self._ids

    def _batch(self, layout):
        e = self.tenv
        if layout == "compact":
            return abi.ObsBatch(e._feat, 1, e._batch_stride, e._cap, e._cobs_buf.data_ptr(), e._cidx.data_ptr(), e._ccnt.data_ptr())
        return abi.ObsBatch(e._feat, 0, e._batch_stride, 0, e._obs_buf.data_ptr(), None, None)

    def record(self, ids, logits, values, layout="compact", hero=None):
        """rmj_ppo_record_device on the observation batch the environment produced last in `layout` ("compact": obs_compact /
        step_obs_compact, logits [rows, A'] and values [rows] by compact slot; "dense": obs / step_obs, logits [n, 4, A'], values [n, 4])."""
        t = self.t
        assert logits.dtype == t.float32 and logits.is_contiguous() and values.dtype == t.float32 and values.is_contiguous()
        b = self._batch(layout)
        hp = self.hero if hero is None else hero
        self.link.call(self.L.rmj_ppo_record_device, self.h, C.byref(b), hp, ids, logits, int(logits.shape[-1]), values)

    def close_segments(self, ended, reward):
        """rmj_ppo_close_device: ended [n] uint8 (non-zero: the hero's open trajectory of the game ends here), reward [n] float32"""
        t = self.t
        assert ended.dtype == t.uint8 and ended.is_contiguous() and reward.dtype == t.float32 and reward.is_contiguous()
        self.link.call(self.L.rmj_ppo_close_device, self.h, ended, reward)

    def clear(self):
        """empty the pool and forget the open trajectories (rmj_ppo_clear); the boundary bookkeeping starts afresh"""
        self.link.call(self.L.rmj_ppo_clear, self.h)
        self._reset_boundary()

    def counts(self):
        """fill = valid + open + dropped; overflowed = transitions that found no slot; segments = trajectories closed complete (waits)"""
        c = abi.PpoCounts()
        vecenv._chk(self.L.rmj_ppo_counts(self.h, C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in abi.PpoCounts._fields_}

    # ---- the worker's loops
    def _forward(self, policy, baseline, layout, hero64):
        """observation batch -> (merged logits in the selector's [n, 4, A'] layout, the policy's logits and values in the batch's layout)"""
        t, e = self.t, self.tenv
        if layout == "compact":
            obs, index, count = self._obs
            logits, values = policy(obs)
            bl = baseline(obs)
            bl = bl[0] if isinstance(bl, tuple) else bl
            idx = index.to(t.int64)
            is_hero = hero64[idx >> 2] == (idx & 3)
            merged = t.where(is_hero[:, None], logits, bl).to(t.float32).contiguous()
            a = int(merged.shape[-1])
            if self._full is None or self._full.shape[-1] != a:
                self._full = t.zeros((self.n * 4 + 1, a), dtype=t.float32, device=e.device)   # (+ a sink row for the rows behind the count)
            live = t.arange(idx.shape[0], device=e.device) < count.to(t.int64).reshape(-1)[0]
            self._full[t.where(live, idx, t.full_like(idx, self.n * 4))] = merged
            return self._full[: self.n * 4].view(self.n, 4, a), merged, values.to(t.float32).reshape(-1).contiguous()
        obs = self._obs
        logits, values = policy(obs.reshape(self.n * 4, e.channels, e.width) if obs.is_contiguous() else obs.flatten(0, 1))
        bl = baseline(obs.flatten(0, 1))
        bl = bl[0] if isinstance(bl, tuple) else bl
        seat = t.arange(4, device=e.device)[None, :]
        merged = t.where((hero64[:, None] == seat)[:, :, None], logits.view(self.n, 4, -1), bl.view(self.n, 4, -1)).to(t.float32).contiguous()
        return merged, merged, values.to(t.float32).reshape(self.n, 4).contiguous()

    def _first_obs(self, layout):
        e = self.tenv
        self._obs = e.obs_compact(sync_count=False) if layout == "compact" else e.obs(only_active=True)
        if not hasattr(e, "_rt"):
            e.round_track()   # the baseline of the round tracker

    def _boundary(self, ended, delta, meta, kidx):
        """(ended [n] u8, delta [n, 4] i32, meta [n, 4] i32) of the trajectories that end here under the collector's rule"""
        t = self.t
        if self.boundary == "round":
            return ended, delta, meta
        rnd = ended != 0
        first = rnd & self._fresh
        self._meta0 = t.where(first[:, None], meta, self._meta0)
        self._fresh = self._fresh & ~rnd
        self._acc = self._acc + delta
        closing = ((kidx != self._prev_kidx) | (ended == 2)) & rnd
        done = closing & (self.pool["open_len"] != 0)        # (:251 `and kyoku_buffers[ei]`: an empty trajectory keeps its start scores)
        out = (done.to(t.uint8), t.where(done[:, None], self._acc, t.zeros_like(self._acc)), t.where(done[:, None], self._meta0, t.zeros_like(meta)))
        over = done | (ended == 2)                           # (a game that ends takes its open account with it)
        self._acc = t.where(over[:, None], t.zeros_like(self._acc), self._acc)
        self._fresh = self._fresh | over
        self._prev_kidx = t.where(over, kidx, self._prev_kidx).clone()
        return out

    def collect(self, policy, baseline, n_steps, reward_fn=None, kyoku_scale=1.0 / 1000.0, layout="compact", auto_reset=True, on_step=None):
        """n_steps iterations of the worker's loop (_ppo_worker.py:151-281) over all games:
        observation batch -> policy(obs) = (logits, values), baseline(obs) = logits (or a tuple whose first item is) -> merged by hero ->
        select_ids -> record -> step + the next batch -> round_track -> reward -> close_segments.
        Reward of a trajectory: kyoku_scale x the hero's score change (step_rl's kyoku term), or reward_fn(delta [n, 4] i32, meta [n, 4] i32,
        ended [n] u8, hero [n] u8) -> [n] float32 - where the worker's learned reward model (GRP) plugs in; its value is read for the games
        that end a trajectory in this step.  layout: "compact" (the acting seats' rows: policy sees [rows, C, W]; rows behind the device
        count hold old data) or "dense" ([n * 4, C, W]).  No host synchronisation on a shared stream.  on_step(dict) sees every step's
        tensors (ids, logits, values, ended, reward, ...) before the next step overwrites them."""
        t, e = self.t, self.tenv
        if getattr(self, "_obs", None) is None or self._layout != layout:
            self._first_obs(layout)
            self._layout = layout
        hero64 = self._hero64
        if self.boundary == "kyoku_idx" and self._prev_kidx is None:
            self._prev_kidx = e.round_track()[3].clone()   # (no step since the last call: only kyoku_idx is read)
        for _ in range(int(n_steps)):
            self._seed += 1
            sel_logits, logits, values = self._forward(policy, baseline, layout, hero64)
            ids = self.select_ids(sel_logits, self._seed)
            self.record(ids, logits, values, layout)
            if on_step is not None:
                on_step({"phase": "record", "ids": ids, "select_logits": sel_logits, "logits": logits, "values": values, "obs": self._obs, "seed": self._seed})
            self._obs = e.step_obs_compact(ids, sync_count=False, auto_reset=auto_reset) if layout == "compact" else e.step_obs(ids, auto_reset=auto_reset)
            rt = e.round_track()
            ended, delta, meta = self._boundary(*rt)
            if reward_fn is None:
                reward = delta.gather(1, hero64[:, None])[:, 0].to(t.float32) * float(kyoku_scale)
            else:
                reward = reward_fn(delta, meta, ended, self.hero).to(t.float32)
            reward = reward.contiguous()
            self.close_segments(ended.contiguous(), reward)
            if on_step is not None:
                on_step({"phase": "close", "ended": ended, "reward": reward, "round_ended": rt[0], "delta": delta, "meta": rt[2], "kyoku_idx": rt[3]})
        return self

    def transitions(self):
        """The worker's result (_ppo_worker.py:345-353): {"features" [N, C, W] f32, "mask" [N, A] u8, "action" [N] i64, "log_prob",
        "advantage", "return" [N] f32} on the device - the transitions of the trajectories closed so far, in pool order
        (rmj_ppo_emit_device).  Reads the count on the host to size the tensors."""
        t, e = self.t, self.tenv
        k = self.counts()["valid"]
        out = {"features": t.empty((k, e.channels, e.width), dtype=t.float32, device=e.device), "mask": t.empty((k, self.A), dtype=t.uint8, device=e.device),
               "action": t.empty((k,), dtype=t.int64, device=e.device), "log_prob": t.empty((k,), dtype=t.float32, device=e.device),
               "advantage": t.empty((k,), dtype=t.float32, device=e.device), "return": t.empty((k,), dtype=t.float32, device=e.device)}
        self.emit_into(out, k)
        return out

    def emit_into(self, out, rows):
        """rmj_ppo_emit_device into caller-owned tensors of `rows` rows; returns the device count tensor [2] (valid, left out)"""
        t = self.t
        cnt = t.zeros((2,), dtype=t.int32, device=self.tenv.device)
        b = abi.PpoBatch(out["features"].data_ptr(), out["mask"].data_ptr(), out["action"].data_ptr(), out["log_prob"].data_ptr(),
                         out["advantage"].data_ptr(), out["return"].data_ptr(), cnt.data_ptr(), int(rows), 0)
        self.link.call(self.L.rmj_ppo_emit_device, self.h, C.byref(b))
        return cnt

    def stats(self):
        """the worker's kyoku statistics (:355-366) over the trajectories closed so far, plus the pool's counts"""
        t = self.t
        c = self.counts()
        f = c["fill"]
        sl = self.pool["seg_len"][:f]
        last = sl > 0
        lens, rew = sl[last].to(t.float64), self.pool["seg_reward"][:f][last].to(t.float64)
        vals = self.pool["value"][:f][self.pool["valid"][:f] != 0].to(t.float64)
        out = dict(c, transitions=c["valid"], kyokus=c["segments"])
        if c["segments"]:
            out.update(kyoku_length_mean=float(lens.mean()), kyoku_reward_mean=float(rew.mean()), kyoku_reward_std=float(rew.std(unbiased=False)),
                       kyokus_per_game=c["segments"] / self.n, value_pred_mean=float(vals.mean()), value_pred_std=float(vals.std(unbiased=False)))
        return out

    def evaluate(self, policy, baseline, max_steps=4000, check_every=64, rank_rewards=None):
        """evaluate_episodes (:393-466): every game is dealt afresh and played to its end with seat 0 on the arg-max of `policy` and the other
        seats on the arg-max of `baseline`; nothing is recorded.  Returns (rank [n] int64 of seat 0, reward [n] float32: 10 / 4 / -4 / -10
        by rank, or `rank_rewards`; done [n] bool - False where max_steps ended the loop first)."""
        t, e = self.t, self.tenv
        e.env.reset()
        self.link.call(self.L.rmj_round_track_reset, e.env.h)
        self._obs = None
        seat0 = t.zeros((self.n,), dtype=t.int64, device=e.device)
        obs = e.obs_compact(sync_count=False)
        for i in range(int(max_steps)):
            self._obs = obs
            sel_logits, _l, _v = self._forward(policy, baseline, "compact", seat0)
            ids = self.select_ids(sel_logits, 0, hero=self._no_hero)
            obs = e.step_obs_compact(ids, sync_count=False, auto_reset=False)
            if (i + 1) % int(check_every) == 0 and bool(e.done().all()):
                break
        self._obs = None
        rr = rank_rewards if rank_rewards is not None else (e.RANK_REWARDS_3P if e.sanma else e.RANK_REWARDS_4P)
        rank = e.ranks()[:, 0]
        table = t.tensor([0.0] + list(rr) + [0.0] * (4 - len(rr)), dtype=t.float32, device=e.device)
        return rank, table[rank], e.done()
