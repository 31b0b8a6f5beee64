"""Sampled worlds on the device: forks of live positions whose hidden tiles are re-dealt from the deciding seat's point of view
(rmj_copy_games_device + rmj_determinize_device), played out by the device policy and read back as score changes - the building block of
Monte Carlo move evaluation (PIMC), determinized tree search and value targets on sampled worlds.

    ws = WorldSet(tenv, worlds=16, max_rows=1024)
    obs, index = tenv.obs_compact()                      # index[r] = game * 4 + seat of an acting seat
    ws.fork(index[:1024], seed=7)                        # world (r, k) is game r * 16 + k of ws.env
    ws.env.step(ids)                                     # optional: any existing call steps the worlds (e.g. the move under evaluation)
    ws.playout(policy_seed=3, max_steps=400)
    delta, rank, done = ws.values()                      # [rows, 16] each

The sample is uniform over placements of the hidden tiles (header: rmj_determinize_device), not over worlds consistent with what the
opponents did; fork() returns the per-world status, whose bits 4..6 name opponents in riichi whose sampled hand is not tenpai.
fork(..., riichi_tenpai=True) walks those hands to tenpai on the device (RMJ_DETF_RIICHI_TENPAI): what comes out is the nearest tenpai
hand by fewest exchanges from a uniform deal, with seeded ties - not a posterior: no furiten consistency with the seat's discards, no
weighting by discards or calls, and a riichi seat that holds its drawn tile (14, 11, ... tiles) is left as dealt."""
from __future__ import annotations

from . import torch_env


class WorldSet:
    def __init__(self, tenv, worlds=16, max_rows=1024):
        """K = `worlds` sampled worlds for each of up to R = `max_rows` rows: a TorchVecEnv of R * K games with tenv's mode, rule bits,
        event ring and stream handling, and no MJAI logging."""
        self.src = tenv
        self.K, self.R = int(worlds), int(max_rows)
        if self.K < 1 or self.R < 1:
            raise ValueError("worlds and max_rows must be positive")
        e = tenv.env
        self.env = torch_env.TorchVecEnv(self.R * self.K, game_mode=e.game_mode, device=tenv.device.index, skip_mjai_logging=True,
                                         share_stream=tenv.shared, features=tenv.features, rule_bits=e.rule_bits, event_ring=e.event_ring)
        self.rows = 0
        self.hero = self.score0 = self.slot = None

    def fork(self, index, count=None, seed=0, hold=None, riichi_tenpai=False):
        """Row r of index [rows <= R] int32 = game * 4 + seat (an acting seat of the source, e.g. obs_compact's index): the source's
        game is copied into the worlds r * K .. r * K + K - 1 and each is determinized from the seat's view with `seed` (the world's
        slot is its global game: the same (seed, slot) gives the same world).  count: the device count of obs_compact(sync_count=False);
        hold and riichi_tenpai: as in TorchVecEnv.determinize, hold per row (with riichi_tenpai a world in which a tile was exchanged
        carries abi.DET_SWAPPED, and bits 4..6 remain only where the walk found no way to tenpai).  Remembers the hero seat and its score at the fork.  Returns the status uint8
        [rows, K] (abi.DET_*)."""
        t, K = self.src.torch, self.K
        idx = index.to(device=self.env.device, dtype=t.int32).contiguous().reshape(-1)
        rows = int(idx.shape[0])
        if rows > self.R:
            raise ValueError(f"{rows} rows for a WorldSet of max_rows={self.R}")
        self.rows = rows
        if not rows:
            return t.zeros((0, K), dtype=t.uint8, device=self.env.device)
        rep = idx.repeat_interleave(K)
        slot = t.arange(rows * K, device=self.env.device, dtype=t.int32)
        game, seat = rep >> 2, rep & 3
        self.env.copy_games(slot, self.src, game)    # (rows behind the count may name no game: the copy skips what is out of range)
        cnt = None if count is None else (count.reshape(-1)[:1].to(t.int64) * K).clamp(max=rows * K).to(t.int32)
        h = None
        if hold is not None:
            h = (hold.to(device=self.env.device, dtype=t.uint8) if t.is_tensor(hold) else t.as_tensor(hold, dtype=t.uint8, device=self.env.device))
            h = h.expand(rows).repeat_interleave(K)
        st = self.env.determinize(slot * 4 + seat, seed, count=cnt, hold=h, riichi_tenpai=riichi_tenpai)
        self.slot, self.hero = slot.to(t.int64), seat.to(t.int64)
        sc = self.src.scores()
        self.score0 = sc[game.to(t.int64).clamp(0, self.src.n - 1), self.hero].clone()
        return st.view(rows, K)

    def playout(self, policy_seed, max_steps, call_rate_256=64, chunk=64):
        """The worlds under the device policy that plays to win (rmj_step_greedy, auto_reset=False) until every forked world is done or
        `max_steps` steps are made; the host looks at the done flags every `chunk` steps.  Returns the steps issued."""
        made = 0
        while made < max_steps and self.rows:
            n = min(int(chunk), max_steps - made)
            self.env.env.step_greedy(policy_seed, n, auto_reset=False, call_rate_256=call_rate_256)
            made += n
            if bool(self.env.done()[: self.rows * self.K].all()):
                break
        return made

    def values(self):
        """(score_delta int32 [rows, K]: the hero's score now minus its score at the fork, rank int64 [rows, K]: its rank now (1 = first),
        done bool [rows, K]) of the worlds of the last fork."""
        t = self.src.torch
        n = self.rows * self.K
        if not n:
            z = t.zeros((0, self.K), dtype=t.int32, device=self.env.device)
            return z, z.to(t.int64), z.bool()
        sc = self.env.scores()[:n]
        delta = (sc[self.slot, self.hero] - self.score0).to(t.int32)
        rank = self.env.ranks()[:n][self.slot, self.hero]
        return delta.view(self.rows, self.K), rank.view(self.rows, self.K), self.env.done()[:n].clone().view(self.rows, self.K)
