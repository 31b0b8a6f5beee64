"""Restatement of the PPO worker's transition bookkeeping (riichienv-ml trainers/_ppo_worker.py:129-391 collect_episodes) in plain
Python / numpy float64, fed with RECORDED per-step data - it needs neither a GPU nor the oracle.  What it restates:

  * per-game kyoku buffers (:141, :186-193), completed kyokus with their reward (:251-259, :268-276), the GAE loop (:305-326) in Python
    floats over f32 values and an f32 reward, the flattening (:328-353) with one rounding to f32;
  * the library's pool order rule: transitions take slots in (call, game) order - slot = fill + the number of recording games with a
    smaller index in the same call; a transition that finds no slot is counted as overflowed and breaks its game's open trajectory,
    which is then dropped when it closes (a trajectory with a hole is never emitted);
  * the opponents' arg-max (:227-228) with the library's rules for ties and non-finite logits;
  * log_prob = log_softmax(masked_fill(logits, ~mask, -1e9))[action] (:175-182) in float64.

The worker's own boundary rule (a kyoku_idx change or the game's end, :240-281) and the round rule (every round end) are both just
`ended` vectors for close(); boundary_kyoku_idx() derives the former from recorded (round_ended, kyoku_idx) the way the worker does."""
import numpy as np

FILL = np.float32(-1e9)


def argmax_ref(mask_row, logits_row):
    """the id an opponent seat takes: arg-max of the logits over the legal ids, ties to the lowest id; NaN and -inf lose to anything
    finite or +inf; if nothing else is legal, the lowest legal id.  logits_row None: all logits equal.  -1 without a legal id."""
    legal = np.flatnonzero(np.asarray(mask_row) != 0)
    if not len(legal):
        return -1
    if logits_row is None:
        return int(legal[0])
    best, bid = None, -1
    for i in legal:
        v = np.float32(logits_row[i])
        key = -np.inf if np.isnan(v) else float(v)
        if bid < 0 or key > best:
            best, bid = key, int(i)
    return bid


def argmax_rows(masks, logits):
    """argmax_ref of many rows at once: masks [k, A], logits [k, A] f32 -> ids [k] (-1 for a row without a legal id)"""
    masks = np.asarray(masks) != 0
    lg = np.asarray(logits, np.float32)
    key = np.where(masks & ~np.isnan(lg), lg, -np.inf)
    ids = key.argmax(axis=1)                                     # (the first of equal maxima)
    first = masks.argmax(axis=1)
    none = np.isneginf(key.max(axis=1))                          # nothing finite or +inf is legal: the lowest legal id
    ids = np.where(none, first, ids)
    return np.where(masks.any(axis=1), ids, -1).astype(np.int32)


def select_ref(sampled_ids, hero, acting, masks, logits):
    """ids [n, 4] of rmj_select_ids_device: the hero seat keeps the sampler's id, every other acting seat takes argmax_ref.
    hero None: every seat keeps the sampler's id; hero[g] = 255: every seat of g takes the arg-max."""
    n = len(sampled_ids)
    out = np.full((n, 4), -1, np.int32)
    for g in range(n):
        for p in range(4):
            if not acting[g][p]:
                continue
            if hero is None or int(hero[g]) == p:
                out[g, p] = sampled_ids[g][p]
            else:
                out[g, p] = argmax_ref(masks[g][p], None if logits is None else logits[g][p])
    return out


def log_prob_ref(masks, logits, actions):
    """float64 log_softmax(masked_fill(logits, ~mask, -1e9))[action] of rows [k, A] (f32 logits, the f32 fill value)"""
    x = np.where(np.asarray(masks) != 0, np.asarray(logits, np.float32), FILL).astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - m).sum(axis=1))
    k = np.arange(len(x))
    return (x[k, np.asarray(actions, np.int64)] - m[:, 0]) - lse


def gae_ref(values, reward, gamma, lam):
    """_ppo_worker.py:314-326 in Python floats: (advantages, returns) as lists of float"""
    T = len(values)
    adv, ret = [0.0] * T, [0.0] * T
    gae = 0.0
    for t in reversed(range(T)):
        if t == T - 1:
            r, next_value = float(reward), 0.0
        else:
            r, next_value = 0.0, float(values[t + 1])
        delta = r + gamma * next_value - float(values[t])
        gae = delta + gamma * lam * gae
        adv[t] = gae
        ret[t] = gae + float(values[t])
    return adv, ret


def boundary_kyoku_idx(round_ended, kyoku_idx, prev_kidx, open_len):
    """the worker's rule for one step: a trajectory closes when kyoku_idx differs from the value at its last close (or the game ends) and
    it is not empty (:251, :267-268).  Returns (closes [n] bool, new prev_kidx); the caller accumulates the score change in between."""
    round_ended, kyoku_idx = np.asarray(round_ended), np.asarray(kyoku_idx)
    closing = ((kyoku_idx != prev_kidx) | (round_ended == 2)) & (round_ended != 0)
    done = closing & (np.asarray(open_len) != 0)
    over = done | (round_ended == 2)
    return done, np.where(over, kyoku_idx, prev_kidx)


class PoolRef:
    def __init__(self, n_games, capacity, gamma, lam, hero):
        self.n, self.capacity, self.gamma, self.lam = int(n_games), int(capacity), float(gamma), float(lam)
        self.hero = np.asarray(hero, np.int64)
        self.clear()

    def clear(self):
        self.slots = []                                   # pool order: dict per transition
        self.buffers = [[] for _ in range(self.n)]        # kyoku_buffers: slot numbers of the open trajectory
        self.broken = [False] * self.n
        self.serial = [0] * self.n
        self.completed = []                               # (game, serial, [slots], reward) in closing order
        self.overflowed = self.dropped = 0

    def open_len(self):
        return np.array([len(b) for b in self.buffers], np.int64)

    def record(self, ids, row_of):
        """one call: ids [n, 4]; row_of(g) -> (features, mask [A], logits [A'], value) of game g's hero row, or None when the observation
        batch has no such row.  Returns the list of (game, slot) written, in order."""
        wrote, fill = [], len(self.slots)
        ids = np.asarray(ids)
        for g in np.flatnonzero((self.hero <= 3) & (ids[np.arange(self.n), np.minimum(self.hero, 3)] >= 0)).tolist():   # ascending games
            h = int(self.hero[g])
            row = row_of(g)
            if row is None or fill + len(wrote) >= self.capacity:
                self.overflowed += 1
                self.broken[g] = True
                continue
            feat, mask, logits, value = row
            slot = fill + len(wrote)
            wrote.append((g, slot))
            self.slots.append({"features": feat, "mask": np.asarray(mask, np.uint8), "logits": np.asarray(logits, np.float32), "action": int(ids[g][h]),
                               "value": np.float32(value), "game": g, "serial": self.serial[g], "t": len(self.buffers[g]),
                               "prev": self.buffers[g][-1] if self.buffers[g] else -1, "valid": False, "advantage": None, "return": None})
            self.buffers[g].append(slot)
        return wrote

    def close(self, ended, reward):
        for g in np.flatnonzero(np.asarray(ended) != 0).tolist():
            traj = self.buffers[g]
            if not traj and not self.broken[g]:
                continue                                   # (:307-308 T == 0)
            if self.broken[g]:
                self.dropped += len(traj)
            else:
                r = np.float32(reward[g])
                adv, ret = gae_ref([self.slots[s]["value"] for s in traj], r, self.gamma, self.lam)
                for s, a, q in zip(traj, adv, ret):
                    self.slots[s].update(valid=True, advantage=np.float32(a), **{"return": np.float32(q)})
                self.completed.append((g, self.serial[g], list(traj), float(r)))
            self.buffers[g] = []
            self.broken[g] = False
            self.serial[g] += 1

    def counts(self):
        valid = sum(1 for s in self.slots if s["valid"])
        fill = len(self.slots)
        return {"fill": fill, "valid": valid, "dropped": self.dropped, "overflowed": self.overflowed, "segments": len(self.completed),
                "open": fill - valid - self.dropped}

    def emit(self):
        """the worker's result dict over the valid slots in pool order (+ "slot": their pool slots); log_prob in float64"""
        v = [i for i, s in enumerate(self.slots) if s["valid"]]
        S = [self.slots[i] for i in v]
        if not S:
            return {"slot": np.zeros(0, np.int64)}
        masks, logits = np.stack([s["mask"] for s in S]), np.stack([s["logits"][: len(S[0]["mask"])] for s in S])
        actions = np.array([s["action"] for s in S], np.int64)
        return {"slot": np.array(v, np.int64), "features": [s["features"] for s in S], "mask": masks, "action": actions,
                "log_prob": log_prob_ref(masks, logits, actions), "logits": logits,
                "advantage": np.array([s["advantage"] for s in S], np.float32), "return": np.array([s["return"] for s in S], np.float32)}

    def stats(self):
        lens = [len(t) for _, _, t, _ in self.completed]
        rews = [r for _, _, _, r in self.completed]
        return {"kyoku_length_mean": float(np.mean(lens)), "kyoku_reward_mean": float(np.mean(rews)), "kyoku_reward_std": float(np.std(rews))} if lens else {}
