"""Float64 restatement of the trainer-side masked categorical sampler (sample_ids_row in riichienv_amd/csrc/rmj_policy.hip.h: the
kernel behind rmj_sample_ids_device / TorchVecEnv.sample_ids and the draw in front of rmj_step_sample_encode_device).  numpy only.

For every seat that is to act (active bit set, game not done, nlegal > 0) and every id < A (82 in 4P, 60 in 3P) whose mask byte
is set:

    base = sm64(seed ^ sm64(game_offset + g)) + (step_count << 10)
    h    = sm64(base + (seat << 8) + id)
    u    = min(((float32)(h >> 40) + 0.5f) * 2^-24f, 1 - 2^-24)        (float32, bit for bit as on the device: strictly in (0, 1))
    key  = logit - log(-log(u))                                         (float64; NaN -> -inf)

and the id with the largest key wins, ties to the lower id.  -1 for every other seat.  Only the cells named above are read, so a
caller may fill all others (padding columns >= A, illegal ids, rows of seats that do not act) with anything."""
import math

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
U_MAX = np.float32(np.nextafter(np.float32(1.0), np.float32(0.0)))     # 1 - 2^-24, the largest float32 below 1
TOP24 = 0xFFFFFF


def sm64(x):
    """splitmix64's output function (rmj_common.hip.h sm64) over uint64 arrays, wrapping like the device."""
    z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def game_base(seed, game_offset, games, step_counts):
    """base of the games `games` (local indices) at their step counts: sm64(seed ^ sm64(game_offset + g)) + (step_count << 10)"""
    g = np.asarray(games, dtype=np.uint64) + np.uint64(game_offset)
    s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        return sm64(s ^ sm64(g)) + (np.asarray(step_counts, dtype=np.uint64) << np.uint64(10))


def id_hash(base, seat, ids):
    with np.errstate(over="ignore"):
        return sm64(np.asarray(base, dtype=np.uint64) + (np.asarray(seat, dtype=np.uint64) << np.uint64(8)) + np.asarray(ids, dtype=np.uint64))


def hash_to_u(top24):
    """The 24-bit hash value (h >> 40) -> u in float32, as the kernel rounds it: (x + 0.5f) rounds to even above 2^23, and the top
    value (which rounds to 2^24, u = 1) is clamped to the largest float32 below 1."""
    x = np.asarray(top24, dtype=np.uint32).astype(np.float32)
    u = (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return np.minimum(u, U_MAX)


def gumbel(u):
    """-log(-log(u)) in float64 of the float32 u"""
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def snapshot(env):
    """The sampler's inputs of a TorchVecEnv, on the host: what the kernel reads at the next launch."""
    return {
        "status": env.status_raw.cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
        "nlegal": env.nlegal.cpu().numpy().copy(),
        "mask": env.mask.cpu().numpy().copy(),
        "step_counts": np.asarray(env.env.step_counts(), dtype=np.uint64).copy(),
        "game_offset": int(env.env.game_offset),
        "game_mode": int(env.env.game_mode),
    }


def acting(snap):
    """bool [n, 4]: the seats the sampler draws for (active bit, game not done, nlegal > 0)"""
    st = snap["status"]
    am = np.where(((st >> 16) & 0xFF) != 0, 0, st & 0xF)
    return (((am[:, None] >> np.arange(4)[None, :]) & 1) == 1) & (snap["nlegal"] != 0)


def sample_ref(snap, seed, logits=None):
    """(ids int32 [n, 4], top float64 [n, 4], second float64 [n, 4]): the drawn id, its key and the runner-up's key (-inf where the
    seat has one candidate; NaN where nobody draws).  logits: float32 [n, 4, stride] (stride >= A) or None."""
    n = snap["status"].shape[0]
    A = 60 if snap["game_mode"] >= 3 else 82
    cand = acting(snap)[:, :, None] & (snap["mask"][:, :, :A] != 0)
    g, s, i = np.nonzero(cand)                                   # (game, seat, id) order
    base = game_base(seed, snap["game_offset"], np.arange(n), snap["step_counts"])
    h = id_hash(base[g], s, i)
    key = gumbel(hash_to_u((h >> np.uint64(40)).astype(np.uint32)))
    if logits is not None:
        lg = np.asarray(logits)
        assert lg.dtype == np.float32 and lg.ndim == 3 and lg.shape[:2] == (n, 4) and lg.shape[2] >= A
        key = lg[g, s, i].astype(np.float64) + key
    key = np.where(np.isnan(key), -np.inf, key)
    row = g.astype(np.int64) * 4 + s
    order = np.lexsort((i, -key, row))                           # per row: largest key first, ties to the lower id
    row, i, key = row[order], i[order], key[order]
    first = np.flatnonzero(np.r_[True, row[1:] != row[:-1]]) if row.size else np.zeros(0, np.int64)
    ids = np.full(n * 4, -1, np.int32)
    top = np.full(n * 4, np.nan)
    second = np.full(n * 4, np.nan)
    ids[row[first]] = i[first]
    top[row[first]] = key[first]
    second[row[first]] = -np.inf
    nxt = first + 1
    has2 = nxt < row.size
    has2[has2] = row[nxt[has2]] == row[first[has2]]
    second[row[first[has2]]] = key[nxt[has2]]
    return ids.reshape(n, 4), top.reshape(n, 4), second.reshape(n, 4)


def close_rows(top, second, rel=1e-4):
    """bool [n, 4]: rows whose top-two float64 keys are within tau = rel * (1 + |top|) - there the float32 keys of the device may
    order them either way.  Rows whose two keys are both +inf or both -inf are exact ties (lower id) and are not close."""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(top) & np.isfinite(second)
        return fin & (top - second <= rel * (1.0 + np.abs(top)))


def softmax_legal(logits_row, legal_ids):
    """float64 probabilities of the legal ids under softmax(logits) (uniform without logits); -inf / NaN ids get 0"""
    if logits_row is None:
        return np.full(len(legal_ids), 1.0 / len(legal_ids))
    z = np.asarray(logits_row, dtype=np.float64)[legal_ids]
    z = np.where(np.isnan(z), -np.inf, z)
    p = np.exp(z - z.max())
    return p / p.sum()


def chi2_sf(x, k):
    """P(X >= x) for X ~ chi-square with k degrees of freedom: the regularized upper incomplete gamma Q(k / 2, x / 2)
    (power series below a + 1, Lentz's continued fraction above)."""
    a, y = 0.5 * k, 0.5 * x
    if y <= 0:
        return 1.0
    lg = a * math.log(y) - y - math.lgamma(a)
    if y < a + 1:
        term = total = 1.0 / a
        d = a
        for _ in range(10000):
            d += 1
            term *= y / d
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return max(0.0, 1.0 - total * math.exp(lg))
    tiny = 1e-300
    b = y + 1 - a
    c, dd = 1 / tiny, 1 / b
    f = dd
    for m in range(1, 10000):
        an = -m * (m - a)
        b += 2
        dd = an * dd + b
        dd = tiny if abs(dd) < tiny else dd
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        dd = 1 / dd
        delta = dd * c
        f *= delta
        if abs(delta - 1) < 1e-16:
            break
    return math.exp(lg) * f


def chi_square(observed, expected, min_expected=5.0):
    """(statistic, degrees of freedom, p) of observed counts against expected counts, bins merged (smallest expectation first) until
    every merged bin expects at least min_expected draws."""
    obs = np.asarray(observed, dtype=np.float64)
    exp = np.asarray(expected, dtype=np.float64)
    order = np.argsort(exp, kind="stable")
    bins, o_acc, e_acc = [], 0.0, 0.0
    for j in order:
        o_acc += obs[j]
        e_acc += exp[j]
        if e_acc >= min_expected:
            bins.append((o_acc, e_acc))
            o_acc = e_acc = 0.0
    if e_acc > 0 or o_acc > 0:
        if bins:
            o_last, e_last = bins.pop()
            bins.append((o_last + o_acc, e_last + e_acc))
        else:
            bins.append((o_acc, e_acc))
    ob = np.array([b[0] for b in bins])
    eb = np.array([b[1] for b in bins])
    stat = float(((ob - eb) ** 2 / eb).sum())
    df = len(bins) - 1
    return stat, df, (chi2_sf(stat, df) if df > 0 else 1.0)
