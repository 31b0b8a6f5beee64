"""The yardstick of rmj_determinize_ex_device with RMJ_DETF_RIICHI_TENPAI: host only, from an abi.StateView and the definition in
include/riichi_mi355x.h, with the oracle's shanten numbers and nothing of the library's code.  It extends tests/determinize_ref.py.

After the permutation has been applied and before anything is sorted: Q = the canonical indices of the pool whose location is no hand
slot of a seat that has declared riichi.  For r = 0, 1, 2 with r + 1 < NP and bit r of `hold` clear, seat s = (a + 1 + r) mod NP is
repaired if it has declared riichi and hand_len = n with n mod 3 = 1: cur = shanten(hand); for k = 0 .. 11 while cur > 0, over slots i < n
(type d) and partners j in Q (type t) with d != t let v = shanten(hand - d + t); want = cur - 1 if a pair reaches it, else cur; no pair
with v == want ends the walk; else the pair with the least (key, i, j) exchanges its two tiles in place and cur = want."""
import numpy as np

from oracle import oracle
from tests import determinize_ref as ref
from tests.determinize_ref import GOLD, M64, mix

STEPS = 12


def swap_key(seed, global_game, seat, r, k, i, j):
    base = mix((seed + global_game) & M64)
    return mix((base + (1024 + ((((seat * 4 + r) * 16 + k) * 16 + i) * 256 + j)) * GOLD) & M64)


def _counts(tiles):
    c = [0] * 34
    for t in tiles:
        c[t >> 2] += 1
    return c


def shanten(tiles, sanma):
    return int(oracle.shanten(np.array([_counts(tiles)], np.uint8), sanma)[0])


def has_waits(tiles, n_melds, sanma):
    """the existing NOTEN criterion: a hand of 13 tiles with its melds that some type it does not hold four times completes"""
    if len(tiles) + 3 * n_melds != 13:
        return False
    c = _counts(tiles)
    rows = []
    for t in range(34):
        if c[t] < 4:
            x = list(c)
            x[t] += 1
            rows.append(x)
    return bool((oracle.shanten(np.array(rows, np.uint8), sanma) == -1).any())


def repair(new, view, seat, n_players, seed, global_game, hold=0):
    """the walks on `new` (the view after the permutation, unsorted); returns the census: one dict per repaired seat with the shanten
    at the start and at the end and the verdict of every exchange ("down" / "side")"""
    sanma = n_players == 3
    locs = ref.pool(view, seat, n_players, hold)
    riichi = {s for s in range(n_players) if view.players[s].riichi_declared}
    partners = [j for j, loc in enumerate(locs) if not (loc[0] == "hand" and loc[1] in riichi)]
    census = []
    for r in range(n_players - 1):
        s = (seat + 1 + r) % n_players
        n = view.players[s].hand_len
        if (hold >> r) & 1 or s not in riichi or n % 3 != 1:
            continue
        hand = new.players[s].hand
        cur = shanten(hand[:n], sanma)
        walk = {"seat": s, "r": r, "start": cur, "steps": [], "partners": len(partners)}
        for k in range(STEPS):
            if cur <= 0:
                break
            base = _counts(hand[:n])
            ptype = {j: ref._get(new, locs[j]) >> 2 for j in partners}
            pairs = sorted({(hand[i] >> 2, t) for i in range(n) for t in set(ptype.values()) if hand[i] >> 2 != t})
            if not pairs:
                break
            rows = []
            for d, t in pairs:
                x = list(base)
                x[d] -= 1
                x[t] += 1
                rows.append(x)
            v = dict(zip(pairs, (int(q) for q in oracle.shanten(np.array(rows, np.uint8), sanma))))
            want = cur - 1 if cur - 1 in v.values() else cur
            best = None
            for i in range(n):
                for j in partners:
                    if v.get((hand[i] >> 2, ptype[j])) == want:
                        cand = (swap_key(seed, global_game, seat, r, k, i, j), i, j)
                        best = cand if best is None or cand < best else best
            if best is None:
                break
            _, i, j = best
            x, y = hand[i], ref._get(new, locs[j])
            hand[i] = y
            ref._put(new, locs[j], x)
            walk["steps"].append("down" if want < cur else "side")
            cur = want
        walk["end"] = cur
        census.append(walk)
    return census


def determinize_view(view, seat, n_players, seed, global_game, hold=0):
    """(the view after the flagged re-deal - hands, wall and drawn_tile, as tests/determinize_ref.determinize_view restates the
    unflagged one -, the status bits the definition gives: DET_SWAPPED and RIICHI_NOTEN << r, the census of the walks)"""
    new = ref.copy_view(view)
    locs = ref.pool(view, seat, n_players, hold)
    perm = ref.order(seed, global_game, seat, len(locs))
    for r, loc in enumerate(locs):
        ref._put(new, loc, ref._get(view, locs[perm[r]]))
    census = repair(new, view, seat, n_players, seed, global_game, hold)
    for s in sorted({loc[1] for loc in locs if loc[0] == "hand"}):
        p = new.players[s]
        n = p.hand_len
        drawn = s == view.current_player and view.drawn_tile >= 0 and n % 3 == 2
        for j, t in enumerate(sorted(p.hand[: n - 1 if drawn else n])):
            p.hand[j] = t
        if drawn:
            new.drawn_tile = p.hand[n - 1]
    status = 128 if any(w["steps"] for w in census) else 0
    for r in range(n_players - 1):
        s = (seat + 1 + r) % n_players
        p = new.players[s]
        if not (hold >> r) & 1 and p.riichi_declared and not has_waits(list(p.hand[: p.hand_len]), p.n_melds, n_players == 3):
            status |= 16 << r
    return new, status, census
