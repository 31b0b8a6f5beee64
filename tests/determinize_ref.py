"""The yardstick of rmj_determinize_device: host only, from an abi.StateView and the definition in include/riichi_mi355x.h, nothing of
the library's code.

The hidden pool of (view, viewpoint seat a), in canonical order: for r = 0, 1, 2 with r + 1 < NP and bit r of `hold` clear the slots
players[(a + 1 + r) mod NP].hand[0 .. hand_len); then wall[j] ascending except the revealed dora indicators, j + rinshan_draw_count =
D + 2 k for k < n_dora (D = 4, 3P: 8).  The permutation sorts the canonical indices by 64-bit keys; the new tile at canonical position r
is the old tile at canonical position perm[r].  Then every re-dealt hand is sorted, except that a re-dealt current player holding a
drawn tile (drawn_tile set, hand_len = 2 mod 3) keeps its last slot last and drawn_tile names the tile now in it."""
import ctypes as C

from riichienv_amd import abi

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix(z):
    z = (z + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def order(seed, global_game, seat, m):
    base = mix((seed + global_game) & M64)
    key = [mix((base + (seat * 256 + i) * GOLD) & M64) for i in range(m)]
    return sorted(range(m), key=lambda i: (key[i], i))


def pool(view, seat, n_players, hold=0):
    """the canonical order as locations: ("hand", s, slot) / ("wall", j)"""
    out = []
    for r in range(n_players - 1):
        if (hold >> r) & 1:
            continue
        s = (seat + 1 + r) % n_players
        out += [("hand", s, j) for j in range(view.players[s].hand_len)]
    first = 8 if n_players == 3 else 4
    shown = {first + 2 * k - view.rinshan_draw_count for k in range(view.n_dora)}
    out += [("wall", j) for j in range(view.wall_len) if j not in shown]
    return out


def _get(view, loc):
    return view.players[loc[1]].hand[loc[2]] if loc[0] == "hand" else view.wall[loc[1]]


def _put(view, loc, tile):
    if loc[0] == "hand":
        view.players[loc[1]].hand[loc[2]] = tile
    else:
        view.wall[loc[1]] = tile


def copy_view(view):
    return abi.StateView.from_buffer_copy(bytes(C.string_at(C.byref(view), C.sizeof(view))))


def determinize_view(view, seat, n_players, seed, global_game, hold=0):
    """the view after rmj_determinize_device of (its game, seat), as far as the definition goes: hands, wall and drawn_tile (active_mask
    of a WAIT_RESPONSE view follows from the claims of the new hands and is not restated here)"""
    new = copy_view(view)
    locs = pool(view, seat, n_players, hold)
    perm = order(seed, global_game, seat, len(locs))
    for r, loc in enumerate(locs):
        _put(new, loc, _get(view, locs[perm[r]]))
    for s in sorted({loc[1] for loc in locs if loc[0] == "hand"}):
        p = new.players[s]
        n = p.hand_len
        drawn = s == view.current_player and view.drawn_tile >= 0 and n % 3 == 2
        head = sorted(p.hand[: n - 1 if drawn else n])
        for j, t in enumerate(head):
            p.hand[j] = t
        if drawn:
            new.drawn_tile = p.hand[n - 1]
    return new
