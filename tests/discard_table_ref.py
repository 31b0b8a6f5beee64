"""The yardstick of the discard efficiency table (rmj_discard_table*, LogSampleBuilder(efficiency=True)): host only, numpy over
oracle.shanten and nothing of the library's.

For a hand histogram c[34] of n tiles and a visible histogram v[34]:
  valid types   all 34 in 4P; type 0 and types 8..33 in 3P
  sh(x)         oracle.shanten (calculate_shanten / _3p with tiles / 3 groups)
  x of 3k+1:    A(x) = { t valid : x[t] < 4 and sh(x + t) < sh(x) }, accept = |A|, ukeire = sum over A of max(0, max(0, 4 - v[t]) - x[t]),
                mask = the bits of A
  column t<34   n % 3 == 2 and c[t] > 0: x = c - e_t, shanten[t] = sh(x), accept, ukeire, mask of x; else shanten 127 and the rest 0
  column 34     shanten = sh(c); n % 3 == 1: accept, mask of c; n % 3 == 2: accept and ukeire are, separately, the maxima over the t
                with shanten[t] <= shanten[34], mask 0; n % 3 == 0: the shanten only.  ukeire[34] of a 3n+1 hand: calculate_best_ukeire
                walks the discards of such a hand too - the maximum of ukeire(c - e_d) over the held d with sh(c - e_d) <= sh(c)
An absent row (more than 14 tiles, a count above 4, a seat that does not exist): every shanten 127, the rest 0."""
import numpy as np

NONE, COLS = 127, 35
FIELDS = ("shanten", "accept", "ukeire", "mask")
SANMA_TYPES = [0, 8] + list(range(9, 34))
_ROWS = {}   # (hand bytes, visible bytes, sanma) -> row: most events of a game change one seat


def empty(n):
    return {"shanten": np.full((n, COLS), NONE, np.int8), "accept": np.zeros((n, COLS), np.uint8), "ukeire": np.zeros((n, COLS), np.uint8),
            "mask": np.zeros((n, COLS), np.uint64)}


def table(counts, visible=None, sanma=False):
    """{"shanten" i8, "accept" u8, "ukeire" u8, "mask" u64}, each [n, 35], of the histograms counts [n, 34] against visible [n, 34] (None:
    zeros): every hand the definition names goes through ONE oracle.shanten call."""
    from oracle import oracle

    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 34)
    n = counts.shape[0]
    vis = np.zeros_like(counts) if visible is None else np.asarray(visible, dtype=np.int64).reshape(-1, 34)
    valid = np.array(SANMA_TYPES if sanma else list(range(34)))
    eye = np.eye(34, dtype=np.int64)
    bit = np.array([1 << int(t) for t in valid], dtype=np.uint64)
    out = empty(n)
    blocks, rows, at = [], [], 0
    for i in range(n):
        c = counts[i]
        tot = int(c.sum())
        if tot > 14 or int(c.max(initial=0)) > 4:
            continue
        held = np.flatnonzero(c > 0) if tot % 3 else np.zeros(0, np.int64)
        bases = c[None, :] - eye[held]                       # the hand without one tile of every held type
        if tot % 3 == 1:
            bases = np.concatenate([c[None, :], bases])      # ... behind the hand itself
        ok = bases[:, valid] < 4                             # x[t] < 4
        draws = bases[:, None, :] + np.where(ok[:, :, None], eye[valid][None, :, :], 0)   # (a draw that is not ok stays the base: never below it)
        blocks.append(np.concatenate([c[None, :], bases, draws.reshape(-1, 34)]))
        rows.append((i, tot % 3, held, bases, ok, at))
        at += blocks[-1].shape[0]
    if not blocks:
        return out
    sh = oracle.shanten(np.concatenate(blocks).astype(np.uint8), sanma).astype(np.int64)
    for i, r, held, bases, ok, at in rows:
        nb = bases.shape[0]
        cur, sb = sh[at], sh[at + 1: at + 1 + nb]
        sd = sh[at + 1 + nb: at + 1 + nb + nb * valid.size].reshape(nb, valid.size)
        A = ok & (sd < sb[:, None])
        accept = A.sum(axis=1)
        left = np.maximum(0, np.maximum(0, 4 - vis[i][valid])[None, :] - bases[:, valid])
        ukeire = (A * left).sum(axis=1)
        mask = (A.astype(np.uint64) * bit[None, :]).sum(axis=1, dtype=np.uint64)
        out["shanten"][i, 34] = cur
        if r == 2:
            out["shanten"][i, held], out["accept"][i, held], out["ukeire"][i, held], out["mask"][i, held] = sb, accept, ukeire, mask
            keep = sb <= cur
            out["accept"][i, 34] = accept[keep].max(initial=0)
            out["ukeire"][i, 34] = ukeire[keep].max(initial=0)
        elif r == 1:
            out["accept"][i, 34], out["mask"][i, 34] = accept[0], mask[0]
            keep = sb[1:] <= cur                             # calculate_best_ukeire's walk over the discards of the 3n+1 hand
            out["ukeire"][i, 34] = ukeire[1:][keep].max(initial=0)
    return out


def view_histograms(view, seat, n_players):
    """(hand [34], visible [34]) of seat `seat` of an abi.StateView: the concealed tiles by type; every seat's discards, every seat's meld
    tiles and the revealed dora indicators (encode.rs:317-327)"""
    c, v = np.zeros(34, np.uint8), np.zeros(34, np.uint8)
    p = view.players[seat]
    for t in p.hand[: p.hand_len]:
        c[t >> 2] += 1
    for s in range(n_players):
        q = view.players[s]
        for t in q.discards[: q.n_discards]:
            v[t >> 2] += 1
        for m in q.melds[: q.n_melds]:
            for t in m.tiles[: m.n_tiles]:
                v[t >> 2] += 1
    for t in view.dora[: view.n_dora]:
        v[t >> 2] += 1
    return c, v


def rows_of_views(pairs, n_players):
    """the table of every (view, seat) of `pairs`, stacked; a seat >= n_players is an absent row"""
    sanma = n_players == 3
    out = empty(len(pairs))
    todo, where = {}, []
    for i, (view, seat) in enumerate(pairs):
        if seat >= n_players:
            where.append(None)
            continue
        c, v = view_histograms(view, seat, n_players)
        key = (c.tobytes(), v.tobytes(), sanma)
        if key not in _ROWS:
            todo.setdefault(key, (c, v))
        where.append(key)
    if todo:
        keys = list(todo)
        t = table(np.stack([todo[k][0] for k in keys]), np.stack([todo[k][1] for k in keys]), sanma)
        if len(_ROWS) > 200000:
            _ROWS.clear()
        for j, k in enumerate(keys):
            _ROWS[k] = {f: t[f][j].copy() for f in FIELDS}
    for i, key in enumerate(where):
        if key is not None:
            for f in FIELDS:
                out[f][i] = _ROWS[key][f]
    return out


def log_rows(log, mode, keys):
    """{(event index, seat): (view, seat)} resolved to rows: the table of the seats in `keys` (a set of (event index, seat)) of one log
    of MJAI event dicts replayed in an oracle.Game, from the state BEFORE each event is applied."""
    from oracle import oracle

    n = 3 if mode >= 3 else 4
    game = oracle.Game(game_mode=mode, skip_log=True)
    order, pairs = [], []
    for i, ev in enumerate(log):
        want = [s for s in range(n) if (i, s) in keys]
        if want:
            view = game.peek()   # (a StateView of its own: it outlives the events applied below)
            for s in want:
                order.append((i, s))
                pairs.append((view, s))
        game.apply_event(ev, replay=True)
    t = rows_of_views(pairs, n)
    return {k: {f: t[f][j] for f in FIELDS} for j, k in enumerate(order)}


def best_discard(shanten, accept, ukeire, mask_row, sanma):
    """The CPU counterpart of riichienv_amd.efficiency.best_discard for ONE row: plain Python over the legal discard ids."""
    types = SANMA_TYPES if sanma else list(range(34))
    best = None
    for i, t in enumerate(types):
        if not mask_row[i]:
            continue
        key = (int(shanten[t]), -int(ukeire[t]), -int(accept[t]), i)
        if best is None or key < best:
            best = key
    return -1 if best is None else best[3]
