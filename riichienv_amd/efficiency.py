"""Tile efficiency on top of the discard efficiency table (VecRiichiEnv.discard_table, TorchVecEnv.discard_table_compact, the
"dt_*" fields of LogSampleBuilder(efficiency=True)): the most efficient legal discard of every row, and a row as text."""
from .abi import DTAB_NONE

TILE_NAMES = [f"{r}{s}" for s in "mps" for r in range(1, 10)] + ["E", "S", "W", "N", "P", "F", "C"]
SANMA_TYPES = [0, 8] + list(range(9, 34))   # discard id 0..26 of the 3P action space -> tile type


def discard_types(sanma):
    """tile type of the discard ids (0..33 in 4P, 0..26 in 3P)"""
    return SANMA_TYPES if sanma else list(range(34))


def best_discard(table, mask, sanma=False):
    """The discard id per row with the lowest shanten after it among the ids legal in `mask` [k, A] (the action mask; ids 0..33 by tile
    type in 4P, 0..26 over the types [0, 8, 9..33] in 3P); ties go to the highest ukeire, then the highest accept, then the lowest id.
    table: {"shanten", "accept", "ukeire"} tensors [k, 35] (a "dt_" prefix is accepted).  int64 [k], -1 where no discard is legal.
    Torch ops only, on the tensors' device."""
    import torch

    get = lambda f: (table[f] if f in table else table["dt_" + f])
    cols = torch.as_tensor(discard_types(sanma), dtype=torch.int64, device=get("shanten").device)
    sh = get("shanten").to(torch.int64).index_select(1, cols)
    uk = get("ukeire").to(torch.int64).index_select(1, cols)
    ac = get("accept").to(torch.int64).index_select(1, cols)
    ids = torch.arange(cols.shape[0], dtype=torch.int64, device=sh.device)
    # one key per id, ordered as the rule is: shanten up, ukeire down, accept down, id up (every field below 256)
    key = ((sh + 2) << 24) + ((255 - uk) << 16) + ((255 - ac) << 8) + ids
    legal = mask[:, : cols.shape[0]].to(sh.device) != 0
    key = torch.where(legal, key, torch.full_like(key, 1 << 40))
    best = key.argmin(dim=1)
    return torch.where(legal.any(dim=1), best, torch.full_like(best, -1))


def describe(row):
    """One table row ({"shanten", "accept", "ukeire"[, "mask"]}: arrays of 35, a "dt_" prefix is accepted) as text, a line per discard
    and one for the hand: `cut 3p: 1-shanten, 5 kinds / 17 tiles [2m 5m ...]`."""
    get = lambda f: (row[f] if f in row else row.get("dt_" + f))
    sh, ac, uk, mk = get("shanten"), get("accept"), get("ukeire"), get("mask")

    def line(what, c):
        s = int(sh[c])
        txt = f"{what}: " + ("agari" if s < 0 else "tenpai" if s == 0 else f"{s}-shanten") + f", {int(ac[c])} kinds / {int(uk[c])} tiles"
        if mk is not None and int(mk[c]):
            txt += " [" + " ".join(TILE_NAMES[t] for t in range(34) if (int(mk[c]) >> t) & 1) + "]"
        return txt

    if int(sh[34]) == DTAB_NONE:
        return "(absent row)"
    return "\n".join([line("hand", 34)] + [line("cut " + TILE_NAMES[c], c) for c in range(34) if int(sh[c]) != DTAB_NONE])
