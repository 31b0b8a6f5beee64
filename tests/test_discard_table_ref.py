"""The yardstick of the discard efficiency table (tests/discard_table_ref.py) against what the oracle already pins: its column 34 is
calculate_shanten, calculate_effective_tiles_with_discard and calculate_best_ukeire (4P and 3P) on sampled hands of every size class;
and riichienv_amd.efficiency.best_discard against a plain-Python counterpart on hand-made rows.  No GPU."""
import numpy as np
import pytest

from riichienv_amd import abi
from tests import discard_table_ref as D
from tests import shanten_sampler as S

SEED, N = 11, 256
_CACHE = {}


def sampled(sanma):
    """(hands [256, 34], visible [256, 34], the yardstick's table) of a mode: made once, shared, never changed"""
    if sanma not in _CACHE:
        hands = S.sample_hands(SEED, N, sanma)
        vis = np.array([S.sample_visible(SEED, i, hands[i]) for i in range(N)], dtype=np.uint8)
        _CACHE[sanma] = (hands, vis, D.table(hands, vis, sanma))
    return _CACHE[sanma]


@pytest.mark.parametrize("sanma", [False, True])
def test_column_34_is_what_the_oracle_pins(sanma):
    from oracle import oracle

    hands, vis, t = sampled(sanma)
    tot = hands.sum(axis=1).astype(int)
    assert (t["shanten"][:, 34] == oracle.shanten(hands, sanma)).all()
    eff = oracle.effective_tiles(hands, sanma)
    uke = oracle.best_ukeire(hands, vis, sanma)
    drawn = tot % 3 != 0            # (the reference asserts on a 3n hand)
    assert drawn.sum() == N, "the sampler makes 3n+1 and 3n+2 hands only"
    assert (t["accept"][:, 34].astype(np.uint32) == eff).all(), np.flatnonzero(t["accept"][:, 34] != eff)[:4]
    assert (t["ukeire"][:, 34].astype(np.uint32) == uke).all(), np.flatnonzero(t["ukeire"][:, 34] != uke)[:4]
    full = tot % 3 == 2
    assert not t["mask"][full, 34].any()
    one = tot % 3 == 1
    assert (t["shanten"][one, :34] == D.NONE).all() and not t["accept"][one, :34].any()
    pop = np.array([[bin(int(m)).count("1") for m in row] for row in t["mask"]])
    assert (pop[:, :34] == t["accept"][:, :34]).all() and (pop[one, 34] == t["accept"][one, 34]).all()
    held = hands[full] > 0
    assert ((t["shanten"][full, :34] != D.NONE) == held).all(), "a column for every held type of a 3n+2 hand and no other"


def test_the_sampled_hands_cover_what_the_kernels_branch_on():
    raising, short = 0, {1: 0, 2: 0}
    for sanma in (False, True):
        hands, _, t = sampled(sanma)
        tot = hands.sum(axis=1).astype(int)
        assert set(tot.tolist()) == set(S.SIZES), "every size class"
        cols = t["shanten"][:, :34].astype(int)
        raising += int(((cols != D.NONE) & (cols > t["shanten"][:, 34:35].astype(int))).sum())
        if sanma:
            free = (hands[:, 27:34] == 0).sum(axis=1)
            for r in (1, 2):
                short[r] += int(((free < 3) & (tot % 3 == r)).sum())
    print(f"entries that raise the shanten: {raising}; 3P hands with fewer than three free honor slots: {short[2]} of 3n+2, {short[1]} of 3n+1")
    assert raising > 0 and short[1] > 0 and short[2] > 0


def test_absent_rows_and_raw_sanma_histograms():
    big = np.zeros((3, 34), np.uint8)
    big[0, :15] = 1                 # 15 tiles
    big[1, 3] = 5                   # a count of 5
    big[2, :14] = 1
    t = D.table(big)
    for f in ("accept", "ukeire", "mask"):
        assert not t[f][:2].any()
    assert (t["shanten"][:2] == D.NONE).all() and t["shanten"][2, 34] != D.NONE
    # a held 2m..8m of a raw 3P histogram gets its column; no 2m..8m is ever accepted
    hands = S.sample_hands(SEED, 32, False)
    t3 = D.table(hands, None, True)
    full = hands.sum(axis=1) % 3 == 2
    assert (t3["shanten"][full, 1:8][hands[full, 1:8] > 0] != D.NONE).all()
    assert not (t3["mask"] & np.uint64(0xFE)).any()


def _row(sh, uk, ac):
    t = D.empty(1)
    for c, (s, u, a) in enumerate(zip(sh, uk, ac)):
        t["shanten"][0, c], t["ukeire"][0, c], t["accept"][0, c] = s, u, a
    return t


@pytest.mark.parametrize("sanma", [False, True])
def test_best_discard_on_hand_made_rows(sanma):
    import torch

    from riichienv_amd import efficiency

    types = D.SANMA_TYPES if sanma else list(range(34))
    A = abi.ACTION_SPACE_3P if sanma else abi.ACTION_SPACE_4P
    col = {t: i for i, t in enumerate(types)}
    sh, uk, ac = [D.NONE] * 35, [0] * 35, [0] * 35
    # held: 1m (2-shanten), 2p / 5p (1-shanten, 5p has the larger ukeire), 9s (1-shanten, the ukeire of 5p, fewer kinds), E (as 9s: a later id)
    for t, (s, u, a) in {0: (2, 30, 9), 10: (1, 12, 4), 13: (1, 16, 5), 26: (1, 16, 4), 27: (1, 16, 4)}.items():
        sh[t], uk[t], ac[t] = s, u, a
    sh[34], uk[34], ac[34] = 1, 16, 5
    rows, masks, want = [], [], []

    def case(legal_types, answer):
        m = np.zeros(A, np.uint8)
        for t in legal_types:
            m[col[t]] = 1
        m[40] = 1                                   # an id beyond the discards never matters
        rows.append(_row(sh, uk, ac))
        masks.append(m)
        want.append(-1 if answer is None else col[answer])

    case([0, 10, 13, 26, 27], 13)                   # lowest shanten, then the highest ukeire, then the most kinds
    case([0, 10, 26, 27], 26)                       # the tie of 9s and E goes to the lower id
    case([0], 0)                                    # a riichi mask: one legal discard, whatever it costs
    case([], None)                                  # no discard is legal
    case([0, 10], 10)
    table = {f: torch.from_numpy(np.concatenate([r[f] for r in rows])) for f in ("shanten", "accept", "ukeire")}
    mask = torch.from_numpy(np.stack(masks))
    got = efficiency.best_discard(table, mask, sanma).tolist()
    ref = [D.best_discard(r["shanten"][0], r["accept"][0], r["ukeire"][0], m, sanma) for r, m in zip(rows, masks)]
    assert ref == want and got == want, (got, ref, want)
    assert efficiency.best_discard({"dt_" + f: v for f, v in table.items()}, mask, sanma).tolist() == want
    text = efficiency.describe({f: r[0] for f, r in rows[0].items()})
    assert text.splitlines()[0].startswith("hand: 1-shanten, 5 kinds / 16 tiles") and "cut 5p: 1-shanten, 5 kinds / 16 tiles" in text
