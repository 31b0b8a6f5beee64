"""CPU checks of the determinize definition: rmj_determinize_order (the library's host code, the code the kernel runs) against the
restatement of tests/determinize_ref.py, the uniformity of the definition itself, and the restatement's pool on hand-built views."""
import itertools

import pytest

from riichienv_amd import abi, vecenv
from tests import determinize_ref as ref

SEEDS = (0, 0x1234567890ABCDEF, (1 << 64) - 1)


@pytest.mark.parametrize("m", [0, 1, 2, 5, 64, 65, 164])
def test_order_equals_the_restatement(m):
    for seed in SEEDS:
        for game in (0, 1, (1 << 32) + 7):
            for seat in range(4):
                got = [int(x) for x in vecenv.determinize_order(seed, game, seat, m)]
                assert got == ref.order(seed, game, seat, m), (seed, game, seat, m)
                assert sorted(got) == list(range(m))


def test_order_refuses_what_the_keys_do_not_cover():
    with pytest.raises(vecenv.RmjError):
        vecenv.determinize_order(1, 2, 0, 257)


def test_definition_is_uniform_over_permutations():
    """24 000 fixed (seed, game, seat) triples on a pool of five: every one of the 120 permutations occurs, each 140 .. 260 times (the
    expectation is 200; the restatement gives 154 .. 233, chi-square 136.3 on 119 degrees of freedom - the inputs are fixed, nothing
    here can flake)"""
    count = dict.fromkeys(itertools.permutations(range(5)), 0)
    for s in range(24000):
        count[tuple(ref.order(7919 * s + 12345, s % 64, s % 4, 5))] += 1
    assert len(count) == 120 and min(count.values()) > 0
    print("permutation counts", min(count.values()), "..", max(count.values()),
          "chi-square", round(sum((c - 200) ** 2 / 200 for c in count.values()), 1))
    assert all(140 <= c <= 260 for c in count.values()), (min(count.values()), max(count.values()))


def _view(n_players, hands, wall, n_dora, rinshan):
    v = abi.StateView()
    for s in range(n_players):
        v.players[s].hand_len = len(hands[s])
        for j, t in enumerate(hands[s]):
            v.players[s].hand[j] = t
    v.wall_len = len(wall)
    for j, t in enumerate(wall):
        v.wall[j] = t
    v.n_dora, v.rinshan_draw_count = n_dora, rinshan
    v.drawn_tile = -1
    return v


def test_pool_after_a_kan():
    """one rinshan tile drawn, a second indicator showing: wall[] starts at wall-row position 1, the indicators sit at row positions 4
    and 6 = wall[3] and wall[5]; seat 2 looks at seats 3, 0, 1 in that order"""
    hands = [[0, 1, 2], [10, 11, 12, 13], [20, 21], [30, 31, 32, 33, 34]]
    v = _view(4, hands, list(range(100, 112)), n_dora=2, rinshan=1)
    want = [("hand", 3, j) for j in range(5)] + [("hand", 0, j) for j in range(3)] + [("hand", 1, j) for j in range(4)] + \
           [("wall", j) for j in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11)]
    assert ref.pool(v, 2, 4) == want
    # ... and the re-deal moves exactly these tiles: multiset kept, everything else in place
    new = ref.determinize_view(v, 2, 4, seed=5, global_game=9)
    old_tiles = sorted(hands[3] + hands[0] + hands[1] + [100 + j for j in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11)])
    assert sorted([new.players[s].hand[j] for s in (3, 0, 1) for j in range(len(hands[s]))] + [new.wall[j] for j in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11)]) == old_tiles
    assert list(new.players[2].hand[:2]) == [20, 21] and (new.wall[3], new.wall[5]) == (103, 105)
    for s in (3, 0, 1):
        h = list(new.players[s].hand[: len(hands[s])])
        assert h == sorted(h)
    perm = ref.order(5, 9, 2, len(want))
    assert new.wall[11] == ref._get(v, want[perm[len(want) - 1]])   # (the wall keeps the permuted order: nothing is sorted there)


def test_pool_with_a_held_opponent_and_a_drawn_tile():
    """hold = 2: opponent r = 1 (toimen) keeps its hand; seat 1, the current player, holds a drawn tile: its last slot stays last"""
    hands = [[0, 1, 2, 3], [40, 44, 48, 52, 56], [20, 21, 22, 23], [30, 31, 32, 33]]
    v = _view(4, hands, list(range(100, 110)), n_dora=1, rinshan=0)
    v.current_player, v.drawn_tile = 1, 56
    want = [("hand", 1, j) for j in range(5)] + [("hand", 3, j) for j in range(4)] + [("wall", j) for j in (0, 1, 2, 3, 5, 6, 7, 8, 9)]
    assert ref.pool(v, 0, 4, hold=2) == want
    new = ref.determinize_view(v, 0, 4, seed=1, global_game=0, hold=2)
    assert list(new.players[2].hand[:4]) == hands[2] and list(new.players[0].hand[:4]) == hands[0]
    h = list(new.players[1].hand[:5])
    assert h[:4] == sorted(h[:4]) and new.drawn_tile == h[4]
    perm = ref.order(1, 0, 0, len(want))
    assert h[4] == ref._get(v, want[perm[4]])


def test_pool_3p_with_kita():
    """3P: two opponents, the first indicator at wall-row position 8; one kita replacement drawn (rinshan 1) -> wall[7] is shown; kita
    tiles are no part of the view's hands and stay"""
    hands = [[36, 37, 38], [72, 73, 74, 75], [100, 101, 102, 103, 104]]
    v = _view(3, hands, list(range(1, 21)), n_dora=1, rinshan=1)
    v.players[1].n_kita, v.players[1].kita[0] = 1, 120
    want = [("hand", 2, j) for j in range(5)] + [("hand", 0, j) for j in range(3)] + [("wall", j) for j in range(20) if j != 7]
    assert ref.pool(v, 1, 3) == want
    new = ref.determinize_view(v, 1, 3, seed=3, global_game=2)
    assert new.wall[7] == 8 and new.players[1].kita[0] == 120 and list(new.players[1].hand[:4]) == hands[1]
    assert list(new.players[3].hand) == [0] * 14
