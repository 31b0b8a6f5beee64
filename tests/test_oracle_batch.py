"""oracle.Batch (orc_batch_*: n oracle games kept between calls, stepped and encoded on host threads) pinned on oracle.Game stepped one
game at a time from Python: after each uneven chunk of steps, status, state, step counts, scores, legal lists, masks and waits of every
game, encode_extended / encode of chosen rows and the aux blocks of every game; and at the end, rollout_policy with the sum of the
chunks.  4P and 3P, both policies, with walls of their own."""
import numpy as np
import pytest

from riichienv_amd import abi
from riichienv_amd.shard import game_seed
from oracle import oracle
from tests.parity_util import diff_dict, normalize_view

CHUNKS = (1, 37, 3, 120, 59)


def _args(mode, n, rng):
    """dealer, round, scores, honba, sticks on every other game; walls of their own on every third (255 = shuffle)"""
    np_, size = (3, 108) if mode >= 3 else (4, 136)
    start = 35000 if np_ == 3 else 25000
    oya = np.full(n, -1, np.int32)
    rw = np.full(n, -1, np.int32)
    honba = np.full(n, -1, np.int32)
    ky = np.full(n, -1, np.int32)
    scores = np.full((n, np_), start, np.int32)
    walls = np.full((n, size), 255, np.uint8)
    tiles = [t for t in range(136) if mode < 3 or not (4 <= t // 4 <= 10)]   # 3P: no 2m..8m
    for g in range(n):
        if g % 2:
            oya[g], rw[g], honba[g], ky[g] = rng.integers(np_), rng.integers(2), rng.integers(4), rng.integers(3)
        if g % 3 == 0:
            walls[g] = rng.permutation(tiles)
    return dict(oya=oya, round_wind=rw, scores=scores, honba=honba, kyotaku=ky, walls=walls)


def _game(mode, rule, seed, off, g, args):
    o = oracle.Game(game_mode=mode, seed=game_seed(seed, off + g), rule_bits=rule)
    w = args["walls"][g]
    o.reset(wall=None if w[0] == 255 else [int(x) for x in w], oya=int(args["oya"][g]), round_wind=int(args["round_wind"][g]),
            scores=[int(x) for x in args["scores"][g]], honba=int(args["honba"][g]), kyotaku=int(args["kyotaku"][g]))
    return o


@pytest.mark.parametrize("mode,rule,policy", [(2, abi.RULE_TENHOU, "greedy"), (1, abi.RULE_MJSOUL, "random"),
                                              (5, abi.RULE_MJSOUL, "greedy"), (4, abi.RULE_TENHOU, "random")])
def test_batch_equals_games_stepped_one_by_one(mode, rule, policy):
    n, seed, pseed, rate, off = 12, 420 + mode, 0xBEEF, 96, 300
    args = _args(mode, n, np.random.default_rng(mode))
    b = oracle.Batch(mode, rule, seed, n, game_offset=off, threads=3, **args)
    games = [_game(mode, rule, seed, off, g, args) for g in range(n)]
    np_ = 3 if mode >= 3 else 4
    rng = np.random.default_rng(99)
    for chunk in CHUNKS:
        b.step(policy, pseed, chunk, call_rate_256=rate)
        for g, o in enumerate(games):
            for _ in range(chunk):
                if o.status()[2]:
                    o.reset()
                    continue
                acts = o.random_actions(pseed, off + g) if policy == "random" else o.greedy_actions(pseed, off + g, rate)
                o.step([int(x) for x in acts])
        st = b.state()
        assert (b.status() == st["status"]).all()
        for g, o in enumerate(games):
            oa, op, od = o.status()
            assert tuple(st["status"][g]) == (oa, op, od), g
            d = diff_dict(normalize_view(st["views"][g]), normalize_view(o.peek()))
            assert not d, (g, d[:10])
            assert int(st["steps"][g]) == o.step_count
            assert [int(x) for x in st["scores"][g][:np_]] == [o.peek().players[p].score for p in range(np_)]
            for s in range(4):
                if (oa >> s) & 1 and not od:
                    assert [int(x) for x in st["legal"][g, s, : st["legal_count"][g, s]]] == o.legal(s), (g, s)
                    assert (st["mask"][g, s] == o.mask(s)).all() and int(st["waits"][g, s]) == o.waits(s), (g, s)
                else:
                    assert st["legal_count"][g, s] == 0 and st["mask"][g, s].sum() == 0 and st["waits"][g, s] == 0
        # encoder rows: every seat of a few games, in a shuffled order with repeats
        gs = np.repeat(rng.choice(n, 5, replace=False), np_)
        ss = np.tile(np.arange(np_), 5)
        perm = rng.permutation(len(gs))
        gs, ss = np.concatenate([gs[perm], gs[:2]]), np.concatenate([ss[perm], ss[:2]])
        ext, base = b.encode_extended(gs, ss), b.encode(gs, ss)
        for i, (g, s) in enumerate(zip(gs, ss)):
            assert np.array_equal(ext[i], games[g].encode_extended(int(s))), (g, s)
            assert np.array_equal(base[i], games[g].encode(int(s), sanma=mode >= 3)), (g, s)
        kawa, yaku = b.aux()
        for g, o in enumerate(games):
            assert np.array_equal(kawa[g], o.encode_kawa_overview()) and np.array_equal(yaku[g], o.encode_yaku_possibility()), g
    whole = oracle.rollout_policy(mode, rule, seed, n, policy, pseed, sum(CHUNKS), call_rate_256=rate, game_offset=off, threads=2, **args)
    st = b.state()
    for k in ("status", "steps", "scores", "legal", "legal_count", "mask", "waits", "digest"):
        assert np.array_equal(st[k], whole[k]), k
    assert bytes(st["views"]) == bytes(whole["views"])


def test_batch_rejects_rows_out_of_range():
    b = oracle.Batch(5, abi.RULE_MJSOUL, 1, 3, threads=2)
    with pytest.raises(IndexError):
        b.encode_extended([0, 3], [0, 0])
    with pytest.raises(IndexError):
        b.encode([0], [3])   # 3P: no seat 3
    assert b.encode_extended([], []).shape == (0, 215, 27)


def test_default_threads_follow_the_job_not_the_machine(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "5")
    assert oracle.default_threads() == 5
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert oracle.default_threads() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    import os

    assert oracle.default_threads() == max(1, min(len(os.sched_getaffinity(0)), 16))
