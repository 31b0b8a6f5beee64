"""oracle.rollout_policy (orc_rollout_policy: a whole batch stepped under a device policy's oracle twin on host threads) pinned on
oracle.Game stepped one game at a time from Python, the way the GPU parity tests step it: status, state, step counts, scores, legal
lists, masks, waits and the digest of every line logged across restarts."""
import numpy as np
import pytest

from riichienv_amd import abi
from riichienv_amd.shard import game_seed
from oracle import oracle
from tests.parity_util import diff_dict, normalize_view


def _reset_args(mode, n, rng):
    """per-game reset arguments: every other game keeps the defaults (-1), the rest get a dealer, round, scores, honba and sticks"""
    np_ = 3 if mode >= 3 else 4
    oya = np.full(n, -1, np.int32)
    rw = np.full(n, -1, np.int32)
    honba = np.full(n, -1, np.int32)
    ky = np.full(n, -1, np.int32)
    start = 35000 if np_ == 3 else 25000
    scores = np.full((n, np_), start, np.int32)
    for g in range(1, n, 2):
        oya[g] = rng.integers(np_)
        rw[g] = rng.integers(2)
        honba[g] = rng.integers(6)
        ky[g] = rng.integers(5)
        s = rng.integers(1, 60, np_) * 1000
        s[0] += start * np_ - s.sum() - 1000 * ky[g]   # any total: the game does not check
        scores[g] = s
    return dict(oya=oya, round_wind=rw, scores=scores, honba=honba, kyotaku=ky)


def _python_rollout(mode, rule, seed, n, policy, pseed, steps, rate, off, args):
    games, digests = [], []
    for g in range(n):
        o = oracle.Game(game_mode=mode, seed=game_seed(seed, off + g), rule_bits=rule)
        if args is None:
            o.reset()
        else:
            o.reset(oya=int(args["oya"][g]), round_wind=int(args["round_wind"][g]), scores=[int(x) for x in args["scores"][g]],
                    honba=int(args["honba"][g]), kyotaku=int(args["kyotaku"][g]))
        lines = []
        for _ in range(steps):
            if o.status()[2]:
                lines += o.log()
                o.reset()
                continue
            acts = o.random_actions(pseed, off + g) if policy == "random" else o.greedy_actions(pseed, off + g, rate)
            o.step([int(x) for x in acts])
        lines += o.log()
        games.append(o)
        digests.append(oracle.log_digest(lines))
    return games, digests


@pytest.mark.parametrize("mode,rule,policy,with_args", [(2, abi.RULE_TENHOU, "greedy", False), (2, abi.RULE_MJSOUL, "greedy", True),
                                                        (1, abi.RULE_TENHOU, "random", True), (5, abi.RULE_MJSOUL, "greedy", True),
                                                        (4, abi.RULE_TENHOU, "random", False), (4, abi.RULE_MJSOUL, "greedy", False)])
def test_rollout_policy_equals_games_stepped_one_by_one(mode, rule, policy, with_args):
    n, seed, pseed, steps, rate, off = 24, 310 + mode, 0xFACE, 400, 96, 1000
    args = _reset_args(mode, n, np.random.default_rng(mode * 7 + with_args)) if with_args else None
    r = oracle.rollout_policy(mode, rule, seed, n, policy, pseed, steps, call_rate_256=rate, game_offset=off, threads=3,
                              **(args or {}))
    games, digests = _python_rollout(mode, rule, seed, n, policy, pseed, steps, rate, off, args)
    restarts = 0
    for g, o in enumerate(games):
        oa, op, od = o.status()
        assert tuple(r["status"][g]) == (oa, op, od), g
        d = diff_dict(normalize_view(r["views"][g]), normalize_view(o.peek()))
        assert not d, (g, d[:10])
        assert int(r["steps"][g]) == o.step_count, g
        v = o.peek()
        assert [int(x) for x in r["scores"][g][: 3 if mode >= 3 else 4]] == [v.players[p].score for p in range(3 if mode >= 3 else 4)], g
        for s in range(4):
            if (oa >> s) & 1 and not od:
                assert [int(x) for x in r["legal"][g, s, : r["legal_count"][g, s]]] == o.legal(s), (g, s)
                assert (r["mask"][g, s] == o.mask(s)).all(), (g, s)
                assert int(r["waits"][g, s]) == o.waits(s), (g, s)
            else:
                assert r["legal_count"][g, s] == 0 and r["mask"][g, s].sum() == 0 and r["waits"][g, s] == 0, (g, s)
        assert int(r["digest"][g]) == digests[g], g
        restarts += int(o.step_count) < steps
    # the digests are of whole logs: games that restarted carry more than their current log
    assert restarts > 0 or any(int(r["digest"][g]) != oracle.log_digest(o.log()) for g, o in enumerate(games))


def test_rollout_policy_walls_and_no_auto_reset():
    """explicit walls deal what they say; without auto-reset a finished game stays finished and its digest is of its one log"""
    mode, rule, n, seed = 2, abi.RULE_TENHOU, 6, 77
    rng = np.random.default_rng(5)
    walls = np.stack([rng.permutation(136) for _ in range(n)]).astype(np.uint8)
    r = oracle.rollout_policy(mode, rule, seed, n, "greedy", 3, 400, auto_reset=False, walls=walls, threads=2)
    for g in range(n):
        o = oracle.Game(game_mode=mode, seed=game_seed(seed, g), rule_bits=rule)
        o.reset(wall=[int(x) for x in walls[g]])
        for _ in range(400):
            if o.status()[2]:
                continue
            o.step([int(x) for x in o.greedy_actions(3, g, 64)])
        assert tuple(r["status"][g]) == o.status()
        assert int(r["digest"][g]) == oracle.log_digest(o.log())
        assert not diff_dict(normalize_view(r["views"][g]), normalize_view(o.peek()))


def test_log_digest():
    """FNV-1a 64 over the lines joined with '\\n'"""
    def ref(text):
        h = 0xCBF29CE484222325
        for b in text.encode():
            h = ((h ^ b) * 0x100000001B3) & (2 ** 64 - 1)
        return h

    assert oracle.log_digest([]) == 0xCBF29CE484222325
    assert oracle.log_digest(["a"]) == 0xAF63DC4C8601EC8C          # published FNV-1a 64 of "a"
    a, b = ['{"type":"start_game"}', '{"type":"end_game"}'], ['{"type":"start_game"}']
    assert oracle.log_digest(a + b) == ref("\n".join(a + b))
    assert oracle.log_digest(a) != oracle.log_digest(["".join(a)])
