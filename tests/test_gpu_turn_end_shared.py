"""The end of a turn nobody claimed runs once per call, behind both phase branches (r4_turn_end in csrc/rmj_step4.hip.h): every game
against the oracle on every launch path.

A wave carries four games (a quad: games 4q .. 4q+3).  The turn of one game ends behind a discard nobody can claim, the turn of its
neighbour behind claims that were all passed; both now leave through one copy of "riichi accepted, turn counter and current player
advanced, next tile dealt, first turn over".  What can go wrong is per row and shows in the game's own records: a missing or doubled
tsumo / reach_accepted event, a wrong drawer, an abortive check where the reference has none, an exhaustive draw that pauses or bails
differently.  So every game's status, acting seats' lists, scores and whole MJAI log are compared with oracle.Game playing the same
policy under the same seed - in 4p-red-half and 3p-red-half, with 256 games (64 quads: the smallest batch RMJ_QUEUE_FORCE=1 hands out
as tickets) and with 5 (a full wave and a wave of one row), fused (RMJ_QUEUE_CHUNK=0), as tickets (RMJ_QUEUE_FORCE=1), one launch per
step with the host's actions and with action ids.

The mixed case must have occurred: test_oracle_games_mix_both_turn_ends counts it from the oracle's games alone (see there)."""
import json

import numpy as np
import pytest

from riichienv_amd import abi, vecenv
from riichienv_amd.shard import game_seed

pytestmark = pytest.mark.gpu

SEED, PSEED, RATE = 4242, 0xC0FFEE, 64
MODES = (2, 5)                      # 4p-red-half, 3p-red-half
SIZES = (256, 5)
STEPS = {"random": 300, "greedy": 200, "host": 150}
RING = 16384                        # keeps every record of the longest run (at most a few events per step)

_ORACLE = {}


def _a_type(a):
    return int(a) & 0xFF


def _oracle(mode, n, policy):
    """The batch played by oracle.Game, once per (mode, n, policy) and never changed afterwards.  Per game: the log lines of everything it
    played (auto-reset: a finished game is reset by the step that finds it done), the final status / lists / scores, and per step how the
    turn ended: 'A' a discard that drew no claim, 'B' claims that were all passed, 'C' a discard that drew claims, '.' anything else;
    host policy: the actions of every step as well (no reset: 150 steps do not finish a half game - asserted)."""
    key = (mode, n, policy)
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import oracle

    steps = STEPS[policy]
    games = [oracle.Game(game_mode=mode, seed=game_seed(SEED + mode, g)) for g in range(n)]
    for o in games:
        o.reset()
    lines = [[] for _ in range(n)]
    kinds = [[] for _ in range(n)]
    acts_all = np.full((steps, n, 4), abi.NO_ACTION, dtype=np.uint64)
    for t in range(steps):
        for g, o in enumerate(games):
            oa, op, od = o.status()
            if od:
                assert policy != "host", "a game finished inside the host-driven run"
                lines[g] += o.log()
                o.reset()
                kinds[g].append(".")
                continue
            acts = [int(x) for x in (o.greedy_actions(PSEED, g, RATE) if policy == "greedy" else o.random_actions(PSEED, g))]
            acts_all[t, g] = acts
            given = [_a_type(a) for s, a in enumerate(acts) if (oa >> s) & 1 and a != abi.NO_ACTION]
            o.step(acts)
            ph2 = o.status()[1]
            if op == abi.WAIT_ACT and given == [abi.DISCARD]:
                kinds[g].append("C" if ph2 == abi.WAIT_RESPONSE else "A")
            elif op == abi.WAIT_RESPONSE and given and all(x == abi.PASS for x in given) and json.loads(o.log()[-1])["type"] in ("tsumo", "ryukyoku"):
                kinds[g].append("B")   # (a passed chankan / kita offer ends in the kan's own draw: never after a dahai)
            else:
                kinds[g].append(".")
    final = []
    for g, o in enumerate(games):
        lines[g] += o.log()
        oa, op, od = o.status()
        v = o.peek()
        final.append(dict(status=(oa, op, od), legal={s: o.legal(s) for s in range(4) if (oa >> s) & 1 and not od},
                          scores=[v.players[p].score for p in range(4)]))
    _ORACLE[key] = dict(lines=lines, kinds=kinds, final=final, acts=acts_all)
    return _ORACLE[key]


def _mixed_counts(kinds):
    """(per step, per call): the steps at which one game of a quad ends its turn behind a claim-free discard ('A') while another ends it
    behind an all-pass answer ('B').  Per step: the games side by side as the oracle stepped them - what a launch per step sees.  Per
    call: a fused rollout answers the claims on a discard in the call that made it ('C' and the step after it are one call), so its
    calls run ahead of the steps; the same count over each game's sequence of calls."""
    def calls(k):
        out, i = [], 0
        while i < len(k):
            if k[i] == "C" and i + 1 < len(k):
                out.append(k[i + 1])
                i += 2
            else:
                out.append(k[i])
                i += 1
        return out

    def count(seqs):
        c = 0
        for q in range(0, len(seqs), 4):
            quad = seqs[q:q + 4]
            for t in range(max(len(s) for s in quad)):
                here = {s[t] for s in quad if t < len(s)}
                c += "A" in here and "B" in here
        return c

    return count(kinds), count([calls(k) for k in kinds])


def _exhaustive_draws(lines):
    return sum(1 for ls in lines for x in ls if '"type":"ryukyoku"' in x.replace(" ", "") and "exhaustive" in x.lower())


def _check(env, want, tag):
    n = env.n
    assert not env.events_lost().any()
    act, ph, dn = env.status()
    legal, cnt = env.legal()
    sc = env.scores()
    for g in range(n):
        f = want["final"][g]
        assert (int(act[g]), int(ph[g]), int(dn[g])) == f["status"], (tag, g)
        for s, ol in f["legal"].items():
            assert [int(x) for x in legal[g, s, : cnt[g, s]]] == ol, (tag, g, s)
        assert [int(x) for x in sc[g]] == f["scores"], (tag, g)


def _first_difference(dev, ora, g, tag):
    i = next((i for i, (a, b) in enumerate(zip(dev, ora)) if a != b), min(len(dev), len(ora)))
    return (f"{tag} game {g}: logs part at line {i} of {len(dev)} (device) / {len(ora)} (oracle): device {dev[i] if i < len(dev) else None} "
            f"oracle {ora[i] if i < len(ora) else None}; before it: {ora[max(0, i - 3):i]}")


def _drained(env, roll):
    cur = env.log_positions()[0].copy()
    roll()
    return env.drain_logs(cursor=cur)


@pytest.mark.parametrize("path", ["fused", "tickets"])
@pytest.mark.parametrize("policy", ["random", "greedy"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_fused_rollout_equals_oracle(mode, n, policy, path, monkeypatch):
    """step_random (300 steps) / step_greedy (call rate 64, 200 steps) with auto-reset as ONE fused launch: claims are answered in the
    call of the discard, so a wave's rows leave through both turn-end sites in nearly every call."""
    if path == "tickets":
        monkeypatch.setenv("RMJ_QUEUE_FORCE", "1")
    else:
        monkeypatch.setenv("RMJ_QUEUE_CHUNK", "0")
    want = _oracle(mode, n, policy)
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=SEED + mode, event_ring=RING)
    env.reset()
    if policy == "greedy":
        logs = _drained(env, lambda: env.step_greedy(PSEED, STEPS[policy], auto_reset=True, call_rate_256=RATE))
    else:
        logs = _drained(env, lambda: env.step_random(PSEED, STEPS[policy], auto_reset=True))
    tag = f"mode{mode}-{n}-{policy}-{path}"
    for g in range(n):
        if logs[g] != want["lines"][g]:
            pytest.fail(_first_difference(logs[g], want["lines"][g], g, tag))
    _check(env, want, tag)
    env.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_step_by_host_actions_equals_oracle(mode, n):
    """one launch per step under the caller's packed actions (validated against the stored lists): the WaitAct rows of a wave leave
    through the no-claim site, its WaitResponse rows through the all-pass site"""
    want = _oracle(mode, n, "host")
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=SEED + mode, event_ring=RING)
    env.reset()

    def roll():
        for t in range(STEPS["host"]):
            env.step(want["acts"][t])

    logs = _drained(env, roll)
    tag = f"mode{mode}-{n}-host"
    for g in range(n):
        if logs[g] != want["lines"][g]:
            pytest.fail(_first_difference(logs[g], want["lines"][g], g, tag))
    _check(env, want, tag)
    env.close()


@pytest.mark.parametrize("mode", MODES)
def test_step_by_action_ids_equals_oracle(mode):
    """the id path (Observation.find_action + step): the ids of the oracle's random picks go to the device, and the oracle takes the
    FIRST legal action with that id like find_action does (ids do not tell a red five from a plain one)"""
    torch = pytest.importorskip("torch")
    from oracle import oracle
    from riichienv_amd.torch_env import TorchVecEnv

    n = 64
    enc = oracle.lib().orc_action_encode_3p if mode >= 3 else oracle.lib().orc_action_encode
    games = [oracle.Game(game_mode=mode, seed=game_seed(SEED + mode, g)) for g in range(n)]
    for o in games:
        o.reset()
    env = TorchVecEnv(n, game_mode=mode, seed=SEED + mode, skip_mjai_logging=False, share_stream=True, event_ring=RING)
    for t in range(STEPS["host"]):
        ids = np.full((n, 4), -1, dtype=np.int32)
        for g, o in enumerate(games):
            oa = o.status()[0]
            picks = o.random_actions(PSEED, g)
            acts = [abi.NO_ACTION] * 4
            for s in range(4):
                a = int(picks[s])
                if (oa >> s) & 1 and a != abi.NO_ACTION:
                    ids[g, s] = enc(a)
                    acts[s] = next(x for x in o.legal(s) if enc(x) == ids[g, s])
            o.step(acts)
        env.step(torch.from_numpy(ids).to(env.device), auto_reset=False)
    torch.cuda.synchronize()
    act, ph, dn = env.env.status()
    for g, o in enumerate(games):
        assert (int(act[g]), int(ph[g]), int(dn[g])) == o.status(), g
        assert env.env.mjai_log(g) == o.log(), g


@pytest.mark.parametrize("policy", ["random", "greedy", "host"])
@pytest.mark.parametrize("mode", MODES)
def test_oracle_games_mix_both_turn_ends(mode, policy):
    """From the oracle's 256 games alone (nothing here reads the device): the number of steps / fused calls at which two games of a quad
    end their turns through the two different sites (_mixed_counts), and the exhaustive draws in the logs.  Measured with SEED = 4242
    (mixed quad-steps as stepped, mixed quad-calls of a fused rollout, exhaustive draws):
        4p-red-half: random 4159 / 4134 / 766, greedy 5517 / 5367 / 235, host actions 2103 / 2096 / 256
        3p-red-half: random 2238 / 2219 / 1096, greedy 2782 / 2798 / 260, host actions 1117 / 1103 / 512
    The floors are a quarter of these (MIXED_MEASURED): a batch that stops reaching the mixed case is a gap in what the comparisons prove."""
    want = _oracle(mode, 256, policy)
    per_step, per_call = _mixed_counts(want["kinds"])
    draws = _exhaustive_draws(want["lines"])
    print(f"mode {mode} {policy}: mixed quads per step {per_step}, per call {per_call}, exhaustive draws {draws}")
    floors = [m // 4 for m in MIXED_MEASURED[(mode, policy)]]
    assert min(floors) >= 50
    assert per_step >= floors[0] and per_call >= floors[1] and draws >= floors[2], ((per_step, per_call, draws), floors)


# (mode, policy): (mixed quad-steps as stepped, mixed quad-calls of a fused rollout, exhaustive draws) of the 256 oracle games
MIXED_MEASURED = {(2, "random"): (4159, 4134, 766), (2, "greedy"): (5517, 5367, 235), (2, "host"): (2103, 2096, 256),
                  (5, "random"): (2238, 2219, 1096), (5, "greedy"): (2782, 2798, 260), (5, "host"): (1117, 1103, 512)}
