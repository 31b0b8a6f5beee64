"""The reference's agari fixtures settled on every step path, against the oracle and against the fixtures' own answers.

Scoring a win runs through e4_calc, but the step kernels build its input themselves: r4_seat_eval (csrc/rmj_step4.hip.h) for the
four-games-per-wave kernels, the fused and ticket rollouts, and seat_calc_impl (csrc/rmj_step.hip.h) for the one-game kernel and the
full path.  tests/test_gpu_hand.py holds only k_eval_hands to the fixtures.  Here each fixture file becomes one batch of game states
(tests/fixture_states.py: every case twice - the second replica moves the dealer and adds honba and riichi sticks - plus one more, so
the batch is no multiple of 4; shuffled, so the rows of a wave hold different hands), each state one discard before its win.  The
discard is a host step on the path's kernel: the offer it opens - the legality form, r4_yaku_check in the four-games-per-wave tier,
with haitei / houtei / ippatsu derived from state - must give the winner the oracle's list and mask, and nobody else an offer.  Then
the path settles the win: state, scores, win_results and MJAI log must equal the oracle's, and han / fu / yaku the fixture's.  The
census of settled yaku ids must equal the fixtures' own, so every yaku id in the files is settled on every path; the full path's
step counts say which tier took each of the two steps."""
import collections

import numpy as np
import pytest

from riichienv_amd import abi, vecenv
from tests import fixture_states as fs
from tests.parity_util import diff_dict, fmt_action, normalize_view, view_bytes

pytestmark = pytest.mark.gpu

# path: (environment switches read at handle creation, how the win is stepped)
PATHS = {
    "one-game": ({"RMJ_STEP4": "0"}, "host"),
    "step4-rows4": ({"RMJ_STEP4": "1", "RMJ_ROWS": "4"}, "host"),
    "step4-rows1": ({"RMJ_STEP4": "1", "RMJ_ROWS": "1"}, "host"),
    "greedy-step": ({"RMJ_ROWS": "4"}, "greedy1"),
    "fused": ({"RMJ_QUEUE_CHUNK": "0", "RMJ_ROWS": "4"}, "rollout"),
    "tickets": ({"RMJ_QUEUE_FORCE": "1", "RMJ_ROWS": "4"}, "rollout"),
}

ROLL_STEPS = 3   # the rollout paths: the win, then steps of finished games (auto_reset=False), which the full path counts
# fixtures whose discard step leaves the four-games-per-wave tier: 4P case 165 is a riichi hand that draws the fourth tile of its
# win type, and the Ankan-after-riichi wait probe is the full path's (R4BAIL 16 in csrc/rmj_step4.hip.h)
DISCARD_LEAVES_ROW_FORM = {"agari_4p.json": {165}, "agari_3p.json": set()}
# full-path steps of the batch's n games in the discard step and in the win step(s), k = the games of the cases above: the one-game
# kernel is the full path; the four-games-per-wave tier makes every other discard and settles every win in row form, and the rollouts
# spend exactly the steps after the win there - so none of the wins left row form
FULL_PATH = {"host": lambda n, k, path: (n, n) if path == "one-game" else (k, 0), "greedy1": lambda n, k, path: (k, 0),
             "rollout": lambda n, k, path: (k, (ROLL_STEPS - 1) * n)}

_BATCH = {}


def _batch(name):
    """the states of one fixture file, shuffled, with the oracle's answers: (cases, states, reset args, before, after)"""
    if name in _BATCH:
        return _BATCH[name]
    from oracle import oracle

    np_ = fs.FILES[name]
    cases = fs.load(name)
    order = [(i, r) for r in range(2) for i in range(len(cases))] + [(0, 0)]
    rng = np.random.default_rng(4242)
    order = [order[k] for k in rng.permutation(len(order))]
    n = len(order)
    assert n % 4
    states = []
    for g, (i, r) in enumerate(order):
        st, _ = fs.build_case(cases[i], np_, **fs.replica(i, r, np_))
        states.append((i, st))
    ulen = 108 if np_ == 3 else 136
    walls = np.zeros((n, ulen), np.uint8)
    oya, rw, honba, ky = (np.zeros(n, np.int32) for _ in range(4))
    scores = np.zeros((n, np_), np.int32)
    before, after = [], []
    for g, (i, st) in enumerate(states):
        u = fs.universe(np_)
        rest = [t for t in u if t not in set(st.wall)]
        walls[g] = list(reversed(st.wall + rest))
        oya[g], rw[g], honba[g], ky[g] = st.oya, st.round_wind, st.honba, st.kyotaku
        scores[g] = st.scores
        o = oracle.Game(game_mode=fs.GAME_MODE[np_], seed=1000 + g, rule_bits=fs.RULE)
        o.reset(wall=[int(x) for x in walls[g]] + [0] * (136 - ulen), oya=int(oya[g]), round_wind=int(rw[g]),
                scores=[int(x) for x in scores[g]], honba=int(honba[g]), kyotaku=int(ky[g]))
        o.poke(st.view)
        o.step({st.pre[0]: st.pre[1]})
        before.append((o.status(), o.legal(st.winner), o.mask(st.winner).copy()))
        o.step({st.winner: st.action})
        after.append((view_bytes(o.peek()), o.win_results(), o.log()))
    args = dict(walls=walls, oya=oya, round_wind=rw, scores=scores, honba=honba, kyotaku=ky)
    _BATCH[name] = (cases, states, args, before, after)
    return _BATCH[name]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(fs.FILES))
def test_fixtures_settle_on_every_path(name, path, monkeypatch):
    env_vars, how = PATHS[path]
    for k in ("RMJ_STEP4", "RMJ_QUEUE_CHUNK", "RMJ_QUEUE_FORCE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    cases, states, args, before, after = _batch(name)
    np_ = fs.FILES[name]
    n = len(states)
    env = vecenv.VecRiichiEnv(n, game_mode=fs.GAME_MODE[np_], seeds=np.arange(1000, 1000 + n, dtype=np.uint64), rule_bits=fs.RULE,
                              reference_rng=False, event_ring=256)
    env.reset(**args)
    for g, (i, st) in enumerate(states):
        env.poke(g, st.view)

    # the discard before the win (a host step on this path's kernel), and the offer it opens: the winner's list and mask, nobody else's
    f0 = env.total_full_path()
    a = np.full((n, 4), abi.NO_ACTION, np.uint64)
    for g, (i, st) in enumerate(states):
        a[g, st.pre[0]] = st.pre[1]
    env.step(a)
    full_pre = env.total_full_path() - f0
    act, ph, dn = env.status()
    legal, cnt = env.legal()
    mask = env.mask()
    for g, (i, st) in enumerate(states):
        so, lo, mo = before[g]
        assert (int(act[g]), int(ph[g]), int(dn[g])) == so and so[0] == 1 << st.winner, (name, path, "case", i, "game", g, "status",
                                                                                         (act[g], ph[g], dn[g]), so)
        lg = [int(x) for x in legal[g, st.winner, : cnt[g, st.winner]]]
        assert lg == lo, (name, path, "case", i, "game", g, "legal", [fmt_action(a) for a in lg], [fmt_action(a) for a in lo])
        assert (mask[g, st.winner] == mo).all(), (name, path, "case", i, "game", g, "mask")

    f0 = env.total_full_path()
    if how == "host":
        a = np.full((n, 4), abi.NO_ACTION, np.uint64)
        for g, (i, st) in enumerate(states):
            a[g, st.winner] = st.action
        env.step(a)
    elif how == "greedy1":
        env.step_greedy(fs.PSEED, 1, auto_reset=False, call_rate_256=fs.CALL_RATE)
    else:
        env.step_greedy(fs.PSEED, ROLL_STEPS, auto_reset=False, call_rate_256=fs.CALL_RATE)
    full = env.total_full_path() - f0

    census, want = collections.Counter(), collections.Counter()
    compared = 0
    for g, (i, st) in enumerate(states):
        vb, wr, log = after[g]
        where = (name, path, "case", i, "game", g)
        v = env.peek(g)
        if view_bytes(v) != vb:
            d = diff_dict(normalize_view(v), normalize_view(abi.StateView.from_buffer_copy(vb)))
            assert not d, (*where, "state", d[:8])
        got = env.win_results(g)
        assert got == wr, (*where, "win_results", got, wr)
        assert env.mjai_log(g) == log, (*where, "log", env.mjai_log(g)[-3:], log[-3:])
        w = got[st.winner]
        if not st.excluded:   # (held to the oracle above either way)
            e = cases[i]["expected"]
            assert (w["is_win"], w["han"], w["fu"], w["yaku"]) == (e["is_win"], e["han"], e["fu"], e["yaku"]), (*where, "fixture", w, e)
            census.update(w["yaku"])
            want.update(e["yaku"])
            compared += 1
    assert not env.events_lost().any()
    row = n - (full - (ROLL_STEPS - 1) * n if how == "rollout" else full)
    print(f"\n{name} {path}: {n} wins, {compared} held to the fixture; full-path steps: discard {full_pre}, win {full}; wins settled "
          f"in row form {row}, in the full path {n - row}; yaku census {dict(sorted(census.items()))}")
    k = sum(1 for i, _ in states if i in DISCARD_LEAVES_ROW_FORM[name])
    assert (full_pre, full) == FULL_PATH[how](n, k, path), (name, path, full_pre, full, n, k)
    assert census == want, (name, path, sorted((census - want).items()), sorted((want - census).items()))
    ids = {y for c in cases for y in c["expected"]["yaku"]}
    assert set(census) == ids
    env.close()
