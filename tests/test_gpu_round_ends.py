"""Every game of a greedy-policy rollout with auto-reset against the oracle, through every kind of round end the row-form code settles.

The fused rollout settles Tsumo and Ron, pays honba and riichi sticks, handles exhaustive draws, deals the next round and restarts
finished games in row form between the passes of a step (r4_round_end, step4_pass2 in csrc/rmj_step4.hip.h) - its own copy of the
rules, apart from the full path's settlement in rmj_step.hip.h.  Here whole batches run under the greedy device policy (it wins,
riichi's and calls: round ends of every shape) on each launch path, and EVERY game is compared with oracle.rollout_policy: status,
state, step counts, scores, the acting seats' legal lists / masks / waits, and a digest of the whole MJAI log every slot wrote (drained
after each chunk, so nothing is lost to the ring).  Part of each batch starts from seeded conditions (honba and sticks on the table,
all-last deals with everyone under the goal, a seat about to bust, tied scores, dealers in every seat) so that the rare settlements
come through the natural fused path.  The census of the compared logs (tests/round_end_census.py) must then reach floors set at
about half of what a measured run of this very test saw (CENSUS_MEASURED): a kind the batch stops reaching is a gap in what the
comparison proves, even when every game still matches."""
import collections
import time

import numpy as np
import pytest

from riichienv_amd import abi, vecenv
from tests import round_end_census
from tests.parity_util import diff_dict, normalize_view

pytestmark = pytest.mark.gpu

PSEED, RATE = 0xC0FFEE, 96
CHUNKS = (300, 1, 399, 7, 250, 243)           # the fused and ticket paths: uneven rollout calls, logs drained after each
STEP_CHUNK = 100                               # the per-step path: n_steps = 1 calls, logs drained every STEP_CHUNK of them
N_STEPS = sum(CHUNKS)
N_GAMES = 2048

# (mode, rule, path): "fused" = one quad per wave (RMJ_QUEUE_CHUNK=0), "tickets" = k_step4_queue (RMJ_QUEUE_FORCE=1), "step" = one
# launch per step
CASES = [(m, r, p) for m, r in ((1, abi.RULE_TENHOU), (1, abi.RULE_MJSOUL), (2, abi.RULE_TENHOU), (2, abi.RULE_MJSOUL),
                                (4, abi.RULE_TENHOU), (5, abi.RULE_MJSOUL)) for p in ("fused", "tickets")]
CASES += [(2, abi.RULE_MJSOUL, "step"), (5, abi.RULE_MJSOUL, "step")]

# kinds with no floor: listed and reported only.  Abortive draws leave the row-form tier for the serial full path (the docstring of
# test_gpu_greedy.py::test_wins_and_round_ends_stay_in_the_four_games_per_wave_tier), and so do robbed kans (chankan); nobody has
# measured pao under this policy; the zero-payment draw at the end of a game is the census' own ambiguity
NO_FLOOR = set(round_end_census.ABORTIVE_KINDS) | {"pao", "chankan", "draw_tenpai_0_or_all"}

# The census of one MI355X run of this test (2 048 games x 1 200 steps; the launch paths of a (mode, rule) play the same games, and their
# censuses were equal), kinds with a floor only.  Kinds left out were never reached and cannot be: a triple Ron under TENHOU (its
# seeded deals draw `sanchaho`) or in 3P, four seats tenpai in 3P, the West round of an East game.
CENSUS_MEASURED = {
    "mode1-tenhou": dict(tsumo_dealer=1155, tsumo_nondealer=3215, ron_single=12672, ron_double=38, win_kyotaku=10546, ron_double_kyotaku=33,
                win_honba=8446, tsumo_nondealer_honba=1584, rinshan=157, haitei=270, houtei=534, draw_tenpai_0=677, draw_tenpai_1=3200,
                draw_tenpai_2=5082, draw_tenpai_3=3645, draw_tenpai_4=939, renchan_win=3563, renchan_tenpai_draw=6814, rotation=15473,
                kyotaku_carried=3539, game_end=4498, bust=391, south_entry=1099, tied_top=54),
    "mode1-mjsoul": dict(tsumo_dealer=1127, tsumo_nondealer=3333, ron_single=12455, ron_double=62, ron_triple=64, win_kyotaku=10404,
                ron_double_kyotaku=44, win_honba=8454, tsumo_nondealer_honba=1627, rinshan=137, haitei=256, houtei=537,
                draw_tenpai_0=585, draw_tenpai_1=3251, draw_tenpai_2=5142, draw_tenpai_3=3689, draw_tenpai_4=957, renchan_win=3639,
                renchan_tenpai_draw=6900, rotation=15365, kyotaku_carried=3312, game_end=4495, bust=396, south_entry=1077, tied_top=49),
    "mode2-tenhou": dict(tsumo_dealer=1183, tsumo_nondealer=3288, ron_single=12708, ron_double=64, win_kyotaku=10645, ron_double_kyotaku=53,
                win_honba=9156, tsumo_nondealer_honba=1743, rinshan=147, haitei=277, houtei=531, draw_tenpai_0=719, draw_tenpai_1=3169,
                draw_tenpai_2=5098, draw_tenpai_3=3572, draw_tenpai_4=974, renchan_win=4236, renchan_tenpai_draw=6824, rotation=17160,
                kyotaku_carried=3599, game_end=2100, bust=527, south_entry=2517, west_entry=352, tied_top=44),
    "mode2-mjsoul": dict(tsumo_dealer=1270, tsumo_nondealer=3270, ron_single=12520, ron_double=70, ron_triple=64, win_kyotaku=10473,
                ron_double_kyotaku=57, win_honba=9191, tsumo_nondealer_honba=1747, rinshan=156, haitei=271, houtei=528,
                draw_tenpai_0=702, draw_tenpai_1=3118, draw_tenpai_2=5132, draw_tenpai_3=3655, draw_tenpai_4=977, renchan_win=4170,
                renchan_tenpai_draw=6976, rotation=17059, kyotaku_carried=3496, game_end=2032, bust=606, south_entry=2533,
                west_entry=336, tied_top=37),
    "mode4-tenhou": dict(tsumo_dealer=4361, tsumo_nondealer=8515, ron_single=23731, ron_double=172, win_kyotaku=30879, ron_double_kyotaku=167,
                win_honba=15482, tsumo_nondealer_honba=3539, rinshan=887, haitei=396, houtei=556, draw_tenpai_0=975, draw_tenpai_1=4430,
                draw_tenpai_2=5595, draw_tenpai_3=2251, renchan_win=9776, renchan_tenpai_draw=7091, rotation=22433,
                kyotaku_carried=7002, game_end=10276, bust=835, south_entry=1255, tied_top=33),
    "mode5-mjsoul": dict(tsumo_dealer=4493, tsumo_nondealer=8426, ron_single=23294, ron_double=143, win_kyotaku=30618, ron_double_kyotaku=133,
                win_honba=17112, tsumo_nondealer_honba=3999, rinshan=915, haitei=395, houtei=488, draw_tenpai_0=1056,
                draw_tenpai_1=4646, draw_tenpai_2=5695, draw_tenpai_3=2312, renchan_win=11152, renchan_tenpai_draw=7586, rotation=25813,
                kyotaku_carried=7619, game_end=4276, bust=1422, south_entry=5288, west_entry=348, tied_top=18),
}
FLOORS = {key: {k: v // 2 for k, v in c.items()} for key, c in CENSUS_MEASURED.items()}   # about half of what was observed


def _case_id(mode, rule, path):
    return f"mode{mode}-{'mjsoul' if rule == abi.RULE_MJSOUL else 'tenhou'}-{path}"


def _seeded_conditions(mode, n):
    """reset arguments of the first deal, per game (the oracle gets the same): a fifth of the batch each keeps the defaults, has honba
    1-5 and sticks 1-4 on the table, starts the last regular round with every seat under the goal (extensions), has one seat at
    1 000 points or less (busts), or starts from tied scores; dealers in every seat throughout.  In 4P every 32nd game is dealt from
    _triple_ron_wall instead (walls: a row that starts with 255 shuffles its own)"""
    np_ = 3 if mode >= 3 else 4
    start, goal = (35000, 40000) if np_ == 3 else (25000, 30000)
    last_wind = 0 if mode in (1, 4) else 1
    rng = np.random.default_rng(1000 + mode)
    oya = np.arange(n, dtype=np.int32) % np_
    rw = np.zeros(n, np.int32)
    honba = np.zeros(n, np.int32)
    ky = np.zeros(n, np.int32)
    scores = np.full((n, np_), start, np.int32)
    for g in range(n):
        kind = g % 5
        if kind == 1:
            honba[g], ky[g] = rng.integers(1, 6), rng.integers(1, 5)
        elif kind == 2:
            rw[g], oya[g] = last_wind, np_ - 1
            scores[g] = rng.integers(start // 1000 - 8, goal // 1000, np_) * 1000
            ky[g] = rng.integers(0, 3)
        elif kind == 3:
            scores[g] = start
            scores[g, g % np_] = int(rng.choice([0, 500, 1000]))
            scores[g, (g + 1) % np_] += start - scores[g, g % np_]
            rw[g] = rng.integers(0, last_wind + 1)
        elif kind == 4:
            top = goal + 2000
            scores[g] = (start * np_ - 2 * top) // (np_ - 2) // 100 * 100
            scores[g, :2] = top
            if g % 2:
                rw[g], oya[g] = last_wind, np_ - 1
    args = dict(oya=oya, round_wind=rw, scores=scores, honba=honba, kyotaku=ky)
    if np_ == 4:   # every 32nd game of a 4P batch: three seats wait on the tile the dealer discards first (MJSOUL: a triple Ron)
        walls = np.full((n, 136), 255, np.uint8)
        for g in range(0, n, 32):
            walls[g] = _triple_ron_wall(rng)
            oya[g], rw[g], honba[g], ky[g] = 0, 0, g % 3, g % 2
            scores[g] = start
        args["walls"] = walls
    return args


def _triple_ron_wall(rng):
    """A wall (draw order) that deals, with the dealer in seat 0: the dealer 123456789m 22s 78s and a 5p to draw - riichi, and 5p is the
    one discard that keeps tenpai; seats 1-3 123456789m with EE 34p, SS 67p, WW 46p - each waits on 5p with ittsu.  The greedy policy
    declares riichi, discards the 5p and every other seat takes it.  Deal (GameState::_initialize_round): seat p's hand is wall blocks
    [16k + 4p, 16k + 4p + 4) for k < 3 and entry 48 + p; the dealer draws entry 52."""
    hands = [list(range(9)) + [19, 19, 24, 25], list(range(9)) + [27, 27, 11, 12], list(range(9)) + [28, 28, 14, 15],
             list(range(9)) + [29, 29, 12, 14]]
    used = collections.Counter()

    def tile(t):
        used[t] += 1
        return t * 4 + used[t] - 1

    ids = [[tile(t) for t in h] for h in hands]
    draw = tile(13)
    rest = [t for t in range(136) if t not in {x for h in ids for x in h} | {draw}]
    rng.shuffle(rest)
    w = [0] * 136
    for p in range(4):
        for k in range(3):
            w[16 * k + 4 * p: 16 * k + 4 * p + 4] = ids[p][4 * k: 4 * k + 4]
        w[48 + p] = ids[p][12]
    w[52] = draw
    w[53:] = rest
    return np.array(w, np.uint8)


_ORACLE = {}


def _oracle(mode, rule, seed, off, args):
    """oracle.rollout_policy of the batch - shared by the launch paths of one (mode, rule)"""
    from oracle import oracle

    key = (mode, rule, seed, off)
    if key not in _ORACLE:
        t0 = time.time()
        _ORACLE[key] = oracle.rollout_policy(mode, rule, seed, N_GAMES, "greedy", PSEED, N_STEPS, call_rate_256=RATE, game_offset=off, **args)
        print(f"oracle: {N_GAMES} games x {N_STEPS} steps in {time.time() - t0:.1f} s")
    return _ORACLE[key]


def _first_difference(mode, rule, seed, off, g, args, dev_lines):
    """the oracle replayed for one game, one step at a time: where its log and the device's part"""
    from oracle import oracle
    from riichienv_amd.shard import game_seed

    o = oracle.Game(game_mode=mode, seed=game_seed(seed, off + g), rule_bits=rule)
    wall = args["walls"][g] if "walls" in args and args["walls"][g][0] != 255 else None
    o.reset(wall=None if wall is None else [int(x) for x in wall], oya=int(args["oya"][g]), round_wind=int(args["round_wind"][g]),
            scores=[int(x) for x in args["scores"][g]], honba=int(args["honba"][g]), kyotaku=int(args["kyotaku"][g]))
    lines = []
    for _ in range(N_STEPS):
        if o.status()[2]:
            lines += o.log()
            o.reset()
            continue
        o.step([int(x) for x in o.greedy_actions(PSEED, off + g, RATE)])
    lines += o.log()
    i = next((i for i, (a, b) in enumerate(zip(dev_lines, lines)) if a != b), min(len(dev_lines), len(lines)))
    return (f"game {g}: first difference at line {i} of {len(dev_lines)} (device) / {len(lines)} (oracle): "
            f"device {dev_lines[i] if i < len(dev_lines) else None} oracle {lines[i] if i < len(lines) else None}; "
            f"before it: {lines[max(0, i - 3):i]}")


def _roll(env, path):
    """the rollout on one launch path; returns every slot's drained log lines"""
    cur = env.log_positions()[0].copy()
    logs = [[] for _ in range(env.n)]

    def drain():
        for g, lines in enumerate(env.drain_logs(cursor=cur)):
            logs[g] += lines

    if path == "step":
        for k in range(N_STEPS):
            env.step_greedy(PSEED, 1, auto_reset=True, call_rate_256=RATE)
            if (k + 1) % STEP_CHUNK == 0:
                drain()
    else:
        for chunk in CHUNKS:
            env.step_greedy(PSEED, chunk, auto_reset=True, call_rate_256=RATE)
            drain()
    drain()
    assert not env.events_lost().any()
    return logs


@pytest.mark.parametrize("mode,rule,path", CASES, ids=[_case_id(*c) for c in CASES])
def test_greedy_rollout_round_ends_equal_oracle(mode, rule, path, monkeypatch):
    from oracle import oracle

    if path == "tickets":
        monkeypatch.setenv("RMJ_QUEUE_FORCE", "1")
    elif path == "fused":
        monkeypatch.setenv("RMJ_QUEUE_CHUNK", "0")
    n, seed, off = N_GAMES, 7300 + 10 * mode + (rule == abi.RULE_MJSOUL), 5 * N_GAMES
    args = _seeded_conditions(mode, n)
    t0 = time.time()
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, rule_bits=rule, event_ring=8192, game_offset=off)
    reset = {k: v for k, v in args.items() if k != "walls"}
    if "walls" in args:   # the games with a wall of their own are reset apart from those that shuffle theirs
        own = args["walls"][:, 0] != 255
        env.reset(select=~own, **reset)
        env.reset(select=own, walls=args["walls"], **reset)
    else:
        env.reset(**reset)
    s0, f0 = env.total_steps(), env.total_full_path()
    logs = _roll(env, path)
    steps, full = env.total_steps() - s0, env.total_full_path() - f0
    t_dev = time.time() - t0
    want = _oracle(mode, rule, seed, off, args)

    # the logs first: a wrong settlement shows there with its round, and the report names the first line that differs
    for g in range(n):
        if oracle.text_digest("\n".join(logs[g]).encode()) != int(want["digest"][g]):
            pytest.fail(_first_difference(mode, rule, seed, off, g, args, logs[g]))
    act, ph, dn = env.status()
    assert (act == want["status"][:, 0]).all() and (ph == want["status"][:, 1]).all() and (dn == want["status"][:, 2]).all(), \
        np.nonzero((act != want["status"][:, 0]) | (ph != want["status"][:, 1]) | (dn != want["status"][:, 2]))[0][:10]
    assert (env.step_counts() == want["steps"]).all()
    np_ = 3 if mode >= 3 else 4
    bad = np.nonzero((env.scores()[:, :np_] != want["scores"][:, :np_]).any(axis=1))[0]
    assert not len(bad), [(int(g), env.scores()[g].tolist(), want["scores"][g].tolist()) for g in bad[:5]]
    for g in range(n):
        v = env.peek(g)
        if bytes(v) != bytes(want["views"][g]):
            d = diff_dict(normalize_view(v), normalize_view(want["views"][g]))
            assert not d, (g, d[:10])
    legal, cnt = env.legal()
    acting = (((act[:, None] >> np.arange(4)) & 1) == 1) & (dn[:, None] == 0)
    assert (np.where(acting, cnt, 0) == want["legal_count"]).all() and (cnt[~acting] == 0).all()
    used = np.arange(abi.MAX_LEGAL)[None, None, :] < want["legal_count"][:, :, None]
    assert (np.where(used, legal, 0) == want["legal"]).all()
    assert (env.mask()[acting] == want["mask"][acting]).all() and (env.mask()[~acting] == 0).all()
    assert (env.waits()[acting] == want["waits"][acting]).all()

    # the full path's share of the game-steps: the bound of the four-games-per-wave tier test, so the round ends counted went through
    # row form
    bound = 0.001 if mode < 3 else 0.004
    assert steps >= n * N_STEPS * 0.9 and full / steps < bound, (steps, full)

    notes = collections.Counter()
    c = round_end_census.census(logs, notes)
    cid = _case_id(mode, rule, path)
    print(f"\n{cid}: device {t_dev:.1f} s, {steps} game-steps, full path {full} ({full / steps:.2e}); census: "
          f"{round_end_census.format_census(c)}; notes {dict(notes)}")
    assert not notes["context count mismatch"]
    floors = FLOORS[cid.rsplit("-", 1)[0]]
    assert all(floors[k] >= 1 for k in floors)
    low = {k: (c[k], f) for k, f in floors.items() if c[k] < f}
    assert not low, ("census below its floors (kind: (count, floor))", low)
    env.close()
