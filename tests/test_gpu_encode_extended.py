"""Observation.encode_extended (k_encode_ext: encode_ext_scalars / encode_ext_melds in csrc/rmj_encode.hip.h) held to the oracle on whole
batches, on every path that leaves the legal lists and the state behind in its own way, under the greedy device policy (it riichis,
calls, kans and wins):

  * "step":    one rmj_step_greedy launch per step; after every step the rows of EVERY acting seat of every game, written by the kernel
               with only_active = 1 (other rows zeroed, and checked to be all zero);
  * "fused" / "tickets": uneven rollout chunks (RMJ_QUEUE_CHUNK=0 / RMJ_QUEUE_FORCE=1, as tests/test_gpu_round_ends.py); after each
               chunk ALL seats of all games through the host-copy entry point (only_active = 0), with encode_kawa_overview,
               encode_yaku_possibility and encode_furiten_ron_possibility of every game;
  * "torch":   TorchVecEnv(extended=True).obs(only_active=True) (only_active = 2) after each chunk: acting rows equal the oracle, the
               other rows keep the sentinel the buffer was filled with, bit for bit.  These games start from the default deals of
               TorchVecEnv's constructor (a second reset would move them to their next episode seeds).

The oracle side is oracle.Batch (the same games on host threads).  Outside "torch", every 16th game starts from a wall of its own: the dealer is dealt
nine terminal / honor types (Kyushu), a closed quad (Ankan) or a complete hand (Tsumo and shanten -1), so those channels are reached on
purpose.  A census counts, per channel 74..214, the compared rows in which it is nonzero; each must reach its floor, set at half of
what this very test measured (CENSUS_MEASURED): a channel the batch stops reaching is a gap in what the comparison proves.  Channels
that are constant by construction are asserted constant instead (constant_channels)."""
import collections
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from riichienv_amd import abi, vecenv

pytestmark = pytest.mark.gpu

PSEED, RATE = 0xE7C0DE, 96
N_GAMES, N_BIG = 2047, 4097                # not multiples of 4; the 4097-game case is the fused path of mode 2
STEP_STEPS = 200                           # "step": compared after every one of these steps
CHUNKS = (1, 83, 7, 150, 59)               # "fused", "tickets", "torch": uneven rollout calls (300 steps)
OFFSET = 3 * N_GAMES + 5                   # nonzero game_offset: the policy and the episode seeds use global indices

MODES = [(2, abi.RULE_TENHOU), (1, abi.RULE_MJSOUL), (4, abi.RULE_TENHOU), (5, abi.RULE_MJSOUL)]
CASES = [(m, r, p) for m, r in MODES for p in ("step", "fused", "tickets")] + [(2, abi.RULE_TENHOU, "torch"), (5, abi.RULE_MJSOUL, "torch")]


def _case_id(mode, rule, path):
    return f"mode{mode}-{'mjsoul' if rule == abi.RULE_MJSOUL else 'tenhou'}-{path}"


def _n_games(mode, path):
    return N_BIG if (mode, path) == (2, "fused") else N_GAMES


# ---- channels constant by construction (asserted constant, no floor)
# 194 / 195: the pass context reads last_discard's first member, the seat number (0..3), as a tile id: type 0 (and in 3P column 0),
#            never an aka id - always 0.  (196, "is dora", does vary: tile ids 0..3 are 1m.)
# 206..214: riichi_sutehais is never set on a reachable path - always 0.
# 181:      a chi's consume tiles come out of the legal-action generator in ascending order (t0 < t1), so the "diff 1 with t0 > t1"
#           channel is never set - always 0.
# 3P:       the channels of a fourth seat (77 decay, 90..93 efficiency, 97 ankan, 158..177 fuuro, 203..205 third opponent's tedashi)
#           and the chi channels 179..181 - always 0.
_CONST_ALL = [181, 194, 195] + list(range(206, 215))
_CONST_3P = [77, 90, 91, 92, 93, 97] + list(range(158, 178)) + [179, 180, 203, 204, 205]


def constant_channels(mode):
    return sorted(set(_CONST_ALL) | (set(_CONST_3P) if mode >= 3 else set()))


# ---- seeded deals
def _deal_wall(hands, draws, sanma, rng):
    """A wall (draw order) that deals hands[p] (34-types, 13 each) to the seat p places after the dealer and then draws `draws` in turn
    (GameState::_initialize_round: player idx gets wall blocks [4 NP k + 4 idx, + 4) for k < 3 and entry 12 NP + idx; the draws
    follow from entry 13 NP).  The rest is shuffled."""
    np_ = len(hands)
    pool = collections.defaultdict(list)
    for t in range(136):
        if not sanma or not 1 <= t // 4 <= 7:
            pool[t // 4].append(t)
    ids = [[pool[t].pop() for t in h] for h in hands]
    dr = [pool[t].pop() for t in draws]
    rest = [t for ts in pool.values() for t in ts]
    rng.shuffle(rest)
    w = [0] * (108 if sanma else 136)
    for p in range(np_):
        for k in range(3):
            w[4 * np_ * k + 4 * p: 4 * np_ * k + 4 * p + 4] = ids[p][4 * k: 4 * k + 4]
        w[12 * np_ + p] = ids[p][12]
    w[13 * np_: 13 * np_ + len(dr)] = dr
    w[13 * np_ + len(dr):] = rest
    out = np.full(136, 255, np.uint8)
    out[: len(w)] = w
    return out


def _seed_kinds(sanma):
    """(name, dealer's 13 types, first draw): Kyushu (nine terminal / honor types), Ankan (four East), a complete hand (Tsumo)"""
    if sanma:
        return [("kyushu", [0, 8, 9, 17, 18, 26, 27, 28, 29, 10, 11, 12, 13], 14),
                ("ankan", [27, 27, 27, 27, 9, 10, 11, 12, 13, 14, 24, 25, 26], 30),
                ("tsumo", [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22], 22)]
    return [("kyushu", [0, 8, 9, 17, 18, 27, 28, 29, 30, 10, 11, 12, 13], 14),
            ("ankan", [27, 27, 27, 27, 0, 1, 2, 12, 13, 14, 24, 25, 26], 30),
            ("tsumo", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13], 13)]


def seeded_conditions(mode, n):
    """reset arguments per game (the oracle gets the same): dealers in every seat; every 16th game is dealt one of the seeded walls
    with the dealer in seat 0 (a row that starts with 255 shuffles its own)"""
    sanma = mode >= 3
    np_ = 3 if sanma else 4
    rng = np.random.default_rng(4400 + mode)
    oya = (np.arange(n, dtype=np.int32) % np_).astype(np.int32)
    walls = np.full((n, 136), 255, np.uint8)
    kinds = _seed_kinds(sanma)
    free = [t for t in range(34) if not sanma or not 1 <= t <= 7]
    for i, g in enumerate(range(0, n, 16)):
        _, dealer, draw = kinds[i % len(kinds)]
        # the other seats: random hands from what the dealer's tiles leave
        left = collections.Counter({t: 4 for t in free})
        left.subtract(dealer + [draw])
        bag = [t for t, c in left.items() for _ in range(c)]
        rng.shuffle(bag)
        hands = [dealer] + [sorted(bag[13 * k: 13 * k + 13]) for k in range(np_ - 1)]
        walls[g] = _deal_wall(hands, [draw], sanma, rng)
        oya[g] = 0
    return dict(oya=oya, walls=walls)


def _conditions(mode, path, n):
    return None if path == "torch" else seeded_conditions(mode, n)


# ---- census
def census_add(counts, ext):
    """counts[ch - 74] += rows of ext [m, 215, W] in which channel ch is nonzero"""
    if len(ext):
        counts += (ext[:, 74:, :] != 0).any(axis=2).sum(axis=0)


def check_constant(mode, ext, where):
    for ch in constant_channels(mode):
        bad = np.nonzero((ext[:, ch, :] != 0).any(axis=1))[0]
        assert not len(bad), (f"{where}: channel {ch} is constant 0 by construction, nonzero in {len(bad)} rows")


def _first_difference(dev, want, games, seats, where):
    """game, seat and the first differing (channel, column) with both values, for every differing row (the first few)"""
    bad = np.nonzero((dev.reshape(len(dev), -1).view(np.uint32) != want.reshape(len(want), -1).view(np.uint32)).any(axis=1))[0]
    out = []
    for i in bad[:4]:
        ch, col = np.argwhere(dev[i].view(np.uint32) != want[i].view(np.uint32))[0]
        out.append(f"game {int(games[i])} seat {int(seats[i])} channel {ch} column {col}: device {dev[i, ch, col]!r} "
                   f"oracle {want[i, ch, col]!r}")
    return f"{where}: {len(bad)} rows differ; " + "; ".join(out)


def _acting(status, np_):
    act, dn = status[:, 0].astype(np.int64), status[:, 2]
    a = (((act[:, None] >> np.arange(4)) & 1) == 1) & (dn[:, None] == 0)
    a[:, np_:] = False
    return a


def oracle_rollout(mode, rule, path, n, seed, args, on_compare):
    """the oracle's side of one case: steps oracle.Batch as the device path steps and calls on_compare(k, status, games, seats, ext,
    batch) at every comparison point - the acting rows on "step" / "torch", every seat of every game on "fused" / "tickets"."""
    from oracle import oracle

    b = oracle.Batch(mode, rule, seed, n, game_offset=OFFSET, **(args or {}))
    np_ = 3 if mode >= 3 else 4
    chunks = (1,) * STEP_STEPS if path == "step" else CHUNKS
    for k, c in enumerate(chunks):
        b.step("greedy", PSEED, c, call_rate_256=RATE)
        st = b.status()
        if path in ("step", "torch"):
            games, seats = np.nonzero(_acting(st, np_))
        else:
            games, seats = np.repeat(np.arange(n), np_), np.tile(np.arange(np_), n)
        on_compare(k, st, games, seats, b.encode_extended(games, seats), b)


def measure_census(mode, rule, path):
    """the census of one case, from the oracle alone (how CENSUS_MEASURED was taken)"""
    n = _n_games(mode, path)
    counts = np.zeros(141, np.int64)
    rows = [0]

    def on_compare(k, st, games, seats, ext, b):
        census_add(counts, ext)
        rows[0] += len(ext)

    oracle_rollout(mode, rule, path, n, 8100 + 10 * mode + (rule == abi.RULE_MJSOUL), _conditions(mode, path, n), on_compare)
    return rows[0], counts


# Measured with measure_census (the oracle's trajectories, which the device equals when this test passes): compared rows and, per channel
# 74..214, the rows in which it is nonzero (tests/golden/encode_extended_census.json).  The floors are half of each count; the channels
# of constant_channels have none.  Counts of 0 outside them are fourth-meld slots that some cases never fill (floor 0: reported only).
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_extended_census.json")) as _f:
    CENSUS_MEASURED = json.load(_f)["cases"]
FLOORS = {cid: [0 if 74 + i in constant_channels(int(cid[4])) else c // 2 for i, c in enumerate(m["nonzero_rows"])]
          for cid, m in CENSUS_MEASURED.items()}


def _census_report(counts):
    groups = [("74-77 decay", 74, 78), ("78-93 efficiency", 78, 94), ("94-97 ankan", 94, 98), ("98-177 fuuro", 98, 178),
              ("178 riichi", 178, 179), ("179-181 chi", 179, 182), ("182 pon", 182, 183), ("183 daiminkan", 183, 184), ("184 ankan", 184, 185),
              ("185 kakan", 185, 186), ("186 tsumo/ron", 186, 187), ("187 kyushu", 187, 188), ("188 pass", 188, 189),
              ("189-191 candidates", 189, 192), ("192 complete", 192, 193), ("193 riichi decl", 193, 194), ("194-196 pass ctx", 194, 197),
              ("197-205 tedashi", 197, 206)]
    return ", ".join(f"{name} {int(counts[a - 74:b - 74].max())}" for name, a, b in groups)


def _device_env(mode, rule, path, n, seed, args, monkeypatch):
    if path == "tickets":
        monkeypatch.setenv("RMJ_QUEUE_FORCE", "1")
    elif path == "fused":
        monkeypatch.setenv("RMJ_QUEUE_CHUNK", "0")
    if path == "torch":
        from riichienv_amd.torch_env import TorchVecEnv

        tenv = TorchVecEnv(n, game_mode=mode, seed=seed, extended=True, rule_bits=rule, game_offset=OFFSET)
        return tenv.env, tenv   # (reset by the constructor)
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, rule_bits=rule, game_offset=OFFSET, skip_mjai_logging=True)
    own = args["walls"][:, 0] != 255
    env.reset(select=~own, oya=args["oya"])
    env.reset(select=own, walls=args["walls"], oya=args["oya"])
    return env, None


@pytest.mark.parametrize("mode,rule,path", CASES, ids=[_case_id(*c) for c in CASES])
def test_encode_extended_equals_oracle_on_every_game(mode, rule, path, monkeypatch):
    import torch

    n, seed = _n_games(mode, path), 8100 + 10 * mode + (rule == abi.RULE_MJSOUL)
    sanma = mode >= 3
    np_, w = (3, 27) if sanma else (4, 34)
    args = _conditions(mode, path, n)
    env, tenv = _device_env(mode, rule, path, n, seed, args, monkeypatch)
    dev = torch.device("cuda", 0)
    buf = torch.empty((n, 4, 215, w), dtype=torch.float32, device=dev) if path == "step" else None
    sentinel = np.float32(-7.25)
    counts = np.zeros(141, np.int64)
    t = collections.Counter()
    rows = [0]

    def on_compare(k, st, games, seats, want, b):
        t0 = time.time()
        where = f"{_case_id(mode, rule, path)} compare {k} (step {env.step_counts().max()})"
        env.step_greedy(PSEED, 1 if path == "step" else CHUNKS[k], auto_reset=True, call_rate_256=RATE)
        act, ph, dn = env.status()
        assert (act == st[:, 0]).all() and (ph == st[:, 1]).all() and (dn == st[:, 2]).all(), \
            (where, "status", np.nonzero((act != st[:, 0]) | (ph != st[:, 1]) | (dn != st[:, 2]))[0][:8])
        acting = _acting(st, np_)
        if path == "step":
            buf.fill_(sentinel)
            torch.cuda.synchronize()        # (the library's own stream does not wait for torch's)
            vecenv._chk(env.L.rmj_encode_extended_device(env.h, 1, C.c_void_p(buf.data_ptr())))
            env.sync()
            a = torch.as_tensor(acting, device=dev)
            got = buf[torch.as_tensor(games, device=dev), torch.as_tensor(seats, device=dev)].cpu().numpy()
            rest = buf[~a]
            nz = int((rest != 0).flatten(1).any(dim=1).sum())
            assert nz == 0, (where, f"{nz} rows of seats that do not act are not zero (only_active = 1)")
        elif path == "torch":
            tenv._obs_buf.fill_(sentinel)   # (the library issues on torch's stream: ordered after the fill)
            o = tenv.obs(only_active=True)
            tenv.torch.cuda.synchronize()
            a = torch.as_tensor(acting, device=dev)
            got = o[torch.as_tensor(games, device=dev), torch.as_tensor(seats, device=dev)].cpu().numpy()
            rest = o[~a].view(torch.int32)
            bad = int((rest != int(sentinel.view(np.int32))).flatten(1).any(dim=1).sum())
            assert bad == 0, (where, f"{bad} rows of seats that do not act were written (only_active = 2)")
        else:
            full = env.encode_extended(only_active=False)
            got = full[games, seats]
            assert not full[:, np_:].any(), (where, "rows of absent seats are not zero")
            kawa, yaku = b.aux()
            dk, dy = env.encode_kawa_overview(), env.encode_yaku_possibility()
            for name, d, o_ in (("kawa_overview", dk, kawa), ("yaku_possibility", dy, yaku)):
                bad = np.nonzero((d.reshape(n, -1) != o_.reshape(n, -1)).any(axis=1))[0]
                assert not len(bad), (where, name, [(int(g), np.argwhere(d[g] != o_[g])[0].tolist()) for g in bad[:4]])
            fr = env.encode_furiten_ron_possibility()
            assert (fr == 1.0).all(), (where, "furiten_ron is not all ones")
        t["device"] += time.time() - t0
        if got.view(np.uint32).tobytes() != want.view(np.uint32).tobytes():
            pytest.fail(_first_difference(got, want, games, seats, where))
        check_constant(mode, want, where)
        census_add(counts, want)
        rows[0] += len(want)

    t0 = time.time()
    oracle_rollout(mode, rule, path, n, seed, args, on_compare)
    total = time.time() - t0
    cid = _case_id(mode, rule, path)
    print(f"\n{cid}: {n} games, {rows[0]} rows compared in {total:.1f} s (device and compare {t['device']:.1f} s, oracle "
          f"{total - t['device']:.1f} s); census: {_census_report(counts)}")
    print(f"census {cid}: rows={rows[0]} counts={counts.tolist()}")
    assert rows[0] == CENSUS_MEASURED[cid]["rows"], (rows[0], CENSUS_MEASURED[cid]["rows"])
    low = {74 + i: (int(counts[i]), f) for i, f in enumerate(FLOORS[cid]) if counts[i] < f}
    assert not low, ("census below its floors (channel: (count, floor))", low)
    env.close()
