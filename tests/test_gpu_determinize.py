"""rmj_determinize_device on the GPU: the re-deal against the restatement of tests/determinize_ref.py, what must not change, the
published outputs against a poke of the same view and against the oracle's future, held hands, status codes, WorldSet and the example.
Every test works on a copy of one batch per mode: 64 games after 120 steps of the device policy that plays to win and calls often."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from riichienv_amd import abi
from riichienv_amd.shard import game_seed
from tests import determinize_ref as ref
from tests.parity_util import diff_dict, fmt_action, normalize_view, view_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, SEED, RING = 64, 120, 4242, 4096
MODES = [2, 5]


@functools.lru_cache(maxsize=None)
def _base(mode):
    """(the batch - never stepped or determinized again -, its rows: one acting (game * 4 + seat) per game, its views)"""
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(N, game_mode=mode, seed=SEED, event_ring=RING)
    env.reset()
    env.step_greedy(5, STEPS, auto_reset=False, call_rate_256=128)
    idx = env.legal_compact()[0].astype(np.int32)
    rows = np.array([idx[idx >> 2 == g][0] for g in sorted(set((idx >> 2).tolist()))], np.int32)
    views = {int(i) >> 2: env.peek(int(i) >> 2) for i in rows}
    return env, rows, views


def _np(mode):
    return 3 if mode >= 3 else 4


def _norm(v, response_mask=True):
    d = normalize_view(v)
    d.pop("wall_seed", None)
    d.pop("hand_index", None)
    if not response_mask and d["phase"] == abi.WAIT_RESPONSE:
        d.pop("active_mask")
    return d


def _outputs(env):
    legal, cnt = env.legal()
    return legal, cnt, env.mask(), env.waits(), env.status()


def _game_outputs(env, g):
    legal, cnt, mask, waits, status = _outputs(env)
    return [x[g].tobytes() for x in (legal, cnt, mask, waits) + tuple(status)]


def _seat_outputs(o, g, s):
    legal, cnt, mask, waits, status = o
    return [int(x) for x in legal[g, s, : cnt[g, s]]], mask[g, s].tobytes(), int(waits[g, s])


@pytest.mark.parametrize("mode", MODES)
def test_redeal_equals_the_restatement(mode):
    base, rows, views = _base(mode)
    w = base.clone()
    st = w.determinize(rows, 77)
    census = {"response": 0, "melds": 0, "riichi": 0, "kan": 0, "moved": 0}
    for i, st_i in zip(rows.tolist(), st.tolist()):
        g, a = i >> 2, i & 3
        assert st_i & 15 == abi.DET_OK, (g, a, st_i)
        before, after = views[g], w.peek(g)
        want = ref.determinize_view(before, a, _np(mode), 77, g)
        d = diff_dict(_norm(after, False), _norm(want, False))
        assert not d, (g, a, d[:6])
        if before.phase == abi.WAIT_RESPONSE:   # the viewpoint seat stays, the discarder never answers
            assert (after.active_mask >> a) & 1 and not (after.active_mask >> before.last_discard_pid) & 1, (g, a, after.active_mask)
        census["response"] += before.phase == abi.WAIT_RESPONSE
        census["melds"] += any(p.n_melds for p in before.players)
        census["riichi"] += any(p.riichi_declared for p in before.players)
        census["kan"] += before.rinshan_draw_count > 0
        census["moved"] += view_bytes(before) != view_bytes(after)
    print("census", mode, census)
    assert census["moved"] == len(rows) and census["melds"] > 0 and census["riichi"] > 0
    w.close()


def _visible(v, a):
    """everything of a normalized view but the opponents' hands, the wall and what follows from them"""
    d = _norm(v, False)
    d.pop("wall")
    d.pop("drawn_tile")
    for s, p in enumerate(d["players"]):
        if s != a:
            p.pop("hand")
    return d


def _tiles(v):
    out = list(v.wall[: v.wall_len]) + list(v.dora[: v.n_dora])
    for p in v.players:
        out += list(p.hand[: p.hand_len]) + list(p.discards[: p.n_discards]) + list(p.kita[: p.n_kita])
        for m in p.melds[: p.n_melds]:
            out += list(m.tiles[: m.n_tiles])
    return sorted(out)


@pytest.mark.parametrize("mode", MODES)
def test_what_the_seat_sees_does_not_change(mode):
    base, rows, views = _base(mode)
    w = base.clone()
    enc0, ext0, out0 = base.encode(), base.encode_extended(), _outputs(base)
    w.determinize(rows, 1234567)
    enc1, ext1, out1 = w.encode(), w.encode_extended(), _outputs(w)
    for i in rows.tolist():
        g, a = i >> 2, i & 3
        before, after = views[g], w.peek(g)
        assert _tiles(before) == _tiles(after), g
        assert not diff_dict(_visible(before, a), _visible(after, a)), g
        assert enc0[g, a].tobytes() == enc1[g, a].tobytes() and ext0[g, a].tobytes() == ext1[g, a].tobytes(), (g, a)
        assert _seat_outputs(out0, g, a) == _seat_outputs(out1, g, a), (g, a)
    w.close()


@pytest.mark.parametrize("mode", MODES)
def test_wall_digest_goes_on_answering(mode):
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(N, game_mode=mode, seeds=np.arange(N, dtype=np.uint64) + 1000, event_ring=RING)
    env.reset()
    env.step_greedy(5, STEPS, auto_reset=False, call_rate_256=128)
    idx = env.legal_compact()[0].astype(np.int32)
    rows = np.array([idx[idx >> 2 == g][0] for g in sorted(set((idx >> 2).tolist()))], np.int32)
    want = env.wall_digests()
    assert all(len(s) == 16 and len(d) == 64 for s, d in want)
    walls = [bytes(env.peek(g).wall) for g in range(N)]
    for seed in (3, 4):   # (the second call finds the digest frozen)
        assert (env.determinize(rows, seed) & 15 == 0).all()
        assert env.wall_digests() == want
    assert sum(bytes(env.peek(g).wall) != walls[g] for g in range(N)) > N // 2
    env.close()


def _compare_oracle(env, games, step_no):
    act, ph, dn = env.status()
    legal, cnt = env.legal()
    mask = env.mask()
    for g, o in games.items():
        oa, op, od = o.status()
        assert (act[g], ph[g], dn[g]) == (oa, op, od), (g, step_no, (act[g], ph[g], dn[g]), (oa, op, od))
        d = diff_dict(_norm(env.peek(g)), _norm(o.peek()))
        assert not d, (g, step_no, d[:8])
        for s in range(4):
            if (oa >> s) & 1 and not od:
                gl, ol = [int(x) for x in legal[g, s, : cnt[g, s]]], o.legal(s)
                assert gl == ol, (g, step_no, s, [fmt_action(x) for x in gl], [fmt_action(x) for x in ol])
                assert (mask[g, s] == o.mask(s)).all(), (g, step_no, s)


@pytest.mark.parametrize("mode", MODES)
def test_published_outputs_and_the_future(mode):
    """the determinized record poked into a fresh game publishes the same lists, masks, waits and status; the oracle poked with the same
    view and the determinized game itself make the same 400 steps (or reach the end of the game) under one stream of actions.
    3P: the reference takes the round's dora and ura indicators out of the wall when the round is dealt and a view cannot carry them, so
    the poked oracle reveals and settles with the indicators of its own first deal.  A 3P game therefore leaves the comparison at the
    step that reveals a new indicator - which is checked against the determinized wall instead: wall-row position 8 + 2 k - or ends the
    round; every step before that is compared.  4P indicators are read from the wall: no such limit."""
    from oracle import oracle
    from riichienv_amd import vecenv

    base, rows, views = _base(mode)
    w = base.clone()
    st = w.determinize(rows, 99)
    fresh = vecenv.VecRiichiEnv(N, game_mode=mode, seed=1, event_ring=RING)
    fresh.reset()
    for i in rows.tolist():
        fresh.poke(i >> 2, w.peek(i >> 2))
    ow, of = _outputs(w), _outputs(fresh)
    for i in rows.tolist():
        g = i >> 2
        assert [x[g] for x in ow[4]] == [x[g] for x in of[4]], g
        for s in range(4):
            if (ow[4][0][g] >> s) & 1:
                assert _seat_outputs(ow, g, s) == _seat_outputs(of, g, s), (g, s)
    fresh.close()
    # the oracle's future: the games that answer a discard first, then others, twelve in all
    order = sorted(rows.tolist(), key=lambda i: (views[i >> 2].phase != abi.WAIT_RESPONSE, i))
    games = {}
    for i in order[:12]:
        g = i >> 2
        o = oracle.Game(game_mode=mode, seed=game_seed(SEED, g))
        o.reset()
        o.poke(w.peek(g))
        games[g] = o
    start = {g: w.peek(g) for g in games}
    compared = 0
    _compare_oracle(w, games, -1)
    for k in range(400):
        acts = np.full((N, 4), abi.NO_ACTION, dtype=np.uint64)
        live = False
        for g, o in games.items():
            if not o.status()[2]:
                acts[g] = [int(x) for x in o.random_actions(31, g)]
                o.step([int(x) for x in acts[g]])
                live = True
        if not live:
            break
        w.step(acts)
        if mode >= 3:
            for g in list(games):
                v, v0 = w.peek(g), start[g]
                for j in range(v0.n_dora, v.n_dora if v.hand_index == v0.hand_index else 0):
                    assert v.dora[j] == v0.wall[8 + 2 * j - v0.rinshan_draw_count], (g, k, j)
                if v.n_dora != v0.n_dora or v.hand_index != v0.hand_index or v.is_done:
                    del games[g]
        _compare_oracle(w, games, k)
        compared += len(games)
    print("oracle steps compared", mode, compared)
    assert compared > (1000 if mode < 3 else 150)
    w.close()


@pytest.mark.parametrize("mode", MODES)
def test_held_hands_and_reproducible_worlds(mode):
    from riichienv_amd import vecenv

    base, rows, views = _base(mode)
    w, w2 = base.clone(), base.clone()
    w.determinize(rows, 5, hold=7)
    changed = 0
    for i in rows.tolist():
        g, a = i >> 2, i & 3
        after = w.peek(g)
        assert not diff_dict(_norm(after, False), _norm(ref.determinize_view(views[g], a, _np(mode), 5, g, hold=7), False)), g
        assert [bytes(p.hand) for p in after.players] == [bytes(p.hand) for p in views[g].players], g
        changed += bytes(after.wall) != bytes(views[g].wall)
    assert changed > N // 2
    # one held opponent per row, by turns; the same (seed, slot) again gives the same world
    hold = (1 << (np.arange(len(rows)) % 3)).astype(np.uint8)
    w.close()
    w = base.clone()
    w.determinize(rows, 6, hold=hold)
    w2.determinize(rows, 6, hold=hold)
    for i, h in zip(rows.tolist(), hold.tolist()):
        g, a = i >> 2, i & 3
        after = w.peek(g)
        assert view_bytes(after) == view_bytes(w2.peek(g)), g
        assert not diff_dict(_norm(after, False), _norm(ref.determinize_view(views[g], a, _np(mode), 6, g, hold=h), False)), g
        for r in range(_np(mode) - 1):
            if (h >> r) & 1:
                s = (a + 1 + r) % _np(mode)
                assert bytes(after.players[s].hand) == bytes(views[g].players[s].hand), (g, s)
    # eight copies of one row in eight slots: eight different worlds
    i = next(i for i in rows.tolist() if len(ref.pool(views[i >> 2], i & 3, _np(mode))) >= 30)
    eight = vecenv.VecRiichiEnv(8, game_mode=mode, seed=1, event_ring=RING)
    eight.reset()
    eight.copy_games(np.arange(8), base, [i >> 2] * 8)
    assert (eight.determinize(np.arange(8) * 4 + (i & 3), 21) & 15 == 0).all()
    hands = {tuple(bytes(p.hand) for s, p in enumerate(eight.peek(k).players) if s != (i & 3)) for k in range(8)}
    assert len(hands) == 8
    for k in range(8):
        assert not diff_dict(_norm(eight.peek(k), False), _norm(ref.determinize_view(views[i >> 2], i & 3, _np(mode), 21, k), False)), k
    for e in (w, w2, eight):
        e.close()


def _torch_copy(mode, base):
    """a TorchVecEnv whose games are the base batch's"""
    from riichienv_amd.torch_env import TorchVecEnv

    tenv = TorchVecEnv(N, game_mode=mode, seed=SEED, skip_mjai_logging=False, event_ring=RING)
    tenv.env.copy_games(np.arange(N), base, np.arange(N))
    return tenv


@pytest.mark.parametrize("mode", MODES)
def test_status_codes(mode):
    torch = pytest.importorskip("torch")
    from riichienv_amd import vecenv

    base, rows, views = _base(mode)
    npl = _np(mode)
    w = base.clone()
    acts = [i for i in rows.tolist() if views[i >> 2].phase == abi.WAIT_ACT]
    idle, over, kan, fine = acts[0], acts[1], acts[2], acts[3]
    v = w.peek(over >> 2)
    v.is_done = 1
    w.poke(over >> 2, v)
    v = w.peek(kan >> 2)                       # the answer to a robbed kan: somebody else is asked, the kan is pending
    other = ((kan & 3) + 1) % npl
    v.phase, v.active_mask, v.pending_kan_pid, v.pending_kan_action = abi.WAIT_RESPONSE, 1 << other, kan & 3, abi.pack_action(abi.KAKAN, 0, [0, 1, 2])
    w.poke(kan >> 2, v)
    idle_seat = next(s for s in range(npl) if not (views[idle >> 2].active_mask >> s) & 1)
    index = np.array([(idle >> 2) * 4 + idle_seat, over, N * 4 + 1, -5, (kan >> 2) * 4 + other, fine, (acts[6] >> 2) * 4 + 3 if npl == 3 else N * 4], np.int32)   # (the last: a seat that does not exist in 3P)
    keep = {g: (view_bytes(w.peek(g)), _game_outputs(w, g)) for g in (idle >> 2, over >> 2, kan >> 2)}
    st = w.determinize(index, 8)
    assert st.tolist() == [abi.DET_NOT_ACTING] * 4 + [abi.DET_CHANKAN, st[5], abi.DET_NOT_ACTING] and st[5] & 15 == abi.DET_OK, st
    for g, (vb, ob) in keep.items():
        assert view_bytes(w.peek(g)) == vb and _game_outputs(w, g) == ob, g
    assert view_bytes(w.peek(fine >> 2)) != view_bytes(views[fine >> 2])
    with pytest.raises(vecenv.RmjError):       # the host form refuses two rows for one game, and touches nothing
        w.determinize(np.array([acts[4], acts[5], acts[4]], np.int32), 8)
    assert view_bytes(w.peek(acts[5] >> 2)) == view_bytes(views[acts[5] >> 2])
    w.close()
    # the device form: the lowest of the rows that name a game is carried out; rows behind the count are left alone
    tenv = _torch_copy(mode, base)
    dup = next((i for i in rows.tolist() if bin(views[i >> 2].active_mask).count("1") > 1), None)
    pairs = [acts[4], acts[4]] + ([dup, (dup >> 2) * 4 + max(s for s in range(4) if (views[dup >> 2].active_mask >> s) & 1)] if dup is not None else [])
    index = torch.tensor(pairs + acts[6:10], dtype=torch.int32, device=tenv.device)
    count = torch.tensor([len(pairs) + 2], dtype=torch.int32, device=tenv.device)
    st = tenv.determinize(index, 8, count=count).cpu().numpy()
    torch.cuda.synchronize()
    assert st[0] & 15 == abi.DET_OK and st[1] == abi.DET_DUPLICATE, st
    if dup is not None:
        assert st[2] & 15 == abi.DET_OK and st[3] == abi.DET_DUPLICATE, st
    for i in pairs[::2] + acts[6:8]:
        g, a = i >> 2, i & 3
        assert not diff_dict(_norm(tenv.env.peek(g), False), _norm(ref.determinize_view(views[g], a, npl, 8, g), False)), g
    for i in acts[8:10]:
        assert view_bytes(tenv.env.peek(i >> 2)) == view_bytes(views[i >> 2]), i
    assert st[len(pairs) + 2:].tolist() == [0, 0]
    tenv.env.close()


@pytest.mark.parametrize("mode", MODES)
def test_riichi_noten_bits_agree_with_the_hidden_targets(mode):
    base, rows, views = _base(mode)
    seen = 0
    for seed in (1, 2, 3):
        w = base.clone()
        st = w.determinize(rows, seed)
        ht = w.hidden_targets(rows)["opp_flags"]
        for k in range(len(rows)):
            for r in range(3):
                noten = bool(ht[k, r] & abi.HIDDEN_RIICHI) and not ht[k, r] & abi.HIDDEN_TENPAI
                assert bool((st[k] >> (4 + r)) & 1) == noten, (seed, k, r, st[k], ht[k])
                seen += noten
        w.close()
    print("riichi hands that are not tenpai", mode, seen)
    assert seen > 0


def _same(a, ga, b, gb):
    assert not diff_dict(normalize_view(a.peek(ga)), normalize_view(b.peek(gb)))
    la, ca = a.legal()
    lb, cb = b.legal()
    live = np.arange(la.shape[-1])[None, :] < ca[ga][:, None]
    assert (ca[ga] == cb[gb]).all() and (np.where(live, la[ga], 0) == np.where(live, lb[gb], 0)).all()
    assert (a.mask()[ga] == b.mask()[gb]).all() and (a.waits()[ga] == b.waits()[gb]).all()
    assert [x[ga] for x in a.status()] == [x[gb] for x in b.status()]
    assert a.mjai_log(ga) == b.mjai_log(gb)


@pytest.mark.parametrize("mode", MODES)
def test_world_set(mode):
    torch = pytest.importorskip("torch")
    from riichienv_amd.search import WorldSet

    base, rows, views = _base(mode)
    tenv = _torch_copy(mode, base)
    R, K = 8, 4
    ws = WorldSet(tenv, worlds=K, max_rows=R)
    index = torch.tensor(rows[:R].tolist(), dtype=torch.int32, device=tenv.device)
    results = []
    for _ in range(2):
        st = ws.fork(index, seed=11).cpu().numpy()
        torch.cuda.synchronize()
        assert st.shape == (R, K) and (st & 15 == abi.DET_OK).all()
        for r, i in enumerate(rows[:R].tolist()):
            g, a = i >> 2, i & 3
            for k in range(K):
                v = ws.env.env.peek(r * K + k)
                assert not diff_dict(_norm(v, False), _norm(ref.determinize_view(views[g], a, _np(mode), 11, r * K + k), False)), (r, k)
                assert bytes(v.players[a].hand) == bytes(views[g].players[a].hand) and v.players[a].score == views[g].players[a].score
        ws.playout(policy_seed=3, max_steps=6000)
        delta, rank, done = (x.cpu().numpy() for x in ws.values())
        torch.cuda.synchronize()
        assert done.all()
        sc, rk = ws.env.env.scores(), ws.env.env.ranks()
        for r, i in enumerate(rows[:R].tolist()):
            g, a = i >> 2, i & 3
            for k in range(K):
                assert delta[r, k] == sc[r * K + k, a] - views[g].players[a].score and rank[r, k] == rk[r * K + k, a], (r, k)
        results.append((delta.copy(), rank.copy()))
    assert (results[0][0] == results[1][0]).all() and (results[0][1] == results[1][1]).all()
    assert len({int(x) for x in results[0][0].reshape(-1)}) > 1
    for i in rows[:R].tolist():
        _same(tenv.env, i >> 2, base, i >> 2)
    ws.env.env.close()
    tenv.env.close()


def test_pimc_example_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pimc_discard.py"), "--roots", "2", "--worlds", "4"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "2 roots" in p.stdout and p.stdout.count("mean score change") >= 2, p.stdout
