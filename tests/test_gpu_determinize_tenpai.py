"""rmj_determinize_ex_device with RMJ_DETF_RIICHI_TENPAI on the GPU: flags = 0 against the old entry, the flagged re-deal against the
restatement of tests/determinize_tenpai_ref.py, what must not change, the published outputs against the oracle's future, held hands,
status codes and WorldSet.  The batch is the one of tests/test_gpu_determinize.py: 64 games after 120 steps of the device policy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from riichienv_amd import abi
from riichienv_amd.shard import game_seed
from tests import determinize_ref as ref
from tests import determinize_tenpai_ref as tref
from tests.parity_util import diff_dict, view_bytes
from tests.test_gpu_determinize import (MODES, N, RING, SEED, _base, _compare_oracle, _game_outputs, _norm, _np, _outputs, _same, _seat_outputs,
                                        _torch_copy)

pytestmark = pytest.mark.gpu

HI = abi.DET_SWAPPED | abi.DET_RIICHI_NOTEN * 7


def _ex(env, rows, seed, flags, hold=None):
    """rmj_determinize_ex itself: (return code, status)"""
    idx = np.ascontiguousarray(rows, dtype=np.int32)
    st = np.zeros(len(idx), np.uint8)
    h = None if hold is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hold, dtype=np.uint8), (len(idx),)))
    d = abi.Determinize(seed, None if h is None else h.ctypes.data, st.ctypes.data)
    return env.L.rmj_determinize_ex(env.h, idx.ctypes.data, len(idx), C.byref(d), flags), st


@pytest.mark.parametrize("mode", MODES)
def test_flags_zero_is_the_old_entry(mode):
    base, rows, views = _base(mode)
    old, new = base.clone(), base.clone()
    st_old = old.determinize(rows, 77)
    rc, st_new = _ex(new, rows, 77, 0)
    assert rc == 0 and st_old.tobytes() == st_new.tobytes() and not (st_new & abi.DET_SWAPPED).any()
    for i in rows.tolist():
        g = i >> 2
        assert view_bytes(old.peek(g)) == view_bytes(new.peek(g)), g
        assert _game_outputs(old, g) == _game_outputs(new, g), g
    # an unknown flag bit: refused, nothing touched
    keep = [view_bytes(new.peek(i >> 2)) for i in rows.tolist()]
    for flags in (2, 3, 0x80000000):
        rc, _ = _ex(new, rows, 78, flags)
        assert rc != 0
    assert keep == [view_bytes(new.peek(i >> 2)) for i in rows.tolist()]
    old.close()
    new.close()


@pytest.mark.parametrize("mode", MODES)
def test_flagged_redeal_equals_the_restatement(mode):
    """seeds 1, 2, 3 on the 64 rows.  Census on the MI355X: mode 2 - 21 riichi seats, 21 walks, 21 swapped worlds, 78 exchanges of which 3
    sideways, NOTEN bits 0 with the flag and 21 without; mode 5 - 21 walks, 21 swapped worlds, 66 exchanges, none sideways, 0 against 21."""
    base, rows, views = _base(mode)
    census = {"swapped": 0, "walks": 0, "exchanges": 0, "side": 0, "noten": 0, "noten_plain": 0, "riichi_seats": 0}
    for seed in (1, 2, 3):
        w, plain = base.clone(), base.clone()
        st = w.determinize(rows, seed, riichi_tenpai=True)
        st_plain = plain.determinize(rows, seed)
        ht = w.hidden_targets(rows)["opp_flags"]
        for k, (i, st_i) in enumerate(zip(rows.tolist(), st.tolist())):
            g, a = i >> 2, i & 3
            assert st_i & 15 == abi.DET_OK, (g, a, st_i)
            want, want_st, walks = tref.determinize_view(views[g], a, _np(mode), seed, g)
            d = diff_dict(_norm(w.peek(g), False), _norm(want, False))
            assert not d, (seed, g, a, walks, d[:6])
            assert st_i & HI == want_st, (seed, g, a, st_i, want_st, walks)   # DET_SWAPPED and the NOTEN bits: a bit that stays, stays in the restatement
            for r in range(3):
                noten = bool(ht[k, r] & abi.HIDDEN_RIICHI) and not ht[k, r] & abi.HIDDEN_TENPAI
                assert bool((st_i >> (4 + r)) & 1) == noten, (seed, k, r, st_i, ht[k])
                census["riichi_seats"] += bool(ht[k, r] & abi.HIDDEN_RIICHI)
            census["swapped"] += bool(st_i & abi.DET_SWAPPED)
            census["walks"] += len(walks)
            census["exchanges"] += sum(len(x["steps"]) for x in walks)
            census["side"] += sum(x["steps"].count("side") for x in walks)
            census["noten"] += bin(st_i >> 4 & 7).count("1")
            census["noten_plain"] += bin(int(st_plain[k]) >> 4 & 7).count("1")
        w.close()
        plain.close()
    print("census", mode, census)
    assert census["swapped"] > 0
    assert census["noten"] < census["noten_plain"]


def _all_tiles(v):
    out = list(v.wall[: v.wall_len])
    for p in v.players:
        out += list(p.hand[: p.hand_len]) + list(p.discards[: p.n_discards]) + list(p.kita[: p.n_kita])
        for m in p.melds[: p.n_melds]:
            out += list(m.tiles[: m.n_tiles])
    return sorted(out)


@pytest.mark.parametrize("mode", MODES)
def test_what_the_seat_sees_does_not_change(mode):
    base, rows, views = _base(mode)
    w = base.clone()
    out0 = _outputs(base)
    st = w.determinize(rows, 2, riichi_tenpai=True)
    out1 = _outputs(w)
    every = set(range(136)) if mode < 3 else {t for t in range(136) if not 1 <= t >> 2 <= 7}
    for i in rows.tolist():
        g, a = i >> 2, i & 3
        before, after = views[g], w.peek(g)
        assert _seat_outputs(out0, g, a) == _seat_outputs(out1, g, a), (g, a)
        assert _all_tiles(before) == _all_tiles(after) and set(_all_tiles(after)) == every, g
        hidden = [ref._get(after, loc) for loc in ref.pool(after, a, _np(mode))]
        assert len(set(hidden)) == len(hidden), g
        assert bytes(after.players[a].hand) == bytes(before.players[a].hand), g
    assert (st & 15 == abi.DET_OK).all()
    w.close()


@pytest.mark.parametrize("mode", MODES)
def test_published_outputs_and_the_future(mode):
    """the comparison of tests/test_gpu_determinize.py on flagged worlds, the swapped ones first: the record poked into a fresh game
    publishes the same outputs, and the oracle poked with the same view makes the same 60 steps (3P: until a new indicator is revealed
    or the round ends, as there)"""
    from oracle import oracle
    from riichienv_amd import vecenv

    base, rows, views = _base(mode)
    for seed in (1, 2, 3):   # the first of the seeds with a swapped world (the census of the test above holds that there is one)
        w = base.clone()
        st = w.determinize(rows, seed, riichi_tenpai=True)
        if (st & abi.DET_SWAPPED).any():
            break
        w.close()
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
    swapped = {int(i): bool(s & abi.DET_SWAPPED) for i, s in zip(rows.tolist(), st.tolist())}
    order = sorted(rows.tolist(), key=lambda i: (not swapped[i], views[i >> 2].phase != abi.WAIT_RESPONSE, i))
    games = {}
    for i in order[:12]:
        g = i >> 2
        o = oracle.Game(game_mode=mode, seed=game_seed(SEED, g))
        o.reset()
        o.poke(w.peek(g))
        games[g] = o
    assert any(swapped[i] for i in order[:12])
    start = {g: w.peek(g) for g in games}
    compared = 0
    _compare_oracle(w, games, -1)
    for k in range(60):
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
    assert compared >= (200 if mode < 3 else 12)
    w.close()


@pytest.mark.parametrize("mode", MODES)
def test_hold_status_codes_and_duplicates(mode):
    torch = pytest.importorskip("torch")
    from riichienv_amd import vecenv

    base, rows, views = _base(mode)
    npl = _np(mode)
    # every opponent held: no hand moves, nothing is repaired
    w = base.clone()
    st = w.determinize(rows, 5, hold=7, riichi_tenpai=True)
    assert not (st & abi.DET_SWAPPED).any() and not (st >> 4).any()
    for i in rows.tolist():
        g, a = i >> 2, i & 3
        assert [bytes(p.hand) for p in w.peek(g).players] == [bytes(p.hand) for p in views[g].players], g
        assert not diff_dict(_norm(w.peek(g), False), _norm(ref.determinize_view(views[g], a, npl, 5, g, hold=7), False)), g
    w.close()
    # one held opponent per row, by turns
    hold = (1 << (np.arange(len(rows)) % 3)).astype(np.uint8)
    w = base.clone()
    st = w.determinize(rows, 3, hold=hold, riichi_tenpai=True)
    for i, h, st_i in zip(rows.tolist(), hold.tolist(), st.tolist()):
        g, a = i >> 2, i & 3
        want, want_st, walks = tref.determinize_view(views[g], a, npl, 3, g, hold=h)
        assert not diff_dict(_norm(w.peek(g), False), _norm(want, False)), (g, walks)
        assert st_i == want_st, (g, st_i, want_st)
        for r in range(npl - 1):
            if (h >> r) & 1:
                assert bytes(w.peek(g).players[(a + 1 + r) % npl].hand) == bytes(views[g].players[(a + 1 + r) % npl].hand), (g, r)
    w.close()
    # status codes: rows that are not carried out leave the game alone
    w = base.clone()
    acts = [i for i in rows.tolist() if views[i >> 2].phase == abi.WAIT_ACT]
    idle, fine = acts[0], acts[3]
    idle_seat = next(s for s in range(npl) if not (views[idle >> 2].active_mask >> s) & 1)
    index = np.array([(idle >> 2) * 4 + idle_seat, N * 4 + 1, -5, fine], np.int32)
    st = w.determinize(index, 8, riichi_tenpai=True)
    assert st[:3].tolist() == [abi.DET_NOT_ACTING] * 3 and st[3] & 15 == abi.DET_OK, st
    assert view_bytes(w.peek(idle >> 2)) == view_bytes(views[idle >> 2])
    with pytest.raises(vecenv.RmjError):       # the host form refuses two rows for one game, and touches nothing
        w.determinize(np.array([acts[4], acts[5], acts[4]], np.int32), 8, riichi_tenpai=True)
    assert view_bytes(w.peek(acts[5] >> 2)) == view_bytes(views[acts[5] >> 2])
    w.close()
    # the device form: the lowest of the rows that name a game is carried out; rows behind the count are left alone
    tenv = _torch_copy(mode, base)
    pairs = [acts[4], acts[4]]
    index = torch.tensor(pairs + acts[6:10], dtype=torch.int32, device=tenv.device)
    count = torch.tensor([len(pairs) + 2], dtype=torch.int32, device=tenv.device)
    st = tenv.determinize(index, 8, count=count, riichi_tenpai=True).cpu().numpy()
    torch.cuda.synchronize()
    assert st[0] & 15 == abi.DET_OK and st[1] == abi.DET_DUPLICATE, st
    for k, i in [(0, acts[4]), (2, acts[6]), (3, acts[7])]:
        g, a = i >> 2, i & 3
        want, want_st, _ = tref.determinize_view(views[g], a, npl, 8, g)
        assert not diff_dict(_norm(tenv.env.peek(g), False), _norm(want, False)), g
        assert st[k] == want_st, (k, st)
    for i in acts[8:10]:
        assert view_bytes(tenv.env.peek(i >> 2)) == view_bytes(views[i >> 2]), i
    assert st[len(pairs) + 2:].tolist() == [0, 0]
    tenv.env.close()


@pytest.mark.parametrize("mode", MODES)
def test_world_set(mode):
    torch = pytest.importorskip("torch")
    from riichienv_amd.search import WorldSet

    base, rows, views = _base(mode)
    tenv = _torch_copy(mode, base)
    R, K = 8, 4
    # the rows with an opponent in riichi first, so that the walks have something to do
    pick = sorted(rows.tolist(), key=lambda i: (not any(p.riichi_declared for s, p in enumerate(views[i >> 2].players) if s != (i & 3)), i))[:R]
    ws = WorldSet(tenv, worlds=K, max_rows=R)
    index = torch.tensor(pick, dtype=torch.int32, device=tenv.device)
    results = []
    for _ in range(2):
        st = ws.fork(index, seed=11, riichi_tenpai=True).cpu().numpy()
        torch.cuda.synchronize()
        assert st.shape == (R, K) and (st & 15 == abi.DET_OK).all()
        for r, i in enumerate(pick):
            g, a = i >> 2, i & 3
            for k in range(K):
                v = ws.env.env.peek(r * K + k)
                want, want_st, walks = tref.determinize_view(views[g], a, _np(mode), 11, r * K + k)
                assert not diff_dict(_norm(v, False), _norm(want, False)), (r, k, walks)
                assert st[r, k] == want_st, (r, k, st[r, k], want_st)
                assert bytes(v.players[a].hand) == bytes(views[g].players[a].hand)
        ws.playout(policy_seed=3, max_steps=6000)
        delta, rank, done = (x.cpu().numpy() for x in ws.values())
        torch.cuda.synchronize()
        assert done.all()
        results.append((st.copy(), delta.copy(), rank.copy()))
    assert all((x == y).all() for x, y in zip(*results))
    for i in pick:
        _same(tenv.env, i >> 2, base, i >> 2)
    ws.env.env.close()
    tenv.env.close()


def test_pimc_example_takes_the_switch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "examples", "pimc_discard.py"), "--roots", "2", "--worlds", "4", "--riichi-tenpai"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "2 roots" in p.stdout and "repaired by exchanges" in p.stdout and p.stdout.count("mean score change") >= 2, p.stdout
