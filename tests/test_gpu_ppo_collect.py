"""The PPO transition collector (riichienv_amd.ppo.PPOCollector: rmj_select_ids_device, rmj_ppo_record_device, rmj_ppo_close_device,
rmj_ppo_emit_device) held to the restatement of the worker's bookkeeping (tests/ppo_collect_ref.py).

Parity: 4 096 games x 400 steps with auto-reset, 4p-red-half and 3p-red-half, every feature set of the mode, dense and compact
observation layouts, logits and values from a seeded generator (and one run with a small conv net).  Every step's inputs (ids, the hero
rows' masks, logits, values, the boundaries and rewards) are recorded on the host and replayed through the restatement:
  * features, mask, action, pool order (game, serial, t, prev per slot), counts: equal.  The feature rows are compared on the device
    (slot by slot against the observation rows right after every record call, and the emitted rows against the pool at the end);
  * advantage, return: bit-equal to the restatement's Python-float GAE rounded to f32;
  * log_prob: within 4 x e_ref of the float64 restatement, e_ref = max |CPU torch f32 log_softmax(masked_fill(..)).gather(..) - float64|
    measured on the same rows (>= 100 000 rows over the runs of a mode).  Figures go to profiles/ppo_collect.json when the directory is
    writable.  The seeded logits are finite with |logit| < 1e8 (asserted: the excluded share is zero).
  * select ids: the hero seat's id = rmj_sample_ids_device's for the same seed and state, every other acting seat's id = the
    restatement's arg-max.  A separate test feeds NaN, -inf, +inf and tied logits, with NaN in every cell the kernel must not read.
Edges: a short pool, clear, hero = 255, the two boundary rules on renchan rounds, a bound stream without share_stream."""
import json
import os

import numpy as np
import pytest

from riichienv_amd import abi
from tests import ppo_collect_ref as R

pytestmark = pytest.mark.gpu

N, STEPS = 4096, 400
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGP = {}   # mode -> list of (rows, e_ref, e_dev) of the parity runs


def _env(mode, features, n=N, seed=77, **kw):
    from riichienv_amd.torch_env import TorchVecEnv

    return TorchVecEnv(n, game_mode=mode, seed=seed, features=features, **kw)


class SeededModels:
    """policy(obs) = (logits N(0, 3), values N(0, 1)), baseline(obs) = logits: one seeded device generator, rows x A"""

    def __init__(self, torch, device, A, seed):
        self.t, self.A = torch, A
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.device = device

    def policy(self, obs):
        k = obs.shape[0]
        return (self.t.randn((k, self.A), generator=self.gen, device=self.device) * 3.0, self.t.randn((k,), generator=self.gen, device=self.device))

    def baseline(self, obs):
        return self.t.round(self.t.randn((obs.shape[0], self.A), generator=self.gen, device=self.device) * 2.0)   # (rounded: ties between ids)


class Recorder:
    """on_step hook: replays every step through the restatement and checks what can be checked at once"""

    def __init__(self, col, capacity):
        self.col, self.e, self.t = col, col.tenv, col.t
        t = self.t
        self.hero = col.hero.cpu().numpy()
        self.ref = R.PoolRef(col.n, capacity, col.gamma, col.gae_lambda, self.hero)
        self.g = t.arange(col.n, device=self.e.device)
        self.h64 = col._hero64
        self.feat_ok = t.ones((), dtype=t.bool, device=self.e.device)
        self.steps = self.select_rows = self.opp_rows = 0
        self.round_ended, self.honba, self.closes, self.kidx, self.open_before = [], [], [], [], []

    def __call__(self, d):
        t, e, col = self.t, self.e, self.col
        if d["phase"] == "close":
            ended, reward = d["ended"].cpu().numpy(), d["reward"].cpu().numpy()
            self.round_ended.append(d["round_ended"].cpu().numpy().copy())
            self.honba.append(d["meta"][:, 2].cpu().numpy().copy())
            self.closes.append(ended.copy())
            self.kidx.append(d["kyoku_idx"].cpu().numpy().copy())
            self.open_before.append(self.ref.open_len())
            self.ref.close(ended, reward)
            return
        if not self.steps:
            self.kidx0 = e.round_track()[3].cpu().numpy().copy()           # (no step since the collector's call: kyoku_idx before the first step)
        self.steps += 1
        ids_d, sel = d["ids"], d["select_logits"]
        # the hero rows of this step, found independently of the kernel: dense rows by (game, hero), compact rows through the index
        if col._layout == "compact":
            obs, index, count = d["obs"]
            k = int(count.item())
            assert k <= index.shape[0]
            inv = t.full((col.n * 4,), -1, dtype=t.int64, device=e.device)
            inv[index[:k].to(t.int64)] = t.arange(k, device=e.device)
            row = inv[self.g * 4 + self.h64]
            rowc = row.clamp(min=0)
            hero_obs, hero_logits, hero_values = obs[rowc], d["logits"][rowc], d["values"][rowc]
        else:
            row = self.g * 4 + self.h64
            hero_obs, hero_logits, hero_values = d["obs"][self.g, self.h64], d["logits"][self.g, self.h64], d["values"][self.g, self.h64]
        hero_mask = e.mask[self.g, self.h64][:, : col.A]
        sampled = e.sample_ids(sel, seed=d["seed"]).cpu().numpy()          # the same seed and state: the hero's draw
        ids = ids_d.cpu().numpy()
        masks = e.mask.cpu().numpy()[:, :, : col.A]
        acting = sampled >= 0
        want = R.argmax_rows(masks.reshape(-1, col.A), sel.cpu().numpy().reshape(col.n * 4, -1)[:, : col.A]).reshape(col.n, 4)
        is_hero = np.arange(4)[None, :] == self.hero[:, None]
        want = np.where(acting, np.where(is_hero, sampled, want), -1)
        assert np.array_equal(ids, want), f"step {self.steps}: select ids differ at {np.argwhere(ids != want)[:4].tolist()}"
        self.select_rows += int(acting.sum())
        self.opp_rows += int((acting & ~is_hero).sum())
        hm, hl, hv, rw = hero_mask.cpu().numpy(), hero_logits.cpu().numpy(), hero_values.cpu().numpy(), row.cpu().numpy()
        step = self.steps
        wrote = self.ref.record(ids, lambda g: None if rw[g] < 0 else ((step, g), hm[g], hl[g], hv[g]))
        if wrote:
            gs = t.tensor([g for g, _ in wrote], device=e.device)
            ss = t.tensor([s for _, s in wrote], device=e.device)
            self.feat_ok &= (col.pool["features"][ss] == hero_obs[gs]).all()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check(col, rec, mode, expect_overflow=False):
    t = col.t
    ref, c = rec.ref, col.counts()
    assert c == ref.counts(), (c, ref.counts())
    if not expect_overflow:
        assert c["overflowed"] == 0 and c["dropped"] == 0 and c["valid"] > 0 and c["open"] > 0
    assert bool(rec.feat_ok), "a recorded feature row differs from the observation row of its (game, hero)"
    f = c["fill"]
    for key in ("game", "serial", "t", "prev", "action"):
        assert np.array_equal(col.pool[key][:f].cpu().numpy(), np.array([s[key] for s in ref.slots], np.int32)), key
    assert np.array_equal(col.pool["valid"][:f].cpu().numpy() != 0, np.array([s["valid"] for s in ref.slots], bool))
    tr, e = col.transitions(), ref.emit()
    k = c["valid"]
    assert all(tr[key].shape[0] == k for key in tr) and len(e["slot"]) == k
    if not k:
        return tr, e
    slots = t.as_tensor(e["slot"], device=col.tenv.device)
    assert bool((tr["features"] == col.pool["features"][slots]).all()), "emitted features differ from the pool rows of the restatement's slots"
    assert tr["action"].dtype == t.int64 and np.array_equal(tr["action"].cpu().numpy(), e["action"])
    assert np.array_equal(tr["mask"].cpu().numpy(), e["mask"])
    for key in ("advantage", "return"):
        got = tr[key].cpu().numpy()
        bad = np.flatnonzero(_bits(got) != _bits(e[key]))
        assert not len(bad), f"{key}: {len(bad)} of {k} differ in bits, first {got[bad[:3]]} vs {e[key][bad[:3]]}"
    # log_prob: the tolerance is measured on these rows (CPU torch f32 = the worker's arithmetic against float64)
    legal = e["logits"][e["mask"] != 0]
    excluded = int((~np.isfinite(legal) | (np.abs(legal) >= 1e8)).sum())
    assert excluded == 0, "the seeded logits must stay inside the log_prob contract"
    lg, mk = t.from_numpy(e["logits"]), t.from_numpy(e["mask"]).bool()
    cpu32 = t.log_softmax(lg.masked_fill(~mk, -1e9), dim=-1).gather(1, t.from_numpy(e["action"])[:, None])[:, 0].numpy()
    e_ref = float(np.abs(cpu32.astype(np.float64) - e["log_prob"]).max())
    e_dev = float(np.abs(tr["log_prob"].cpu().numpy().astype(np.float64) - e["log_prob"]).max())
    print(f"log_prob rows {k} e_ref {e_ref:.3e} device {e_dev:.3e}")
    LOGP.setdefault(mode, []).append((k, e_ref, e_dev))
    assert e_dev <= 4 * e_ref, (e_dev, e_ref, k)
    st, rs = col.stats(), ref.stats()
    assert st["kyokus"] == len(ref.completed) and abs(st["kyoku_length_mean"] - rs["kyoku_length_mean"]) < 1e-9
    assert abs(st["kyoku_reward_mean"] - rs["kyoku_reward_mean"]) < 1e-6 and abs(st["kyoku_reward_std"] - rs["kyoku_reward_std"]) < 1e-6
    return tr, e


def _run(mode, features, layout, capacity=None, n=N, steps=STEPS, boundary="round", seed=5, hero=None, net=None, **envkw):
    import torch

    from riichienv_amd.ppo import PPOCollector

    e = _env(mode, features, n=n, **envkw)
    e.env.step_random(policy_seed=9, n_steps=450, auto_reset=True)   # the games start anywhere in their course: some end inside the run
    capacity = capacity or int(n * steps * 0.45)

    col = PPOCollector(e, capacity, hero=hero, boundary=boundary, seed=seed)
    m = SeededModels(torch, e.device, col.A, 1000 + seed)
    rec = Recorder(col, capacity)
    col.collect(net or m.policy, m.baseline, steps, layout=layout, on_step=rec)
    return e, col, rec


PARITY = [(2, f, lay) for f in ("base", "discard_shanten", "extended") for lay in ("compact", "dense")] + \
         [(5, f, lay) for f in ("base", "extended") for lay in ("compact", "dense")]


@pytest.mark.parametrize("mode,features,layout", PARITY)
def test_collect_parity(mode, features, layout):
    e, col, rec = _run(mode, features, layout)
    _check(col, rec, mode)
    ended = np.stack(rec.round_ended)
    per_game = (ended != 0).sum(0)
    print(f"boundaries per game: min {per_game.min()} median {np.median(per_game)} max {per_game.max()}; games that ended: {(ended == 2).any(0).sum()}; "
          f"games below 2: {np.flatnonzero(per_game < 2)[:8].tolist()} status {e.status_raw.cpu().numpy()[np.flatnonzero(per_game < 2)[:8]].tolist()}")
    # the run must be long enough to mean something: the games cross several kyokus and some cross a game end
    assert np.median(per_game) >= 3 and (per_game >= 2).mean() >= 0.99 and (ended == 2).any(0).sum() >= 50
    assert rec.opp_rows > 100000 and rec.select_rows > rec.opp_rows
    col.close()


def test_log_prob_sample_and_report():
    """the rows behind e_ref: at least 100 000 per mode over the parity runs; the figures are written down"""
    if not LOGP:                                                   # (run on its own: one parity run provides the rows)
        e, col, rec = _run(2, "base", "compact")
        _check(col, rec, 2)
    out = {}
    for mode, runs in LOGP.items():
        rows = sum(r[0] for r in runs)
        assert rows >= 100000, (mode, rows)
        out[str(mode)] = {"rows": rows, "e_ref_max": max(r[1] for r in runs), "device_max": max(r[2] for r in runs),
                          "runs": [{"rows": r[0], "e_ref": r[1], "device": r[2]} for r in runs]}
    path = os.path.join(ROOT, "profiles", "ppo_collect.json")
    try:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["log_prob"] = out
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def test_collect_parity_conv_net():
    """logits and values from a small real network over the compact rows (the arithmetic a trainer runs)"""
    import torch

    torch.manual_seed(3)
    dev = torch.device("cuda", 0)
    body = torch.nn.Sequential(torch.nn.Conv1d(74, 16, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(16 * 34, 83)).to(dev)

    def net(obs):
        with torch.no_grad():
            y = body(obs)
        return y[:, :82].contiguous() * 4.0, y[:, 82].contiguous()

    e, col, rec = _run(2, "base", "compact", net=net)
    _check(col, rec, "net")
    col.close()


def test_select_ids_non_finite_and_unread_cells():
    """NaN, -inf, +inf and tied logits in the legal cells; NaN in every cell the kernel must not read (illegal ids, seats that do not act)"""
    import torch

    from riichienv_amd.ppo import PPOCollector

    for mode in (2, 5):
        e = _env(mode, "base", n=N, seed=31)
        col = PPOCollector(e, 16, seed=9)
        A = col.A
        gen = torch.Generator(device=e.device).manual_seed(17)
        hero = col.hero.cpu().numpy()
        kinds = 0
        for it in range(12):
            e.step_sample_obs(None, seed=100 + it)
            for _ in range(20):
                e.step(e.sample_ids(None, seed=1000 + it))
            lg = torch.round(torch.randn((N, 4, A + 3), generator=gen, device=e.device) * 2.0)
            sp = torch.rand((N, 4, A + 3), generator=gen, device=e.device)
            lg[sp < 0.15] = float("nan")
            lg[(sp >= 0.15) & (sp < 0.3)] = float("-inf")
            lg[(sp >= 0.3) & (sp < 0.35)] = float("inf")
            rowkind = torch.rand((N, 4, 1), generator=gen, device=e.device)
            lg = torch.where(rowkind < 0.1, torch.full_like(lg, float("nan")), lg)            # rows without any usable logit
            lg = torch.where((rowkind >= 0.1) & (rowkind < 0.2), torch.full_like(lg, float("-inf")), lg)
            unread = torch.ones_like(lg, dtype=torch.bool)
            unread[:, :, :A] = (e.mask[:, :, :A] == 0) | ~e.active()[:, :, None]
            lg = torch.where(unread, torch.full_like(lg, float("nan")), lg).contiguous()
            sampled = e.sample_ids(lg, seed=7 + it).cpu().numpy()
            for hp, hv in ((col.hero, hero), (col._no_hero, np.full(N, 255)), (None, None)):
                ids = col.select_ids(lg, 7 + it, hero=hp).cpu().numpy()
                acting = sampled >= 0
                want = R.argmax_rows(e.mask.cpu().numpy()[:, :, :A].reshape(-1, A), lg.cpu().numpy().reshape(N * 4, -1)[:, :A]).reshape(N, 4)
                draws = np.ones((N, 4), bool) if hv is None else np.arange(4)[None, :] == hv[:, None]
                want = np.where(acting, np.where(draws, sampled, want), -1)
                assert np.array_equal(ids, want), (mode, it, np.argwhere(ids != want)[:4].tolist())
            lgc = lg.cpu().numpy()[:, :, :A]
            legal = (e.mask.cpu().numpy()[:, :, :A] != 0) & acting[:, :, None]
            kinds |= 1 * bool((np.isnan(lgc) & legal).any()) | 2 * bool((np.isposinf(lgc) & legal).any()) | 4 * bool((np.isneginf(lgc) & legal).any())
            assert acting.sum() > N // 2
        assert kinds == 7
        # the slice used by sample_ids above has stride A + 3: also the plain stride
        col.close()


def _guarded(t, shape, dtype, dev, fill):
    """a tensor of `shape` in front of 64 guard elements"""
    n = int(np.prod(shape))
    buf = t.full((n + 64,), fill, dtype=dtype, device=dev)
    return buf, buf[:n].view(shape)


def test_short_pool_counts_overflow_and_emits_no_broken_trajectory():
    import torch

    n, steps, cap = 1024, 300, 20000
    e, col, rec = _run(2, "base", "compact", capacity=cap, n=n, steps=steps)
    c = col.counts()
    assert c["fill"] == cap and c["overflowed"] > 1000 and c["dropped"] > 0
    tr, ref = _check(col, rec, "short", expect_overflow=True)
    # emitted trajectories are whole: every game's emitted slots are complete runs t = 0 .. len - 1 of one serial
    slots = ref["slot"]
    game, serial, tt = (col.pool[k][:cap].cpu().numpy()[slots] for k in ("game", "serial", "t"))
    seen = {}
    for g, s, x in zip(game, serial, tt):
        seen.setdefault((g, s), []).append(x)
    assert all(v == list(range(len(v))) for v in seen.values())
    seg_len = col.pool["seg_len"][:cap].cpu().numpy()
    assert sorted(len(v) for v in seen.values()) == sorted(seg_len[seg_len > 0].tolist())
    # nothing is written past the caller's rows, and rows beyond the caller's capacity are left out: guard words stay intact
    k, dev, rows = c["valid"], e.device, c["valid"] - 7
    bufs = {"features": _guarded(torch, (rows, e.channels, e.width), torch.float32, dev, -7.0), "mask": _guarded(torch, (rows, col.A), torch.uint8, dev, 0xAB),
            "action": _guarded(torch, (rows,), torch.int64, dev, -77), "log_prob": _guarded(torch, (rows,), torch.float32, dev, -7.0),
            "advantage": _guarded(torch, (rows,), torch.float32, dev, -7.0), "return": _guarded(torch, (rows,), torch.float32, dev, -7.0)}
    cnt = col.emit_into({key: v[1] for key, v in bufs.items()}, rows)
    assert cnt.cpu().tolist() == [k, c["fill"] - k]
    for key, (buf, view) in bufs.items():
        fill = {"mask": 0xAB, "action": -77}.get(key, -7.0)
        assert bool((buf[-64:] == fill).all()), key
        assert bool((view == tr[key][:rows]).all()), key
    col.close()


def test_clear_then_second_collection_equals_fresh_collector():
    import torch

    from riichienv_amd.ppo import PPOCollector

    n, steps, cap = 1024, 120, 60000

    def models(e, A):
        return SeededModels(torch, e.device, A, 4242)

    a = _env(2, "base", n=n, seed=12)
    ca = PPOCollector(a, cap, seed=3)
    m = SeededModels(torch, a.device, ca.A, 1)
    ca.collect(m.policy, m.baseline, 60)
    assert ca.counts()["fill"] > 0
    ca.clear()
    assert ca.counts() == {"fill": 0, "valid": 0, "dropped": 0, "overflowed": 0, "segments": 0, "open": 0}
    # a fresh environment brought to the same state, a fresh collector, the same seeds from here on
    b = _env(2, "base", n=n, seed=12)
    b.copy_games(torch.arange(n, device=b.device), a, torch.arange(n, device=a.device))
    a.round_track(), b.round_track()
    cb = PPOCollector(b, cap, hero=ca.hero.clone(), seed=3)
    cb._seed = ca._seed
    cb._first_obs("compact")
    cb._layout = "compact"
    ca._first_obs("compact")
    ma, mb = models(a, ca.A), models(b, cb.A)
    ca.collect(ma.policy, ma.baseline, steps)
    cb.collect(mb.policy, mb.baseline, steps)
    assert ca.counts() == cb.counts() and ca.counts()["valid"] > 1000
    ta, tb = ca.transitions(), cb.transitions()
    for key in ta:
        assert torch.equal(ta[key].view(torch.uint8), tb[key].view(torch.uint8)) if ta[key].dtype != torch.int64 else torch.equal(ta[key], tb[key]), key


def test_hero_255_records_nothing_and_evaluate_plays_argmax():
    import torch

    from riichienv_amd.ppo import PPOCollector

    n = 512
    e = _env(2, "base", n=n, seed=8)
    hero = torch.full((n,), 255, dtype=torch.uint8)
    hero[::2] = 1
    col = PPOCollector(e, 40000, hero=hero)
    m = SeededModels(torch, e.device, col.A, 6)
    col.collect(m.policy, m.baseline, 150)
    c = col.counts()
    games = col.pool["game"][: c["fill"]].cpu().numpy()
    assert c["fill"] > 1000 and (games % 2 == 0).all() and c["overflowed"] == 0
    rank, reward, done = col.evaluate(m.policy, m.baseline, max_steps=3000)
    assert bool(done.all()) and col.counts()["fill"] == c["fill"]
    rank, reward = rank.cpu().numpy(), reward.cpu().numpy()
    assert set(np.unique(rank)) <= {1, 2, 3, 4} and np.array_equal(reward, np.array([0, 10, 4, -4, -10], np.float32)[rank])
    col.close()


def test_boundary_rules_differ_exactly_on_renchan_rounds():
    """the same games, seeds and models under both rules: identical transitions in the pool, different trajectories exactly where a round
    end left kyoku_idx unchanged (a renchan: the next round's honba is the previous one's + 1 with the same dealer)"""
    n, steps = 2048, 400
    ea, ca, ra = _run(2, "base", "compact", n=n, steps=steps, boundary="round", seed=21)
    eb, cb, rb = _run(2, "base", "compact", n=n, steps=steps, boundary="kyoku_idx", seed=21)
    _check(ca, ra, "round-rule")
    _check(cb, rb, "kyoku-rule")
    f = ca.counts()["fill"]
    assert f == cb.counts()["fill"]
    for key in ("game", "action", "value", "log_prob"):
        assert np.array_equal(ca.pool[key][:f].cpu().numpy(), cb.pool[key][:f].cpu().numpy()), key
    ended = np.stack(ra.round_ended)
    assert np.array_equal(ended, np.stack(rb.round_ended))
    close_a, close_b = np.stack(ra.closes) != 0, np.stack(rb.closes) != 0
    kidx, honba, empty = np.stack(ra.kidx), np.stack(ra.honba), np.stack(rb.open_before) == 0
    assert np.array_equal(close_a, ended != 0)
    before = np.concatenate([ra.kidx0[None], kidx[:-1]])
    renchan = (ended == 1) & (kidx == before)                        # a round ended, the game goes on, kyoku_idx stayed
    differ = close_a != close_b
    assert renchan.sum() > 50, "no renchan occurred: the comparison proves nothing"
    assert not (close_b & ~close_a).any()                           # the worker's rule closes only where a round ended
    assert not (differ & ~(renchan | empty)).any()                  # they differ on renchan rounds (and where the hero never decided: nothing to close)
    assert (renchan & ~differ).sum() <= empty.astype(int)[ended != 0].sum()
    # round_track's meta tells that these were renchan: the round dealt there carries a honba counter (reported at the game's next boundary)
    seen = 0
    for s, g in np.argwhere(renchan & differ)[:2000]:
        later = np.flatnonzero(ended[s + 1:, g])
        if len(later):
            assert honba[s + 1 + later[0], g] >= 1, (s, g)
            seen += 1
    assert seen > 20
    assert ca.counts()["segments"] > cb.counts()["segments"]


def test_own_stream_without_share_stream_gives_the_same_pool():
    import torch

    n, steps = 1024, 150
    ea, ca, ra = _run(2, "base", "compact", n=n, steps=steps, seed=33)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eb, cb, rb = _run(2, "base", "compact", n=n, steps=steps, seed=33, share_stream=False)
        tb = cb.transitions()
    side.synchronize()
    ta = ca.transitions()
    assert ca.counts() == cb.counts() and ca.counts()["valid"] > 1000
    for key in ta:
        assert bool((ta[key] == tb[key]).all()), key
    assert not eb.shared


def test_ppo_example_runs():
    """examples/ppo_collect.py: one pool with a tiny conv policy"""
    import importlib.util

    path = os.path.join(ROOT, "examples", "ppo_collect.py")
    spec = importlib.util.spec_from_file_location("ppo_collect_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stats = mod.main(n=512, steps=200)
    assert stats["transitions"] > 0 and stats["kyokus"] > 0 and stats["overflowed"] == 0


def test_refused_arguments():
    import ctypes as C

    from riichienv_amd import vecenv
    from riichienv_amd.ppo import PPOCollector

    e = _env(5, "base", n=64)
    L = e.env.L
    h = C.c_void_p()
    for cfg in (abi.PpoConfig(abi.FEATURES_DISCARD_SHANTEN, 16, 0.99, 0.95), abi.PpoConfig(7, 16, 0.99, 0.95), abi.PpoConfig(abi.FEATURES_BASE, 0, 0.99, 0.95)):
        assert L.rmj_ppo_create(e.env.h, C.byref(cfg), C.byref(h)) == -1 and not h.value
    col = PPOCollector(e, 16)
    assert L.rmj_ppo_record_device(col.h, None, None, None, None, 60, None) == -1
    assert L.rmj_ppo_close_device(col.h, None, None) == -1
    assert L.rmj_ppo_emit_device(col.h, None) == -1
    wrong = abi.ObsBatch(abi.FEATURES_EXTENDED, 0, 0, 0, e._obs_buf.data_ptr(), None, None)
    x = col._ids.data_ptr()
    assert L.rmj_ppo_record_device(col.h, C.byref(wrong), x, x, x, 60, x) == -1
    with pytest.raises(vecenv.RmjError):
        vecenv._chk(L.rmj_select_ids_device(e.env.h, x, 10, 0, None, x))
    e.env.close()      # destroys the collector with the handle
    col.close()
