"""GPU: the GRP rank model's rows, labels and rewards built on the device (rmj_grp_rows_device, rmj_logset_grp_device,
riichienv_amd.grp: grp_rows, GrpDataset, DeviceRewardPredictor) against the plain restatement tests/grp_ref.py.  Every comparison of x
is on the int32 bit patterns, equal everywhere."""
import ctypes as C
import json

import numpy as np
import pytest

from riichienv_amd import abi, datasets, grp, vecenv
from tests import grp_ref as R

pytestmark = pytest.mark.gpu
_GAMES = {}


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _mlp(n, seed):
    """the shape of riichienv-ml's rank model: Linear 4n+4 -> 128 -> 64 -> n"""
    torch, dev = _torch()
    torch.manual_seed(seed)
    nn = torch.nn
    return nn.Sequential(nn.Linear(4 * n + 4, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, n)).to(dev).eval()


# ------------------------------------------------------------------ the pure entry
@pytest.mark.parametrize("n", [4, 3])
def test_pure_rows_on_the_sweep_and_the_extremes(n):
    torch, dev = _torch()
    init, delta, meta = R.sweep_case()
    end = [[a + b for a, b in zip(i, d)] for i, d in zip(init, delta)]
    want = R.bits(R.rows(init, end, meta, n))
    ti, td, tm = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (init, delta, meta))
    got = grp.live_rows(ti, td, tm, n).cpu().numpy()
    assert got.shape == (len(init), n, 4 * n + 4)
    bad = np.argwhere(R.bits(got) != want)
    assert not len(bad), f"{len(bad)} values differ in bits, first at {bad[:4].tolist()}"
    # every row count around a wave and the kernel's block (256 threads), each into a buffer with guard words behind it
    for rows in (1, 63, 64, 65, 257):
        f = n * (4 * n + 4)
        buf = torch.full((rows * f + 64,), -7.0, dtype=torch.float32, device=dev)
        off = 300
        grp.live_rows(ti[off: off + rows], td[off: off + rows], tm[off: off + rows], n, out=buf[: rows * f].view(rows, n, 4 * n + 4))
        h = buf.cpu().numpy()
        assert np.array_equal(R.bits(h[: rows * f]).reshape(rows, n, 4 * n + 4), want[off: off + rows]), rows
        assert (h[rows * f:] == -7.0).all(), rows
    assert grp.live_rows(ti[:0], td[:0], tm[:0], n).shape == (0, n, 4 * n + 4)


# ------------------------------------------------------------------ the log-set entry on hand-made logs
def _hand_made(seats):
    S = 35000 if seats == 3 else 25000
    pad = [0] * (seats - 3)

    def sc(*v):
        return list(v) + [S] * (seats - 3)

    logs = [
        [{"type": "start_game"}, {"type": "end_game"}],                                                       # no kyoku
        R.hand_made_log([(dict(scores=sc(S, S, S)), ("hora", 0, 1, [8000, -8000, 0] + pad))], seats),         # one kyoku
        R.hand_made_log([(dict(scores=sc(S, S, S)), ("ryukyoku", [1500, -1500, 0] + pad)),                    # the last kyoku has no end scores
                         (dict(scores=sc(S + 1500, S - 1500, S), kyoku=2), None)], seats, end_game=False),
        R.hand_made_log([(dict(scores=sc(S, S, S), kyoku=0), ("hora", 1, 1, [-2000, 4000, -2000] + pad))], seats),       # ju = -1
        R.hand_made_log([(dict(scores=sc(S, S, S), kyotaku=300, honba=255, key="kyoutaku"), ("hora", 2, 0, [-1000, 0, 1000] + pad))], seats),
        R.hand_made_log([(dict(scores=sc(S, S, S), bakaze="W", kyoku=3), ("hora", 2, 0, [-1000, 0, 1000] + pad)),
                         (dict(scores=sc(S - 1000, S, S + 1000), bakaze="N", kyoku=4, oya=2), ("reach_hora", 2, 2, [-500, -500, 1000] + pad))], seats),
        R.hand_made_log([(dict(scores=sc(S, S, S)), ("ryukyoku", [0] * seats))], seats),                       # all equal
        R.hand_made_log([(dict(scores=sc(S - 100, S + 100, S + 100)), ("hora_scores", 0, 1, sc(S + 100, S - 100, S + 100)))], seats),   # pairwise ties
        R.hand_made_log([(dict(scores=sc(-32000, 100, 2 * S + 31900)), ("hora", 1, 0, [-48000, 48000, 0] + pad))], seats),   # negative scores
    ]
    long_log = R.hand_made_log([(dict(scores=sc(S, S, S)), ("hora", 0, 1, [1000, -1000, 0] + pad)), (dict(scores=sc(S + 1000, S - 1000, S), kyoku=2), None)], seats)
    filler = [ev for _ in range(90) for ev in ({"type": "tsumo", "actor": 1, "pai": "3p"}, {"type": "dahai", "actor": 1, "pai": "3p", "tsumogiri": True})]
    logs.append(long_log[:3] + filler + long_log[3:])                                                          # a kyoku of three 64-event tiles
    return logs + R.random_logs(300, seats, seed=17 + seats)


def _text(logs):
    return [("\n".join(json.dumps(ev) for ev in log) + "\n").encode() for log in logs]


def _assert_rows(got, ref, what):
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g["kyoku_offsets"].tolist() == ref["kyoku_offsets"].tolist(), what
    assert np.array_equal(g["meta"], ref["meta"]), (what, np.argwhere(g["meta"] != ref["meta"])[:4].tolist())
    assert g["rank"].dtype == np.uint8 and np.array_equal(g["rank"], ref["rank"]), (what, np.argwhere(g["rank"] != ref["rank"])[:4].tolist())
    assert np.array_equal(g["log_of"], ref["log_of"]), what
    bad = np.argwhere(R.bits(g["x"]) != R.bits(ref["x"]))
    assert g["x"].shape == ref["x"].shape and not len(bad), (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("seats,mode", [(4, 2), (3, 5)])
def test_logset_rows_of_hand_made_logs(seats, mode):
    logs = _hand_made(seats)
    ref = R.logset_rows(logs, seats)
    K = len(ref["meta"])
    assert K > 1500 and ref["x"].shape == (K, seats, 4 * seats + 4)           # the table crosses many blocks and waves
    assert ref["kyoku_offsets"][1] == 0 and (ref["meta"][:, 1] == -1).any() and (ref["meta"][:, 3] == 300).any() and (ref["end"] < 0).any()
    texts = _text(logs)
    sources = {"GrpDataset.from_text": grp.GrpDataset.from_text(texts, game_mode=mode), "GrpDataset(dicts)": grp.GrpDataset(logs, game_mode=mode),
               "builder.from_text": datasets.LogSampleBuilder.from_text(texts, game_mode=mode), "builder(dicts)": datasets.LogSampleBuilder(logs, game_mode=mode)}
    for what, src in sources.items():
        _assert_rows(src.grp_rows(), ref, what)
        _assert_rows(grp.grp_rows(src), ref, what)
        src.close()
    # the logs given by ranges in reverse order
    whole = b"".join(texts)
    ends = np.cumsum([len(t) for t in texts])
    ranges = np.stack([ends - [len(t) for t in texts], ends], axis=1)[::-1].copy()
    ds = grp.GrpDataset.from_text(whole, ranges=ranges, game_mode=mode)
    _assert_rows(ds.grp_rows(), R.logset_rows(logs[::-1], seats), "reversed ranges")
    # tensors(): every (kyoku, seat) row in order, one-hot labels
    s = {k: v.cpu().numpy() for k, v in ds.tensors().items()}
    rr = R.logset_rows(logs[::-1], seats)
    assert np.array_equal(R.bits(s["x"]), R.bits(rr["x"]).reshape(K * seats, -1)) and np.array_equal(s["rank"], rr["rank"].reshape(-1))
    assert np.array_equal(s["y"], np.eye(seats, dtype=np.float32)[rr["rank"].reshape(-1)])
    assert np.array_equal(s["log"], np.repeat(rr["log_of"], seats)) and np.array_equal(s["seat"], np.tile(np.arange(seats), K))
    ds.close()


def test_a_log_that_does_not_parse_gets_rank_255_and_its_neighbours_are_untouched():
    logs = _hand_made(4)[:40]
    texts = _text(logs)
    spoil = 20
    lines = texts[spoil].split(b"\n")
    at = next(i for i, ev in enumerate(logs[spoil]) if ev["type"] == "tsumo")
    lines[at] = lines[at][: len(lines[at]) // 2]
    texts[spoil] = b"\n".join(lines)
    as_dicts = list(logs)
    as_dicts[spoil] = [ev if i != at else {"type": "none"} for i, ev in enumerate(logs[spoil])]
    ref = R.logset_rows(as_dicts, 4, bad={spoil})
    assert (ref["rank"] == 255).any()
    with pytest.raises(ValueError, match=rf"log {spoil}: line {at + 1}: ERR_JSON"):
        grp.GrpDataset.from_text(texts, game_mode=2)
    ds = grp.GrpDataset.from_text(texts, game_mode=2, on_error="drop")
    assert ds.dropped == [(spoil, at + 1, "ERR_JSON")]
    _assert_rows(ds.grp_rows(), ref, "spoiled")
    s = {k: v.cpu().numpy() for k, v in ds.tensors().items()}
    keep = (ref["rank"] != 255).reshape(-1)
    assert keep.sum() == len(s["x"]) and spoil not in s["log"] and np.array_equal(R.bits(s["x"]), R.bits(ref["x"]).reshape(len(keep), -1)[keep])
    ds.close()


def test_refused_arguments():
    torch, dev = _torch()
    L = vecenv.load_lib()
    logs = _hand_made(4)[:6]
    ds = grp.GrpDataset(logs, game_mode=2)
    K = ds.n_kyokus
    meta = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    x = torch.zeros((K, 4, 20), dtype=torch.float32, device=dev)
    o = abi.GrpOut(meta.data_ptr(), x.data_ptr(), None, None)
    assert L.rmj_logset_grp_device(ds.logset.handle, 4, None, None, C.byref(o), None) == -1          # a host-packed set has no score tables
    assert L.rmj_logset_grp_device(ds.logset.handle, 5, meta.data_ptr(), meta.data_ptr(), C.byref(o), None) == -1
    assert L.rmj_logset_grp_device(None, 4, None, None, C.byref(o), None) == -1
    assert L.rmj_grp_rows_device(0, meta.data_ptr(), meta.data_ptr(), meta.data_ptr(), K, 2, x.data_ptr(), None) == -1
    assert L.rmj_grp_rows_device(0, None, meta.data_ptr(), meta.data_ptr(), K, 4, x.data_ptr(), None) == -1
    assert L.rmj_grp_rows_device(0, meta.data_ptr() + 4, meta.data_ptr(), meta.data_ptr(), 1, 4, x.data_ptr(), None) == -1
    with pytest.raises(TypeError):
        grp.GrpDataset(logs, game_mode=2, no_such_argument=1)
    ds.close()


# ------------------------------------------------------------------ whole games
def _games(mode, n=256):
    """n device-played games of `mode`: (the TorchVecEnv that keeps the text alive, text uint8 and offsets int64 on the device, the logs
    as lists of dicts parsed with json.loads)"""
    if mode not in _GAMES:
        from riichienv_amd.torch_env import TorchVecEnv

        tenv = TorchVecEnv(n, game_mode=mode, seed=51 + mode, skip_mjai_logging=False, event_ring=8192)
        env = tenv.env
        env.reset()
        for _ in range(40):
            env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
            if env.status()[2].all():
                break
        assert env.status()[2].all() and int(env.events_lost().sum()) == 0
        text, offs = tenv.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
        text, offs = text.clone(), offs.clone()
        raw, o = text.cpu().numpy().tobytes(), offs.cpu().tolist()
        texts = [raw[o[g]: o[g + 1]] for g in range(n)]
        logs = [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in texts]
        env.close()
        _GAMES[mode] = (text, offs, texts, logs)
    return _GAMES[mode]


@pytest.mark.parametrize("mode", [2, 5])
def test_whole_games_from_device_text(mode):
    torch, dev = _torch()
    n = 3 if mode >= 3 else 4
    text, offs, texts, logs = _games(mode)
    ref = R.logset_rows(logs, n)
    K = len(ref["meta"])
    assert K >= 256 * 4
    ds = grp.GrpDataset.from_device_text(text, offs, game_mode=mode)
    _assert_rows(ds.grp_rows(), ref, ("device text", mode))
    s = ds.tensors()
    assert np.array_equal(R.bits(s["x"].cpu().numpy()), R.bits(ref["x"]).reshape(K * n, -1))
    assert np.array_equal(s["y"].cpu().numpy(), np.eye(n, dtype=np.float32)[ref["rank"].reshape(-1)])
    # one epoch of batches is a permutation of tensors()
    gen = torch.Generator().manual_seed(4)
    got = [(x, y) for x, y in ds.batches(1000, generator=gen)]
    assert all(x.shape[0] == 1000 and x.dtype == torch.float32 and y.shape == (1000, n) for x, y in got[:-1]) and 0 < got[-1][0].shape[0] <= 1000
    rows = np.concatenate([np.concatenate([x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32)], axis=1) for x, y in got])
    full = np.concatenate([s["x"].cpu().numpy().view(np.int32), s["y"].cpu().numpy().view(np.int32)], axis=1)
    assert rows.shape == full.shape and not np.array_equal(rows, full)
    assert np.array_equal(rows[np.lexsort(rows.T)], full[np.lexsort(full.T)])
    plain = [x for x, _ in ds.batches(1 << 20, shuffle=False)]
    assert len(plain) == 1 and torch.equal(plain[0], s["x"])
    ds.close()


# ------------------------------------------------------------------ DeviceRewardPredictor
def _restate_returns(s, rewards, koff, gamma):
    T = {}
    for l, k, seat in zip(s["log"], s["kyoku"], s["seat"]):
        T[(l, k, seat)] = T.get((l, k, seat), 0) + 1
    return [float(rewards[int(koff[l]) + k - 1][seat]) * (gamma ** (T[(l, k, seat)] - int(t) - 1)) for l, k, seat, t in zip(s["log"], s["kyoku"], s["seat"], s["t"])]


@pytest.mark.parametrize("mode", [2, 5])
def test_kyoku_rewards_equal_the_formula_and_feed_finalize(mode):
    torch, dev = _torch()
    n = 3 if mode >= 3 else 4
    _text_d, _offs, texts, logs = _games(mode)
    texts, logs = texts[:32], logs[:32]
    ref = R.logset_rows(logs, n)
    K = len(ref["meta"])
    model = _mlp(n, 11)
    pts = [10.0, 4.0, -4.0, -10.0] if n == 4 else [10.0, 0.5, -10.0]
    pred = grp.DeviceRewardPredictor(model, pts, num_players=n)
    gamma = 0.97
    b = datasets.LogSampleBuilder.from_text(texts, game_mode=mode, gamma=gamma)
    got = pred.kyoku_rewards(b)
    assert got.dtype == torch.float64 and tuple(got.shape) == (K, 4) and got.is_cuda
    with torch.inference_mode():
        x = torch.from_numpy(ref["x"]).to(dev).reshape(K * n, 4 * n + 4)
        want = torch.softmax(model(x), dim=1) @ torch.tensor(pts, device=dev).float() - float(np.mean(pts))
    assert torch.equal(got[:, :n], want.reshape(K, n).to(torch.float64))
    if n == 3:
        assert bool((got[:, 3] == 0).all())
    assert float(got.abs().max()) > 0.01
    b.run()
    b.finalize(got)
    s = {k: v.cpu().numpy() for k, v in b.samples().items()}
    assert len(s["action"]) > 1000 and b.counts()["overflowed"] == 0
    table = got.cpu().numpy()
    want_ret = np.array(_restate_returns(s, table, b.kyoku_offsets, gamma), dtype=np.float64)
    assert s["return64"].tobytes() == want_ret.tobytes()
    assert s["return"].tobytes() == want_ret.astype(np.float32).tobytes()
    b.close()


# ------------------------------------------------------------------ the live path: PPOCollector's reward_fn
@pytest.mark.parametrize("mode", [2, 5])
def test_reward_fn_follows_the_opening_scores_through_game_ends(mode):
    from riichienv_amd.ppo import PPOCollector
    from riichienv_amd.torch_env import TorchVecEnv

    torch, dev = _torch()
    n, games, steps = (3 if mode >= 3 else 4), 64, 300
    tenv = TorchVecEnv(games, game_mode=mode, seed=7, features="base")
    tenv.env.step_random(policy_seed=9, n_steps=700, auto_reset=True)        # the games stand anywhere in their course: some end inside the run
    col = PPOCollector(tenv, games * steps, seed=3)
    A = col.A
    gen = torch.Generator(device=dev).manual_seed(5)

    def policy(obs):
        return torch.randn((obs.shape[0], A), generator=gen, device=dev) * 3.0, torch.randn((obs.shape[0],), generator=gen, device=dev)

    def baseline(obs):
        return torch.randn((obs.shape[0], A), generator=gen, device=dev)

    model = _mlp(n, 23)
    pts = [10.0, 4.0, -4.0, -10.0] if n == 4 else [10.0, 0.0, -10.0]
    pred = grp.DeviceRewardPredictor(model, pts, num_players=n)
    fn = pred.reward_fn(tenv)
    opening = tenv.scores().cpu().numpy().astype(np.int64).copy()
    rec = []
    col.collect(policy, baseline, steps, reward_fn=fn, on_step=lambda d: rec.append({k: d[k].cpu().numpy().copy() for k in ("ended", "delta", "meta", "reward")})
                if d["phase"] == "close" else None)
    hero = col.hero.cpu().numpy()
    fresh = np.array([(35000 if n == 3 else 25000)] * n + [0] * (4 - n), dtype=np.int64)
    # the walk: every game's opening scores by the same rule, the restatement's row of the hero, the same model on a batch of the same shape
    open_ = opening.copy()
    ended_once = np.zeros(games, bool)
    closes = after_restart = 0
    for s, d in enumerate(rec):
        ended, delta, meta = d["ended"], d["delta"].astype(np.int64), d["meta"]
        if not ended.any():
            assert not d["reward"].any(), s
            continue
        hx = np.stack([R.row(open_[g], open_[g] + delta[g], meta[g], n, min(int(hero[g]), n - 1)) for g in range(games)]).astype(np.float32)
        with torch.inference_mode():
            r = torch.softmax(model(torch.from_numpy(hx).to(dev)), dim=1) @ torch.tensor(pts, device=dev).float() - float(np.mean(pts))
        want = np.where(ended != 0, r.cpu().numpy(), np.float32(0))
        assert np.array_equal(R.bits(d["reward"]), R.bits(want)), (s, np.flatnonzero(R.bits(d["reward"]) != R.bits(want))[:4].tolist())
        closes += int((ended != 0).sum())
        after_restart += int(((ended != 0) & ended_once).sum())
        for g in np.flatnonzero(ended):
            open_[g] = fresh if ended[g] == 2 else open_[g] + delta[g]
        ended_once |= ended == 2
    assert closes > games and int(ended_once.sum()) > 0 and after_restart > 0, (closes, int(ended_once.sum()), after_restart)
    assert np.array_equal(fn.open.cpu().numpy(), open_)
    col.close()


def test_the_example_runs():
    """examples/grp_from_text.py: text -> GrpDataset -> a few optimiser steps -> kyoku_rewards -> finalize -> one batch"""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "grp_from_text.py")
    spec = importlib.util.spec_from_file_location("grp_from_text_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(games=32, steps=10)
    assert out["grp_rows"] == out["kyokus"] * 4 and out["samples"] > 1000 and out["batch"][0] == 256 and np.isfinite(out["loss"])
    assert 0 < out["target_abs_max"] < 10.0       # |reward| <= max |pts_weight - mean|: the returns come from the model, not from score changes
