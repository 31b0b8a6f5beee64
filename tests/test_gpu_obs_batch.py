"""Observation batches (k_encode_batch: rmj_encode_batch_device, rmj_step_ids_encode_batch_device, rmj_step_sample_encode_batch_device and
TorchVecEnv(features=...)) held to the oracle.

Every feature set in both layouts, after uneven greedy rollout chunks and single steps of whole batches (seeded deals as in
tests/test_gpu_encode_extended.py, a nonzero game_offset, batches that are not a multiple of 4 and cross a scan block of 1 024 games):
  * compact rows byte-equal to the oracle: BASE = encode() (and rmj_encode_compact_device), EXTENDED = encode_extended(),
    DISCARD_SHANTEN = encode() rows 0..73 + encode_extended() rows 74..93 (78..93 constant along the columns);
  * index = the oracle's acting (game, seat) pairs, strictly increasing; count = their number;
  * dense rows of the acting seats = the compact rows, every other row keeps the sentinel fill bit for bit.
Then the edges (a short capacity, padded and refused strides, refused feature sets), the step entries against the unfused calls on a
clone, the torch layer against the C entries, and a HIP-graph capture of the extended compact loop."""
import ctypes as C

import numpy as np
import pytest

from riichienv_amd import abi, vecenv
from tests.test_gpu_encode_extended import _acting, seeded_conditions

pytestmark = pytest.mark.gpu

PSEED, RATE = 0xB47C, 96
CHUNKS = (1, 1, 43, 1, 97, 2, 1, 60)
OFFSET = 12289
SENT = np.float32(-3.5)
SENT_I = int(SENT.view(np.int32))
MODES = [(m, r) for m in (1, 2, 4, 5) for r in (abi.RULE_TENHOU, abi.RULE_MJSOUL)]


def _rule_name(rule):
    return "mjsoul" if rule == abi.RULE_MJSOUL else "tenhou"


def _sets(mode):
    return ["base", "extended"] + ([] if mode >= 3 else ["discard_shanten"])


def _want(name, base, ext):
    if name == "base":
        return base
    if name == "extended":
        return ext
    return np.concatenate([base, ext[:, 74:94]], axis=1)


def _first_difference(dev, want, idx, where):
    d, w = dev.reshape(len(dev), -1).view(np.uint32), want.reshape(len(want), -1).view(np.uint32)
    bad = np.nonzero((d != w).any(axis=1))[0]
    out = []
    for i in bad[:4]:
        e = int(np.nonzero(d[i] != w[i])[0][0])
        cw = want.shape[-1]
        out.append(f"row {i} (game {int(idx[i]) // 4} seat {int(idx[i]) % 4}) channel {e // cw} column {e % cw}: device "
                   f"{dev.reshape(len(dev), -1)[i, e]!r} oracle {want.reshape(len(want), -1)[i, e]!r}")
    return f"{where}: {len(bad)} rows differ; " + "; ".join(out)


class Buffers:
    """device buffers of one feature set on an environment that keeps its own stream: torch fills them on torch's stream, so every
    fill is followed by a device synchronisation before the library writes"""

    def __init__(self, torch, n, ch, w, row_stride=0, capacity=None):
        self.t = torch
        self.n, self.ch, self.w = n, ch, w
        self.rs = row_stride or ch * w
        self.cap = 4 * n if capacity is None else capacity
        dev = torch.device("cuda", 0)
        self.compact = torch.empty((max(self.cap, 1), self.rs), dtype=torch.float32, device=dev)
        self.index = torch.empty((max(self.cap, 1),), dtype=torch.int32, device=dev)
        self.count = torch.empty((1,), dtype=torch.int32, device=dev)
        self.dense = torch.empty((n, 4, self.rs), dtype=torch.float32, device=dev)

    def fill(self):
        self.compact.fill_(float(SENT))
        self.index.fill_(-7)
        self.count.fill_(-7)
        self.dense.fill_(float(SENT))
        self.t.cuda.synchronize()

    def args(self, compact):
        if compact:
            return dict(compact=True, d_index_ptr=self.index.data_ptr(), capacity=self.cap, d_count_ptr=self.count.data_ptr(),
                        row_stride=self.rs if self.rs != self.ch * self.w else 0)
        return dict(compact=False, row_stride=self.rs if self.rs != self.ch * self.w else 0)

    def rows(self, buf):
        return buf[..., : self.ch * self.w].unflatten(-1, (self.ch, self.w))


def _check_batch(torch, env, name, buf, games, seats, want, where, pads=False):
    """compact and dense outputs of one feature set against the oracle's rows `want` of the acting pairs (games, seats)"""
    k = len(games)
    want_idx = (games * 4 + seats).astype(np.int32)
    buf.fill()
    env.encode_batch_device(name, buf.compact.data_ptr(), **buf.args(True))
    env.encode_batch_device(name, buf.dense.data_ptr(), **buf.args(False))
    env.sync()
    assert int(buf.count.item()) == k, (where, name, "count", int(buf.count.item()), k)
    idx = buf.index.cpu().numpy()
    assert (idx[:k] == want_idx).all(), (where, name, "index", np.nonzero(idx[:k] != want_idx)[0][:8])
    assert (np.diff(idx[:k]) > 0).all(), (where, name, "index not strictly increasing")
    assert (idx[k:] == -7).all(), (where, name, "index entries behind the count were written")
    dev = torch.as_tensor(want, device=buf.compact.device)
    got = buf.rows(buf.compact[:k])
    if not torch.equal(got.view(torch.int32), dev.view(torch.int32)):
        pytest.fail(_first_difference(got.cpu().numpy(), want, want_idx, f"{where} {name} compact"))
    rest = buf.compact[k:].view(torch.int32)
    assert bool((rest == SENT_I).all()), (where, name, "compact rows behind the count were written")
    if pads:
        assert bool((buf.compact[:k, buf.ch * buf.w:].view(torch.int32) == SENT_I).all()), (where, name, "pad floats written (compact)")
        assert bool((buf.dense[..., buf.ch * buf.w:].view(torch.int32) == SENT_I).all()), (where, name, "pad floats written (dense)")
    dg, ds = torch.as_tensor(games, device=dev.device), torch.as_tensor(seats, device=dev.device)
    drows = buf.rows(buf.dense)
    assert torch.equal(drows[dg, ds].view(torch.int32), got.view(torch.int32)), (where, name, "dense acting rows differ from the compact rows")
    act = torch.zeros((buf.n, 4), dtype=torch.bool, device=dev.device)
    act[dg, ds] = True
    untouched = (drows[~act].view(torch.int32) == SENT_I).flatten(1).all(dim=1)
    assert bool(untouched.all()), (where, name, f"{int((~untouched).sum())} dense rows of seats that do not act were written")
    return got


def _status_equal(env, st, where):
    act, ph, dn = env.status()
    assert (act == st[:, 0]).all() and (ph == st[:, 1]).all() and (dn == st[:, 2]).all(), (where, "status")


@pytest.mark.parametrize("mode,rule", MODES, ids=[f"mode{m}-{_rule_name(r)}" for m, r in MODES])
def test_every_feature_set_and_layout_equals_the_oracle(mode, rule):
    import torch
    from oracle import oracle

    n = 4097 if (mode, rule) == (2, abi.RULE_TENHOU) else 1027
    seed = 9100 + 10 * mode + (rule == abi.RULE_MJSOUL)
    sanma = mode >= 3
    np_, w = (3, 27) if sanma else (4, 34)
    args = seeded_conditions(mode, n)
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, rule_bits=rule, game_offset=OFFSET, skip_mjai_logging=True)
    own = args["walls"][:, 0] != 255
    env.reset(select=~own, oya=args["oya"])
    env.reset(select=own, walls=args["walls"], oya=args["oya"])
    b = oracle.Batch(mode, rule, seed, n, game_offset=OFFSET, **args)
    bufs = {s: Buffers(torch, n, abi.FEATURE_CHANNELS[abi.FEATURES[s]], w) for s in _sets(mode)}
    ref = Buffers(torch, n, 74, w)
    claims, rows = 0, 0
    for k, c in enumerate(CHUNKS):
        where = f"mode{mode}-{_rule_name(rule)} chunk {k}"
        env.step_greedy(PSEED, c, auto_reset=True, call_rate_256=RATE)
        b.step("greedy", PSEED, c, call_rate_256=RATE)
        st = b.status()
        _status_equal(env, st, where)
        acting = _acting(st, np_)
        claims += int((acting.sum(axis=1) >= 2).sum())
        games, seats = np.nonzero(acting)
        base, ext = b.encode(games, seats), b.encode_extended(games, seats)
        for s in _sets(mode):
            want = _want(s, base, ext)
            got = _check_batch(torch, env, s, bufs[s], games, seats, want, where)
            if s == "discard_shanten":
                g = got[:, 78:94]
                assert bool((g == g[:, :, :1]).all()), (where, "rows 78..93 are not constant along the columns")
            if s == "base":   # the existing compact encoder writes the same rows
                ref.fill()
                env.encode_compact_device(ref.compact.data_ptr(), ref.index.data_ptr(), ref.cap, ref.count.data_ptr())
                env.sync()
                assert torch.equal(ref.rows(ref.compact[: len(games)]).view(torch.int32), got.view(torch.int32)), (where, "rmj_encode_compact_device")
        rows += len(games)
    print(f"\nmode{mode}-{_rule_name(rule)}: {n} games, {rows} acting rows x {len(_sets(mode))} feature sets compared, "
          f"{claims} game states with two or more acting seats")
    assert claims > 0, "no compared state had a game with two or more acting seats"
    env.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_edges_capacity_stride_and_refusals(mode):
    import torch
    from oracle import oracle

    n, seed = 1029, 9300 + mode
    w = 27 if mode >= 3 else 34
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=seed, game_offset=OFFSET, skip_mjai_logging=True)
    env.reset()
    b = oracle.Batch(mode, abi.RULE_TENHOU, seed, n, game_offset=OFFSET)
    env.step_greedy(PSEED, 37, auto_reset=True, call_rate_256=RATE)
    b.step("greedy", PSEED, 37, call_rate_256=RATE)
    st = b.status()
    _status_equal(env, st, "edges")
    games, seats = np.nonzero(_acting(st, 3 if mode >= 3 else 4))
    base, ext = b.encode(games, seats), b.encode_extended(games, seats)
    k = len(games)
    for s in _sets(mode):
        ch = abi.FEATURE_CHANNELS[abi.FEATURES[s]]
        want = _want(s, base, ext)
        # a padded stride: rows equal, pad floats untouched
        pad = Buffers(torch, n, ch, w, row_stride=(ch * w + 1) // 2 * 2 + 6)
        _check_batch(torch, env, s, pad, games, seats, want, f"mode{mode} stride {pad.rs}", pads=True)
        # a capacity below the batch: exactly `cap` rows, the count is the full number
        cap = k // 3
        short = Buffers(torch, n, ch, w, capacity=cap)
        short.fill()
        env.encode_batch_device(s, short.compact.data_ptr(), **short.args(True))
        env.sync()
        assert int(short.count.item()) == k
        assert torch.equal(short.rows(short.compact[:cap]).view(torch.int32), torch.as_tensor(want[:cap], device="cuda").view(torch.int32))
        assert (short.index[:cap].cpu().numpy() == (games * 4 + seats)[:cap]).all()
        assert bool((short.compact[cap:].view(torch.int32) == SENT_I).all()) and bool((short.index[cap:] == -7).all())
        # refused strides: odd, below C x W
        dense = ch * w
        for bad in (dense + 1 + dense % 2, (dense - 1) // 2 * 2, 2):   # odd; even but below C x W; tiny
            with pytest.raises(vecenv.RmjError, match="row stride"):
                env.encode_batch_device(s, short.compact.data_ptr(), **dict(short.args(True), row_stride=bad))
        if (ch * w) % 2:   # 215 x 27: the dense stride is odd - only the default (0) may name it
            with pytest.raises(vecenv.RmjError, match="row stride"):
                env.encode_batch_device(s, short.compact.data_ptr(), **dict(short.args(True), row_stride=ch * w))
        with pytest.raises(vecenv.RmjError, match="null"):
            env.encode_batch_device(s, 0, **short.args(True))
        with pytest.raises(vecenv.RmjError, match="null"):
            env.encode_batch_device(s, short.compact.data_ptr(), compact=True, d_index_ptr=None, capacity=cap, d_count_ptr=short.count.data_ptr())
        # the host-copy entry returns the same rows
        hrows, hidx = env.encode_batch(s, compact=True)
        assert hrows.view(np.uint32).tobytes() == want.view(np.uint32).tobytes() and (hidx == games * 4 + seats).all()
        drows, didx = env.encode_batch(s, compact=False)
        assert (didx == hidx).all() and drows[games, seats].view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    with pytest.raises(vecenv.RmjError, match="unknown feature set"):
        env.encode_batch_device(7, short.compact.data_ptr(), **short.args(False))
    if mode >= 3:
        with pytest.raises(vecenv.RmjError, match="4-player only"):
            env.encode_batch_device(abi.FEATURES_DISCARD_SHANTEN, short.compact.data_ptr(), **short.args(False))
        ids = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
        before = env.step_counts().copy()
        with pytest.raises(vecenv.RmjError, match="4-player only"):
            env.step_ids_encode_batch_device(ids.data_ptr(), abi.FEATURES_DISCARD_SHANTEN, short.compact.data_ptr())
        assert (env.step_counts() == before).all(), "a refused call stepped the games"
    env.close()


@pytest.mark.parametrize("mode", [2, 5])
def test_step_entries_equal_step_then_encode_on_a_clone(mode):
    import torch

    n = 1029
    w = 27 if mode >= 3 else 34
    a = vecenv.VecRiichiEnv(n, game_mode=mode, seed=9500 + mode, game_offset=OFFSET, skip_mjai_logging=True)
    a.reset()
    a.step_random(5, 20, auto_reset=True)
    b = a.clone()
    dev = torch.device("cuda", 0)
    logits = torch.randn((n, 4, 82), device=dev, dtype=torch.float32).contiguous()
    ids_a = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    ids_b = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    sets = _sets(mode)
    ba = {s: Buffers(torch, n, abi.FEATURE_CHANNELS[abi.FEATURES[s]], w) for s in sets}
    bb = {s: Buffers(torch, n, abi.FEATURE_CHANNELS[abi.FEATURES[s]], w) for s in sets}
    L = a.L
    for step in range(60):
        s = sets[step % len(sets)]
        compact = (step // len(sets)) % 2 == 0
        x, y = ba[s], bb[s]
        x.fill()
        y.fill()
        out_a, out_b = (x.compact, y.compact) if compact else (x.dense, y.dense)
        seed = 1000 + step
        lg = logits if step % 3 else None
        if step % 2 == 0:   # ids: sampled on A, the same ids into both
            vecenv._chk(L.rmj_sample_ids_device(a.h, None if lg is None else C.c_void_p(lg.data_ptr()), 82 if lg is not None else 0, seed,
                                                C.c_void_p(ids_a.data_ptr())))
            a.sync()
            vecenv._chk(L.rmj_step_ids_device(a.h, C.c_void_p(ids_a.data_ptr()), 1))
            a.encode_batch_device(s, out_a.data_ptr(), **x.args(compact))
            b.step_ids_encode_batch_device(ids_a.data_ptr(), s, out_b.data_ptr(), auto_reset=True, **y.args(compact))
            ids_b.copy_(ids_a)
        else:
            vecenv._chk(L.rmj_sample_ids_device(a.h, None if lg is None else C.c_void_p(lg.data_ptr()), 82 if lg is not None else 0, seed,
                                                C.c_void_p(ids_a.data_ptr())))
            vecenv._chk(L.rmj_step_ids_device(a.h, C.c_void_p(ids_a.data_ptr()), 1))
            a.encode_batch_device(s, out_a.data_ptr(), **x.args(compact))
            b.step_sample_encode_batch_device(None if lg is None else lg.data_ptr(), 82 if lg is not None else 0, seed, ids_b.data_ptr(), s,
                                              out_b.data_ptr(), auto_reset=True, **y.args(compact))
        a.sync()
        b.sync()
        torch.cuda.synchronize()
        where = f"mode{mode} step {step} {s} {'compact' if compact else 'dense'}"
        assert torch.equal(ids_a, ids_b), where
        assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)), where
        if compact:
            assert torch.equal(x.index, y.index) and torch.equal(x.count, y.count), where
            assert int(x.count.item()) > 0, where
        assert (a.step_counts() == b.step_counts()).all(), where
    for g in range(n):
        assert bytes(a.peek(g)) == bytes(b.peek(g)), ("state", g)
    a.close()
    b.close()


def _acting_rows(e):
    act = e.active().cpu().numpy()
    g, s = np.nonzero(act)
    return g, s


@pytest.mark.parametrize("mode,features", [(2, "base"), (2, "discard_shanten"), (2, "extended"), (5, "base"), (5, "extended")])
def test_torch_env_feature_sets_equal_the_c_entries(mode, features):
    import torch
    from riichienv_amd.torch_env import GymVectorAdapter, TorchVecEnv

    n = 517
    e = TorchVecEnv(n, game_mode=mode, seed=9700 + mode, features=features, game_offset=OFFSET)
    ch, w = abi.FEATURE_CHANNELS[abi.FEATURES[features]], (27 if mode >= 3 else 34)
    assert (e.channels, e.width) == (ch, w) and e.extended == (features == "extended")

    def want():
        torch.cuda.synchronize()
        return e.env.encode_batch(features, compact=True)

    def same(got, idx, where):
        rows, widx = want()
        assert got.shape[1:] == (ch, w), where
        assert (idx == widx).all(), (where, "index")
        assert got.view(np.uint32).tobytes() == rows.view(np.uint32).tobytes(), (where, "rows")

    def dense_same(obs, where):
        torch.cuda.synchronize()
        g, s = _acting_rows(e)
        same(obs[torch.as_tensor(g, device="cuda"), torch.as_tensor(s, device="cuda")].cpu().numpy(), (g * 4 + s).astype(np.int32), where)

    for r in range(8):
        o, i = e.obs_compact()
        same(o.cpu().numpy(), i.cpu().numpy(), f"round {r} obs_compact")
        dense_same(e.obs(only_active=True), f"round {r} obs")
        dense_same(e.step_obs(e.sample_ids(None, seed=10 * r + 1)), f"round {r} step_obs")
        ids, obs = e.step_sample_obs(None, seed=10 * r + 2)
        dense_same(obs, f"round {r} step_sample_obs")
        o, i = e.step_obs_compact(e.sample_ids(None, seed=10 * r + 3))
        same(o.cpu().numpy(), i.cpu().numpy(), f"round {r} step_obs_compact")
        ids, o, i = e.step_sample_obs_compact(None, seed=10 * r + 4)
        assert ids.shape == (n, 4)
        same(o.cpu().numpy(), i.cpu().numpy(), f"round {r} step_sample_obs_compact")
        obs, reward, term, info = e.step_rl(e.sample_ids(None, seed=10 * r + 5))
        assert obs is not None
        dense_same(obs, f"round {r} step_rl")
    full, idx, cnt = e.step_obs_compact(e.sample_ids(None, seed=99), sync_count=False)
    k = int(cnt.item())
    same(full[:k].cpu().numpy(), idx[:k].cpu().numpy(), "sync_count=False")
    # a capacity below the batch grows on demand and re-encodes the same state
    e._cobs = None
    o, i = e.obs_compact(capacity=2)
    assert e._cap >= len(i) > 2
    same(o.cpu().numpy(), i.cpu().numpy(), "grown")
    gym = GymVectorAdapter(e)
    assert gym.single_observation_shape["features"] == (ch, w) and gym.features == features
    obs, _info = gym.reset(seed=1)
    assert tuple(obs["features"].shape) == (n, ch, w)


def test_extended_compact_loop_inside_a_hip_graph():
    """sample_ids + step_obs_compact (extended, sync_count=False) captured once on a side stream and replayed: the same games, rows,
    index and count as the eager loop of a twin environment"""
    import torch
    from riichienv_amd.torch_env import TorchVecEnv

    n, per_graph, replays = 1024, 4, 10

    def iteration(e, k):
        return e.step_obs_compact(e.sample_ids(None, seed=5 + k), sync_count=False)

    a = TorchVecEnv(n, game_mode=2, seed=91, features="extended", share_stream=True)
    b = TorchVecEnv(n, game_mode=2, seed=91, features="extended", share_stream=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a.bind_stream()
        iteration(a, 0)                      # warm-up on the capture stream: the buffers exist before the capture
    iteration(b, 0)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for k in range(per_graph):
            iteration(a, k)
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    a.bind_stream(torch.cuda.current_stream())
    for _ in range(replays):
        for k in range(per_graph):
            iteration(b, k)
    torch.cuda.synchronize()
    assert (a.env.step_counts() == b.env.step_counts()).all()
    ka, kb = int(a._ccnt.item()), int(b._ccnt.item())
    assert ka == kb and ka > 0
    assert torch.equal(a._cidx[:ka], b._cidx[:kb])
    assert torch.equal(a._cobs[:ka].view(torch.int32), b._cobs[:kb].view(torch.int32))
