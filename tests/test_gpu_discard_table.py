"""Discard efficiency table (csrc/rmj_dtable.hip.h: rmj_discard_table_hands, rmj_discard_table(_device), LogSampleBuilder(efficiency=True),
riichienv_amd.efficiency) against the host yardstick tests/discard_table_ref.py (numpy over oracle.shanten): the raw entry on sampled
histograms, the live entry on the device's own state, the extended features' channels 78..80 as an independent device path, the
builder's rows against an oracle replay of the same logs, and best_discard against its plain-Python counterpart."""
import json
import os

import numpy as np
import pytest

from riichienv_amd import abi
from tests import discard_table_ref as D
from tests import log_check_ref
from tests import shanten_sampler as S
from tests.test_discard_table_ref import sampled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "126_204_0_mjai.jsonl")
STOPS = (40, 120, 200, 300)
# base seeds at which 8 games reach every coverage condition of the live test by step 300 (policy seed 5, call rate 64): found on the
# CPU by stepping oracle.Batch under the policies' twins and applying the yardstick
SEEDS = {(2, "greedy"): 3, (2, "random"): 203, (5, "greedy"): 2, (5, "random"): 62}
_LIVE, _BUILT = {}, {}


def _same(got, want, what):
    for f in D.FIELDS:
        g = got[f].view(np.uint64) if f == "mask" else got[f]
        assert g.dtype == want[f].dtype and g.shape == want[f].shape, (what, f, g.dtype, g.shape)
        bad = np.flatnonzero((g != want[f]).any(axis=1))
        assert bad.size == 0, (what, f, bad.size, bad[:4].tolist(), g[bad[:2]].tolist(), want[f][bad[:2]].tolist())


# ---------------------------------------------------------------- 1. the raw entry
@pytest.mark.parametrize("sanma", [False, True])
def test_raw_entry_equals_the_yardstick(sanma):
    from riichienv_amd import vecenv

    hands, vis, want = sampled(sanma)
    bare = D.table(hands, None, sanma)
    for n in (1, 4, 5, 256):                      # four waves share a block: 5 is the tail
        _same(vecenv.discard_table(hands[:n], vis[:n], sanma), {f: want[f][:n] for f in D.FIELDS}, f"n = {n}, visible")
        _same(vecenv.discard_table(hands[:n], None, sanma), {f: bare[f][:n] for f in D.FIELDS}, f"n = {n}, nothing visible")
    assert vecenv.discard_table(hands[:4], vis[:4], sanma)["mask"].dtype == np.uint64


def test_raw_entry_absent_rows_and_sanma_histograms_with_manzu():
    from riichienv_amd import vecenv

    odd = np.zeros((5, 34), np.uint8)
    odd[0, :15] = 1                               # 15 tiles
    odd[1, 3] = 5                                 # a count of 5
    odd[2, :14] = 1
    odd[3, 9] = 255                               # a count whose low bits look like 7
    odd[4, 27:34] = 2                             # 14 tiles next to them
    for sanma in (False, True):
        got = vecenv.discard_table(odd, None, sanma)
        _same(got, D.table(odd, None, sanma), f"odd rows, sanma {sanma}")
        assert (got["shanten"][[0, 1, 3]] == abi.DTAB_NONE).all() and (got["shanten"][[2, 4], 34] != abi.DTAB_NONE).all()
    # raw 3P histograms that hold 2m..8m: the sampler's 4P hands fed as 3P
    hands = S.sample_hands(11, 24, False)
    vis = np.array([S.sample_visible(11, i, hands[i]) for i in range(24)], dtype=np.uint8)
    assert int((hands[:, 1:8].sum(axis=1) > 0).sum()) >= 20
    _same(vecenv.discard_table(hands, vis, True), D.table(hands, vis, True), "4P hands as 3P")


# ---------------------------------------------------------------- 2. the live entry, and what tests 3 and 5 read
def _live(mode, policy):
    """8 games of (mode, policy) stepped to every stop; per stop the host entry's table of all 4 n rows, the yardstick's on env.peek(g),
    the hand lengths, and the compact extended batch with the device entry's table and the masks of its rows: made once, shared"""
    if (mode, policy) not in _LIVE:
        from riichienv_amd.torch_env import TorchVecEnv

        n, np_ = 8, 3 if mode >= 3 else 4
        env = TorchVecEnv(n, game_mode=mode, seed=SEEDS[mode, policy], features="extended")
        index = np.arange(4 * n, dtype=np.int32)
        stops, at = [], 0
        for stop in STOPS:
            if policy == "greedy":
                env.env.step_greedy(5, stop - at, auto_reset=False, call_rate_256=64)
            else:
                env.env.step_random(5, stop - at, auto_reset=False)
            at = stop
            views = [env.env.peek(g) for g in range(n)]
            obs, idx = env.obs_compact()
            dev = env.discard_table_compact(idx)
            stops.append(dict(stop=stop, got=env.env.discard_table(index), want=D.rows_of_views([(v, s) for v in views for s in range(4)], np_),
                              lens=np.array([v.players[s].hand_len if s < np_ else 0 for v in views for s in range(4)]),
                              obs=obs.cpu().numpy().copy(), idx=idx.cpu().numpy().copy(), dev={f: v.cpu().numpy() for f, v in dev.items()}, dev_t=dev,
                              mask=env.mask.reshape(4 * n, -1)[idx.long()].clone()))
        env.env.close()
        _LIVE[mode, policy] = stops
    return _LIVE[mode, policy]


@pytest.mark.parametrize("policy", ["greedy", "random"])
@pytest.mark.parametrize("mode", [2, 5])
def test_live_entry_equals_the_yardstick_on_the_devices_state(mode, policy):
    np_ = 3 if mode >= 3 else 4
    cover = dict(r2=0, r1=0, melds=0, tenpai=0, thin=0, dead=0)
    for st in _live(mode, policy):
        got, want, lens = st["got"], st["want"], st["lens"]
        _same(got, want, f"mode {mode} {policy} step {st['stop']}")
        present = got["shanten"][:, 34] != abi.DTAB_NONE
        assert present.tolist() == [s < np_ for _ in range(8) for s in range(4)], "seat 3 of a 3P game is an absent row"
        _same({f: v[st["idx"]] for f, v in got.items()}, {f: (v.view(np.uint64) if f == "mask" else v) for f, v in st["dev"].items()}, "device entry against host entry")
        sh, ac, uk = got["shanten"].astype(int), got["accept"].astype(int), got["ukeire"].astype(int)
        cover["r2"] += int((present & (lens % 3 == 2)).sum())
        cover["r1"] += int((present & (lens % 3 == 1)).sum())
        cover["melds"] += int((present & (lens <= 11)).sum())
        cover["tenpai"] += int((sh[:, :34] == 0).sum())
        cover["thin"] += int((uk[:, :34] < 4 * ac[:, :34]).sum())          # entries of single discards: column 34 holds maxima taken apart
        cover["dead"] += int(((uk[:, :34] == 0) & (ac[:, :34] > 0)).sum())
    print(f"mode {mode} {policy}: {cover}")
    assert all(v > 0 for v in cover.values()), cover


@pytest.mark.parametrize("mode", [2, 5])
def test_count_bad_indices_and_flags(mode):
    import ctypes as C

    import torch

    from riichienv_amd import vecenv
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(6, game_mode=mode, seed=9)
    env.env.step_random(3, 60, auto_reset=True)
    index = torch.arange(24, dtype=torch.int32, device=env.device)
    full = env.discard_table_compact(index)
    cut = 13
    out = {f: torch.full_like(v, 0x5A) for f, v in full.items()}
    count = torch.tensor([cut], dtype=torch.int32, device=env.device)
    assert env.discard_table_compact(index, count=count, out=out) is out
    torch.cuda.synchronize()
    for f in D.FIELDS:
        assert (out[f][:cut] == full[f][:cut]).all(), f
        assert (out[f][cut:] == 0x5A).all(), f"{f}: a row behind the count was written"
    assert full["mask"].dtype == torch.int64
    # a negative index, indices out of range, seat 3 in 3P
    got = env.env.discard_table(np.array([0, 24, -1, 1 << 30, 23, 3], dtype=np.int32))
    absent = [1, 2, 3] + ([4, 5] if mode >= 3 else [])
    assert (got["shanten"][absent] == abi.DTAB_NONE).all() and not any(got[f][absent].any() for f in ("accept", "ukeire", "mask"))
    assert got["shanten"][0, 34] != abi.DTAB_NONE and (mode >= 3 or got["shanten"][4, 34] != abi.DTAB_NONE)
    # flags must be 0; without the mask array the other three are written all the same
    b = abi.DiscardTableOut(full["shanten"].data_ptr(), full["accept"].data_ptr(), full["ukeire"].data_ptr(), None)
    assert env.env.L.rmj_discard_table_device(env.env.h, C.c_void_p(index.data_ptr()), 24, None, 1, C.byref(b)) == -1   # RMJ_ERR_ARG
    three = {f: torch.full_like(full[f], 0x5A) for f in ("shanten", "accept", "ukeire")}
    b = abi.DiscardTableOut(three["shanten"].data_ptr(), three["accept"].data_ptr(), three["ukeire"].data_ptr(), None)
    vecenv._chk(env.env.L.rmj_discard_table_device(env.env.h, C.c_void_p(index.data_ptr()), 24, None, 0, C.byref(b)))
    env.sync()
    torch.cuda.synchronize()
    assert all((three[f] == full[f]).all() for f in three)
    env.env.close()


# ---------------------------------------------------------------- 3. an independent device path: the extended features' efficiency channels
def _channels_agree(features, sh34, ac34, uk34, sanma, what):
    """channels 78, 79, 80 (one value in every column) against column 34 of the table, as float32"""
    want = [np.maximum(sh34.astype(np.float32), np.float32(0)) / np.float32(8), ac34.astype(np.float32) / np.float32(27 if sanma else 34),
            uk34.astype(np.float32) / np.float32(80)]
    for k, w in enumerate(want):
        ch = features[:, 78 + k, :]
        assert ch.dtype == np.float32 and (ch == ch[:, :1]).all(), (what, 78 + k)
        bad = np.flatnonzero(ch[:, 0] != w)
        assert bad.size == 0, (what, 78 + k, bad.size, ch[bad[:4], 0].tolist(), w[bad[:4]].tolist())


@pytest.mark.parametrize("policy", ["greedy", "random"])
@pytest.mark.parametrize("mode", [2, 5])
def test_column_34_is_what_the_extended_features_carry(mode, policy):
    rows, thirteen = 0, 0
    for st in _live(mode, policy):
        d = st["dev"]
        assert st["obs"].shape[0] == st["idx"].shape[0] == d["shanten"].shape[0]
        _channels_agree(st["obs"], d["shanten"][:, 34], d["accept"][:, 34], d["ukeire"][:, 34], mode >= 3, f"mode {mode} {policy} step {st['stop']}")
        rows += st["idx"].shape[0]
        thirteen += int((st["lens"][st["idx"]] % 3 == 1).sum())
    print(f"mode {mode} {policy}: {rows} acting rows, {thirteen} of them 3n+1 hands")
    assert rows > 0


# ---------------------------------------------------------------- 4. the builder
def _logs(mode):
    logs = list(log_check_ref.oracle_logs(mode, 4))
    if mode == 2:
        with open(GOLDEN) as f:
            logs.append([json.loads(line) for line in f if line.strip()])
    return logs


def _build(logs, mode, **kw):
    from riichienv_amd.datasets import LogSampleBuilder

    b = LogSampleBuilder(logs, game_mode=mode, include_pass=True, **kw)
    b.run()
    counts = b.counts()
    s = {k: v.cpu().numpy() for k, v in b.samples().items()}
    b.close()
    return s, counts


def _built(mode):
    if mode not in _BUILT:
        logs = _logs(mode)
        eff, eff_counts = _build(logs, mode, features="extended", hidden=True, efficiency=True)
        plain, plain_counts = _build(logs, mode, features="extended")
        alone, _ = _build(logs, mode, efficiency=True)
        keys = {}
        for lg, ev, st in zip(eff["log"].tolist(), eff["event"].tolist(), eff["seat"].tolist()):
            keys.setdefault(lg, set()).add((ev, st))
        ref = {}
        for lg, want in keys.items():
            for (ev, st), row in D.log_rows(logs[lg], mode, want).items():
                ref[lg, ev, st] = row
        _BUILT[mode] = dict(logs=logs, eff=eff, eff_counts=eff_counts, plain=plain, plain_counts=plain_counts, alone=alone, ref=ref)
    return _BUILT[mode]


@pytest.mark.parametrize("mode", [2, 5])
def test_builder_rows_equal_the_oracle_replay(mode):
    c = _built(mode)
    s, cn = c["eff"], c["eff_counts"]
    assert cn["failed_logs"] == 0 and cn["overflowed"] == 0 and cn["steps_left"] == 0 and cn["complete_logs"] == len(c["logs"]), cn
    assert s["action"].shape[0] == cn["fill"] == cn["decisions"] > 0, "no sample may be left out"
    ks = list(zip(s["log"].tolist(), s["event"].tolist(), s["seat"].tolist()))
    assert len(set(ks)) == len(ks) and all(k in c["ref"] for k in ks)
    for f in ("shanten", "accept", "ukeire"):
        got, want = s["dt_" + f], np.stack([c["ref"][k][f] for k in ks])
        assert got.dtype == want.dtype and got.shape == want.shape == (len(ks), 35), f
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (f, bad.size, [(ks[i], got[i].tolist(), want[i].tolist()) for i in bad[:2]])
    _channels_agree(s["features"], s["dt_shanten"][:, 34], s["dt_accept"][:, 34], s["dt_ukeire"][:, 34], mode >= 3, f"builder, mode {mode}")
    tot = (s["dt_shanten"][:, :34] != abi.DTAB_NONE).any(axis=1)
    print(f"mode {mode}: {len(ks)} samples, {int(tot.sum())} with a discard to make, {int((s['dt_shanten'][:, :34] == 0).sum())} tenpai entries")
    assert tot.any() and (~tot).any() and (s["dt_shanten"][:, :34] == 0).any()


@pytest.mark.parametrize("mode", [2, 5])
def test_efficiency_changes_no_other_column(mode):
    c = _built(mode)
    today = ["features", "mask", "action", "packed", "return", "return64", "rank", "log", "kyoku", "seat", "t"]
    hidden = ["opp_hand", "opp_shanten", "opp_waits", "opp_flags", "event"]
    new = ["dt_shanten", "dt_accept", "dt_ukeire"]
    assert list(c["plain"]) == today and list(c["eff"]) == today + hidden + new and list(c["alone"]) == today + new
    assert c["plain_counts"] == c["eff_counts"]
    for k in today:
        assert c["plain"][k].dtype == c["eff"][k].dtype and c["plain"][k].tobytes() == c["eff"][k].tobytes(), k
    for k in new:                                  # independent of hidden and of the feature set
        assert c["alone"][k].tobytes() == c["eff"][k].tobytes(), k
    assert c["eff"]["dt_shanten"].dtype == np.int8 and c["eff"]["dt_accept"].dtype == np.uint8 and c["eff"]["dt_ukeire"].dtype == np.uint8


def test_builder_edges():
    from riichienv_amd.datasets import LogSampleBuilder
    from tests import apply_events_util as U

    with pytest.raises(ValueError, match="masked_ok"):
        LogSampleBuilder([U.furiten_log(False)], game_mode=2, masked_ok=True, efficiency=True)
    b = LogSampleBuilder([], game_mode=2, efficiency=True)
    assert b.run() == 0
    s = b.samples()
    assert s["dt_shanten"].shape == (0, 35) and s["dt_accept"].shape == (0, 35) and s["dt_ukeire"].shape == (0, 35)
    b.close()


# ---------------------------------------------------------------- 5. best_discard
@pytest.mark.parametrize("policy", ["greedy", "random"])
@pytest.mark.parametrize("mode", [2, 5])
def test_best_discard_on_a_live_batch(mode, policy):
    from riichienv_amd import efficiency

    sanma = mode >= 3
    nd = 27 if sanma else 34
    picked, none = 0, 0
    for st in _live(mode, policy):
        got = efficiency.best_discard(st["dev_t"], st["mask"], sanma)
        assert got.is_cuda and got.shape == (st["idx"].shape[0],)
        got, mask, d = got.cpu().tolist(), st["mask"].cpu().numpy(), st["dev"]
        for i, g in enumerate(got):
            assert g == D.best_discard(d["shanten"][i], d["accept"][i], d["ukeire"][i], mask[i], sanma), (st["stop"], i)
            if g >= 0:
                assert g < nd and mask[i, g], "the id is a legal discard"
                assert d["shanten"][i, D.SANMA_TYPES[g] if sanma else g] != abi.DTAB_NONE, "a legal discard is a held type"
                picked += 1
            else:
                assert not mask[i, :nd].any()
                none += 1
    print(f"mode {mode} {policy}: {picked} rows with a discard, {none} without")
    assert picked > 0


# ---------------------------------------------------------------- 6. the example
def test_the_example_runs():
    import importlib.util

    spec = importlib.util.spec_from_file_location("discard_table_example", os.path.join(ROOT, "examples", "discard_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(games=16, steps=80, show=2)
    assert out["rows"] > 0 and out["with_discard"] > 0 and 0 <= out["mean_shanten"] < 8
