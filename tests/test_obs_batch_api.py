"""CPU-side checks of the observation-batch interface (rmj_encode_batch_device and its step entries): the descriptor's layout and the
feature-set constants agree with include/riichi_mi355x.h, the library exports the entries, and TorchVecEnv refuses a feature set it
cannot serve before it touches a device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from riichienv_amd import abi, vecenv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "riichi_mi355x.h")
ENTRIES = ["rmj_encode_batch_device", "rmj_encode_batch", "rmj_step_ids_encode_batch_device", "rmj_step_sample_encode_batch_device"]


def test_feature_constants_match_header():
    src = open(HDR).read()
    want = {name: int(v) for name, v in re.findall(r"#define RMJ_FEATURES_([A-Z_]+) (\d+)", src)}
    assert want == {"BASE": abi.FEATURES_BASE, "DISCARD_SHANTEN": abi.FEATURES_DISCARD_SHANTEN, "EXTENDED": abi.FEATURES_EXTENDED,
                    "DISCARD_SHANTEN_CHANNELS": abi.FEATURE_CHANNELS[abi.FEATURES_DISCARD_SHANTEN]}
    assert abi.FEATURE_CHANNELS == {0: 74, 1: 94, 2: 215}


def test_obs_batch_layout_matches_header():
    prog = r'''
#include <cstddef>
#include <cstdio>
#include "riichi_mi355x.h"
int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(RmjObsBatch), offsetof(RmjObsBatch, features), offsetof(RmjObsBatch, compact),
    offsetof(RmjObsBatch, row_stride), offsetof(RmjObsBatch, capacity), offsetof(RmjObsBatch, d_out), offsetof(RmjObsBatch, d_index),
    offsetof(RmjObsBatch, d_count));}
'''
    with tempfile.TemporaryDirectory() as d:
        p, exe = os.path.join(d, "s.cpp"), os.path.join(d, "s")
        open(p, "w").write(prog)
        subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    O = abi.ObsBatch
    assert got == [C.sizeof(O), O.features.offset, O.compact.offset, O.row_stride.offset, O.capacity.offset, O.out.offset,
                   O.index.offset, O.count.offset]


def test_library_exports_the_batch_entries():
    assert set(ENTRIES) <= set(vecenv.EXPORTS)
    lib = vecenv.load_lib()
    for sym in ENTRIES:
        assert getattr(lib, sym) is not None


def test_feature_shape_and_descriptor():
    env = object.__new__(vecenv.VecRiichiEnv)   # (no handle: feature_shape reads the mode only)
    env.game_mode = 2
    assert env.feature_shape("base") == (74, 34)
    assert env.feature_shape("discard_shanten") == (94, 34)
    assert env.feature_shape(abi.FEATURES_EXTENDED) == (215, 34)
    with pytest.raises(ValueError):
        env.feature_shape("sequence")
    env.game_mode = 5
    assert env.feature_shape("extended") == (215, 27)
    with pytest.raises(ValueError):
        env.feature_shape("discard_shanten")
    b = vecenv.VecRiichiEnv.obs_batch("discard_shanten", 0x1000, True, 0x2000, 77, 0x3000, row_stride=3200)
    assert (b.features, b.compact, b.row_stride, b.capacity, b.out, b.index, b.count) == (1, 1, 3200, 77, 0x1000, 0x2000, 0x3000)


@pytest.mark.parametrize("kw", [dict(game_mode=5, features="discard_shanten"), dict(game_mode=1, extended=True, features="base"),
                                dict(game_mode=2, extended=True, features="discard_shanten"), dict(game_mode=2, features="feat_v4")])
def test_torch_env_refuses_a_feature_set_it_cannot_serve(kw):
    pytest.importorskip("torch")
    from riichienv_amd.torch_env import TorchVecEnv

    with pytest.raises(ValueError):
        TorchVecEnv(8, **kw)
