"""CPU: the one place that decides how a device-policy rollout runs (riichienv_amd/csrc/rmj_host.h: rmjh::rollout_plan - per step on k
streams, one fused launch, or one launch handed out as tickets; its grids, chunk, part bounds and what the timers report of it) compiled
as host C++ with g++ and held to (a) a restatement, written out in the program (tests/rollout_plan/rollout_plan_check.cpp), of the
expressions the host code carried in five places before there was a plan, over the full cross product of batch sizes, rollout lengths
and tunables, and (b) a table of cases worked out by hand - once plain and once under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rollout_plan", "rollout_plan_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
# n_games x n_steps x quad x want_streams x queue_chunk x queue_min_chunk x queue_force x max_xcc_id x slots x policy x enc_fused x only_active
CROSS_PRODUCT = 20 * 16 * 3 * 4 * 6 * 2 * 2 * 2 * 3 * 2 * 2 * 2


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_rollout_plan_equals_its_restatement_and_the_cases_by_hand(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "rollout_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + [SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rollout plan OK" in r.stdout
    checks, combos = [int(w) for w in r.stdout.split() if w.isdigit()][:2]
    assert combos == CROSS_PRODUCT
    assert checks >= CROSS_PRODUCT
