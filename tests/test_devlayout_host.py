"""CPU: the layout and slot-chain helpers of the C boundary's host code (riichienv_amd/csrc/rmj_host.h: rmjh::DevLayout, rmjh::SlotChain)
compiled as host C++ with g++ and held to restatements written out in the program (tests/devlayout/devlayout_check.cpp): the pool
constructors' `take` lambda on random size lists (0, 1, 255, 256, 257, above 4 GiB; steps of 4, 16, 32 and 256; guard regions; what
bind() writes and what it leaves alone), and the loop that starts every replay slot's cursors on offset tables with logs of no events in
front, behind and in runs, for every slot count 1..M - once plain and once under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "devlayout", "devlayout_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_devlayout_and_slot_chains_equal_their_restatements(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "devlayout_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + [SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "devlayout OK" in r.stdout
    checks = [int(w) for w in r.stdout.split() if w.isdigit()][0]
    assert checks >= 1_000_000
