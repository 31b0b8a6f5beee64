"""CPU: the per-record MJAI formatter that the device formatter runs (riichienv_amd/csrc/rmj_evtext.h) compiled as host C++ with g++ and
held byte for byte to the host formatter (rmj_host.h: rmjh::format_event / format_events) - every type x seat x tile byte, extreme fields,
>= 1e6 random records in random-length games (tests/evtext/evtext_check.cpp) - once plain and once under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "evtext", "evtext_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_evtext_equals_the_host_formatter(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "evtext_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + [SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "evtext OK" in r.stdout
    single, games = [int(w) for w in r.stdout.split() if w.isdigit()][:2]
    assert single >= 256 * 256 * 6 and games >= 1_000_000
