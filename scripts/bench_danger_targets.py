"""Cost of the deal-in danger targets.  Writes profiles/danger_targets.json.

  live      rmj_danger_targets_device next to rmj_hidden_targets_device over the same obs_compact index of 65 536 4p-red-half games after
            150 greedy steps, windows of the two alternating in one process.
  passes    the same live windows by a library whose danger kernel takes ONE candidate per evaluator pass instead of four (the first step
            of the feature: every 16-lane row of the evaluator but the first idles).  That variant is no part of the library: --build-one-per-pass
            PATH compiles it from a copy of the sources with one statement of rmj_danger.hip.h rewritten (ONE_PER_PASS below) and --one-per-pass-lib
            PATH measures it, in child processes that alternate with children of the library itself.  Both give the same rows (checked).
  builder   run() + finalize() of LogSampleBuilder plain, hidden=True and hidden=True + danger=True over the log set of
            scripts/bench_hidden_targets.py (one LogSet, three builders, windows alternating).
Every figure is a median over windows, each window a host clock around work that ends in a device synchronise, after a warm-up window;
the spread (min, max, and max - min over the median) is written next to it.  The flagship benchmark against the parent commit's is
bench.py's own business: run both in one session and put the lines next to each other (--bench-lines FILE merges them into the result).

    python scripts/bench_danger_targets.py --build-one-per-pass /tmp/one.so          # (needs hipcc, no GPU)
    python scripts/bench_danger_targets.py --one-per-pass-lib /tmp/one.so
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "scripts"))
from bench_hidden_targets import builder_windows, spread  # noqa: E402

# the statement that hands the next candidate to row j of the evaluator, and its one-candidate-per-pass form (rows 1..3 get none)
FOUR_PER_PASS = """                    kq[j] = mlo ? __ffs((int)mlo) - 1 : (mhi ? 31 + __ffs((int)mhi) : -1);
                    if (mlo) mlo &= mlo - 1u; else mhi &= mhi - 1u;"""
ONE_PER_PASS = """                    kq[j] = j ? -1 : (mlo ? __ffs((int)mlo) - 1 : (mhi ? 31 + __ffs((int)mhi) : -1));
                    if (!j) { if (mlo) mlo &= mlo - 1u; else mhi &= mhi - 1u; }"""


def build_one_per_pass(out):
    """the library with ONE_PER_PASS, compiled like __graft_entry__.build() compiles the real one, into `out`"""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(HERE, "riichienv_amd", "csrc"), os.path.join(tmp, "riichienv_amd", "csrc"))
        shutil.copytree(os.path.join(HERE, "include"), os.path.join(tmp, "include"))
        path = os.path.join(tmp, "riichienv_amd", "csrc", "rmj_danger.hip.h")
        src = open(path).read()
        assert src.count(FOUR_PER_PASS) == 1, "rmj_danger.hip.h no longer holds the statement this script rewrites"
        open(path, "w").write(src.replace(FOUR_PER_PASS, ONE_PER_PASS))
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-result", "-Wno-unused-value", "-mllvm",
                               "-disable-machine-licm", os.path.join(tmp, "riichienv_amd", "csrc", "rmj_api.hip"), "-o", out])
    print("built", out)


def live_windows(n_games, windows, calls, with_hidden):
    """{"danger": [...], "danger_ura": [...], "hidden": [...]} seconds per call, windows alternating; rows; a digest of the danger rows"""
    import ctypes as C

    import torch

    from riichienv_amd import abi, vecenv
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(n_games, game_mode=2, seed=1)
    env.env.step_greedy(3, 150, auto_reset=True, call_rate_256=64)
    _, index = env.obs_compact()
    rows = int(index.shape[0])
    L, h, ix = env.env.L, env.env.h, C.c_void_p(index.data_ptr())
    dng = env.danger_compact(index)
    db = abi.row_struct("danger", {"danger": dng})
    hid = env.hidden_compact(index)
    hb = abi.row_struct("hidden", hid)
    calls_of = {"danger": lambda: L.rmj_danger_targets_device(h, ix, rows, None, 0, C.byref(db)),
                "danger_ura": lambda: L.rmj_danger_targets_device(h, ix, rows, None, abi.DANGER_URA, C.byref(db))}
    if with_hidden:
        calls_of["hidden"] = lambda: L.rmj_hidden_targets_device(h, ix, rows, None, C.byref(hb))
    secs = {k: [] for k in calls_of}
    for w in range(windows + 1):          # (window 0 warms up)
        for name, call in calls_of.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                vecenv._chk(call())
            torch.cuda.synchronize()
            if w:
                secs[name].append((time.perf_counter() - t0) / calls)
    plain = env.danger_compact(index)
    tenpai = ((hid["opp_flags"] & abi.HIDDEN_TENPAI) != 0)
    stats = dict(rows=rows, opponent_rows_tenpai=float(tenpai.float().mean()), opponent_rows_with_a_value=float(plain.any(dim=2).float().mean()),
                 nonzero_values=int((plain > 0).sum()), sum_of_values=int(plain.to(torch.int64).sum()), largest=int(plain.max()))
    env.env.close()
    return secs, stats


def live_child(args):
    from riichienv_amd import vecenv

    if args.lib:
        vecenv.LIB_PATH = os.path.abspath(args.lib)
    secs, stats = live_windows(args.games, args.windows, args.calls, with_hidden=not args.lib)
    print("LIVE_CHILD " + json.dumps(dict(seconds=secs, stats=stats)))


def run_live_child(args, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--live-child", "--games", str(args.games), "--windows", str(args.windows), "--calls", str(args.calls)]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [l for l in p.stdout.splitlines() if l.startswith("LIVE_CHILD ")]
    if p.returncode != 0 or not line:
        raise RuntimeError(f"the live child failed (exit {p.returncode}): {p.stderr[-800:]}")
    return json.loads(line[0][len("LIVE_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3, help="run() + finalize() per window")
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50, help="entry calls per window")
    ap.add_argument("--build-one-per-pass", default=None)
    ap.add_argument("--one-per-pass-lib", default=None)
    ap.add_argument("--bench-lines", default=None, help="a file of bench.py result lines, 'parent' or 'this' in front of each: merged into the result")
    ap.add_argument("--live-child", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--skip-builder", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "danger_targets.json"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.build_one_per_pass:
        return build_one_per_pass(args.build_one_per_pass)
    if args.live_child:
        return live_child(args)
    res = dict(workload=f"{args.games} 4p-red-half games after 150 greedy steps (auto-reset), the obs_compact index; a window = {args.calls} calls ending in a "
                        "synchronise, variants alternating")
    # ---- live: children of the library and of the one-per-pass variant, alternating
    order = [None, args.one_per_pass_lib, None, args.one_per_pass_lib] if args.one_per_pass_lib else [None]
    kids = [(lib, run_live_child(args, lib)) for lib in order]
    mine = [k for lib, k in kids if lib is None]
    live = {name: spread([x for k in mine for x in k["seconds"][name]]) for name in ("danger", "danger_ura", "hidden")}
    stats = mine[0]["stats"]
    res["live"] = dict(stats, calls_per_window=args.calls, processes=len(mine), danger_seconds_per_call=live["danger"], danger_ura_seconds_per_call=live["danger_ura"],
                       hidden_seconds_per_call=live["hidden"], danger_over_hidden=live["danger"]["median"] / live["hidden"]["median"],
                       danger_rows_per_second=stats["rows"] / live["danger"]["median"], bytes_written_per_row=444)
    if args.one_per_pass_lib:
        other = [k for lib, k in kids if lib is not None]
        assert all(k["stats"] == stats for k in other), "the one-per-pass library gives other rows"
        one = spread([x for k in other for x in k["seconds"]["danger"]])
        res["passes"] = dict(four_per_pass_seconds_per_call=live["danger"], one_per_pass_seconds_per_call=one, one_over_four=one["median"] / live["danger"]["median"],
                             same_rows=True, processes_each=len(other))
    else:
        res["passes"] = "not measured"
    # ---- the builder
    if not args.skip_builder:
        times, counts, n_logs = builder_windows(args.logs, args.windows, args.runs, {"plain": {}, "hidden": {"hidden": True}, "hidden_danger": {"hidden": True, "danger": True}})
        assert counts["plain"] == counts["hidden"] == counts["hidden_danger"]
        sp = {k: spread(v) for k, v in times.items()}
        res["builder"] = dict(workload=f"{n_logs} self-written 4p-red-half logs, base features, include_pass, skip_single_action; a window = {args.runs} x (clear, run, "
                                       "finalize) ending in a synchronise, variants alternating",
                              samples=counts["plain"]["fill"], steps=counts["plain"]["steps_done"], overflowed=counts["plain"]["overflowed"],
                              plain_seconds=sp["plain"], hidden_seconds=sp["hidden"], hidden_danger_seconds=sp["hidden_danger"],
                              hidden_over_plain=sp["hidden"]["median"] / sp["plain"]["median"], hidden_danger_over_plain=sp["hidden_danger"]["median"] / sp["plain"]["median"],
                              hidden_danger_over_hidden=sp["hidden_danger"]["median"] / sp["hidden"]["median"])
    else:
        res["builder"] = "not measured"
    if args.bench_lines:
        lines = {"parent": [], "this": []}
        for l in open(args.bench_lines):
            who, _, rest = l.strip().partition(" ")
            if who in lines and rest.startswith("{"):
                lines[who].append(json.loads(rest))
        res["bench_py"] = lines
    else:
        res["bench_py"] = "not measured"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
