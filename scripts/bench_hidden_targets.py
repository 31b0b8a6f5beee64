"""Cost of the hidden-hand targets.  Writes profiles/hidden_targets.json.

  builder   run() + finalize() of LogSampleBuilder with hidden=False and hidden=True over the log set of scripts/bench_log_dataset.py
            (one LogSet, two builders, windows of the two alternating): the ratio hidden / plain is reported, not gated.
  parent    the same plain windows taken by the PARENT commit's library and Python in a child process, before and after the windows
            above (--parent-tree DIR: a checkout of the parent commit with its library built).  The plain path launches the same kernels
            in both, so the two medians should lie within the parent's own window-to-window spread.
  live      rmj_hidden_targets_device at 65 536 games over the obs_compact index of a mid-game state.
Every figure is a median over windows, each window a host clock around work that ends in a device synchronise, after a warm-up window;
the spread (min, max, and max - min over the median) is written next to it.

    python scripts/bench_hidden_targets.py --parent-tree /path/to/parent/checkout
    python scripts/bench_hidden_targets.py --plain-child --root DIR      # (internal) the plain windows with DIR's package
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    med = statistics.median(xs)
    return dict(median=med, min=min(xs), max=max(xs), windows=len(xs), spread_over_median=(max(xs) - min(xs)) / med if med else 0.0)


def make_logs(n, seed=1):
    """the logs of scripts/bench_log_dataset.py (its make_logs, restated: the parent's child must not depend on this tree)"""
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(n, game_mode=2, seed=seed, event_ring=8192)
    env.reset()
    for _ in range(40):
        env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
        if env.status()[2].all():
            break
    logs = [[json.loads(s) for s in g] for g in env.mjai_logs()]
    env.close()
    return logs


def window(b, runs):
    """seconds of `runs` x (clear, run, finalize) of one builder, ending in a synchronise"""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        b.clear()
        b.run()
        b.finalize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs


def builder_windows(n_logs, windows, runs, variants):
    """{variant: [seconds per run() + finalize(), one per window]} with the variants alternating window by window; counts of each"""
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.logset import LogSet

    logs = make_logs(n_logs)
    logset = LogSet.from_logs(logs, 4)
    probe = LogSampleBuilder.from_logset(logset, game_mode=2, features="base")     # sizes the pools: the default capacity is twice what is needed
    probe.run()
    capacity = probe.counts()["decisions"] + 1024
    probe.close()
    builders = {name: LogSampleBuilder.from_logset(logset, game_mode=2, features="base", capacity=capacity, **kw) for name, kw in variants.items()}
    times = {name: [] for name in builders}
    for w in range(windows + 1):          # (window 0 warms every builder up)
        for name, b in builders.items():
            dt = window(b, runs)
            if w:
                times[name].append(dt)
    counts = {name: b.counts() for name, b in builders.items()}
    for b in builders.values():
        b.close()
    logset.close()
    return times, counts, len(logs)


def plain_child(args):
    times, counts, n = builder_windows(args.logs, args.windows, args.runs, {"plain": {}})
    print("PLAIN_CHILD " + json.dumps(dict(seconds=times["plain"], samples=counts["plain"]["fill"], steps=counts["plain"]["steps_done"], logs=n)))


def parent_windows(args):
    """the plain windows by the parent commit's package, in a child process"""
    cmd = [sys.executable, os.path.abspath(__file__), "--plain-child", "--root", os.path.abspath(args.parent_tree), "--logs", str(args.logs),
           "--windows", str(args.windows), "--runs", str(args.runs)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    line = [l for l in p.stdout.splitlines() if l.startswith("PLAIN_CHILD ")]
    if p.returncode != 0 or not line:
        raise RuntimeError(f"the parent's child failed (exit {p.returncode}): {p.stderr[-800:]}")
    return json.loads(line[0][len("PLAIN_CHILD "):])


def live_entry(n_games, windows, calls):
    import ctypes as C

    import torch

    from riichienv_amd import abi, vecenv
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(n_games, game_mode=2, seed=1)
    env.env.step_random(3, 60, auto_reset=True)
    _, index = env.obs_compact()
    rows = int(index.shape[0])
    out = env.hidden_compact(index)
    b = abi.row_struct("hidden", out)
    L, secs = env.env.L, []
    for w in range(windows + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            vecenv._chk(L.rmj_hidden_targets_device(env.env.h, C.c_void_p(index.data_ptr()), rows, None, C.byref(b)))
        torch.cuda.synchronize()
        if w:
            secs.append((time.perf_counter() - t0) / calls)
    tenpai = float(((out["opp_flags"] & abi.HIDDEN_TENPAI) != 0).float().mean())
    env.env.close()
    s = spread(secs)
    return dict(games=n_games, rows=rows, calls_per_window=calls, seconds_per_call=s, rows_per_second=rows / s["median"], bytes_written_per_row=132,
                tenpai_share_of_opponent_rows=tenpai)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3, help="run() + finalize() per window")
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=200, help="rmj_hidden_targets_device calls per window")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--plain-child", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "hidden_targets.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if args.plain_child:
        plain_child(args)
        return
    parent = [parent_windows(args)] if args.parent_tree else []
    times, counts, n_logs = builder_windows(args.logs, args.windows, args.runs, {"plain": {}, "hidden": {"hidden": True}})
    if args.parent_tree:
        parent.append(parent_windows(args))
    assert counts["plain"] == counts["hidden"], (counts["plain"], counts["hidden"])
    plain, hidden = spread(times["plain"]), spread(times["hidden"])
    res = dict(workload=f"{n_logs} self-written 4p-red-half logs (step_greedy, call_rate_256=64), base features, include_pass, skip_single_action; "
                        f"a window = {args.runs} x (clear, run, finalize) ending in a synchronise, variants alternating",
               builder=dict(samples=counts["plain"]["fill"], steps=counts["plain"]["steps_done"], overflowed=counts["plain"]["overflowed"],
                            plain_seconds=plain, hidden_seconds=hidden, ratio_hidden_over_plain=hidden["median"] / plain["median"],
                            hidden_samples_per_second=counts["hidden"]["fill"] / hidden["median"]))
    if parent:
        ps = [spread(p["seconds"]) for p in parent]
        allp = spread(parent[0]["seconds"] + parent[1]["seconds"])
        res["builder"]["parent_plain_seconds"] = dict(before=ps[0], after=ps[1], both=allp, samples=parent[0]["samples"])
        res["builder"]["plain_over_parent_plain"] = plain["median"] / allp["median"]
        res["builder"]["plain_within_parent_spread"] = bool(allp["min"] <= plain["median"] <= allp["max"])
    res["live"] = live_entry(args.games, args.windows, args.calls)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
