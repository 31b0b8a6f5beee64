"""Cost of building BC / CQL samples from MJAI logs: ReplayBatch.samples() (the host path) against LogSampleBuilder (the device path)
on the same self-written 4P logs, base features.  Writes profiles/log_dataset.json.

    python scripts/bench_log_dataset.py                      # both paths + the kernel breakdown of the device path
    python scripts/bench_log_dataset.py --trace-child         # (internal) one device run, for rocprofv3 --kernel-trace --stats
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_logs(n, seed=1):
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


def device_path(logs, n_slots, reps=1):
    """the builder on `logs`: construction (host packing, the kyoku tables' parse, upload, pool) timed apart from the replay"""
    import torch

    from riichienv_amd.datasets import LogSampleBuilder

    t0 = time.perf_counter()
    b = LogSampleBuilder(logs, game_mode=2, features="base", n_slots=n_slots)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    best = None
    for i in range(reps + 1):     # (the first run is the warm-up)
        b.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.run()
        b.finalize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i:
            best = dt if best is None else min(best, dt)
    c = b.counts()
    host = dict(b.host_seconds)
    b.close()
    return dict(replay_seconds=best, construct_seconds=build_s, construct_pack_logs_seconds=host["pack_logs"], construct_kyoku_tables_seconds=host["kyoku_tables"],
                samples=c["fill"], events=c["events"], steps=c["steps_done"], logs=len(logs), n_slots=n_slots, failed_logs=c["failed_logs"], overflowed=c["overflowed"])


def host_path(logs):
    from riichienv_amd import replay

    warm = replay.ReplayBatch(logs[:2], game_mode=2)
    for i, _ in enumerate(warm.samples()):
        if i > 20:
            break
    warm.env.close()
    t0 = time.perf_counter()
    rb = replay.ReplayBatch(logs, game_mode=2)
    n = sum(len(s["seat"]) for s in rb.samples())
    rb.env.sync()
    dt = time.perf_counter() - t0
    rb.env.close()
    return dict(seconds=dt, samples=n, events=sum(len(l) for l in logs), logs=len(logs),
                per_event_index="1 kernel, 5 device-to-host copies, a peek per game that discards, Python matching and packing per game")


def trace_child(n_logs, n_slots):
    """one construction, one run, one finalize - what rocprofv3 traces; prints the steps for the parent"""
    import torch

    from riichienv_amd.datasets import LogSampleBuilder

    logs = make_logs(n_logs)
    b = LogSampleBuilder(logs, game_mode=2, features="base", n_slots=n_slots or len(logs))
    b.run()
    b.finalize()
    torch.cuda.synchronize()
    print("TRACE_CHILD " + json.dumps(dict(steps=b.counts()["steps_done"], logs=len(logs))))
    b.close()


def kernel_stats(n_logs, n_slots):
    """rocprofv3 --kernel-trace --stats of one device run in a child process of its own: the kernels by total time, and the launches of the
    replay's kernels per event index counted from the trace"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "logds", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", "--logs", str(n_logs), "--slots", str(n_slots)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as e:
            return {"error": repr(e)}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        child = [l for l in p.stdout.splitlines() if l.startswith("TRACE_CHILD ")]
        if p.returncode != 0 or not files or not child:
            return {"error": f"rocprofv3 exit {p.returncode}", "files": [os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**", "*"), recursive=True)][:20],
                    "stderr": p.stderr[-800:]}
        rows = []
        for f in files:
            with open(f) as fh:
                rows += list(csv.DictReader(fh))
        rows.sort(key=lambda r: -float(r.get("TotalDurationNs", 0) or 0))
        info = json.loads(child[0][len("TRACE_CHILD "):])
        replay_calls = sum(int(r.get("Calls", 0)) for r in rows if "k_log_decide" in r.get("Name", "") or "k_log_scan" in r.get("Name", "") or
                           "k_log_record" in r.get("Name", "") or "k_log_apply" in r.get("Name", ""))
        return dict(what=f"one construction, one run and one finalize of {info['logs']} logs ({info['steps']} steps), the rollout that wrote the logs included",
                    steps=info["steps"], replay_kernel_launches=replay_calls, launches_per_event_index=replay_calls / max(info["steps"], 1),
                    kernels=[dict(kernel=r.get("Name", "")[:96], calls=int(r.get("Calls", 0)), total_ms=float(r.get("TotalDurationNs", 0)) / 1e6,
                                  average_us=float(r.get("AverageNs", 0) or 0) / 1e3, percent=float(r.get("Percentage", 0) or 0)) for r in rows[:12]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=0, help="0 = one slot per log")
    ap.add_argument("--host-logs", type=int, default=64, help="logs the host path replays (it is compared per log)")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--trace-logs", type=int, default=1024, help="logs of the traced run")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_dataset.json"))
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.logs, args.slots)
        return
    logs = make_logs(args.logs)
    slots = args.slots or len(logs)
    dev = device_path(logs, slots, reps=2)
    host = host_path(logs[: args.host_logs])
    dev["samples_per_s"], dev["events_per_s"] = dev["samples"] / dev["replay_seconds"], dev["events"] / dev["replay_seconds"]
    dev["replay_seconds_per_log"] = dev["replay_seconds"] / dev["logs"]
    dev["end_to_end_seconds_per_log"] = (dev["construct_seconds"] + dev["replay_seconds"]) / dev["logs"]
    host["samples_per_s"], host["events_per_s"], host["seconds_per_log"] = host["samples"] / host["seconds"], host["events"] / host["seconds"], host["seconds"] / host["logs"]
    res = dict(workload=f"{len(logs)} self-written 4p-red-half logs (step_greedy, call_rate_256=64), base features, include_pass, skip_single_action",
               device=dev, host=host,
               ratio_per_log_replay_only=host["seconds_per_log"] / dev["replay_seconds_per_log"],
               ratio_per_log_end_to_end=host["seconds_per_log"] / dev["end_to_end_seconds_per_log"],
               what_the_ratios_compare="host: ReplayBatch construction + samples() over its logs, per log (it packs its events from dicts at every index).  "
                                       "replay_only: the builder's run() + finalize() per log, after construction.  end_to_end: construction (pack_logs' Python "
                                       "loop over every event, the kyoku tables' parse of the logs, upload, pool allocation) + run() + finalize(), per log",
               holds_it_back="end to end the builder is bound by its constructor's host work, not by a launch or a copy: see construct_pack_logs_seconds and "
                             "construct_kyoku_tables_seconds against replay_seconds")
    if not args.no_trace:
        res["device_kernel_stats"] = kernel_stats(args.trace_logs, 0)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "device_kernel_stats"}))
    print(json.dumps(res.get("device_kernel_stats", {}))[:1500])


if __name__ == "__main__":
    main()
