"""Cost of ingesting MJAI text on the device (rmj_logset_create_from_text) next to the host ingest it replaces, on the self-written 4P
logs of profiles/log_dataset.json (bench_log_dataset.make_logs), in one process:

  (a) host ingest: json.loads of every line + pack_logs + kyoku_tables + rmj_logset_create
  (b) rmj_logset_create_from_text from host bytes
  (c) the same from text in device memory
  (d) run() + finalize() of the builder on the resulting set

each the best of three after a warm-up, then a rocprofv3 --kernel-trace --stats run of (b) in a child process for the per-kernel split.

    python scripts/bench_log_text_ingest.py --logs 4096 --out profiles/log_text_ingest.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29   # the device-to-device copy figure the project's profiles use (TB/s)


def make_text(n, seed=1):
    """the logs of bench_log_dataset.make_logs as text: per-log byte strings"""
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(n, game_mode=2, seed=seed, event_ring=8192)
    env.reset()
    for _ in range(40):
        env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
        if env.status()[2].all():
            break
    text, offs = env.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
    raw = text.tobytes()
    out = [raw[int(offs[g]): int(offs[g + 1])] for g in range(n)]
    env.close()
    return out


def text_buffer(texts):
    """(uint8 buffer, [M, 2] uint64 byte ranges) of per-log byte strings laid end to end: what the timed create calls take"""
    import numpy as np

    ends = np.cumsum([len(t) for t in texts], dtype=np.uint64)
    return np.frombuffer(b"".join(texts), np.uint8), np.ascontiguousarray(np.stack([ends - np.array([len(t) for t in texts], np.uint64), ends], axis=1))


def best_of(fn, reps=3):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def create_from_text(buf, rng, on_device=False):
    from riichienv_amd import abi, vecenv

    L = vecenv.load_lib()
    h = C.c_void_p()
    if on_device:
        vecenv._chk(L.rmj_logset_create_from_text(0, C.c_void_p(buf.data_ptr()), C.c_void_p(rng.data_ptr()), int(rng.shape[0]), 4, abi.LOGTEXT_ON_DEVICE, C.byref(h)))
    else:
        vecenv._chk(L.rmj_logset_create_from_text(0, buf.ctypes.data, rng.ctypes.data, len(rng), 4, 0, C.byref(h)))
    L.rmj_logset_destroy(h)


def host_ingest(texts):
    from riichienv_amd import datasets, vecenv

    L = vecenv.load_lib()
    t0 = time.perf_counter()
    logs = [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in texts]
    t1 = time.perf_counter()
    recs, off = datasets.pack_logs(logs, 4)
    t2 = time.perf_counter()
    datasets.kyoku_tables(logs, 4)
    t3 = time.perf_counter()
    h = C.c_void_p()
    vecenv._chk(L.rmj_logset_create(0, C.addressof(recs), off.ctypes.data, len(logs), C.byref(h)))
    t4 = time.perf_counter()
    L.rmj_logset_destroy(h)
    return dict(json_loads=t1 - t0, pack_logs=t2 - t1, kyoku_tables=t3 - t2, logset_create=t4 - t3, total=t4 - t0)


def trace_child(n_logs):
    import torch

    buf, rng = text_buffer(make_text(n_logs))
    create_from_text(buf, rng)
    torch.cuda.synchronize()
    print("TRACE_CHILD " + json.dumps(dict(logs=n_logs, bytes=int(buf.size))))


def kernel_stats(n_logs):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ingest", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", "--logs", str(n_logs)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.TimeoutExpired) as e:
            return {"error": repr(e)}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        child = [l for l in p.stdout.splitlines() if l.startswith("TRACE_CHILD ")]
        if p.returncode != 0 or not files or not child:
            return {"error": f"rocprofv3 exit {p.returncode}", "stderr": p.stderr[-800:]}
        rows = []
        for f in files:
            with open(f) as fh:
                rows += list(csv.DictReader(fh))
        info = json.loads(child[0][len("TRACE_CHILD "):])
        lt = [r for r in rows if "k_lt_" in r.get("Name", "")]
        lt.sort(key=lambda r: -float(r.get("TotalDurationNs", 0) or 0))
        out = dict(what=f"one rmj_logset_create_from_text of {info['logs']} logs ({info['bytes']} bytes) from host memory", bytes=info["bytes"],
                   kernels=[dict(name=r["Name"][:60], calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3) for r in lt])
        parse = [r for r in lt if "k_lt_parse" in r["Name"]]
        if parse:
            s = float(parse[0]["TotalDurationNs"]) / 1e9
            out["parse_kernel_bytes_per_second"] = info["bytes"] / s
            out["parse_kernel_share_of_copy_rate"] = info["bytes"] / s / (COPY_TBS * 1e12)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.logs)
        return
    import torch

    from riichienv_amd import datasets

    texts = make_text(args.logs)
    buf, rng = text_buffer(texts)
    host_ingest(texts[:64])
    runs = [host_ingest(texts) for _ in range(3)]
    a = min(runs, key=lambda r: r["total"])
    b = best_of(lambda: create_from_text(buf, rng))
    dbuf = torch.as_tensor(buf, device="cuda")
    drng = torch.as_tensor(rng.astype("int64"), device="cuda")
    torch.cuda.synchronize()
    c = best_of(lambda: create_from_text(dbuf, drng, True))
    bld = datasets.LogSampleBuilder.from_text(texts, game_mode=2, features="base")

    def replay():
        bld.clear()
        bld.run()
        bld.finalize()
        torch.cuda.synchronize()

    d = best_of(replay)
    counts = bld.counts()
    bld.close()
    res = dict(device=torch.cuda.get_device_name(0), logs=args.logs, text_bytes=int(buf.size), events=counts["events"], samples=counts["fill"],
               method="one process; every figure the best of three after a warm-up; wall clock around synchronous calls (d: torch.cuda.synchronize())",
               a_host_ingest_seconds=a, b_from_host_text_seconds=b, c_from_device_text_seconds=c, d_run_finalize_seconds=d,
               ingest_below_replay=bool(b < d), end_to_end_text_to_samples_seconds=b + d,
               note="a byte parser branches per character and is not expected to be near the copy rate")
    if not args.no_trace:
        res["kernel_stats"] = kernel_stats(min(args.logs, 4096))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
