"""Cost of the play statistics (rmj_logset_playstats_device) on self-written 4P logs (bench_log_text_ingest.make_text, the corpus of
bench_log_dataset.py), in one process:

  (a) the kernel: device events around batches of launches on one stream after a warm-up, median per launch -> events/s, and the achieved
      bytes/s against n_events x 96 B (the records of the stream; the walk itself reads 8 bytes of each event's first record)
  (b) the yardstick: rmj_logset_grp_device on the same set, timed the same way - its k_grp_logs walks the same stream - with every output
      and with the walk's outputs alone (meta, rank, log_of)
  (c) the host restatement (tests/play_stats_ref.kyoku_rows over json.loads dicts) on a sample of the logs (default 64) -> events/s

    python scripts/bench_play_stats.py --logs 4096 --out profiles/play_stats.json
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, launches=50, reps=15, warmup=20):
    """median seconds per call of fn: `reps` windows of `launches` calls between two device events, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / 1e3 / launches)
    return statistics.median(per), min(per), max(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from riichienv_amd import abi, vecenv
    from riichienv_amd.logset import LogSet
    from scripts.bench_log_text_ingest import make_text
    from tests import play_stats_ref as R

    texts = make_text(args.logs)
    ls = LogSet.from_text(texts, num_players=4)
    L, dev, K, n = vecenv.load_lib(), ls.device, ls.n_kyokus, 4
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = torch.empty((K, 4, 16), dtype=torch.int32, device=dev)
    meta, x = torch.empty((K, 4), dtype=torch.int32, device=dev), torch.empty((K, n, 4 * n + 4), dtype=torch.float32, device=dev)
    rank, log_of = torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K,), dtype=torch.int32, device=dev)
    full, walk = abi.GrpOut(meta.data_ptr(), x.data_ptr(), rank.data_ptr(), log_of.data_ptr()), abi.GrpOut(meta.data_ptr(), None, rank.data_ptr(), log_of.data_ptr())

    def stats_call():
        vecenv._chk(L.rmj_logset_playstats_device(ls.handle, n, C.c_void_p(rows.data_ptr()), stream))

    def grp_call(o):
        vecenv._chk(L.rmj_logset_grp_device(ls.handle, n, None, None, C.byref(o), stream))

    t_stats = timed(torch, stats_call)
    t_grp = timed(torch, lambda: grp_call(full))
    t_walk = timed(torch, lambda: grp_call(walk))
    t_stats2 = timed(torch, stats_call)           # again after the others: the spread between two windows of the same code
    # the device table against the restatement on the sample, then the restatement's own speed
    sample = texts[: args.host_sample]
    t0 = time.perf_counter()
    logs = [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in sample]
    t_json = time.perf_counter() - t0
    R.table(logs[:2], n)
    t0 = time.perf_counter()
    want = R.table(logs, n)
    t_host = time.perf_counter() - t0
    got = rows[: len(want)].cpu().numpy()
    assert (got == want).all(), "the device table differs from the restatement"
    host_events = sum(len(l) for l in logs)
    ev = ls.n_events
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), logs=args.logs, events=ev, kyokus=K,
               method="one process, one stream; device events around 50 launches, 15 windows after 20 warm-up launches, median (min, max) seconds per launch; "
                      "host: wall clock of one pass of tests/play_stats_ref.table over parsed dicts of a sample of the same logs",
               playstats_seconds=t_stats, playstats_seconds_again=t_stats2, playstats_events_per_second=ev / t_stats[0],
               playstats_record_bytes_per_second=ev * 96 / t_stats[0], playstats_row_bytes=K * 256,
               grp_seconds=t_grp, grp_walk_only_seconds=t_walk, playstats_over_grp_walk=t_stats[0] / t_walk[0],
               host_sample_logs=len(logs), host_sample_events=host_events, host_restatement_seconds=t_host, host_json_seconds=t_json,
               host_events_per_second=host_events / t_host, host_seconds_scaled=t_host / max(host_events, 1) * ev)
    ls.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
