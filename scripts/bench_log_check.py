"""Cost of LogSet.validate() (rmj_logcheck_*) on self-written 4P logs (bench_log_text_ingest.make_text, the corpus of
bench_play_stats.py), in one process, against what it is there to protect:

  (a) validate(): the checking replay of the whole set, two launches per event index
  (b) LogSampleBuilder.run() with base features on the same set: the sample build's replay, four launches per event index and the pool
  (c) the host restatement (tests/log_check_ref.check_log over json.loads dicts) on a sample of the logs (default 64)

(a) and (b) are timed as windows between two device events on one stream, median of the windows, after a warm-up; a window is one whole
call ((a): environment, checker, replay, report; (b): clear() + run() of a builder made once), so (a) carries set-up cost that (b) does
not.  The expectation to confirm or refute: a validation costs less than the sample build.

    python scripts/bench_log_check.py --logs 4096 --out profiles/log_check.json
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, reps=7, warmup=2):
    """median (min, max) seconds per call of fn: `reps` windows of one call between two device events, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / 1e3)
    return statistics.median(per), min(per), max(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.logset import LogSet
    from scripts.bench_log_text_ingest import make_text
    from tests import log_check_ref as R

    texts = make_text(args.logs)
    ls = LogSet.from_text(texts, num_players=4)
    report = ls.validate()
    summary = report.summary()
    t_check = timed(torch, lambda: ls.validate())
    b = LogSampleBuilder.from_logset(ls, game_mode=2, features="base")

    def build():
        b.clear()
        b.run()

    t_build = timed(torch, build)
    counts = b.counts()
    t_check2 = timed(torch, lambda: ls.validate())      # again after the other: the spread between two windows of the same code
    b.close()
    # the restatement on the sample: the same verdicts, then its own speed
    sample = texts[: args.host_sample]
    logs = [[json.loads(l) for l in t.split(b"\n") if l.strip()] for t in sample]
    R.check_log(logs[0], 4, 2)
    t0 = time.perf_counter()
    want = [R.check_log(l, 4, 2) for l in logs]
    t_host = time.perf_counter() - t0
    got = list(zip(*[x[: len(want)].cpu().tolist() for x in (report.code, report.event, report.kyoku, report.seat)]))
    assert got == want, "the device verdicts differ from the restatement"
    host_events, ev = sum(len(l) for l in logs), ls.n_events
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), logs=args.logs, events=ev, kyokus=ls.n_kyokus, longest_log=ls.longest_log,
               method="one process, one stream; device events around one whole call, 7 windows after 2 warm-up calls, median (min, max) seconds; validate() "
                      "includes making its environment and checker, run() is clear() + run() of a builder made once; host: wall clock of "
                      "tests/log_check_ref.check_log over parsed dicts of a sample of the same logs",
               summary=summary, validate_seconds=t_check, validate_seconds_again=t_check2, validate_events_per_second=ev / t_check[0],
               sample_build_seconds=t_build, sample_build_counts=counts, validate_over_sample_build=t_check[0] / t_build[0],
               host_sample_logs=len(logs), host_sample_events=host_events, host_restatement_seconds=t_host, host_events_per_second=host_events / t_host,
               host_seconds_scaled=t_host / max(host_events, 1) * ev)
    ls.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
