"""Cost of the discard efficiency table.  Writes profiles/discard_table.json.

  live      rmj_discard_table_device next to rmj_hidden_targets_device and to rmj_encode_batch_device(extended, compact) - which runs the
            folding ukeire walk once per row - over the same obs_compact index of 65 536 4p-red-half games after 150 greedy steps, windows
            of the three alternating in one process.
  builder   run() + finalize() of LogSampleBuilder plain and efficiency=True over the log set of scripts/bench_hidden_targets.py (one
            LogSet, two builders, windows alternating).
Every figure is a median over windows, each window a host clock around work that ends in a device synchronise, after a warm-up window;
the spread (min, max, and max - min over the median) is written next to it.  The flagship benchmark against the parent commit's is
bench.py's own business: run both in one session and put the lines next to each other (--bench-lines FILE merges them into the result).

    python scripts/bench_discard_table.py
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "scripts"))
from bench_hidden_targets import builder_windows, spread  # noqa: E402


def live_windows(n_games, windows, calls):
    """{"dtable": [...], "dtable_no_mask": [...], "hidden": [...], "encode_extended": [...]} seconds per call, windows alternating; stats of the rows"""
    import ctypes as C

    import torch

    from riichienv_amd import abi, vecenv
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(n_games, game_mode=2, seed=1, features="extended")
    env.env.step_greedy(3, 150, auto_reset=True, call_rate_256=64)
    obs, index = env.obs_compact()
    rows = int(index.shape[0])
    L, h, ix = env.env.L, env.env.h, C.c_void_p(index.data_ptr())
    tab = env.discard_table_compact(index)
    tb = abi.row_struct("discard_table", tab)
    tb3 = abi.row_struct("discard_table", tab)
    tb3.mask = None
    hid = env.hidden_compact(index)
    hb = abi.row_struct("hidden", hid)
    calls_of = {"dtable": lambda: L.rmj_discard_table_device(h, ix, rows, None, 0, C.byref(tb)),
                "dtable_no_mask": lambda: L.rmj_discard_table_device(h, ix, rows, None, 0, C.byref(tb3)),
                "hidden": lambda: L.rmj_hidden_targets_device(h, ix, rows, None, C.byref(hb)),
                "encode_extended": lambda: L.rmj_encode_batch_device(h, env._batch(True))}
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
    sh = tab["shanten"]
    cols = sh[:, :34] != abi.DTAB_NONE
    # the two device paths agree on what they share: channels 78..80 of the rows just encoded against column 34
    # (as integers: torch divides by a scalar through its reciprocal, which is not the encoder's float32 division)
    agree = bool(((obs[:rows, 79, 0] * 34.0).round() == tab["accept"][:, 34].float()).all()) and bool(((obs[:rows, 80, 0] * 80.0).round() == tab["ukeire"][:, 34].float()).all())
    stats = dict(rows=rows, rows_with_a_discard=int(cols.any(dim=1).sum()), columns=int(cols.sum()), mean_shanten=float(sh[:, 34].float().mean()),
                 tenpai_columns=int((sh[:, :34] == 0).sum()), sum_of_ukeire=int(tab["ukeire"].to(torch.int64).sum()), channels_79_80_agree=agree)
    env.env.close()
    return secs, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3, help="run() + finalize() per window")
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50, help="entry calls per window")
    ap.add_argument("--bench-lines", default=None, help="a file of bench.py result lines, 'parent' or 'this' in front of each: merged into the result")
    ap.add_argument("--skip-builder", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "discard_table.json"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    res = dict(workload=f"{args.games} 4p-red-half games after 150 greedy steps (auto-reset), the obs_compact index; a window = {args.calls} calls ending in a "
                        "synchronise, variants alternating")
    secs, stats = live_windows(args.games, args.windows, args.calls)
    live = {name: spread(v) for name, v in secs.items()}
    res["live"] = dict(stats, calls_per_window=args.calls, dtable_seconds_per_call=live["dtable"], dtable_no_mask_seconds_per_call=live["dtable_no_mask"],
                       hidden_seconds_per_call=live["hidden"], encode_extended_seconds_per_call=live["encode_extended"],
                       dtable_over_hidden=live["dtable"]["median"] / live["hidden"]["median"],
                       dtable_over_encode_extended=live["dtable"]["median"] / live["encode_extended"]["median"],
                       dtable_rows_per_second=stats["rows"] / live["dtable"]["median"], bytes_written_per_row=35 * 11)
    if not args.skip_builder:
        times, counts, n_logs = builder_windows(args.logs, args.windows, args.runs, {"plain": {}, "efficiency": {"efficiency": True}})
        assert counts["plain"] == counts["efficiency"]
        sp = {k: spread(v) for k, v in times.items()}
        res["builder"] = dict(workload=f"{n_logs} self-written 4p-red-half logs, base features, include_pass, skip_single_action; a window = {args.runs} x (clear, run, "
                                       "finalize) ending in a synchronise, variants alternating",
                              samples=counts["plain"]["fill"], steps=counts["plain"]["steps_done"], overflowed=counts["plain"]["overflowed"],
                              plain_seconds=sp["plain"], efficiency_seconds=sp["efficiency"], efficiency_over_plain=sp["efficiency"]["median"] / sp["plain"]["median"])
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
