"""Cost of the GRP rank model's rows on the device next to the host route they replace, on self-written 4P logs
(bench_log_text_ingest.make_text), in one process:

  (a) device: GrpDataset.from_text(texts).tensors() - split into ingest (the text parsed into a log set, rmj_logset_create_from_text)
      and rows (rmj_logset_grp_device + the label / filter ops around it, to a synchronised stream); best of three after a warm-up
  (b) host: MjaiReplay.from_jsonl of every log file + take_grp_features of every kyoku + the numpy formulas of GrpReplayDataset for every
      seat, on a sample of the logs (default 64), reported per log and scaled to the full count

    python scripts/bench_grp_rows.py --logs 4096 --out profiles/grp_rows.json
"""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def host_route(paths, n=4):
    """GrpReplayDataset.__iter__'s work per file: parse, features of every kyoku, x and y of every seat"""
    from riichienv_amd.replay import MjaiReplay

    S = 35000.0 if n == 3 else 25000.0
    rows = 0
    for path in paths:
        feats = [k.take_grp_features() for k in MjaiReplay.from_jsonl(path).take_kyokus()]
        if not feats:
            continue
        final = np.array(feats[-1]["round_end_scores"][:n], dtype=np.float64)
        for f in feats:
            for p in range(n):
                scores = np.array([f["round_initial_scores"][i] / S for i in range(n)] + [f["round_end_scores"][i] / S for i in range(n)] +
                                  [f["round_delta_scores"][i] / 12000.0 for i in range(n)], dtype=np.float32)
                meta = np.array([f["chang"] / 3.0, f["ju"] / 3.0, f["ben"] / 4.0, f["liqibang"] / 4.0], dtype=np.float32)
                player = np.zeros(n, dtype=np.float32)
                player[p] = 1.0
                np.concatenate([scores, meta, player])
                y = np.zeros(n, dtype=np.float32)
                y[int((-final).argsort(kind="stable").argsort(kind="stable")[p])] = 1.0
                rows += 1
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from riichienv_amd.grp import GrpDataset
    from scripts.bench_log_text_ingest import make_text

    texts = make_text(args.logs)
    runs = []
    for i in range(4):                      # the first run is the warm-up
        ds = GrpDataset.from_text(texts, game_mode=2)
        s = ds.tensors()
        torch.cuda.synchronize()
        if i:
            runs.append(dict(ingest=ds.host_seconds["ingest"], rows=ds.host_seconds["rows"], total=ds.host_seconds["ingest"] + ds.host_seconds["rows"]))
        n_rows, n_kyokus = int(s["x"].shape[0]), ds.n_kyokus
        ds.close()
    best = min(runs, key=lambda r: r["total"])
    sample = texts[: args.host_sample]
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, t in enumerate(sample):
            paths.append(os.path.join(d, f"{i}.jsonl"))
            with open(paths[-1], "wb") as f:
                f.write(t)
        host_route(paths[:4])
        t0 = time.perf_counter()
        host_rows = host_route(paths)
        host = time.perf_counter() - t0
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), logs=args.logs, kyokus=n_kyokus, rows=n_rows,
               text_bytes=int(sum(len(t) for t in texts)),
               method="one process; device: wall clock around GrpDataset.from_text(...).tensors() to a synchronised stream, best of three after a warm-up; "
                      "host: one pass over a sample of the same logs written to files, scaled per log",
               device_seconds=best, host_sample_logs=len(sample), host_sample_rows=host_rows, host_sample_seconds=host,
               host_seconds_per_log=host / max(len(sample), 1), host_seconds_scaled=host / max(len(sample), 1) * args.logs)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
