"""A verdict for every MJAI log before training on it: JSONL files -> LogSet.from_jsonl (parsed on the device, the logs that do not parse
kept) -> LogSet.validate() -> the summary, the first findings, and a second log set of the good files only, ready for LogSampleBuilder /
GrpDataset.  What riichienv-ml's scripts/validate_logs.py does one log at a time through Python.

    python examples/validate_logs.py --players 4 logs/*.jsonl
    python examples/validate_logs.py --accept UNFINISHED drained/*.jsonl.gz
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(paths, players=4, accept=(), show=10, rule=None):
    from riichienv_amd.logset import LogSet

    logset = LogSet.from_jsonl(paths, num_players=players, on_error="keep")
    report = logset.validate(rule=rule)
    summary = report.summary()
    print(f"{logset.M} logs, {logset.n_events} events, {logset.n_kyokus} kyokus")
    for name, count in summary.items():
        if count:
            print(f"  {name:20s}{count:8d}")
    good = report.good_ids(accept)
    bad = sorted(set(range(logset.M)) - set(good.tolist()))
    for i in bad[:show]:
        print(" ", report.describe(i), f"[{paths[i]}]")
    if len(bad) > show:
        print(f"  ... and {len(bad) - show} more")
    logset.close()
    good_paths = [paths[i] for i in good]
    clean = LogSet.from_jsonl(good_paths, num_players=players)      # every one of them parses: on_error="raise" holds
    print(f"kept {clean.M} of {len(paths)} logs ({clean.n_events} events)")
    return summary, good_paths, clean


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--players", type=int, default=4, choices=(3, 4))
    ap.add_argument("--accept", nargs="*", default=[], help="codes besides OK that count as good, e.g. UNFINISHED")
    ap.add_argument("--show", type=int, default=10)
    ap.add_argument("--rule", default=None, choices=("tenhou", "mjsoul"))
    a = ap.parse_args()
    main(a.paths, a.players, tuple(a.accept), a.show, a.rule)[2].close()
