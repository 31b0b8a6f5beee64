"""Cost of determinizing.  Writes profiles/determinize.json.

On 65 536 4p-red-half games after 150 steps of the device policy that plays to win, over the obs_compact index (one row per acting seat;
rows that share a game with an earlier row are reported as duplicates and not carried out, as the entry point defines):
  determinize  rmj_determinize_device, device time between two events around every single call; before every timed call the working
               batch is overwritten with a fresh copy of the source batch (rmj_copy_games_device, outside the events), so every call
               re-deals the same undetermined state
  hidden       rmj_hidden_targets_device over the same index in the same session (host clock around a window of calls)
  copy         rmj_copy_games_device of the rows' games in the same session (host clock around a window of calls)
  world_set    WorldSet.fork (copy + determinize) and WorldSet.playout to the end of every game for 1 024 rows x 16 worlds (host clock)
Every figure is a median over windows after a warm-up window, with min, max and (max - min) / median next to it.

    python scripts/bench_determinize.py
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def spread(xs):
    med = statistics.median(xs)
    return dict(median=med, min=min(xs), max=max(xs), windows=len(xs), spread_over_median=(max(xs) - min(xs)) / med if med else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--worlds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "determinize.json"))
    a = ap.parse_args()

    import torch

    from riichienv_amd import abi, vecenv
    from riichienv_amd.search import WorldSet
    from riichienv_amd.torch_env import TorchVecEnv

    src = TorchVecEnv(a.games, game_mode=2, seed=1)
    src.env.step_greedy(3, a.steps, auto_reset=False, call_rate_256=64)
    _, index = src.obs_compact()
    index = index.clone()
    rows = int(index.shape[0])
    work = TorchVecEnv(a.games, game_mode=2, seed=2)
    every = torch.arange(a.games, dtype=torch.int32, device=src.device)
    L = src.env.L

    # ---- determinize: events around each call, a fresh copy before it
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    status, det = None, []
    for w in range(a.windows + 1):
        ms = 0.0
        for k in range(a.calls):
            work.copy_games(every, src, every)
            e0.record()
            status = work.determinize(index, seed=1000 * w + k)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        if w:
            det.append(ms / a.calls / 1e3)
    st = status.cpu().numpy()
    carried = int(((st & 15) == abi.DET_OK).sum())
    census = dict(rows=rows, carried_out=carried, duplicate=int((st == abi.DET_DUPLICATE).sum()), chankan=int((st == abi.DET_CHANKAN).sum()),
                  not_acting=int((st == abi.DET_NOT_ACTING).sum()), riichi_noten_worlds=int(((st & 15 == 0) & (st >> 4 != 0)).sum()))

    def host_windows(fn):
        secs = []
        for w in range(a.windows + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            if w:
                secs.append((time.perf_counter() - t0) / a.calls)
        return spread(secs)

    # ---- the same call by the host clock (launch overhead of two kernels included), on games that stay determinized
    det_host = host_windows(lambda: work.determinize(index, seed=5))
    out = src.hidden_compact(index)
    b = abi.HiddenOut(*(out[f].data_ptr() for f in ("opp_hand", "opp_shanten", "opp_waits", "opp_flags")))
    hidden = host_windows(lambda: vecenv._chk(L.rmj_hidden_targets_device(src.env.h, C.c_void_p(index.data_ptr()), rows, None, C.byref(b))))
    games = (index >> 2).to(torch.int32).contiguous()
    copy = host_windows(lambda: work.copy_games(games, src, games))
    d = spread(det)
    res = dict(workload=f"{a.games} 4p-red-half games after {a.steps} steps of step_greedy (call_rate_256=64), the obs_compact index: {rows} rows",
               census=census,
               determinize_seconds_per_call=d, determinize_rows_per_second=rows / d["median"], determinize_carried_out_per_second=carried / d["median"],
               determinize_timing="device events around every call; the working batch is a fresh copy of the source before every timed call",
               determinize_host_clock_seconds_per_call=det_host,
               determinize_host_clock_timing=f"host clock around windows of {a.calls} calls on games that stay determinized from call to call",
               hidden_targets_seconds_per_call=hidden, copy_games_seconds_per_call=copy, calls_per_window=a.calls)
    work.env.close()

    # ---- WorldSet: fork + playout
    ws = WorldSet(src, worlds=a.worlds, max_rows=a.rows)
    g = index >> 2                                   # (the index is in (game, seat) order: the first row of every game)
    first = torch.ones_like(g, dtype=torch.bool)
    first[1:] = g[1:] != g[:-1]
    uniq = index[first][: a.rows]
    fork, play, steps, done = [], [], 0, 0.0
    for w in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ws.fork(uniq, seed=w)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        steps = ws.playout(policy_seed=7, max_steps=6000)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if w:
            fork.append(t1 - t0)
            play.append(t2 - t1)
        done = float(ws.values()[2].float().mean())
    res["world_set"] = dict(rows=int(uniq.shape[0]), worlds=a.worlds, fork_seconds=spread(fork), playout_seconds=spread(play), playout_steps_issued=steps,
                            finished_share=done, note="playout: step_greedy in chunks of 64 steps until every world's game is over, auto_reset=False")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
