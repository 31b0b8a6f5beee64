"""Cost of determinizing.  Writes profiles/determinize.json.

On 65 536 4p-red-half games after 150 steps of the device policy that plays to win, over the obs_compact index (one row per acting seat;
rows that share a game with an earlier row are reported as duplicates and not carried out, as the entry point defines):
  determinize  rmj_determinize_device, device time between two events around every single call; before every timed call the working
               batch is overwritten with a fresh copy of the source batch (rmj_copy_games_device, outside the events), so every call
               re-deals the same undetermined state
  tenpai       the same call with RMJ_DETF_RIICHI_TENPAI (riichi_tenpai=True), timed the same way in windows that alternate with the plain
               call's; with --parent-lib PATH (a library built from the parent commit) the plain call of that library too, on a batch
               of its own, in the same alternation.  Next to it: the share of rows with a repairable seat (an opponent in riichi with
               13, 10, ... tiles), the mean number of exchanges per repaired seat (tiles of the seat's final hand that the plain re-deal
               of the same seed did not give it) and the share of riichi seats left not tenpai with the flag and without it
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
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its plain call is timed in the same session")
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
    pwork = None
    if a.parent_lib:   # a second batch whose calls go to the parent's library (same handle layout, its own code object)
        own, par = vecenv._LIB, C.CDLL(os.path.abspath(a.parent_lib))
        for name, argtypes, *restype in abi.PROTOTYPES:
            if hasattr(par, name):
                getattr(par, name).argtypes = argtypes
                if restype:
                    getattr(par, name).restype = restype[0]
        vecenv._LIB = par
        try:
            pwork = TorchVecEnv(a.games, game_mode=2, seed=2)
        finally:
            vecenv._LIB = own

    # ---- determinize: events around each call, a fresh copy before it; plain, flagged and the parent's plain call window by window
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(env, w, **kw):
        ms, status = 0.0, None
        for k in range(a.calls):
            env.copy_games(every, src, every)
            e0.record()
            status = env.determinize(index, seed=1000 * w + k, **kw)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / a.calls / 1e3, status

    status, det, det_fix, det_par = None, [], [], []
    for w in range(a.windows + 1):
        t_plain, status = window(work, w)
        t_fix, status_fix = window(work, w, riichi_tenpai=True)
        t_par = window(pwork, w)[0] if pwork is not None else None
        if w:
            det.append(t_plain)
            det_fix.append(t_fix)
            if t_par is not None:
                det_par.append(t_par)
    st = status.cpu().numpy()
    # what the repair did in the last call of the last window: the riichi opponents of the carried-out rows before and after
    plain_hid = work.hidden_compact(index)   # (work holds the flagged world of that call)
    fl_fix, hand_fix = plain_hid["opp_flags"].cpu().numpy(), plain_hid["opp_hand"].cpu().numpy().astype(int)
    work.copy_games(every, src, every)
    work.determinize(index, seed=1000 * a.windows + a.calls - 1)
    plain_hid = work.hidden_compact(index)
    fl_plain, hand_plain = plain_hid["opp_flags"].cpu().numpy(), plain_hid["opp_hand"].cpu().numpy().astype(int)
    ok = ((st & 15) == abi.DET_OK)[:, None]
    riichi = ok & ((fl_fix & abi.HIDDEN_RIICHI) != 0)
    repairable = riichi & (hand_fix.sum(axis=2) % 3 == 1)
    exchanged = (abs(hand_fix - hand_plain).sum(axis=2) // 2)[repairable]
    st_fix = status_fix.cpu().numpy()
    tenpai = dict(rows_with_a_repairable_seat_share=float(repairable.any(axis=1).sum() / max(1, ok.sum())),
                  repairable_seats=int(repairable.sum()), riichi_seats=int(riichi.sum()),
                  mean_exchanges_per_repaired_seat=float(exchanged.mean()) if exchanged.size else 0.0,
                  swapped_worlds=int(((st_fix & abi.DET_SWAPPED) != 0).sum()),
                  riichi_seats_not_tenpai_share_with_flag=float((riichi & ((fl_fix & abi.HIDDEN_TENPAI) == 0)).sum() / max(1, riichi.sum())),
                  riichi_seats_not_tenpai_share_without_flag=float((riichi & ((fl_plain & abi.HIDDEN_TENPAI) == 0)).sum() / max(1, riichi.sum())))
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
    b = abi.row_struct("hidden", out)
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
               determinize_tenpai_seconds_per_call=spread(det_fix), determinize_tenpai_over_plain=statistics.median(det_fix) / d["median"],
               determinize_tenpai_census=tenpai,
               determinize_parent_seconds_per_call=spread(det_par) if det_par else "to be measured on the target (--parent-lib)",
               determinize_plain_within_parent_spread=(min(det_par) <= d["median"] <= max(det_par)) if det_par else None,
               hidden_targets_seconds_per_call=hidden, copy_games_seconds_per_call=copy, calls_per_window=a.calls)
    work.env.close()
    if pwork is not None:
        pwork.env.close()

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
