#!/usr/bin/env python3
"""What the PPO transition collector costs at trainer scale (65 536 games of 4p-red-half, base feature set, uniform logits: no
network in any figure).  Per repeat a window of STEPS iterations between two HIP events on one stream, after a warm-up; median and
spread over the repeats:
  A  step_sample_obs_compact alone (the loop the library served before the collector), env.step/s;
  B  select_ids + record + step_obs_compact + round_track + the hero's reward + close_segments per step (emit once, timed apart);
  C  the recording half of B written with torch ops only - boolean-index the hero rows, index_copy_ them and their masks into a
     pool, log_softmax + gather.  GAE per kyoku has no loop-free torch form, so C stops at recording (nothing closes, nothing is
     emitted): its time stands against B's select + record only.
Also the record call alone (HIP events around rmj_ppo_record_device) with the bytes it moves, against the copy roof of
profiles/r06_pmc_write_calibration.txt (6.29 TB/s).  Usage: bench_ppo_collect.py [n_games] [out.json] (the result is merged into out.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from riichienv_amd.ppo import PPOCollector  # noqa: E402
from riichienv_amd.torch_env import TorchVecEnv  # noqa: E402

STEPS, WARM, REPEATS, ROOF = 30, 20, 5, 6.29e12


def window(fn, steps=STEPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "repeats": len(xs)}


def main(n=65536, out=os.path.join(ROOT, "profiles", "ppo_collect.json")):
    dev = torch.device("cuda", 0)
    A, res = 82, {"n_games": n, "steps_per_window": STEPS, "warmup_steps": WARM}
    # A: the parent loop
    env = TorchVecEnv(n, game_mode=2, seed=1)
    env.env.step_random(7, 300, auto_reset=True)
    seed = [0]

    def loop_a():
        seed[0] += 1
        env.step_sample_obs_compact(None, seed=seed[0], sync_count=False)

    window(loop_a, WARM)
    a = [window(loop_a) for _ in range(REPEATS)]
    res["A_step_sample_obs_compact"] = dict(spread(a), env_steps_per_s=round(n / statistics.median(a) * 1e3))
    # B: the collector's loop
    cap = int(n * (WARM + STEPS * REPEATS + 10 * REPEATS + 8) * 0.45)   # (a hero acts in about 3 steps of 10)
    col = PPOCollector(env, cap, seed=2)
    env.obs_compact(sync_count=False)
    env.round_track()
    rows = env._cap
    logits = torch.zeros((rows, A), dtype=torch.float32, device=dev)
    full = torch.zeros((n, 4, A), dtype=torch.float32, device=dev)
    values = torch.zeros((rows,), dtype=torch.float32, device=dev)
    h64 = col._hero64
    t_sel_rec = []

    def loop_b():
        seed[0] += 1
        ids = col.select_ids(full, seed[0])
        col.record(ids, logits, values, "compact")
        env.step_obs_compact(ids, sync_count=False)
        ended, delta, _m, _k = env.round_track()
        col.close_segments(ended, (delta.gather(1, h64[:, None])[:, 0].to(torch.float32) * 1e-3).contiguous())

    def sel_rec():
        col.record(col.select_ids(full, seed[0]), logits, values, "compact")

    def rec_only():
        col.record(col._ids, logits, values, "compact")

    window(loop_b, WARM)
    b = [window(loop_b) for _ in range(REPEATS)]
    c0 = col.counts()
    res["B_collector_loop"] = dict(spread(b), env_steps_per_s=round(n / statistics.median(b) * 1e3), counts=c0)
    res["B_over_A"] = round(statistics.median(b) / statistics.median(a), 3)
    # select + record and record alone on one state (the pool keeps filling: the same rows every time)
    f0 = col.counts()["fill"]
    t_sel_rec = [window(sel_rec, 5) for _ in range(REPEATS)]
    f1 = col.counts()["fill"]
    t_rec = [window(rec_only, 5) for _ in range(REPEATS)]
    f2 = col.counts()["fill"]
    per_call = (f2 - f1) // (5 * REPEATS)
    moved = per_call * (74 * 34 * 4 + A) * 2
    res["B_select_plus_record"] = spread(t_sel_rec)
    res["B_record"] = dict(spread(t_rec), rows_per_call=per_call, bytes_read_and_written=moved,
                           TBps=round(moved / statistics.median(t_rec) / 1e9, 3), share_of_copy_roof=round(moved / statistics.median(t_rec) * 1e3 / ROOF, 3))
    assert col.counts()["overflowed"] == 0 and (f1 - f0) // (5 * REPEATS) == per_call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tr = col.transitions()
    e1.record()
    e1.synchronize()
    res["B_emit_once"] = {"ms": round(e0.elapsed_time(e1), 3), "transitions": int(tr["action"].shape[0])}
    del tr
    # C: recording with torch ops only, on the same state (ids of the last select call)
    pool_f = torch.empty((cap // 4, 74, 34), dtype=torch.float32, device=dev)
    pool_m = torch.empty((cap // 4, A), dtype=torch.uint8, device=dev)
    pool_a = torch.empty((cap // 4,), dtype=torch.int64, device=dev)
    pool_lp = torch.empty((cap // 4,), dtype=torch.float32, device=dev)
    fill = [0]
    obs, index, count = env._cobs, env._cidx, env._ccnt
    g = torch.arange(n, device=dev)

    def torch_record():
        ids = col._ids
        k = int(count.item())                                       # boolean indexing needs the count on the host anyway
        idx = index[:k].to(torch.int64)
        hero_row = (h64[idx >> 2] == (idx & 3)) & (ids.view(-1)[idx] >= 0)
        rows_ = hero_row.nonzero()[:, 0]
        m = rows_.shape[0]
        if fill[0] + m > pool_f.shape[0]:
            fill[0] = 0
        dst = torch.arange(fill[0], fill[0] + m, device=dev)
        gi = idx[rows_]
        mask = env.mask.view(n * 4, 82)[gi]
        act = ids.view(-1)[gi].to(torch.int64)
        pool_f.index_copy_(0, dst, obs[rows_])
        pool_m.index_copy_(0, dst, mask)
        pool_a.index_copy_(0, dst, act)
        lp = torch.log_softmax(logits[rows_].masked_fill(mask == 0, -1e9), dim=-1).gather(1, act[:, None])[:, 0]
        pool_lp.index_copy_(0, dst, lp)
        fill[0] += m

    def torch_sel_rec():
        col.select_ids(full, seed[0])
        torch_record()

    window(torch_sel_rec, 3)
    c = [window(torch_sel_rec, 5) for _ in range(REPEATS)]
    res["C_torch_select_plus_record"] = dict(spread(c), note="recording only: GAE per kyoku has no loop-free torch form, nothing closes or is emitted")
    res["record_B_over_C"] = round(statistics.median(t_sel_rec) / statistics.median(c), 3)
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["cost"] = res
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main(*([int(sys.argv[1])] if len(sys.argv) > 1 else []), **({"out": sys.argv[2]} if len(sys.argv) > 2 else {}))
