#!/usr/bin/env python3
"""Observation batches (rmj_encode_batch_device) at trainer scale: per feature set of the mode,
  * encoder time - compact and dense over the same states, HIP events on the handle's stream - with the bytes written and the rate,
    next to the existing encoders of the same states (rmj_encode_compact_device / rmj_encode_device(2) for encode(),
    rmj_encode_extended_device(2) for encode_extended());
  * trainer loop env.step/s - uniform sample_ids + step + the batch a policy consumes: step_obs_compact (compact) against
    step() + obs() + a gather of the acting rows (dense; what scripts/bench_torch_env.py runs for extended=True);
  * the buffer bytes of each path.
Usage: bench_obs_batch.py [n_games] [mode] [out.json]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from riichienv_amd import abi, vecenv  # noqa: E402
from riichienv_amd.torch_env import TorchVecEnv  # noqa: E402

REPS, LOOP_STEPS, WARM = 20, 60, 10


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def encoders(n, mode):
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=1, skip_mjai_logging=True)
    vecenv._chk(env.L.rmj_set_stream(env.h, C.c_void_p(torch.cuda.current_stream().cuda_stream), 0))
    env.reset()
    env.step_random(7, 40, auto_reset=True)   # mid-round states: claims, melds, riichi
    torch.cuda.synchronize()
    w = 27 if mode >= 3 else 34
    sets = ["base", "extended"] + ([] if mode >= 3 else ["discard_shanten"])
    cap = n + n // 2 + 1
    idx = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {}
    for s in sets:
        ch = abi.FEATURE_CHANNELS[abi.FEATURES[s]]
        row = ch * w * 4
        comp = torch.zeros((cap, ch * w), dtype=torch.float32, device="cuda")
        dense = torch.zeros((n, 4, ch * w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ms_c = timed(lambda: env.encode_batch_device(s, comp.data_ptr(), True, idx.data_ptr(), cap, cnt.data_ptr()))
        k = int(cnt.item())
        ms_d = timed(lambda: env.encode_batch_device(s, dense.data_ptr()))
        r = {"channels": ch, "acting_rows": k, "bytes_written": k * row, "compact_ms": round(ms_c, 4), "dense_ms": round(ms_d, 4),
             "compact_GBps": round(k * row / ms_c / 1e6, 1), "dense_GBps": round(k * row / ms_d / 1e6, 1),
             "compact_buffer_bytes": cap * (row + 4) + 4, "dense_buffer_bytes": n * 4 * row}
        if s == "extended":
            r["existing_dense_ms"] = round(timed(lambda: vecenv._chk(env.L.rmj_encode_extended_device(env.h, 2, C.c_void_p(dense.data_ptr())))), 4)
            r["compact_over_existing_dense"] = round(ms_c / r["existing_dense_ms"], 3)
        if s == "base":
            r["existing_compact_ms"] = round(timed(lambda: env.encode_compact_device(comp.data_ptr(), idx.data_ptr(), cap, cnt.data_ptr())), 4)
            r["existing_dense_ms"] = round(timed(lambda: vecenv._chk(env.L.rmj_encode_device(env.h, 2, C.c_void_p(dense.data_ptr())))), 4)
        out[s] = r
        print(json.dumps({"mode": mode, "n": n, "features": s, "encoder": r}), flush=True)
        del comp, dense
        torch.cuda.empty_cache()
    env.close()
    return out


def loop(n, mode, features, compact):
    e = TorchVecEnv(n, game_mode=mode, seed=2, features=features)
    it = [0]

    def one():
        it[0] += 1
        ids = e.sample_ids(None, seed=it[0])
        if compact:
            return e.step_obs_compact(ids)[0]
        e.step(ids)
        obs = e.obs(only_active=True)
        return obs.reshape(n * 4, e.channels, e.width)[e.active().reshape(-1)]

    for _ in range(WARM):
        one()
    torch.cuda.synchronize()
    s0 = e.env.total_steps()
    t0 = time.perf_counter()
    rows = 0
    for _ in range(LOOP_STEPS):
        rows += one().shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = e.env.total_steps() - s0
    row = e.channels * e.width * 4
    mem = e._cobs_buf.numel() * 4 + e._cidx.numel() * 4 + 4 if compact else e._obs_buf.numel() * 4
    r = {"env_steps_per_s": round(steps / dt), "ms_per_iteration": round(1e3 * dt / LOOP_STEPS, 3), "rows_per_iteration": rows / LOOP_STEPS,
         "buffer_bytes": int(mem), "row_bytes": row}
    e.env.close()
    del e
    torch.cuda.empty_cache()
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    mode = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    res = {"n_games": n, "mode": mode, "device": torch.cuda.get_device_name(0), "encoders": encoders(n, mode), "trainer_loop": {}}
    for s in ["base", "extended"] + ([] if mode >= 3 else ["discard_shanten"]):
        c, d = loop(n, mode, s, True), loop(n, mode, s, False)
        res["trainer_loop"][s] = {"compact": c, "dense": d, "compact_over_dense": round(c["env_steps_per_s"] / d["env_steps_per_s"], 3)}
        print(json.dumps({"mode": mode, "n": n, "features": s, "trainer_loop": res["trainer_loop"][s]}), flush=True)
    if len(sys.argv) > 3:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
        with open(sys.argv[3], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
