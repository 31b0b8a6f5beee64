"""Lossless logs end to end, three ways in one process: the workload of bench.py's log_drain leg (65 536 games of 4p-red-half, event ring
512, rounds x (a chunk-step auto-reset rollout + a drain of every slot's records)) with the text delivered by
  (a) drain_logs(raw=True, out=reused buffer): device gather, one copy of the records, the C formatter on the host's threads (bench.py's path);
  (b) drain_text(): the device formatter (rmj_drain_text), then one copy of the text into the library's pinned buffer;
  (c) rmj_drain_text with RMJ_TEXT_ON_DEVICE: the device formatter, the text stays on the GPU.
The paths alternate (a, b, c, a, b, c, ...) on the same seeds, so they format the same records; for each the SHA-256 of the text and of the
offsets of every timed round (digested outside the timed spans; (c) copied down for it) must agree, with no record lost.
end_to_end_env_steps_per_s = env.steps of the timed rounds / (rollout + drain time); the best of --reps repetitions per path is reported.
usage: python scripts/bench_log_text.py [--games 65536] [--rounds 3] [--chunk 100] [--reps 2] [--paths abc] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from riichienv_amd import abi, vecenv  # noqa: E402

POLICY_SEED = 0xC0FFEE


def _device_copy(v):
    import torch

    from riichienv_amd.torch_env import _CudaArray

    offs = torch.as_tensor(_CudaArray(v.text_offsets, (v.n_games + 1,), "<i8", None), device="cuda").cpu().numpy().astype(np.uint64)
    text = torch.as_tensor(_CudaArray(v.text, (int(v.bytes),), "|u1", None), device="cuda").cpu().numpy() if v.bytes else np.zeros(0, np.uint8)
    return text, offs


def run_path(path, games, rounds, chunk, ring, mode):
    env = vecenv.VecRiichiEnv(games, game_mode=mode, seed=0, rule_bits=abi.RULE_TENHOU, event_ring=ring)
    env.reset()
    env._log_cursor()
    env.step_random(POLICY_SEED, chunk, auto_reset=True)   # untimed first round: sizes the buffers, warms the pinned memory
    text_buf = None
    if path == "a":
        buf0, toffs0 = env.drain_logs(raw=True)
        text_buf = np.empty(int(toffs0[-1]) * 2 + (1 << 20), np.uint8)
        del buf0
    else:
        env._text_call(-1, None, False, path == "c")
    h_text, h_offs = hashlib.sha256(), hashlib.sha256()
    s0 = env.total_steps()
    ev = tb = 0
    roll_s = drain_s = 0.0
    ms = np.zeros(3)
    for _ in range(rounds):
        ta = time.perf_counter()
        env.step_random(POLICY_SEED, chunk, auto_reset=True)
        env.sync()
        tb_ = time.perf_counter()
        if path == "a":
            tms = []
            buf, toffs = env.drain_logs(raw=True, timings=tms, out=text_buf)
            tc = time.perf_counter()
            text = buf[: int(toffs[-1])]
        else:
            v = env._text_call(-1, None, False, path == "c")
            tc = time.perf_counter()
            tms = list(v.ms)
            text, toffs = env._host_text(v) if path == "b" else _device_copy(v)
        roll_s += tb_ - ta
        drain_s += tc - tb_
        ms += np.array(tms)
        ev += int(env.last_drain_events)
        tb += int(toffs[-1])
        h_text.update(memoryview(np.ascontiguousarray(text)))
        h_offs.update(np.ascontiguousarray(toffs, dtype=np.uint64).tobytes())
    made = env.total_steps() - s0
    lost = int(env.events_lost().sum())
    env.close()
    names = ["gather_ms", "copy_ms", "format_ms"] if path == "a" else ["device_format_ms", "copy_ms", "drain_total_ms"]
    out = {"games": games, "rollout_steps": rounds * chunk, "drain_every_steps": chunk, "event_ring": ring, "events": ev, "text_bytes": tb,
           "lost_events": lost, "rollout_s": roll_s, "drain_s": drain_s, "events_per_s": ev / max(drain_s, 1e-9),
           "end_to_end_env_steps_per_s": made / max(roll_s + drain_s, 1e-9), "sha256_text": h_text.hexdigest(), "sha256_offsets": h_offs.hexdigest()}
    out.update({k: float(x) for k, x in zip(names, ms)})
    return out


WHAT = {"a": "drain_logs(raw=True, out=reused): device gather of the records, one copy, C formatter on the host's threads (bench.py log_drain)",
        "b": "drain_text(): device formatter (k_text_size / k_text_write), one copy of the text into the library's pinned buffer",
        "c": "rmj_drain_text with RMJ_TEXT_ON_DEVICE: device formatter, the text stays on the GPU (copied down only for the digest, untimed)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--ring", type=int, default=512)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--paths", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_text_device.json"))
    a = ap.parse_args()
    if vecenv.load_lib().rmj_device_count() < 1:
        print("bench_log_text.py: no GPU visible", file=sys.stderr)
        return 2
    runs = {p: [] for p in a.paths}
    for _ in range(a.reps):
        for p in a.paths:
            runs[p].append(run_path(p, a.games, a.rounds, a.chunk, a.ring, a.mode))
    res = {}
    for p, rs in runs.items():
        best = max(rs, key=lambda r: r["end_to_end_env_steps_per_s"])
        best["all_end_to_end_env_steps_per_s"] = [r["end_to_end_env_steps_per_s"] for r in rs]
        best["what"] = WHAT[p]
        res[p] = best
    digests = {(r["sha256_text"], r["sha256_offsets"]) for rs in runs.values() for r in rs}
    lost = sum(r["lost_events"] for rs in runs.values() for r in rs)
    res["digests_equal"] = len(digests) == 1
    res["lost_events_total"] = lost
    res["workload"] = (f"{a.games} games, mode {a.mode}, event_ring {a.ring}, {a.rounds} x ({a.chunk}-step auto-reset rollout + drain), paths "
                       f"alternated {a.reps} x in one process; end_to_end = env.steps / (rollout + drain time)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({p: {"e2e": res[p]["end_to_end_env_steps_per_s"], "drain_s": res[p]["drain_s"]} for p in a.paths} |
                     {"digests_equal": res["digests_equal"], "lost": lost}))
    return 0 if res["digests_equal"] and lost == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
