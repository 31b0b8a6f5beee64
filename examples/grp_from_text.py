"""The GRP rank model end to end on the device: MJAI text -> one LogSet -> GrpDataset -> a few optimiser steps of a 4n+4 -> 128 -> 64 -> n MLP ->
DeviceRewardPredictor.kyoku_rewards -> LogSampleBuilder.finalize -> one BC/CQL batch whose returns are the model's rewards.

    python examples/grp_from_text.py --games 64 --steps 50
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(games=64, steps=50, batch_size=256):
    import torch

    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.grp import DeviceRewardPredictor, GrpDataset
    from riichienv_amd.logset import LogSet
    from riichienv_amd.torch_env import TorchVecEnv

    # self-play text that never leaves the device (any MJAI JSONL works: LogSet.from_jsonl(paths))
    env = TorchVecEnv(games, game_mode=2, seed=1, skip_mjai_logging=False, event_ring=8192)
    env.env.reset()
    for _ in range(40):
        env.env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
        if env.env.status()[2].all():
            break
    text, offsets = env.drain_text(cursor=env.env.log_positions()[0].copy(), peek=True)

    n = 4
    logset = LogSet.from_device_text(text, offsets, num_players=n)      # parsed once, for both stages
    ds = GrpDataset.from_logset(logset)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(4 * n + 4, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, n)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    done, gen, loss = 0, torch.Generator().manual_seed(0), None
    while done < steps:
        for x, y in ds.batches(batch_size, generator=gen):
            loss = torch.nn.functional.cross_entropy(model(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            done += 1
            if done >= steps:
                break
    print("GRP rows:", int(ds.tensors()["x"].shape[0]), "loss after", steps, "steps:", round(float(loss), 4))

    # the trained model's reward per (kyoku, seat) -> the returns of the BC/CQL samples
    b = LogSampleBuilder.from_logset(logset, game_mode=2)
    rewards = DeviceRewardPredictor(model, [10.0, 4.0, -4.0, -10.0], num_players=n).kyoku_rewards(b)
    b.run()
    b.finalize(rewards)
    features, actions, targets, masks, ranks = next(b.batches(batch_size, generator=gen))
    out = {"grp_rows": int(ds.tensors()["x"].shape[0]), "loss": float(loss), "kyokus": int(rewards.shape[0]), "samples": b.counts()["fill"],
           "batch": tuple(features.shape), "target_abs_max": float(targets.abs().max())}
    print("rewards of", out["kyokus"], "kyokus ->", out["samples"], "samples; one batch:", out["batch"], "|G_t| max", round(out["target_abs_max"], 4))
    b.close()
    ds.close()
    logset.close()
    env.env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=256)
    a = ap.parse_args()
    main(a.games, a.steps, a.batch_size)
