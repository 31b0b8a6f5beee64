"""Behaviour cloning from MJAI logs, with the samples built on the GPU: the real hanchan log under tests/golden is replayed by
LogSampleBuilder, and a small convolutional net is trained for a few batches on (features, action id, mask) - the fields, in the order,
of riichienv-ml's MCDataset.

    python examples/bc_from_logs.py --batches 20
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from riichienv_amd import replay
    from riichienv_amd.datasets import LogSampleBuilder

    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "126_204_0_mjai.jsonl"))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--features", default="base")
    args = ap.parse_args()

    events = replay.load_mjai_jsonl(args.log)
    builder = LogSampleBuilder([events], game_mode=2, features=args.features)
    builder.run()
    print("builder:", builder.counts())
    net = torch.nn.Sequential(torch.nn.Conv1d(builder.channels, 64, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv1d(64, 32, 3, padding=1), torch.nn.ReLU(),
                              torch.nn.Flatten(), torch.nn.Linear(32 * builder.width, builder.A)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    done, gen = 0, torch.Generator().manual_seed(0)
    while done < args.batches:
        for features, actions, targets, masks, ranks in builder.batches(args.batch_size, shuffle=True, generator=gen):
            logits = net(features).masked_fill(masks == 0, -1e9)
            loss = torch.nn.functional.cross_entropy(logits, actions)
            opt.zero_grad()
            loss.backward()
            opt.step()
            done += 1
            print(f"batch {done}: loss {loss.item():.4f}  mean return {targets.mean().item():+.4f}")
            if done >= args.batches:
                break


if __name__ == "__main__":
    main()
