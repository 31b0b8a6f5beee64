"""Behaviour cloning from MJAI text without Python work per event: the JSONL files are read as bytes, parsed into event records on the
GPU (LogSampleBuilder.from_jsonl -> rmj_logset_create_from_text) and replayed into samples there; then self-play text that never leaves
the device goes the same way (TorchVecEnv.drain_text -> LogSampleBuilder.from_device_text).

    python examples/bc_from_text.py --batches 20
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def train(builder, batches, batch_size):
    import torch

    net = torch.nn.Sequential(torch.nn.Conv1d(builder.channels, 64, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                              torch.nn.Linear(64 * builder.width, builder.A)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    done, gen = 0, torch.Generator().manual_seed(0)
    while done < batches:
        for features, actions, targets, masks, ranks in builder.batches(batch_size, shuffle=True, generator=gen):
            loss = torch.nn.functional.cross_entropy(net(features).masked_fill(masks == 0, -1e9), actions)
            opt.zero_grad()
            loss.backward()
            opt.step()
            done += 1
            if done >= batches:
                break
    return float(loss)


def main():
    from riichienv_amd.datasets import LogSampleBuilder
    from riichienv_amd.torch_env import TorchVecEnv

    golden = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", nargs="*", default=[os.path.join(golden, "126_204_0_mjai.jsonl")], help="JSONL files (gzip is detected)")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--games", type=int, default=64, help="self-play games of the device-text part")
    args = ap.parse_args()

    # files -> bytes -> records and score tables on the device; a file that does not parse is skipped and listed
    b = LogSampleBuilder.from_jsonl(args.logs, game_mode=2, on_error="drop")
    b.run()
    print("files:", b.counts(), "dropped:", b.dropped, "ingest seconds:", round(b.host_seconds["ingest"], 4))
    print("loss after", args.batches, "batches:", round(train(b, args.batches, args.batch_size), 4))
    b.close()

    # self-play -> text -> samples, all on the device
    env = TorchVecEnv(args.games, game_mode=2, seed=1, skip_mjai_logging=False, event_ring=8192)
    env.env.reset()
    for _ in range(40):
        env.env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
        if env.env.status()[2].all():
            break
    text, offsets = env.drain_text(cursor=env.env.log_positions()[0].copy(), peek=True)
    b = LogSampleBuilder.from_device_text(text, offsets, game_mode=2)
    b.run()
    print("self-play:", int(text.numel()), "bytes of text on the device ->", b.counts())
    print("loss after", args.batches, "batches:", round(train(b, args.batches, args.batch_size), 4))
    b.close()
    env.env.close()


if __name__ == "__main__":
    main()
