#!/usr/bin/env python3
"""Collect one pool of PPO transitions on the GPU with a tiny conv policy (needs an MI355X; run from the repo root after
`python -c "import __graft_entry__ as g; g.build()"`): what riichienv-ml's PPO worker returns from collect_episodes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from riichienv_amd.ppo import PPOCollector  # noqa: E402
from riichienv_amd.torch_env import TorchVecEnv  # noqa: E402


class TinyPolicy(torch.nn.Module):
    def __init__(self, channels=74, width=34, actions=82):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Conv1d(channels, 32, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten())
        self.pi, self.v = torch.nn.Linear(32 * width, actions), torch.nn.Linear(32 * width, 1)

    @torch.no_grad()
    def forward(self, obs):
        x = self.body(obs)
        return self.pi(x), self.v(x)[:, 0]


def main(n=4096, steps=300):
    env = TorchVecEnv(n, game_mode="4p-red-half", seed=0)
    policy, baseline = TinyPolicy().to(env.device), TinyPolicy().to(env.device)
    col = PPOCollector(env, capacity=n * steps // 2, gamma=0.99, gae_lambda=0.95)   # hero: one seeded seat per game
    col.collect(policy, baseline, steps)                       # hero samples from `policy`, the other seats take `baseline`'s best id
    batch = col.transitions()                                  # features, mask, action, log_prob, advantage, return - on the device
    stats = col.stats()
    print({k: tuple(v.shape) for k, v in batch.items()})
    print({k: round(v, 4) if isinstance(v, float) else v for k, v in stats.items()})
    return stats


if __name__ == "__main__":
    main()
