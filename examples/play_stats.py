"""How two policies played, read from their own logs on the device: two greedy rollouts that differ in how often they call
(call_rate_256 = 0 and 64) -> TorchVecEnv.drain_text -> LogSet.from_device_text -> stats.summarize, printed side by side.  The text, the
records and the per-(kyoku, seat) table never leave the GPU; one small vector of sums per summary does.

    python examples/play_stats.py --games 256 --steps 20000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rollout(games, steps, call_rate_256, game_mode=2, seed=1):
    """the summary of `games` self-played games (at most `steps` steps each) and of seat 0 alone"""
    from riichienv_amd import stats
    from riichienv_amd.logset import LogSet
    from riichienv_amd.torch_env import TorchVecEnv

    env = TorchVecEnv(games, game_mode=game_mode, seed=seed, skip_mjai_logging=False, event_ring=8192)
    env.env.reset()
    done = 0
    while done < steps and not env.env.status()[2].all():
        chunk = min(500, steps - done)
        env.env.step_greedy(7, chunk, auto_reset=False, call_rate_256=call_rate_256)
        done += chunk
    text, offsets = env.drain_text(cursor=env.env.log_positions()[0].copy(), peek=True)
    logset = LogSet.from_device_text(text, offsets, num_players=3 if game_mode >= 3 else 4)
    table = stats.play_stats(logset)                       # rows [K, 4, 16] int32 on the device: also the auxiliary targets of a network
    out = {"kyokus": int(table["rows"].shape[0]), "all": stats.summarize(logset, table=table), "seat0": stats.summarize(logset, hero=[0] * games, table=table)}
    logset.close()
    env.env.close()
    return out


def main(games=256, steps=20000):
    res = {rate: rollout(games, steps, rate) for rate in (0, 64)}
    keys = [k for k in res[0]["all"] if k != "rank_rates"]
    print(f"{games} games each; kyokus: {res[0]['kyokus']} / {res[64]['kyokus']}")
    print(f"{'':22s}{'call_rate_256=0':>18s}{'call_rate_256=64':>18s}")
    for k in keys:
        print(f"{k:22s}{res[0]['all'][k]:18.4f}{res[64]['all'][k]:18.4f}")
    print("seat 0 alone: rank_mean", " / ".join(f"{res[r]['seat0']['rank_mean']:.3f}" for r in (0, 64)),
          " win_rate", " / ".join(f"{res[r]['seat0']['win_rate']:.3f}" for r in (0, 64)))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20000)
    a = ap.parse_args()
    main(a.games, a.steps)
