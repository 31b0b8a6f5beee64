"""The second half of a training sample: what the deciding seat could not see.  A few self-played games -> their own logs ->
LogSampleBuilder(hidden=True) -> per opponent (shimocha, toimen, kamicha) the tenpai rate and the mean shanten at the moment of the
decision, and how often the discard that was chosen lay in some opponent's waits.  Everything between the logs and the sums is on the GPU.

    python examples/hidden_targets.py --games 64 --steps 20000
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def self_written_logs(games, steps, game_mode=2, seed=3):
    """complete games under the device policy that plays to win, as lists of MJAI event dicts"""
    from riichienv_amd import vecenv

    env = vecenv.VecRiichiEnv(games, game_mode=game_mode, seed=seed, event_ring=8192)
    env.reset()
    done = 0
    while done < steps and not env.status()[2].all():
        chunk = min(500, steps - done)
        env.step_greedy(7, chunk, auto_reset=False, call_rate_256=64)
        done += chunk
    finished = env.status()[2].astype(bool)
    logs = [[json.loads(s) for s in g] for g, ok in zip(env.mjai_logs(), finished) if ok]
    env.close()
    return logs


def main(games=64, steps=20000, game_mode=2):
    import torch

    from riichienv_amd import abi
    from riichienv_amd.datasets import LogSampleBuilder

    logs = self_written_logs(games, steps, game_mode)
    b = LogSampleBuilder(logs, game_mode=game_mode, hidden=True, include_pass=False)
    b.run()
    s = b.samples()
    counts = b.counts()
    flags, shanten, waits, action = s["opp_flags"], s["opp_shanten"], s["opp_waits"], s["action"]
    present = (flags & abi.HIDDEN_PRESENT) != 0
    tenpai = (flags & abi.HIDDEN_TENPAI) != 0
    n_opp = 2 if game_mode >= 3 else 3
    out = {"logs": len(logs), "samples": int(action.shape[0]), "overflowed": counts["overflowed"], "tenpai_rate": [], "mean_shanten": []}
    for r in range(n_opp):
        k = present[:, r].sum().clamp(min=1)
        out["tenpai_rate"].append(float(tenpai[:, r].sum() / k))
        out["mean_shanten"].append(float(shanten[:, r][present[:, r]].float().mean()) if bool(present[:, r].any()) else 0.0)
    # a discard's action id is its tile type (4P; the 3P ids are compact: mapped back through the 27 columns)
    n_discard_ids = 27 if game_mode >= 3 else 34
    is_discard = action < n_discard_ids
    tile = action.clamp(max=n_discard_ids - 1)
    if game_mode >= 3:
        tile = torch.tensor([0, 8] + list(range(9, 34)), device=tile.device)[tile]
    danger = ((waits >> tile[:, None]) & 1).any(dim=1) & is_discard
    out["discards"] = int(is_discard.sum())
    out["dealt_into_waits"] = float(danger.sum() / is_discard.sum().clamp(min=1))
    b.close()
    names = ["shimocha", "toimen", "kamicha"]
    print(f"{out['logs']} logs, {out['samples']} decisions ({out['discards']} discards), overflowed {out['overflowed']}")
    for r in range(n_opp):
        print(f"{names[r]:9s} tenpai_rate {out['tenpai_rate'][r]:.4f}  mean_shanten {out['mean_shanten'][r]:.3f}")
    print(f"discards into an opponent's waits: {out['dealt_into_waits']:.4f}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--mode", type=int, default=2)
    a = ap.parse_args()
    main(a.games, a.steps, a.mode)
