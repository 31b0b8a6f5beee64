"""Monte Carlo move evaluation over sampled worlds (PIMC), all of it on the GPU: take a few positions where a seat is to discard, fork
each once per legal discard and K times per fork, re-deal what the seat cannot see in every fork (WorldSet.fork: rmj_copy_games_device +
rmj_determinize_device), make the discard, play every world to the end of the game with the device policy, and print the mean change
of the seat's score per discard.  Positions where seats answer a discard (RMJ_WAIT_RESPONSE) are left out of this example.

    python examples/pimc_discard.py --roots 4 --worlds 16 [--riichi-tenpai]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILES = [f"{n}{s}" for s in "mps" for n in range(1, 10)] + ["E", "S", "W", "N", "P", "F", "C"]


def main(roots=4, worlds=16, games=64, steps=90, game_mode=2, max_steps=4000, seed=5, riichi_tenpai=False):
    import torch

    from riichienv_amd import abi
    from riichienv_amd.search import WorldSet
    from riichienv_amd.torch_env import TorchVecEnv

    sanma = game_mode >= 3
    n_discard = 27 if sanma else 34
    type_of = [0, 8] + list(range(9, 34)) if sanma else list(range(34))   # (3P's discard ids are compact)
    tenv = TorchVecEnv(games, game_mode=game_mode, seed=seed)
    tenv.env.step_greedy(seed, steps, auto_reset=False, call_rate_256=64)
    _obs, index = tenv.obs_compact()
    g, s = (index >> 2).long(), (index & 3).long()
    phase = tenv._status()[1]
    root = index[phase[g] == abi.WAIT_ACT][:roots]
    # one row per (root, legal discard of the hero)
    legal = tenv.mask[(root >> 2).long(), (root & 3).long(), :n_discard].bool()
    r_of, d_of = legal.nonzero(as_tuple=True)
    rows = root[r_of]
    ws = WorldSet(tenv, worlds=worlds, max_rows=max(1, int(rows.shape[0])))
    status = ws.fork(rows, seed=seed, riichi_tenpai=riichi_tenpai)   # (--riichi-tenpai: sampled riichi hands are walked to tenpai)
    ids = torch.full((ws.env.n, 4), -1, dtype=torch.int32, device=ws.env.device)
    k = int(rows.shape[0]) * worlds
    ids[ws.slot, ws.hero] = d_of.repeat_interleave(worlds).to(torch.int32)
    ws.env.step(ids, auto_reset=False)
    made = ws.playout(policy_seed=seed + 1, max_steps=max_steps)
    delta, rank, done = ws.values()
    torch.cuda.synchronize()
    ok = (status & 15) == abi.DET_OK
    print(f"{int(root.shape[0])} roots, {int(rows.shape[0])} discards x {worlds} worlds = {k} playouts of up to {made} steps, "
          f"{int(done.sum())} finished, {int((~ok).sum())} not determinized, {int((status >> 4 & 7 != 0).sum())} with a riichi hand that is not tenpai"
          + (f", {int((status & abi.DET_SWAPPED != 0).sum())} repaired by exchanges" if riichi_tenpai else ""))
    out = []
    for i in range(int(root.shape[0])):
        sel = (r_of == i).nonzero().reshape(-1)
        print(f"game {int(root[i]) >> 2} seat {int(root[i]) & 3}:")
        for j in sel.tolist():
            m, rk = float(delta[j].float().mean()), float(rank[j].float().mean())
            out.append((int(root[i]), type_of[int(d_of[j])], m, rk))
            print(f"  discard {TILES[type_of[int(d_of[j])]]:2s}  mean score change {m:+9.1f}  mean final rank {rk:.2f}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4)
    ap.add_argument("--worlds", type=int, default=16)
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--riichi-tenpai", action="store_true", help="walk the sampled hands of opponents in riichi to tenpai (RMJ_DETF_RIICHI_TENPAI)")
    a = ap.parse_args()
    main(a.roots, a.worlds, a.games, a.steps, a.mode, riichi_tenpai=a.riichi_tenpai)
