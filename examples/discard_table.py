"""Which tile do I cut: the discard efficiency table of live rows - the shanten after every discard, the tile types that then improve the
hand and how many of them are still live - and, next to it, what each of those discards would cost against the opponents (the deal-in
danger row of the same seats).  Attack value and defence cost of the 34 tile types, both made on the GPU from the games' own state.

    python examples/discard_table.py --games 64 --steps 80
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(games=64, steps=80, show=3, game_mode=2, seed=7):
    import torch

    from riichienv_amd import abi, efficiency
    from riichienv_amd.torch_env import TorchVecEnv

    sanma = game_mode >= 3
    env = TorchVecEnv(games, game_mode=game_mode, seed=seed)
    env.env.step_greedy(3, steps, auto_reset=True, call_rate_256=64)
    _, index = env.obs_compact()
    table = env.discard_table_compact(index)
    danger = env.danger_compact(index)                        # [k, 3, 37]: points per opponent and tile kind
    mask = env.mask.reshape(games * 4, -1)[index.long()]
    best = efficiency.best_discard(table, mask, sanma)
    types = torch.as_tensor(efficiency.discard_types(sanma), device=best.device)
    worst = danger[:, :, :34].max(dim=1).values               # the dearest opponent per tile type
    has = best >= 0
    rows = torch.nonzero(has)[:, 0]
    host = {f: v.cpu().numpy() for f, v in table.items()}
    for i in rows[:show].tolist():
        g, s = int(index[i]) >> 2, int(index[i]) & 3
        print(f"game {g} seat {s}")
        print(efficiency.describe({f: v[i] for f, v in host.items()}))
        t = int(types[best[i]])
        print(f"  most efficient legal discard: {efficiency.TILE_NAMES[t]} (ron against it: {int(worst[i, t])} points)")
        costly = [(efficiency.TILE_NAMES[c], int(worst[i, c])) for c in range(34) if host["shanten"][i, c] != abi.DTAB_NONE and int(worst[i, c]) > 0]
        print("  held tiles that deal in: " + (", ".join(f"{n} {p}" for n, p in costly) if costly else "none"))
    sh = table["shanten"][:, 34].float()
    bt = types[best.clamp(min=0)]
    out = {"rows": int(index.shape[0]), "with_discard": int(has.sum()), "mean_shanten": float(sh.mean()) if sh.numel() else 0.0,
           "best_discard_deals_in": float((worst.gather(1, bt[:, None])[:, 0][has] > 0).float().mean()) if bool(has.any()) else 0.0}
    print(f"{out['rows']} acting rows, {out['with_discard']} with a discard to make, mean shanten {out['mean_shanten']:.2f}; "
          f"the most efficient discard deals in on {out['best_discard_deals_in']:.4f} of them")
    env.env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--show", type=int, default=3)
    ap.add_argument("--mode", type=int, default=2)
    a = ap.parse_args()
    main(a.games, a.steps, a.show, a.mode)
