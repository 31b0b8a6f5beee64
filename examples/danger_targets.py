"""Deal-in danger as a training label: what every tile would cost against every opponent at the moment of a decision.  A few self-played
games -> their own logs -> LogSampleBuilder(hidden=True, danger=True) -> how often a discard dealt in, what the label said about the
discards that did and the ones that did not, and how many wait bits of the hidden targets cost nothing (furiten, no yaku).  The labels
are made on the GPU; the log is consulted on the host only to see which discards were followed by a hora.

    python examples/danger_targets.py --games 64 --steps 20000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.hidden_targets import self_written_logs  # noqa: E402


def main(games=64, steps=20000, game_mode=2):
    import torch

    from riichienv_amd import abi
    from riichienv_amd.datasets import LogSampleBuilder

    logs = self_written_logs(games, steps, game_mode)
    b = LogSampleBuilder(logs, game_mode=game_mode, hidden=True, danger=True, include_pass=False)
    b.run()
    s = b.samples()
    counts = b.counts()
    danger, waits, packed = s["danger"], s["opp_waits"], s["packed"]
    np_ = 3 if game_mode >= 3 else 4
    # the discarded kind: the tile id of the packed action; the copy-0 fives are kinds 34..36
    is_discard = (packed & 0xFF) == abi.DISCARD
    tile = (packed >> 8) & 0xFF
    kind = tile >> 2
    for i, red in enumerate((16, 52, 88)):
        kind = torch.where(tile == red, torch.full_like(kind, 34 + i), kind)
    kind = kind.clamp(max=abi.DANGER_KINDS - 1)
    at_kind = danger.gather(2, kind[:, None, None].expand(-1, 3, 1))[:, :, 0]     # [N, 3]: the label of the tile that was discarded
    worst = at_kind.max(dim=1).values
    # which discards dealt in: the events behind the dahai are the horas of the seats that took it
    rows = torch.nonzero(is_discard)[:, 0].cpu().tolist()
    log_c, ev_c, seat_c = s["log"].cpu().tolist(), s["event"].cpu().tolist(), s["seat"].cpu().tolist()
    hit = torch.zeros_like(is_discard)
    paid_label = []
    at_kind_h = at_kind.cpu()
    for i in rows:
        log, j = logs[log_c[i]], ev_c[i] + 1
        while j < len(log) and log[j]["type"] == "hora":
            if log[j].get("target") == seat_c[i] and log[j]["actor"] != seat_c[i]:
                hit[i] = True
                paid_label.append(int(at_kind_h[i, (log[j]["actor"] - seat_c[i] - 1) % np_]))
            j += 1
    safe = is_discard & ~hit
    n_discards = int(is_discard.sum())
    bits = ((waits[:, :, None] >> torch.arange(34, device=waits.device)) & 1) != 0
    free = bits & (danger[:, :, :34] == 0)
    out = {"logs": len(logs), "samples": int(packed.shape[0]), "overflowed": counts["overflowed"], "discards": n_discards,
           "dealt_in": float(hit.sum() / max(n_discards, 1)),
           "mean_danger_dealt_in": float(worst[hit].float().mean()) if bool(hit.any()) else 0.0,
           "mean_danger_safe": float(worst[safe].float().mean()) if bool(safe.any()) else 0.0,
           "winner_label_zero": sum(1 for v in paid_label if v == 0), "horas": len(paid_label),
           "wait_bits": int(bits.sum()), "wait_bits_costing_nothing": float(free.sum() / bits.sum().clamp(min=1))}
    b.close()
    print(f"{out['logs']} logs, {out['samples']} decisions ({n_discards} discards), overflowed {out['overflowed']}")
    print(f"discards that dealt in: {out['dealt_in']:.4f} ({out['horas']} horas; the winner's label was 0 for {out['winner_label_zero']} of them)")
    print(f"mean of the worst opponent's label at the discarded tile: {out['mean_danger_dealt_in']:.0f} points where it dealt in, "
          f"{out['mean_danger_safe']:.0f} where it did not")
    print(f"wait bits of opp_waits that cost nothing (furiten, no yaku): {out['wait_bits_costing_nothing']:.4f} of {out['wait_bits']}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--mode", type=int, default=2)
    a = ap.parse_args()
    main(a.games, a.steps, a.mode)
