"""The yardstick of the hidden-hand targets (rmj_hidden_targets_device, LogSampleBuilder(hidden=True)): host only, from an abi.StateView
with the oracle's hand mathematics and nothing of the library's.

For the pair (hero seat a) and opponent r = 0, 1, 2, seat s = (a + 1 + r) mod NP (3P: r = 2 is absent, all zero):
  opp_hand     the type histogram of players[s].hand (red fives are fives)
  opp_shanten  oracle.shanten of that histogram (calculate_shanten / _3p with total / 3 groups)
  opp_waits    bit t for every type in HandEvaluator(hand, melds).get_waits_u8(): oracle.eval_hands(...).waits
  opp_flags    PRESENT | TENPAI (waits != 0) | RIICHI (riichi_declared) | FURITEN (a wait among the types of the seat's discards, or
               missed_agari_doujun, or missed_agari_riichi) | n_melds << 4"""
import numpy as np

from riichienv_amd import abi

PRESENT, TENPAI, RIICHI, FURITEN = 1, 2, 4, 8
FIELDS = ("opp_hand", "opp_shanten", "opp_waits", "opp_flags")

_SEATS = {}   # (bytes of the PlayerView, sanma) -> (histogram, shanten, waits, flags): most events change one seat


def seat_fields(p, sanma):
    """(histogram uint8 [34], shanten, waits, flags) of one seat's abi.PlayerView for the seats that cannot see it"""
    from oracle import oracle

    key = (bytes(p), bool(sanma))
    hit = _SEATS.get(key)
    if hit is not None:
        return hit
    tiles = list(p.hand[: p.hand_len])
    hist = np.zeros(34, np.uint8)
    for t in tiles:
        hist[t >> 2] += 1
    sh = int(oracle.shanten(hist[None, :], sanma)[0])
    hc = abi.HandCase()
    hc.n_tiles = len(tiles)
    for i, t in enumerate(tiles):
        hc.tiles[i] = t
    hc.n_melds = p.n_melds
    for i in range(p.n_melds):
        hc.melds[i] = p.melds[i]
    hc.win_tile = tiles[-1] if tiles else 0
    hc.is_sanma = 1 if sanma else 0
    waits = int(oracle.eval_hands([hc])[0].waits)
    discards = {int(d) >> 2 for d in p.discards[: p.n_discards]}
    furiten = any((waits >> t) & 1 for t in discards) or bool(p.missed_agari_doujun) or bool(p.missed_agari_riichi)
    flags = PRESENT | (TENPAI if waits else 0) | (RIICHI if p.riichi_declared else 0) | (FURITEN if furiten else 0) | (int(p.n_melds) << 4)
    if len(_SEATS) > 200000:
        _SEATS.clear()
    _SEATS[key] = (hist, sh, waits, flags)
    return _SEATS[key]


def targets_of_view(view, hero, n_players):
    """{"opp_hand" uint8 [3, 34], "opp_shanten" int8 [3], "opp_waits" int64 [3], "opp_flags" uint8 [3]} of hero seat `hero` in `view`"""
    row = {"opp_hand": np.zeros((3, 34), np.uint8), "opp_shanten": np.zeros(3, np.int8), "opp_waits": np.zeros(3, np.int64), "opp_flags": np.zeros(3, np.uint8)}
    if hero >= n_players:
        return row
    for r in range(n_players - 1):
        hist, sh, waits, flags = seat_fields(view.players[(hero + 1 + r) % n_players], n_players == 3)
        row["opp_hand"][r], row["opp_shanten"][r], row["opp_waits"][r], row["opp_flags"][r] = hist, sh, waits, flags
    return row


def log_targets(log, mode, keys=None):
    """{(event index, hero seat): row} of one log of MJAI event dicts replayed in an oracle.Game of game mode `mode`: the row of every
    seat from the state BEFORE each event is applied (peek, then apply_event(ev, replay=True)).  keys: build only these (a set of
    (event index, seat)); the replay is the same."""
    from oracle import oracle

    n = 3 if mode >= 3 else 4
    game = oracle.Game(game_mode=mode, skip_log=True)
    out = {}
    for i, ev in enumerate(log):
        want = [s for s in range(n) if keys is None or (i, s) in keys]
        if want:
            view = game.peek()
            for s in want:
                out[i, s] = targets_of_view(view, s, n)
        game.apply_event(ev, replay=True)
    return out


def stack(rows):
    """a list of rows as one dict of arrays [k, ...]"""
    return {f: np.stack([r[f] for r in rows]) if rows else np.zeros((0,) + ((3, 34) if f == "opp_hand" else (3,))) for f in FIELDS}
