"""The yardstick of the deal-in danger targets (rmj_danger_targets_device, LogSampleBuilder(danger=True)): host only, from an abi.StateView
with oracle.eval_hands and oracle.calculate_score and nothing of the library's.

danger[r][k] of hero seat a: the points seat s = (a + 1 + r) mod NP would win by ron if a discarded a tile of kind k now.  Kind k < 34 is
tile type k as the non-red id 4 k + 1, kinds 34, 35, 36 are the ids 16, 52, 88.  0 unless s holds concealed + 3 x melds = 13, the type is
among get_waits of s, neither it nor any other wait of s is among s's own discards, no missed_agari flag is set and the evaluation is a win;
then ron_agari under riichi / double riichi / ippatsu of s, houtei when drawable_count == 0 and not is_rinshan, the seat's and the round's
wind, the dora indicators revealed now, kita_count = n_kita in 3P and the table's honba - followed by the double-yakuman cap of the
settlement: the yaku ids 47-50 each take 13 off han when their rule bit is off (floor 13), and the score is taken again with fu 0."""
import numpy as np

from riichienv_amd import abi

KINDS = 37
RED_IDS = (16, 52, 88)
_CAP_BITS = {47: 8, 48: 4, 49: 2, 50: 16}   # yaku id -> the RMJ_RULE_*_DOUBLE bit that lets it count twice
_SEATS = {}


def kind_tile(k):
    """the 136-id a kind stands for"""
    return RED_IDS[k - 34] if k >= 34 else 4 * k + 1


def kind_type(k):
    return kind_tile(k) >> 2


def kind_of_tile(t):
    """the kind a discarded 136-id counts as"""
    return 34 + RED_IDS.index(t) if t in RED_IDS else t >> 2


def ura_indicators(view, n_players):
    """_get_ura_indicators of a 4P view; a 3P view cannot carry its indicators (they are extracted from the wall at the deal)"""
    if n_players == 3:
        raise ValueError("a 3P view does not carry the ura indicators")
    out = []
    for i in range(view.n_dora):
        j = max(5 + 2 * i - int(view.rinshan_draw_count), 0)
        if j < view.wall_len:
            out.append(int(view.wall[j]))
    return out


def _case(p, sanma):
    hc = abi.HandCase()
    tiles = list(p.hand[: p.hand_len])
    hc.n_tiles = len(tiles)
    for i, t in enumerate(tiles):
        hc.tiles[i] = t
    hc.n_melds = p.n_melds
    for i in range(p.n_melds):
        hc.melds[i] = p.melds[i]
    hc.is_sanma = 1 if sanma else 0
    return hc


def _ron_case(view, s, n_players, k, uras):
    """the evaluation of seat s winning by ron on a tile of kind k now"""
    p, sanma = view.players[s], n_players == 3
    hc = _case(p, sanma)
    hc.win_tile = kind_tile(k)
    hc.n_dora = view.n_dora
    for i in range(view.n_dora):
        hc.dora[i] = view.dora[i]
    hc.n_ura = len(uras)
    for i, t in enumerate(uras):
        hc.ura[i] = t
    hc.riichi, hc.double_riichi, hc.ippatsu = int(bool(p.riichi_declared)), int(bool(p.double_riichi_declared)), int(bool(p.ippatsu_cycle))
    hc.houtei = int(view.drawable_count == 0 and not view.is_rinshan_flag)
    hc.player_wind = (s + n_players - int(view.oya)) % n_players
    hc.round_wind = int(view.round_wind)
    hc.kita_count = int(p.n_kita) if sanma else 0
    hc.honba = int(view.honba)
    return hc


def ron_result(view, s, n_players, k, ura):
    """the oracle's HandResult of that evaluation (before the double-yakuman cap): what a position's name promises can be read off it"""
    from oracle import oracle

    uras = ura_indicators(view, n_players) if (ura and view.players[s].riichi_declared) else []
    return oracle.eval_hands([_ron_case(view, s, n_players, k, uras)])[0]


def opp_danger(view, s, n_players, ura, rule_bits=abi.RULE_TENHOU):
    """int32 [37]: what seat s of `view` would win by ron on a tile of every kind, whoever discards it"""
    from oracle import oracle

    sanma = n_players == 3
    out = np.zeros(KINDS, np.int32)
    if s >= n_players:
        return out
    p = view.players[s]
    if int(p.hand_len) + 3 * int(p.n_melds) != 13:
        return out
    uras = ura_indicators(view, n_players) if (ura and p.riichi_declared) else []
    houtei = view.drawable_count == 0 and not view.is_rinshan_flag
    key = (bytes(p), s, n_players, tuple(view.dora[: view.n_dora]), tuple(uras), bool(houtei), int(view.oya), int(view.round_wind), int(view.honba), int(rule_bits))
    hit = _SEATS.get(key)
    if hit is not None:
        return hit.copy()
    probe = _case(p, sanma)
    probe.win_tile = p.hand[0]
    waits = int(oracle.eval_hands([probe])[0].waits)
    discards = {int(d) >> 2 for d in p.discards[: p.n_discards]}
    furiten = any((waits >> t) & 1 for t in discards) or bool(p.missed_agari_doujun) or bool(p.missed_agari_riichi)
    if waits and not furiten:
        kinds = [k for k in range(KINDS) if (waits >> kind_type(k)) & 1 and kind_type(k) not in discards]
        cases = [_ron_case(view, s, n_players, k, uras) for k in kinds]
        is_oya = s == int(view.oya)
        for k, res in zip(kinds, oracle.eval_hands(cases)):
            if not res.is_win:
                continue
            value, han = int(res.ron_agari), int(res.han)
            if res.yakuman and han > 13:
                cap = sum(13 for y in res.yaku[: res.n_yaku] if y in _CAP_BITS and not rule_bits & _CAP_BITS[y])
                if cap:
                    han = max(han - cap, 13)
                    value = int(oracle.calculate_score([han], [0], [int(is_oya)], [0], [int(view.honba)], [n_players])[0][1])
            out[k] = value
    if len(_SEATS) > 200000:
        _SEATS.clear()
    _SEATS[key] = out
    return out.copy()


def danger_of_view(view, hero, n_players, ura=False, rule_bits=abi.RULE_TENHOU):
    """int32 [3, 37]: the row of hero seat `hero` in `view`"""
    row = np.zeros((3, KINDS), np.int32)
    if hero >= n_players:
        return row
    for r in range(n_players - 1):
        row[r] = opp_danger(view, (hero + 1 + r) % n_players, n_players, ura, rule_bits)
    return row


def log_danger(log, mode, keys=None, rule_bits=abi.RULE_TENHOU):
    """{(event index, hero seat): row} of one log of MJAI event dicts replayed in an oracle.Game of game mode `mode`: the row of every seat
    from the state BEFORE each event is applied (peek, then apply_event(ev, replay=True)), without ura.  keys: build only these."""
    from oracle import oracle

    n = 3 if mode >= 3 else 4
    game = oracle.Game(game_mode=mode, skip_log=True, rule_bits=rule_bits)
    out = {}
    for i, ev in enumerate(log):
        want = [s for s in range(n) if keys is None or (i, s) in keys]
        if want:
            view = game.peek()
            for s in want:
                out[i, s] = danger_of_view(view, s, n, False, rule_bits)
        game.apply_event(ev, replay=True)
    return out
