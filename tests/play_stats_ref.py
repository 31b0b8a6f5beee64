"""The play statistics of a log as plain Python over json.loads dicts - the restatement that holds rmj_logset_playstats_device
(include/riichi_mi355x.h: RMJ_PLAYSTAT_*), written from the definitions of the columns and not from the kernel - with a second,
independent reading of every hora through its own `target` key, hand-made logs at the sizes where a 64-event walk can go wrong, and a
seeded generator of event soups.  No GPU, no library."""
import random

import numpy as np

WIN, WIN_TSUMO, DEAL_IN, RIICHI, RIICHI_ACCEPTED, RIICHI_TURN, CALLS, CHI, PON, KANS, KITA, DISCARDS, TSUMOGIRI, WIN_TURN, DEALER, END = range(16)
TYPES = ["start_game", "start_kyoku", "tsumo", "dahai", "reach", "reach_accepted", "chi", "pon", "daiminkan", "kan", "ankan", "kakan", "dora", "hora",
         "ryukyoku", "end_kyoku", "end_game", "kita"]
_TILE_EVENTS = ("tsumo", "dahai", "kakan", "ankan", "kita")
_ACTED = ("tsumo", "dahai", "reach", "reach_accepted", "chi", "pon", "daiminkan", "kan", "ankan", "kakan", "hora", "ryukyoku", "kita")


def _seat(ev, key="actor"):
    return int(ev.get(key, 0) or 0)


def _walk(events, n):
    """(rows, horas): rows - one [4][16] list per start_kyoku; horas - (kyoku index, actor, tsumo win?, the seat that dealt in or None) of
    every counted hora, the deal-in derived from the stream"""
    rows, horas, cur = [], [], None
    for ev in events:
        ty = ev.get("type")
        if ty == "start_kyoku":
            cur = [[0] * 16 for _ in range(4)]
            rows.append(cur)
            oya = int(ev["oya"])
            if oya < n:
                cur[oya][DEALER] = 1
            last, reached, won = None, set(), set()           # the last tile event (type, actor); the seats that have their turn columns
            continue
        if cur is None or ty not in _ACTED:
            continue
        a = _seat(ev)
        if a >= n:
            continue                                          # no seat of the game: as if the event were not there
        r = cur[a]
        if ty == "hora":
            r[WIN] += 1
            tsumo, dealt = False, None
            if last is not None and last == ("tsumo", a):
                tsumo = True
                r[WIN_TSUMO] += 1
            elif last is not None and last[1] != a:
                dealt = last[1]
                cur[dealt][DEAL_IN] += 1
            if a not in won:
                won.add(a)
                r[WIN_TURN] = r[DISCARDS]
            for p in range(n):
                cur[p][END] |= 1
            horas.append((len(rows) - 1, a, tsumo, dealt))
        elif ty == "ryukyoku":
            for p in range(n):
                cur[p][END] |= 2
        elif ty == "reach":
            r[RIICHI] += 1
            if a not in reached:
                reached.add(a)
                r[RIICHI_TURN] = 1 + r[DISCARDS]
        elif ty == "reach_accepted":
            r[RIICHI_ACCEPTED] += 1
        elif ty == "chi":
            r[CHI] += 1
            r[CALLS] += 1
        elif ty == "pon":
            r[PON] += 1
            r[CALLS] += 1
        elif ty in ("daiminkan", "kan"):
            r[CALLS] += 1
            r[KANS] += 1
        elif ty in ("ankan", "kakan"):
            r[KANS] += 1
        elif ty == "kita":
            r[KITA] += 1
        elif ty == "dahai":
            r[DISCARDS] += 1
            if ev.get("tsumogiri"):
                r[TSUMOGIRI] += 1
        if ty in _TILE_EVENTS:
            last = (ty, a)
    return rows, horas


def kyoku_rows(events, n):
    """int32 [K, 4, 16]: the rows of one log's kyokus"""
    return np.array(_walk(events, n)[0], dtype=np.int32).reshape(-1, 4, 16)


def table(logs, n, bad=()):
    """int32 [K, 4, 16] of a whole set in table order; the rows of the logs `bad` are -1"""
    parts = [kyoku_rows(log, n) if i not in bad else np.full_like(kyoku_rows(log, n), -1) for i, log in enumerate(logs)]
    return np.concatenate(parts) if parts else np.zeros((0, 4, 16), np.int32)


def kyoku_offsets(logs):
    return np.concatenate([[0], np.cumsum([sum(1 for ev in log if ev.get("type") == "start_kyoku") for log in logs])]).astype(np.int64)


def derived_horas(events, n):
    return _walk(events, n)[1]


def target_horas(events, n):
    """The second reading: (kyoku index, actor, tsumo win?, the seat that dealt in or None) of every hora from its own `target` key -
    actor == target is a tsumo win, any other target dealt in.  Only for logs whose hora events carry `target`."""
    out, k = [], -1
    for ev in events:
        if ev.get("type") == "start_kyoku":
            k += 1
        elif ev.get("type") == "hora" and k >= 0 and _seat(ev) < n:
            a, t = _seat(ev), int(ev["target"])
            out.append((k, a, a == t, None if a == t else t))
    return out


# ------------------------------------------------------------------ hand-made logs
_HAND = ["1m", "2m", "3m", "4m", "5m", "6m", "7m", "8m", "9m", "1p", "2p", "3p", "4p"]


def sk(oya=0, kyoku=1, seats=4, n_scores=None):
    n_scores = seats if n_scores is None else n_scores
    return {"type": "start_kyoku", "bakaze": "E", "kyoku": kyoku, "honba": 0, "kyotaku": 0, "oya": oya, "dora_marker": "1s",
            "scores": [25000] * n_scores, "tehais": [list(_HAND) for _ in range(seats)]}


def E(ty, actor=None, **kw):
    ev = {"type": ty}
    if actor is not None:
        ev["actor"] = actor
    if ty in ("tsumo", "dahai", "kakan", "chi", "pon", "daiminkan", "kan"):
        ev["pai"] = kw.pop("pai", "5p")
    if ty == "dahai":
        ev["tsumogiri"] = kw.pop("tsumogiri", False)
    if ty in ("chi", "pon", "daiminkan", "kan"):
        ev["target"] = kw.pop("target", (actor + 1) % 3)
        ev["consumed"] = ["5p", "5p", "5p"][: 2 if ty in ("chi", "pon") else 3]
    if ty == "ankan":
        ev["consumed"] = ["5p"] * 4
    if ty == "kakan":
        ev["consumed"] = ["5p"] * 3
    if ty == "dora":
        ev["dora_marker"] = "2s"
    ev.update(kw)
    return ev


def _turns(k, seats=4, first=0):
    """k events: tsumo / dahai pairs going round the table"""
    out, p = [], first
    while len(out) < k:
        out += [E("tsumo", p), E("dahai", p, tsumogiri=bool(len(out) & 2))]
        p = (p + 1) % seats
    return out[:k]


def hand_made_logs(seats):
    """{name: events}: every case of the walk named in the docstring of tests/test_gpu_play_stats.py"""
    S = seats
    logs = {}
    for k in (0, 1, 63, 64, 65, 128, 129):                    # logs of exactly k events
        logs[f"len{k}"] = ([sk(seats=S)] + _turns(k - 1, S)) if k else []
    # a START_KYOKU in lane 63 and one in lane 0 of the next pass
    logs["sk_lane63_lane0"] = [sk(seats=S)] + _turns(62, S) + [sk(1, 2, S), sk(2, 3, S)] + _turns(7, S) + [E("hora", 1, target=1)]
    # thirty kyokus of three events each inside one pass
    logs["thirty_kyokus"] = [ev for k in range(30) for ev in (sk(k % S, k + 1, S), E("tsumo", k % S), E("hora", k % S, target=k % S))]
    # a hora in lane 0 of the second pass whose last tile event is lane 63 of the first
    logs["hora_lane0"] = [sk(seats=S)] + _turns(63, S) + [E("hora", 2, target=(62 // 2) % S)]
    # a hora whose last tile event lies two passes back, behind 64 dora events
    logs["hora_two_passes_back"] = [sk(seats=S)] + _turns(10, S) + [E("dora") for _ in range(64 + 60)] + [E("hora", 2, target=0)]
    logs["double_ron"] = [sk(seats=S), E("tsumo", 0), E("dahai", 0), E("hora", 1, target=0), E("hora", 2, target=0)]
    logs["triple_hora"] = [sk(seats=S), E("tsumo", 1), E("dahai", 1), E("hora", 0, target=1), E("hora", 2, target=1), E("hora", 0, target=1)]
    logs["reach_ronned"] = [sk(seats=S)] + _turns(6, S) + [E("tsumo", 0), E("reach", 0), E("dahai", 0), E("hora", 1, target=0)]
    logs["two_reaches"] = [sk(seats=S)] + _turns(4, S) + [E("tsumo", 2), E("reach", 2), E("dahai", 2), E("reach_accepted", 2), E("tsumo", 0), E("dahai", 0),
                                                        E("tsumo", 1), E("dahai", 1), E("tsumo", 2), E("reach", 2), E("dahai", 2), E("ryukyoku")]
    logs["chankan"] = [sk(seats=S), E("tsumo", 0), E("dahai", 0), E("pon", 1, target=0), E("dahai", 1), E("tsumo", 2), E("dahai", 2), E("tsumo", 1),
                       E("kakan", 1), E("hora", 2, target=1)]
    logs["hora_without_tile_event"] = [sk(seats=S), E("hora", 1, target=1), E("reach", 0)]
    logs["hora_after_own_dahai"] = [sk(seats=S), E("tsumo", 1), E("dahai", 1), E("hora", 1, target=1)]
    logs["events_before_first_kyoku"] = [E("start_game")] + _turns(5, S) + [E("reach", 1), E("hora", 1, target=1), E("ryukyoku"), sk(seats=S)] + _turns(4, S)
    # actors 4 and 5: no seats - skipped whole, also as the last tile event before a hora (start_kyoku with six scores keeps the replay walk content)
    logs["actors_4_5"] = [sk(seats=S, n_scores=6), E("tsumo", 0), E("dahai", 0), E("tsumo", 4), E("dahai", 5), E("reach", 4), E("reach_accepted", 5),
                          E("pon", 4, target=0), E("hora", 5, target=0), E("hora", 1, target=0), E("ryukyoku", 4), E("ankan", 5)]
    logs["kans_and_calls"] = [sk(1, 1, S), E("tsumo", 0), E("dahai", 0), E("chi", 1, target=0), E("dahai", 1), E("daiminkan", 2, target=1), E("tsumo", 2),
                              E("ankan", 2), E("tsumo", 2), E("dahai", 2, tsumogiri=True), E("kan", 0, target=2), E("tsumo", 0), E("hora", 0, target=0)]
    if S == 3:   # kita, and an event of seat 3 (no seat of a three-player game)
        logs["kita_and_seat3"] = [sk(2, 1, 3, n_scores=4), E("tsumo", 0), E("kita", 0), E("tsumo", 0), E("dahai", 0), E("tsumo", 3), E("dahai", 3), E("kita", 3),
                                  E("tsumo", 1), E("kita", 1), E("hora", 2, target=1), E("tsumo", 2), E("kita", 2), E("tsumo", 2), E("hora", 2, target=2)]
    return logs


# ------------------------------------------------------------------ the event soup
_SOUP_LENGTHS = [63, 64, 65, 127, 128, 129, 191, 192, 193]


def soup_log(rng, seats):
    """One log of random events: every MJAI type, unknown type strings and events without a type; actors 0..5; tsumogiri at random.  The
    length is 0..400, about half of the logs within +-1 of 64, 128 or 192.  start_kyoku events carry six scores, so that the host's and the
    device's kyoku walks accept the actors 4 and 5."""
    length = rng.choice(_SOUP_LENGTHS) if rng.random() < 0.5 else rng.randint(0, 400)
    p_start = rng.choice([0.01, 0.05, 0.3])
    out = []
    for _ in range(length):
        a = rng.randint(0, 5)
        if rng.random() < p_start:
            out.append(sk(rng.randint(0, 5), rng.randint(1, 4), seats, n_scores=6))
            continue
        ty = rng.choice(TYPES + ["", "tehai", "none", "HORA", "nukidora", None])
        if ty is None:
            out.append({"actor": a})
        elif ty == "start_kyoku":
            out.append(sk(rng.randint(0, 5), rng.randint(1, 4), seats, n_scores=6))
        elif ty in TYPES:
            kw = {}
            if ty == "dahai":
                kw["tsumogiri"] = rng.random() < 0.5
            if ty in ("chi", "pon", "daiminkan", "kan"):
                kw["target"] = rng.randint(0, 5)
            out.append(E(ty, a, **kw))
        else:
            out.append({"type": ty, "actor": a})
    return out


def soup_logs(count, seats, seed):
    rng = random.Random(seed)
    return [soup_log(rng, seats) for _ in range(count)]
