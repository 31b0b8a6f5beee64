"""Plain restatement of the log validation (LogSet.validate, csrc/rmj_logcheck.hip.h) over MJAI event dicts: the first finding of a log as
(code, event, kyoku, seat).  Codes 2-6, 8, 9, 11 and 12 are a Python walk over the dicts; 7 and 10 ask the CPU oracle what the actor is
offered (oracle.Game.apply_event(ev, replay=True), status(), legal(pid)) and match the event against that list by
select_action_from_mjai's rules as lr_select states them (csrc/rmj_logreplay.hip.h).

mutations(log, n) damages a clean log once per entry: name -> (mutated log, the code it must give, the first event index the finding
may have).  Where the issue's wording of a mutation cannot give its code under "the first finding wins", the mutation does a little
more, and says so."""
import copy

from riichienv_amd import abi

OK, PARSE, NO_START_KYOKU, AFTER_END, UNFINISHED, ACTOR, DRAW_OUT_OF_TURN, NOT_OFFERED, TILE_NOT_HELD, TILE_COUNT, NO_LEGAL_MATCH, SCORE_CONTINUITY, \
    SCORE_CONSERVATION = range(13)
NO_SEAT = 255
STRUCTURAL = ("start_game", "start_kyoku", "end_kyoku", "end_game")
KNOWN = ("start_game", "start_kyoku", "tsumo", "dahai", "reach", "reach_accepted", "chi", "pon", "daiminkan", "kan", "ankan", "kakan", "dora", "hora", "ryukyoku",
         "end_kyoku", "end_game", "kita")
CLAIMS = ("chi", "pon", "daiminkan")
DECISIONS = ("dahai", "chi", "pon", "daiminkan", "ankan", "kakan", "reach", "hora", "kita")
TAKES = {"dahai": 1, "kakan": 1, "chi": 2, "pon": 2, "daiminkan": 3, "ankan": 4}
_WANT = {"pon": abi.PON, "chi": abi.CHI, "daiminkan": abi.DAIMINKAN, "ankan": abi.ANKAN}


def _type(ev):
    """the event's type as the records hold it: "kan" is a daiminkan, anything unknown is NONE"""
    ty = ev.get("type")
    return "daiminkan" if ty == "kan" else (ty if ty in KNOWN else "none")


_TID = {}


def tid(name):
    if name not in _TID:
        _TID[name] = abi.mjai_to_tid(name, True)
    return _TID[name]


def name_of(t):
    """lr_name: the tile type, the red fives apart"""
    return 34 + t // 36 if t in (16, 52, 88) else t >> 2


def _count(seen, t):
    """one more tile `t`; True when its type now occurs more than 4 times or its red five more than once"""
    seen[t >> 2] = seen.get(t >> 2, 0) + 1
    over = seen[t >> 2] > 4
    if t in (16, 52, 88):
        seen[34 + t // 36] = seen.get(34 + t // 36, 0) + 1
        over = over or seen[34 + t // 36] > 1
    return over


def _matches(legal, ev, ty, sanma):
    """does lr_select find an entry of `legal` for the event"""
    for a in legal:
        at, tile, cons = abi.unpack_action(int(a))
        tile_eq = tile is not None and "pai" in ev and name_of(tile) == name_of(tid(ev["pai"]))
        if ty == "hora":
            hit = at in (abi.TSUMO, abi.RON)
        elif ty == "dahai":
            hit = at == abi.DISCARD and tile_eq
        elif ty == "reach":
            hit = at == abi.RIICHI
        elif ty == "kita":
            hit = sanma and at == abi.KITA
        elif ty == "kakan":
            hit = at == abi.KAKAN and tile_eq
        else:
            want = sorted(name_of(tid(c)) for c in ev["consumed"][:4])
            hit = at == _WANT[ty] and not (sanma and ty == "chi") and sorted(name_of(c) for c in cons) == want and (ty == "ankan" or tile_eq)
        if hit:
            return True
    return False


_RECS = {}


def _records(ev, n):
    """abi.event_records_from_mjai(ev), kept per event dict: a mutated log shares all but one of its dicts with the log it was made from"""
    hit = _RECS.get(id(ev))
    if hit is None or hit[0] is not ev:
        hit = _RECS[id(ev)] = (ev, abi.event_records_from_mjai(ev, n))
    return hit[1]


def check_log(log, n, mode, rule_bits=abi.RULE_TENHOU):
    """(code, event, kyoku, seat) of the first finding of one log of event dicts; n players, the oracle plays game mode `mode`"""
    from oracle import oracle

    sanma = n == 3
    game = oracle.Game(game_mode=mode, skip_log=True, rule_bits=rule_bits)
    st, due, kc, kyotaku = 0, None, 0, 0        # the kyoku's phase (0 none started, 1 open, 2 over), the seat due to draw
    seen, hands = {}, [dict() for _ in range(4)]
    start = own = alt = None                    # the open kyoku's start scores, and the end scores its own events give (two readings)
    table_open, prev_hora, reached, accepted = False, False, set(), set()
    for i, ev in enumerate(log):
        ty = _type(ev)
        actor = int(ev.get("actor", 0) or 0)
        structural = ty in STRUCTURAL or ty == "none"
        has_actor = ty in ("tsumo", "dahai", "reach", "reach_accepted", "chi", "pon", "daiminkan", "ankan", "kakan", "hora") or (sanma and ty == "kita")
        seat = actor if has_actor or ty in DECISIONS else NO_SEAT
        if st == 0 and not structural:
            return NO_START_KYOKU, i, kc, NO_SEAT
        if st == 2 and not structural and ty != "hora":
            return AFTER_END, i, kc, NO_SEAT
        if st == 1 and ty in ("start_kyoku", "start_game", "end_game"):
            return UNFINISHED, i, kc, NO_SEAT
        if not structural:
            target = int(ev.get("target", 0) or 0)
            if (has_actor and actor >= n) or (ty in CLAIMS and (target >= n or target == actor)):
                return ACTOR, i, kc, seat
            if st == 1:
                a = actor & 3
                if ty == "tsumo" and actor != due:
                    return DRAW_OUT_OF_TURN, i, kc, seat
                am, _phase, done = game.status() if ty in DECISIONS else (0, 0, 0)
                listed = bool(((0 if done else am) >> a) & 1)
                legal = game.legal(a) if listed else []
                robbed = False
                if ty == "hora" and not done and not listed:
                    j = i - 1
                    while j >= 0 and _type(log[j]) == "dora":
                        j -= 1
                    if j >= 0 and int(log[j].get("actor", 0) or 0) != actor:
                        robbed = _type(log[j]) == "kakan" or (_type(log[j]) == "ankan" and len(log[j]["consumed"]) > 0)
                if ty in DECISIONS and not legal and not robbed:
                    return NOT_OFFERED, i, kc, seat
                if ty in TAKES:
                    takes = [tid(ev["pai"])] if ty in ("dahai", "kakan") else [tid(c) for c in ev["consumed"][:4]][: TAKES[ty]]
                    for t in takes:
                        if hands[a].get(t, 0) < takes.count(t):
                            return TILE_NOT_HELD, i, kc, seat
                if ty in ("tsumo", "dora") and _count(seen, tid(ev["pai"] if ty == "tsumo" else ev["dora_marker"])):
                    return TILE_COUNT, i, kc, seat
                if ty in DECISIONS and not robbed and not _matches(legal, ev, ty, sanma):
                    return NO_LEGAL_MATCH, i, kc, seat
        elif ty == "start_kyoku":
            if int(ev["oya"]) >= n:
                return ACTOR, i, kc + 1, NO_SEAT
            seen = {}
            over = False
            for t in [tid(x) for h in ev["tehais"][:n] for x in h] + [tid(ev["dora_marker"])]:
                over = _count(seen, t) or over
            if over:
                return TILE_COUNT, i, kc + 1, NO_SEAT
            scores = [int(x) for x in ev["scores"][:n]]
            now = int(ev.get("kyoutaku", ev.get("kyotaku", 0)))
            if kc:
                differ = [s for s in range(n) if own[s] != scores[s]]
                if differ and alt != scores:   # (a ryukyoku's deltas may hold the riichi deposits already: either reading passes)
                    return SCORE_CONTINUITY, i, kc + 1, differ[0]
                if sum(scores) - sum(start) != -1000 * (now - kyotaku):
                    return SCORE_CONSERVATION, i, kc + 1, NO_SEAT
        # ---- the event is applied
        if ty not in ("none", "end_game"):
            game.apply_event(_records(ev, n), replay=True)
        if ty == "start_kyoku":
            kc, st, due, kyotaku = kc + 1, 1, int(ev["oya"]), int(ev.get("kyoutaku", ev.get("kyotaku", 0)))
            hands = [dict() for _ in range(4)]
            for s, h in enumerate(ev["tehais"][:n]):
                for x in h:
                    hands[s][tid(x)] = hands[s].get(tid(x), 0) + 1
            start, own, alt = [int(x) for x in ev["scores"][:n]], [int(x) for x in ev["scores"][:n]], [int(x) for x in ev["scores"][:n]]
            table_open, prev_hora, reached, accepted = True, False, set(), set()
            continue
        if ty in ("hora", "ryukyoku", "end_kyoku") and st == 1:
            st = 2
        # the kyoku's own end scores, as the kyoku tables compute them for a log's last kyoku (replay.Kyoku._feed)
        if ty in ("end_kyoku", "end_game"):
            table_open = False
        elif table_open:
            first, prev_hora = not prev_hora, ty == "hora"
            if ty == "reach":
                reached.add(actor)
            elif ty == "reach_accepted":
                accepted.add(actor)
            elif ty in ("hora", "ryukyoku"):
                deltas = ev.get("deltas", ev.get("delta"))
                if ev.get("scores") is not None:
                    own = [int(x) for x in ev["scores"][:n]]
                    alt = list(own)
                elif deltas is not None:
                    sticks = accepted if ty == "hora" else reached
                    for s, d in enumerate(deltas[:n]):
                        own[s] = own[s] + d if ty == "hora" and not first else start[s] + d - (1000 if s in sticks else 0)
                        alt[s] = start[s] + d if ty == "ryukyoku" else own[s]
        a = actor & 3
        if ty == "tsumo":
            due = None
            hands[a][tid(ev["pai"])] = hands[a].get(tid(ev["pai"]), 0) + 1
        elif ty == "dahai":
            due = (actor + 1) % n
            hands[a][tid(ev["pai"])] = hands[a].get(tid(ev["pai"]), 0) - 1
        elif ty in ("chi", "pon", "daiminkan", "ankan"):
            due = actor if ty in ("daiminkan", "ankan") else None
            for c in ev["consumed"][:4]:
                hands[a][tid(c)] = hands[a].get(tid(c), 0) - 1
        elif ty == "kakan":
            due = actor
            hands[a][tid(ev["pai"])] = hands[a].get(tid(ev["pai"]), 0) - 1
        elif ty == "kita" and sanma:
            due = actor
    return (UNFINISHED, len(log), kc, NO_SEAT) if st == 1 else (OK, 0, 0, NO_SEAT)


# ---------------------------------------------------------------- mutations
def _hands_before(log, n, at):
    """the seats' concealed hands (tile name -> copies) before event `at`, by the events of its kyoku"""
    hands = [dict() for _ in range(4)]
    for ev in log[:at]:
        ty, a = _type(ev), int(ev.get("actor", 0) or 0) & 3
        if ty == "start_kyoku":
            hands = [dict() for _ in range(4)]
            for s, h in enumerate(ev["tehais"][:n]):
                for x in h:
                    hands[s][x] = hands[s].get(x, 0) + 1
        elif ty == "tsumo":
            hands[a][ev["pai"]] = hands[a].get(ev["pai"], 0) + 1
        elif ty in ("dahai", "kakan"):
            hands[a][ev["pai"]] -= 1
        elif ty in ("chi", "pon", "daiminkan", "ankan"):
            for c in ev["consumed"]:
                hands[a][c] -= 1
    return [{k: v for k, v in h.items() if v > 0} for h in hands]


def _seen_before(log, n, at):
    """tile type -> copies among the dealt tiles, dora markers and draws of the kyoku that event `at` lies in, before `at`; and the names"""
    seen, names = {}, set()
    for ev in log[:at]:
        ty = _type(ev)
        if ty == "start_kyoku":
            seen, names = {}, set()
            tiles = [x for h in ev["tehais"][:n] for x in h] + [ev["dora_marker"]]
        elif ty == "tsumo":
            tiles = [ev["pai"]]
        elif ty == "dora":
            tiles = [ev["dora_marker"]]
        else:
            continue
        for x in tiles:
            seen[tid(x) >> 2] = seen.get(tid(x) >> 2, 0) + 1
            names.add(x)
    return seen, names


_ALL_NAMES = [f"{k}{s}" for s in "mps" for k in range(1, 10)] + ["E", "S", "W", "N", "P", "F", "C"]


def mutations(log, n, positions=("first", "mid", "last")):
    """name -> (mutated log, expected code, first event index the finding may have).  Every kind is tried in the log's first kyoku, a
    middle one and its last (`_first`, `_mid`, `_last`); a kind that a kyoku cannot host is left out there; `positions` keeps
    some of the three.  The log must be a complete game of at least three kyokus."""
    starts = [i for i, e in enumerate(log) if e["type"] == "start_kyoku"]
    ends = starts[1:] + [len(log)]
    assert len(starts) >= 3, "mutations() wants a log of at least three kyokus"
    where = {p: k for p, k in (("first", 0), ("mid", len(starts) // 2), ("last", len(starts) - 1)) if p in positions}
    out = {}

    def put(name, events, code, point):
        out[name] = (events, code, point)

    def edit(i, **kw):
        m = list(log)
        m[i] = dict(log[i], **kw)
        return m

    # 2: no start_kyoku ahead of the first draw - and, without the start_game, at the log's first event
    put("no_start_kyoku", log[: starts[0]] + log[starts[0] + 1:], NO_START_KYOKU, starts[0])
    put("no_start_kyoku_at_first_event", log[starts[0] + 1:], NO_START_KYOKU, 0)
    # 3 at the log's last event: a draw behind everything
    put("tsumo_after_the_end", log + [{"type": "tsumo", "actor": 0, "pai": "1m"}], AFTER_END, len(log))
    # 4: the log cut in the middle of its last kyoku (the finding lies at the log's length)
    cut = (starts[-1] + len(log)) // 2
    put("cut_mid_kyoku", log[:cut], UNFINISHED, cut)
    for pos, k in where.items():
        lo, hi = starts[k], ends[k]
        span = range(lo + 1, hi)
        ty = [_type(log[i]) for i in range(len(log))]
        horas = [i for i in span if ty[i] == "hora"]
        tsumos = [i for i in span if ty[i] == "tsumo"]
        dahais = [i for i in span if ty[i] == "dahai"]
        # 3: a draw right behind the kyoku's (last) hora
        if horas:
            put(f"tsumo_after_hora_{pos}", log[: horas[-1] + 1] + [{"type": "tsumo", "actor": 0, "pai": "1m"}] + log[horas[-1] + 1:], AFTER_END, horas[-1] + 1)
        # 4: "delete a hora" - with the end_kyoku behind it, which would close the kyoku as well as the hora did: what follows (the next
        # start_kyoku, or end_game) then arrives in a kyoku that is not over
        if len(horas) == 1 and ty[horas[0] + 1] == "end_kyoku":
            put(f"no_hora_{pos}", log[: horas[0]] + log[horas[0] + 2:], UNFINISHED, horas[0])
        # 5: an actor that is no seat (on a draw: the kyoku walk of the tables indexes the seats of dahai / reach events and raises there),
        # and a claim from oneself
        if tsumos:
            put(f"actor_is_no_seat_{pos}", edit(tsumos[len(tsumos) // 2], actor=n), ACTOR, tsumos[len(tsumos) // 2])
        pons = [i for i in span if ty[i] == "pon"]
        if pons:
            put(f"pon_from_oneself_{pos}", edit(pons[0], target=log[pons[0]]["actor"]), ACTOR, pons[0])
        # 6: "delete a tsumo so that the next draw is out of turn" - the seat's whole turn, draw and discard: with the discard left in, the
        # first finding is that discard (its seat is offered nothing), one event ahead of the draw; and a draw repeated
        turns = [i for i in tsumos if i + 2 < hi and ty[i + 1] == "dahai" and ty[i + 2] == "tsumo" and log[i + 1]["actor"] == log[i]["actor"]
                 and log[i + 2]["actor"] != log[i]["actor"] and i - 1 > lo and ty[i - 1] == "dahai"]
        if turns:
            i = turns[len(turns) // 2]
            put(f"no_turn_{pos}", log[:i] + log[i + 2:], DRAW_OUT_OF_TURN, i)
        if tsumos:
            i = tsumos[len(tsumos) // 3]
            put(f"tsumo_twice_{pos}", log[: i + 1] + [copy.deepcopy(log[i])] + log[i + 1:], DRAW_OUT_OF_TURN, i + 1)
        # 7: a discard by the seat opposite (3P: the next seat)
        plain = [i for i in dahais if ty[i - 1] == "tsumo"]
        if plain:
            i = plain[len(plain) // 2]
            put(f"dahai_by_another_seat_{pos}", edit(i, actor=(log[i]["actor"] + (2 if n == 4 else 1)) % n), NOT_OFFERED, i)
        # 8: a discard of a tile the seat does not hold; a pon that consumes two copies where the seat holds one
        if plain:
            i = plain[len(plain) // 3]
            held = _hands_before(log, n, i)[log[i]["actor"]]
            put(f"dahai_not_held_{pos}", edit(i, pai=[x for x in _ALL_NAMES if x not in held][0], tsumogiri=False), TILE_NOT_HELD, i)
        for i in pons:
            held = _hands_before(log, n, i)[log[i]["actor"]]
            single = [x for x in held if held[x] == 1]
            if single:
                put(f"pon_of_one_copy_{pos}", edit(i, consumed=[single[0], single[0]]), TILE_NOT_HELD, i)
                break
        # 9: a draw replaced by the fifth copy of a tile type, and by a second red five
        for i in reversed(tsumos):
            if f"fifth_copy_{pos}" in out and f"second_red_five_{pos}" in out:
                break
            seen, names = _seen_before(log, n, i)
            full = [x for x in _ALL_NAMES if seen.get(tid(x) >> 2, 0) >= 4]
            if full and f"fifth_copy_{pos}" not in out:
                put(f"fifth_copy_{pos}", edit(i, pai=full[0]), TILE_COUNT, i)
            red = [x for x in ("5mr", "5pr", "5sr") if x in names]
            if red and f"second_red_five_{pos}" not in out:
                put(f"second_red_five_{pos}", edit(i, pai=red[0]), TILE_COUNT, i)
        # 10: a chi (3P: a pon) whose consumed tiles the seat holds but which form no meld with the tile: tiles of other suits
        for i in [j for j in span if ty[j] == ("pon" if n == 3 else "chi")]:
            held = _hands_before(log, n, i)[log[i]["actor"]]
            pai = log[i]["pai"]
            suit = lambda x: x[1] if x[0].isdigit() else "z"   # noqa: E731
            other = [x for x in held if suit(x) != suit(pai)]
            if len(other) >= 2:
                put(f"meld_of_nothing_{pos}", edit(i, consumed=other[:2]), NO_LEGAL_MATCH, i)
                break
        # 5 again: a dealer that is no seat
        put(f"oya_is_no_seat_{pos}", edit(lo, oya=n), ACTOR, lo)
        # 11, 12: a later kyoku that starts from other scores / with one more stick on the table than the points account for
        if k:
            sc = list(log[lo]["scores"])
            sc[(k + 1) % n] += 100
            put(f"scores_jump_{pos}", edit(lo, scores=sc), SCORE_CONTINUITY, lo)
            key = "kyoutaku" if "kyoutaku" in log[lo] else "kyotaku"
            put(f"one_more_stick_{pos}", edit(lo, **{key: int(log[lo].get(key, 0)) + 1}), SCORE_CONSERVATION, lo)
    return out


def kinds(muts):
    """the codes a mutations() dict covers"""
    return {code for _, code, _ in muts.values()}


# ---------------------------------------------------------------- the corpus
_LOGS = {}


def oracle_logs(mode, count=32):
    """`count` complete games of game mode `mode` written by the oracle (Game.log): half under its random policy, half under the greedy one"""
    import json

    from oracle import oracle

    if (mode, count) not in _LOGS:
        logs = []
        for g in range(count):
            o = oracle.Game(game_mode=mode, seed=9100 + 37 * mode + g)
            o.reset()
            for _ in range(6000):
                if o.status()[2]:
                    break
                o.step([int(x) for x in (o.greedy_actions(61, g, 96) if g % 2 else o.random_actions(61, g))])
            assert o.status()[2], "an oracle game did not finish"
            logs.append([json.loads(x) for x in o.log()])
        _LOGS[mode, count] = logs
    return _LOGS[mode, count]
