"""Round-end census of MJAI logs: which kinds of round end, transition and game end a batch of logs went through.

Pure Python over the logs (no GPU, no oracle).  A log may hold several games one after the other (a slot's drained stream across
auto-reset restarts: ... end_game, start_game ...).  The win conditions that depend on the wall and the calls - chankan, rinshan,
haitei, houtei - come from the replay's win-context reconstruction (riichienv_amd.replay, WinResultContextIterator) with the
corrections its MJAI reader needs (win_contexts below); scripts/parity_coverage.py evaluates the same contexts on the GPU.

Kinds (census keys):
  wins         tsumo_dealer, tsumo_nondealer, ron_single, ron_double, ron_triple (MJSOUL; TENHOU draws `sanchaho`),
               win_kyotaku (a winner collects riichi sticks), ron_double_kyotaku (... in a double Ron), win_honba (honba > 0),
               tsumo_nondealer_honba, pao (the deltas of one win show a second payer, or a single payer of a Tsumo), chankan,
               rinshan, haitei, houtei
  draws        draw_tenpai_<k> (exhaustive draw with k seats tenpai; draw_tenpai_0_or_all when no payment moved and no next round
               tells which), ryukyoku_<reason> for every other reason of rmj_host.h's list (nagashimangan, kyushu_kyuhai, sufuurenta,
               suukansansen, suucha_riichi, sanchaho) and ryukyoku_illegal_action
  transitions  renchan_win (the dealer won and deals again), renchan_tenpai_draw (the dealer was tenpai at an exhaustive draw and
               deals again), rotation (the deal moves on), kyotaku_carried (sticks on the table carried over a draw)
  game ends    game_end (no score below 0), bust (a score below 0), south_entry / west_entry (the first round of that wind after
               rounds of an earlier one: an East game's or a half game's extension), tied_top (two or more seats share the top
               final score: ranks fall back to seat order)
"""
import collections
import json

from riichienv_amd import abi
from riichienv_amd.replay import MjaiReplay

WIN_KINDS = ("tsumo_dealer", "tsumo_nondealer", "ron_single", "ron_double", "ron_triple", "win_kyotaku", "ron_double_kyotaku",
             "win_honba", "tsumo_nondealer_honba", "pao", "chankan", "rinshan", "haitei", "houtei")
DRAW_KINDS = tuple(f"draw_tenpai_{k}" for k in range(5)) + ("draw_tenpai_0_or_all",)
ABORTIVE_KINDS = tuple("ryukyoku_" + r for r in ("nagashimangan", "kyushu_kyuhai", "sufuurenta", "suukansansen", "suucha_riichi",
                                                  "sanchaho", "illegal_action"))
TRANSITION_KINDS = ("renchan_win", "renchan_tenpai_draw", "rotation", "kyotaku_carried")
GAME_END_KINDS = ("game_end", "bust", "south_entry", "west_entry", "tied_top")
KINDS = WIN_KINDS + DRAW_KINDS + ABORTIVE_KINDS + TRANSITION_KINDS + GAME_END_KINDS
_WIND = {"E": 0, "S": 1, "W": 2, "N": 3}


def win_contexts(k, notes=None):
    """[(WinResultContext, hora event, index of the hora within the round)] of one replay Kyoku, with the conditions set right where
    the reference's MJAI reader and its own environment disagree (each correction is counted in `notes`, a Counter); None when the
    reader reconstructs a different number of wins than the round has hora events."""
    notes = collections.Counter() if notes is None else notes
    horas = [e for e in k.mjai_events if e.get("type") == "hora"]
    ctxs = list(k.take_win_result_contexts())
    if len(ctxs) != len(horas):
        notes["context count mismatch"] += 1
        return None
    out = []
    # A tsumo on the replacement draw of a kan / kita: the reference's iterator recognises it by the `doras` list of a Mahjong Soul
    # DealTile (replay/mod.rs:1806-1809) and drops the flag at any other draw (:1735-1736), so for MJAI logs it never sets rinshan;
    # the census marks those wins itself
    hist = [e for e in k.mjai_events if e.get("type") not in ("dora", "reach", "reach_accepted")]
    for i, (c, h) in enumerate(zip(ctxs, horas)):
        at = next(j for j, e in enumerate(hist) if e is h)
        if h["actor"] == h["target"] and at >= 2 and hist[at - 1]["type"] == "tsumo" and hist[at - 2]["type"] in ("ankan", "kakan", "daiminkan", "kita"):
            c.conditions["rinshan"], c.conditions["haitei"] = True, False
            notes["rinshan (marked by the census)"] += 1
        # Two more places where the reference's MJAI reader and its own environment disagree: a kita before the riichi ends the
        # first turn in the environment (state_3p/sanma.rs:39) but is no "call" for the reader's double-riichi flag
        # (mjai_replay.rs:415, :606-611) ...
        if c.conditions["double_riichi"]:
            reach_at = next(j for j, e in enumerate(k.mjai_events) if e.get("type") == "reach" and e.get("actor") == c.seat)
            # (up to the riichi DISCARD: a seat may declare, take a kita and only then discard)
            reach_at = next(j for j, e in enumerate(k.mjai_events) if j > reach_at and e.get("type") == "dahai" and e.get("actor") == c.seat)
            if any(e.get("type") == "kita" for e in k.mjai_events[:reach_at]):
                c.conditions["double_riichi"] = False
                notes["riichi after a kita (reader says double)"] += 1
        # ... and a Ron on a kita finds no winning tile in a hora event without `pai` (mjai_replay.rs:541-559 has no BaBei case:
        # tile 0)
        if h["actor"] != h["target"] and at >= 1 and hist[at - 1]["type"] in ("kita", "hora") and h.get("pai") is None:
            prev = next(e for e in reversed(hist[:at]) if e["type"] != "hora")
            if prev["type"] == "kita":
                north = abi.mjai_to_tid("N")
                c.tiles = list(c.tiles[:-1]) + [north]
                c.agari_tile = north
                notes["ron on a kita"] += 1
        # ... nor does a Ron on a kakan whose kan flushed the pending indicator of an earlier open kan: the `dora` event sits between
        # the kakan and the hora, the reader's last action is Dora (tile 0, and no chankan)
        if h["actor"] != h["target"] and h.get("pai") is None:
            full = [e for e in k.mjai_events if e.get("type") not in ("reach", "reach_accepted")]
            at_f = next(j for j, e in enumerate(full) if e is h)
            before = [e for e in full[:at_f] if e["type"] != "hora"]
            if len(before) >= 2 and before[-1]["type"] == "dora" and before[-2]["type"] == "kakan":
                t = abi.mjai_to_tid(before[-2]["pai"])
                c.tiles = list(c.tiles[:-1]) + [t]
                c.agari_tile = t
                c.conditions["chankan"] = True
                notes["chankan behind a dora event"] += 1
        out.append((c, h, i))
    return out


def _split_games(log):
    games, cur = [], None
    for e in log:
        if e["type"] == "start_game":
            cur = [e]
            games.append(cur)
        elif cur is not None:
            cur.append(e)
    return games


def _split_rounds(game):
    rounds, cur = [], None
    for e in game:
        if e["type"] == "start_kyoku":
            cur = [e]
            rounds.append(cur)
        elif cur is not None and e["type"] not in ("end_kyoku", "end_game"):
            cur.append(e)
    return rounds


def _census_round(rnd, nxt, c, notes):
    """one round (start_kyoku .. its last event) and the next round's start_kyoku of the same game (None: the game ended)"""
    head = rnd[0]
    np_ = len(head["scores"])
    oya, honba = head["oya"], head["honba"]
    sticks = head.get("kyotaku", 0) + sum(e["type"] == "reach_accepted" for e in rnd)
    horas = [e for e in rnd if e["type"] == "hora"]
    draws = [e for e in rnd if e["type"] == "ryukyoku"]
    if horas:
        if horas[0]["actor"] == horas[0]["target"]:
            c["tsumo_dealer" if horas[0]["actor"] == oya else "tsumo_nondealer"] += 1
            if horas[0]["actor"] != oya and honba > 0:
                c["tsumo_nondealer_honba"] += 1
        else:
            c[{1: "ron_single", 2: "ron_double", 3: "ron_triple"}[len(horas)]] += 1
        if sticks > 0:
            c["win_kyotaku"] += 1
            if len(horas) == 2:
                c["ron_double_kyotaku"] += 1
        if honba > 0:
            c["win_honba"] += 1
        for h in horas:
            payers = sum(1 for s, d in enumerate(h["deltas"]) if d < 0 and s != h["actor"])
            if payers != (np_ - 1 if h["actor"] == h["target"] else 1):
                c["pao"] += 1
        ctxs = win_contexts(MjaiReplay.from_events(rnd).rounds[0], notes)
        for ctx, _, _ in ctxs or ():
            for f in ("chankan", "rinshan", "haitei", "houtei"):
                if ctx.conditions[f]:
                    c[f] += 1
        if nxt is not None and any(h["actor"] == oya for h in horas):
            if nxt["oya"] == oya and nxt["bakaze"] == head["bakaze"]:
                c["renchan_win"] += 1
    elif draws:
        d = draws[0]
        reason = d.get("reason", "exhaustive_draw")   # (MJAI logs of other sources leave the reason out of an exhaustive draw)
        if reason == "exhaustive_draw":
            pos = sum(x > 0 for x in d["deltas"])
            if pos:
                c[f"draw_tenpai_{pos}"] += 1
            elif nxt is not None:   # no payment: nobody or everybody tenpai, and the dealer deals again only in the second case
                c[f"draw_tenpai_{np_ if nxt['oya'] == oya else 0}"] += 1
            else:
                c["draw_tenpai_0_or_all"] += 1
            if nxt is not None and nxt["oya"] == oya:
                c["renchan_tenpai_draw"] += 1
        elif reason.startswith("Error"):
            c["ryukyoku_illegal_action"] += 1
        else:
            c["ryukyoku_" + reason] += 1
        if nxt is not None and nxt.get("kyotaku", 0) > 0:
            c["kyotaku_carried"] += 1
    if nxt is not None:
        if nxt["oya"] != oya:
            c["rotation"] += 1
        w0, w1 = _WIND[head["bakaze"]], _WIND[nxt["bakaze"]]
        if w1 > w0 and w1 in (1, 2):
            c["south_entry" if w1 == 1 else "west_entry"] += 1


def _final_scores(rnd):
    """the scores after a round: its start scores, less the riichi deposits, plus the deltas of its end (which carry the sticks won)"""
    sc = list(rnd[0]["scores"])
    for e in rnd:
        if e["type"] == "reach_accepted":
            sc[e["actor"]] -= 1000
        elif e["type"] in ("hora", "ryukyoku"):
            sc = [a + b for a, b in zip(sc, e["deltas"])]
    return sc


def census(logs, notes=None):
    """Counter of KINDS over logs (each a list of MJAI event dicts or JSON strings)"""
    c = collections.Counter({k: 0 for k in KINDS})
    notes = collections.Counter() if notes is None else notes
    for log in logs:
        log = [json.loads(e) if isinstance(e, str) else e for e in log]
        for game in _split_games(log):
            rounds = _split_rounds(game)
            for i, rnd in enumerate(rounds):
                _census_round(rnd, rounds[i + 1][0] if i + 1 < len(rounds) else None, c, notes)
            if rounds and game[-1]["type"] == "end_game":
                sc = _final_scores(rounds[-1])
                c["bust" if min(sc) < 0 else "game_end"] += 1
                if sc.count(max(sc)) > 1:
                    c["tied_top"] += 1
    return c


def format_census(c):
    return ", ".join(f"{k} {c[k]}" for k in KINDS)
