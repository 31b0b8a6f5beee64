"""The GRP rank model's rows restated plainly (numpy and Python only; no torch, no library): the expectation of tests/test_grp_ref.py
and tests/test_gpu_grp_rows.py.

The row of (kyoku, seat p), n players, is 4n + 4 float32:
    init[0..n) / S, end[0..n) / S, delta[0..n) / 12000, chang / 3, ju / 3, ben / 4, liqibang / 4, onehot(p)[0..n)
S = 25000 (4P) / 35000 (3P), delta = end - init.  Every division is Python's int / float (a float64 division), rounded once by np.float32 -
what riichienv-ml's GrpReplayDataset._encode_features and RewardPredictor.calc_all_player_rewards do."""
import numpy as np

_BAKAZE = {"S": 1, "W": 2, "N": 3}


def score_norm(n):
    return 35000.0 if n == 3 else 25000.0


def row(init, end, meta, n, p):
    """one row as a list of np.float32; init / end: n (or more) Python ints, meta: (chang, ju, ben, liqibang)"""
    S = score_norm(n)
    init, end = [int(v) for v in init[:n]], [int(v) for v in end[:n]]
    chang, ju, ben, liqibang = (int(v) for v in meta)
    vals = [v / S for v in init] + [v / S for v in end] + [(e - s) / 12000.0 for s, e in zip(init, end)]
    vals += [chang / 3.0, ju / 3.0, ben / 4.0, liqibang / 4.0]
    vals += [1.0 if q == p else 0.0 for q in range(n)]
    return [np.float32(v) for v in vals]


def rows(init, end, meta, n):
    """[R][>= n] ints, [R][>= n] ints, [R][4] ints -> float32 [R, n, 4n + 4]"""
    out = np.zeros((len(init), n, 4 * n + 4), dtype=np.float32)
    for r in range(len(init)):
        for p in range(n):
            out[r, p] = row(init[r], end[r], meta[r], n, p)
    return out


def rows_reciprocal(init, end, meta, n):
    """the WRONG arithmetic, for telling it apart: float32(int) * float32(1 / constant)"""
    f = np.float32
    out = np.zeros((len(init), n, 4 * n + 4), dtype=np.float32)
    rs, rd, r3, r4 = f(1.0 / score_norm(n)), f(1.0 / 12000.0), f(1.0 / 3.0), f(1.0 / 4.0)
    for r in range(len(init)):
        i, e = [int(v) for v in init[r][:n]], [int(v) for v in end[r][:n]]
        base = [f(v) * rs for v in i] + [f(v) * rs for v in e] + [f(b - a) * rd for a, b in zip(i, e)]
        base += [f(meta[r][0]) * r3, f(meta[r][1]) * r3, f(meta[r][2]) * r4, f(meta[r][3]) * r4]
        for p in range(n):
            out[r, p] = base + [f(1.0 if q == p else 0.0) for q in range(n)]
    return out


def ranks(final_scores, n):
    """the place of every seat (0 = first) in final_scores[:n]: descending, equal scores rank by seat"""
    sc = [int(v) for v in final_scores[:n]]
    order = sorted(range(n), key=lambda q: (-sc[q], q))
    out = [0] * n
    for place, seat in enumerate(order):
        out[seat] = place
    return out


def _kyokus(log):
    """the kyokus of one log of MJAI event dicts: dicts with meta, start, end (both padded to 4 seats) - the start scores are the
    start_kyoku's, the end scores the next kyoku's start scores, and for the last kyoku what its hora / ryukyoku events give (`scores`,
    else `deltas` / `delta` applied to the start scores minus the riichi deposits: accepted ones for a hora, declared ones for a
    ryukyoku; a second hora of the same batch adds its deltas), else the start scores."""
    out, cur = [], None
    for ev in log:
        ty = ev.get("type")
        if ty == "start_kyoku":
            if cur is not None:
                out.append(cur)
            sc = [int(v) for v in ev["scores"]]
            cur = {"meta": (_BAKAZE.get(ev.get("bakaze", "E"), 0), int(ev["kyoku"]) - 1, int(ev.get("honba", 0)), int(ev.get("kyoutaku", ev.get("kyotaku", 0)))),
                   "scores": sc, "end": list(sc), "reached": [False] * len(sc), "accepted": [False] * len(sc), "batch": False}
            continue
        if ty in ("end_kyoku", "end_game"):
            if cur is not None:
                out.append(cur)
            cur = None
            continue
        if cur is None:
            continue
        first = not cur["batch"]
        cur["batch"] = ty == "hora"
        a = ev.get("actor")
        if ty == "reach":
            cur["reached"][a] = True
        elif ty == "reach_accepted":
            cur["accepted"][a] = True
        elif ty in ("hora", "ryukyoku"):
            deltas = ev.get("deltas", ev.get("delta"))
            if ev.get("scores") is not None:
                cur["end"] = [int(v) for v in ev["scores"]]
            elif deltas is not None:
                for i, d in enumerate(deltas[: len(cur["end"])]):
                    if ty == "hora" and not first:
                        cur["end"][i] += int(d)
                    else:
                        sticks = cur["accepted"] if ty == "hora" else cur["reached"]
                        cur["end"][i] = cur["scores"][i] + int(d) - (1000 if sticks[i] else 0)
    if cur is not None:
        out.append(cur)
    for i in range(len(out) - 1):
        out[i]["end"] = list(out[i + 1]["scores"])
    for k in out:
        k["start"] = (k["scores"] + [0] * 4)[:4]
        k["end"] = ((k["end"] if k["end"] else k["scores"]) + [0] * 4)[:4]
    return out


def logset_rows(logs, n, bad=()):
    """logs: lists of MJAI event dicts -> {"x" f32 [K, n, 4n + 4], "meta" i32 [K, 4], "rank" u8 [K, n], "log_of" i32 [K], "kyoku_offsets"
    i64 [M + 1], "start" / "end" i32 [K, 4]} in (log, kyoku) order.  rank: the seat's place in the end scores of its log's LAST kyoku;
    255 for the logs listed in `bad` (logs that do not parse)."""
    meta, start, end, rank, log_of, koff = [], [], [], [], [], [0]
    for l, log in enumerate(logs):
        ks = _kyokus(log)
        final = ranks(ks[-1]["end"], n) if ks else None
        for k in ks:
            meta.append(k["meta"])
            start.append(k["start"])
            end.append(k["end"])
            rank.append([255] * n if l in bad else final)
            log_of.append(l)
        koff.append(len(meta))
    K = len(meta)
    return {"x": rows(start, end, meta, n).reshape(K, n, 4 * n + 4), "meta": np.array(meta, dtype=np.int64).reshape(K, 4).astype(np.int32),
            "rank": np.array(rank, dtype=np.uint8).reshape(K, n), "log_of": np.array(log_of, dtype=np.int32), "kyoku_offsets": np.array(koff, dtype=np.int64),
            "start": np.array(start, dtype=np.int32).reshape(K, 4), "end": np.array(end, dtype=np.int32).reshape(K, 4)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the inputs both test modules share
SWEEP = list(range(-50000, 150001, 100))            # every multiple of 100 from -50 000 to 150 000: 2 001 values
EXTREMES = [2 ** 31 - 1, -(2 ** 31) + 1, 2 ** 24 + 1, -(2 ** 24) - 1, 0, 1, -1]


def sweep_case():
    """(init [R][4], delta [R][4], meta [R][4]) int lists: seat 0's init and seat 1's delta sweep SWEEP, meta runs over 0..20, and a
    handful of rows hold int32 extremes (2^24 + 1: the first integer float32 cannot hold)"""
    init, delta, meta = [], [], []
    for i, v in enumerate(SWEEP):
        init.append([v, 25000, 25000 - (i % 7) * 100, 30000])
        delta.append([0, SWEEP[(i * 7 + 3) % len(SWEEP)], -v if abs(v) < 2 ** 20 else 0, 100 * (i % 5)])
        meta.append([i % 21, (i + 5) % 21, (i + 11) % 21, (i + 17) % 21])
    for i, v in enumerate(EXTREMES):
        init.append([v, EXTREMES[(i + 1) % len(EXTREMES)], 0, v])
        delta.append([0, 0, v, 0] if abs(v) > 2 ** 30 else [v, -v, v, 1])
        meta.append([v, -1, 255, 65535] if abs(v) <= 2 ** 24 + 1 else [0, -1, 255, 65535])
    return init, delta, meta


def tehai(seed=0):
    names = [f"{d}{s}" for s in "mps" for d in range(1, 10)] + ["E", "S", "W", "N", "P", "F", "C"]
    return [names[(seed * 5 + 3 * j) % len(names)] for j in range(13)]


def start_kyoku(scores, bakaze="E", kyoku=1, honba=0, kyotaku=0, oya=0, key="kyotaku", seats=4):
    return {"type": "start_kyoku", "bakaze": bakaze, "dora_marker": "1m", "kyoku": kyoku, "honba": honba, key: kyotaku, "oya": oya,
            "scores": list(scores), "tehais": [tehai(s) for s in range(seats)]}


def hand_made_log(kyokus, seats=4, end_game=True):
    """a short log: kyokus = list of (start_kyoku kwargs, ending) with ending None (no end event), ("hora", actor, target, deltas),
    ("hora_scores", actor, target, scores), ("ryukyoku", deltas) or ("reach_hora", actor, target, deltas) (the winner's accepted riichi)"""
    log = [{"type": "start_game", "names": ["a", "b", "c", "d"][:seats]}]
    for kw, ending in kyokus:
        log.append(start_kyoku(seats=seats, **kw))
        oya = kw.get("oya", 0)
        log.append({"type": "tsumo", "actor": oya, "pai": "5m"})
        if ending is not None and ending[0] == "reach_hora":
            log.append({"type": "reach", "actor": oya})
            log.append({"type": "dahai", "actor": oya, "pai": "5m", "tsumogiri": True})
            log.append({"type": "reach_accepted", "actor": oya})
        else:
            log.append({"type": "dahai", "actor": oya, "pai": "5m", "tsumogiri": True})
        if ending is None:
            continue
        if ending[0] in ("hora", "reach_hora"):
            log.append({"type": "hora", "actor": ending[1], "target": ending[2], "deltas": list(ending[3])})
        elif ending[0] == "hora_scores":
            log.append({"type": "hora", "actor": ending[1], "target": ending[2], "scores": list(ending[3])})
        else:
            log.append({"type": "ryukyoku", "deltas": list(ending[1])})
        log.append({"type": "end_kyoku"})
    if end_game:
        log.append({"type": "end_game"})
    return log


def random_logs(n_logs, seats, seed, max_kyokus=12):
    """n_logs hand-made logs of 1 .. max_kyokus kyokus with running scores, every kind of ending, ties and negative scores"""
    rng = np.random.default_rng(seed)
    logs = []
    for _ in range(n_logs):
        sc = [35000 if seats == 3 else 25000] * seats
        ks = []
        for k in range(int(rng.integers(1, max_kyokus + 1))):
            kw = dict(scores=list(sc), bakaze="ESWN"[int(rng.integers(0, 4))], kyoku=int(rng.integers(0, 5)), honba=int(rng.integers(0, 9)),
                      kyotaku=int(rng.choice([0, 1, 2, 300])), oya=int(rng.integers(0, seats)), key=str(rng.choice(["kyotaku", "kyoutaku"])))
            pay = int(rng.choice([0, 1000, 7700, 12000, 32000]))
            w, l = int(rng.integers(0, seats)), int(rng.integers(0, seats))
            d = [0] * seats
            d[w] += pay
            d[l] -= pay
            kind = int(rng.integers(0, 5))
            ending = [None, ("hora", w, l, d), ("hora_scores", w, l, [a + b for a, b in zip(sc, d)]), ("ryukyoku", d), ("reach_hora", w, l, d)][kind]
            if kind == 4:
                kw["oya"] = w        # the dealer reaches in hand_made_log: make it the winner so that the deposit rule matters
            ks.append((kw, ending))
            sc = [a + b for a, b in zip(sc, d)]
        logs.append(hand_made_log(ks, seats=seats, end_game=bool(rng.integers(0, 2))))
    return logs
