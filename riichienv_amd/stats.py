"""How the agents played: the per-(kyoku, seat) play statistics of a log set (LogSet.play_stats: rmj_logset_playstats_device,
csrc/rmj_playstats.hip.h) and the rates a maintainer reads after a run.

    play_stats(source)                  LogSet.play_stats of a LogSet, or of the set a LogSampleBuilder / GrpDataset holds
    summarize(source_or_table, hero)    a dict of floats: win rate, tsumo share, deal-in rate, riichi rate and turn, call rate, ...
    COLUMNS                             the names of the 16 columns; rows[..., COLUMNS.index("WIN")]

The table is built by one kernel over the resident records; summarize forms every sum on the table's device as int64, moves them to the
host in one transfer and divides there in float64.  The per-(kyoku, seat) columns are also the usual auxiliary targets of a mahjong
network (will this seat win / deal in this round): play_stats(source)["rows"] is a device tensor in the table order of grp_rows."""
from __future__ import annotations

import numpy as np

from . import abi
from .logset import LogSet

COLUMNS = tuple(abi.PLAYSTAT_NAMES)
_C = {name: i for i, name in enumerate(COLUMNS)}


def _logset(source):
    return source if isinstance(source, LogSet) else getattr(source, "logset", None)


def play_stats(source, num_players=None):
    """LogSet.play_stats of `source` - a LogSet, or anything that holds one as `.logset` (LogSampleBuilder, GrpDataset): rows [K, 4, 16] i32,
    valid [K] bool, log_of [K] i64, kyoku_offsets [M + 1] i64 on the device, nothing read back"""
    ls = _logset(source)
    if ls is None:
        raise TypeError("play_stats takes a LogSet or an object that holds one as .logset")
    return ls.play_stats(num_players)


def _table_of(source, num_players, table=None):
    """the table dict summarize works on: rows, valid, log_of, num_players and - where the source has them - start_scores / end_scores
    [K, 4] and rank [K, n] (0 = first)"""
    import torch

    ls = _logset(source)
    if ls is not None:
        t = dict(table) if table is not None else ls.play_stats(num_players)
        if ls.n_kyokus:
            if ls.owns_tables:
                t["start_scores"], t["end_scores"] = ls.device_scores()
            else:
                t["start_scores"], t["end_scores"] = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=ls.device) for a in (ls.start_scores, ls.end_scores))
            t["rank"] = ls.final_ranks(t["num_players"])
        return t
    if isinstance(source, dict):
        t = {k: (v if isinstance(v, (int, type(None))) or torch.is_tensor(v) else torch.as_tensor(np.asarray(v))) for k, v in source.items()}
    else:
        t = {"rows": source if torch.is_tensor(source) else torch.as_tensor(np.asarray(source))}
    rows = t["rows"]
    if rows.dim() != 3 or tuple(rows.shape[1:]) != (4, len(COLUMNS)):
        raise ValueError("a play-statistics table is [K, 4, 16]")
    if num_players is not None or t.get("num_players") is None:
        t["num_players"] = int(4 if num_players is None else num_players)
    if t.get("valid") is None:
        t["valid"] = rows[:, 0, 0] >= 0                       # the rows of a log that did not parse are -1 everywhere
    return t


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def summarize(source_or_table, hero=None, num_players=None, table=None):
    """The rates of a run as a dict of floats.  source_or_table: a LogSet (or its holder), the dict LogSet.play_stats returns, or a bare
    [K, 4, 16] table (numpy or torch; num_players 4 unless given).  With a LogSet, `table` may be the dict its play_stats() already
    returned: the kernel is then not run again, and the set adds only its score tables and ranks (LogSet.final_ranks).

    hero=None pools every seat < num_players: a sample is a (kyoku, seat) pair.  hero as an [M] integer array or tensor picks one seat per
    log (joined through log_of) - the hero seat of a PPOCollector evaluation; a log whose hero is no seat contributes nothing.  The kyokus of
    logs that did not parse (valid False, rows of -1) are left out.  An empty denominator gives nan.

      kyokus               the samples: (kyoku, seat) pairs pooled, or kyokus with a hero
      win_rate             samples with WIN > 0 / kyokus
      tsumo_share          sum WIN_TSUMO / sum WIN
      deal_in_rate         samples with DEAL_IN > 0 / kyokus
      riichi_rate          samples with RIICHI > 0 / kyokus
      riichi_accept_share  samples with RIICHI_ACCEPTED > 0 / samples with RIICHI > 0
      call_rate            samples with CALLS > 0 / kyokus
      ryukyoku_rate        samples whose kyoku saw a RYUKYOKU / kyokus
      mean_riichi_turn     sum RIICHI_TURN / samples with RIICHI_TURN > 0
      mean_win_turn        sum WIN_TURN over the samples with WIN > 0 / their number
      dealer_win_rate      dealer samples with WIN > 0 / dealer samples
      tsumogiri_share      sum TSUMOGIRI / sum DISCARDS
      win_points_mean, deal_in_points_mean   mean of end - start over the samples with WIN > 0, of start - end over those with DEAL_IN > 0
                           (only where the kyoku score tables are there: a LogSet, or start_scores / end_scores in the dict)
      rank_mean, rank_rates   the mean final place (0 = first) and the share of every place, one sample per log and pooled / hero seat
                           (only where the ranks are there: a LogSet - the rank column of grp_rows() - or rank [K, n] in the dict)"""
    import torch

    t = _table_of(source_or_table, num_players, table)
    rows, n = t["rows"], int(t["num_players"])
    dev, K = rows.device, rows.shape[0]
    c = rows.to(torch.int64)
    valid = t["valid"].to(dev).to(torch.bool)
    seats = torch.arange(4, device=dev)
    if hero is None:
        sel = valid[:, None] & (seats < n)[None, :]
    else:
        if t.get("log_of") is None:
            raise ValueError("a hero per log needs the table's log_of")
        h = (hero if torch.is_tensor(hero) else torch.as_tensor(np.asarray(hero))).to(dev).to(torch.int64)
        hk = h[t["log_of"].to(dev).to(torch.int64)] if K else torch.zeros((0,), dtype=torch.int64, device=dev)
        sel = valid[:, None] & (seats[None, :] == hk[:, None]) & (seats < n)[None, :]

    def col(name):
        return c[:, :, _C[name]]

    def count(mask):
        return (mask & sel).sum()

    def total(x, mask=None):
        return (x * (sel if mask is None else sel & mask)).sum()

    win, deal = col("WIN") > 0, col("DEAL_IN") > 0
    sums = [sel.sum(), count(win), total(col("WIN")), total(col("WIN_TSUMO")), count(deal), count(col("RIICHI") > 0), count(col("RIICHI_ACCEPTED") > 0),
            count(col("CALLS") > 0), count((col("END") & abi.PLAYSTAT_END_RYUKYOKU) != 0), total(col("RIICHI_TURN")), count(col("RIICHI_TURN") > 0),
            total(col("WIN_TURN"), win), count((col("DEALER") > 0) & win), count(col("DEALER") > 0), total(col("TSUMOGIRI")), total(col("DISCARDS"))]
    points = t.get("start_scores") is not None and t.get("end_scores") is not None
    if points:
        gain = t["end_scores"].to(dev).to(torch.int64) - t["start_scores"].to(dev).to(torch.int64)
        sums += [total(gain, win), total(-gain, deal)]
    ranks = t.get("rank") is not None and t.get("log_of") is not None
    if ranks:
        lo = t["log_of"].to(dev).to(torch.int64)
        first = torch.ones((K,), dtype=torch.bool, device=dev)
        first[1:] = lo[1:] != lo[:-1]                         # a log's first kyoku row: one sample per log
        rk = torch.full((K, 4), 255, dtype=torch.int64, device=dev)
        rk[:, :n] = t["rank"].to(dev).to(torch.int64)[:, :n]
        rsel = sel & first[:, None] & (rk < n)
        sums += [rsel.sum(), (rk * rsel).sum()] + [((rk == r) & rsel).sum() for r in range(n)]
    s = [int(v) for v in torch.stack(sums).cpu().tolist()]    # the one transfer
    ky, wins = s[0], s[1]
    out = {"kyokus": float(ky), "win_rate": _ratio(wins, ky), "tsumo_share": _ratio(s[3], s[2]), "deal_in_rate": _ratio(s[4], ky), "riichi_rate": _ratio(s[5], ky),
           "riichi_accept_share": _ratio(s[6], s[5]), "call_rate": _ratio(s[7], ky), "ryukyoku_rate": _ratio(s[8], ky), "mean_riichi_turn": _ratio(s[9], s[10]),
           "mean_win_turn": _ratio(s[11], wins), "dealer_win_rate": _ratio(s[12], s[13]), "tsumogiri_share": _ratio(s[14], s[15])}
    at = 16
    if points:
        out["win_points_mean"], out["deal_in_points_mean"] = _ratio(s[at], wins), _ratio(s[at + 1], s[4])
        at += 2
    if ranks:
        out["rank_mean"] = _ratio(s[at + 1], s[at])
        out["rank_rates"] = [_ratio(v, s[at]) for v in s[at + 2: at + 2 + n]]
    return out
