"""A verdict for every log of a device log set before samples are built from it: LogSet.validate() (rmj_logcheck_*,
csrc/rmj_logcheck.hip.h) - what riichienv-ml's scripts/validate_logs.py does one log at a time through Python - as a checking replay on
the device: no Python work per event, no host synchronisation inside the replay, no samples and no pool.

Every log gets its first finding (the lowest event index; at one event the lowest code): `code`, `event` (the index of the offending
MJAI event in the log, from 0), `kyoku` (the start_kyoku events of the log up to there), `seat` (255: the event names none) and a
`detail` word.  The codes and when each is raised are listed at RMJ_LOGCHECK_* in include/riichi_mi355x.h; in short:

  OK  PARSE (the set keeps a log that did not parse, on_error="keep": not replayed, `event` = the set's error line)
  NO_START_KYOKU  AFTER_END  UNFINISHED (a log drained from a game still in progress ends this way: the caller may accept the code)
  ACTOR  DRAW_OUT_OF_TURN  NOT_OFFERED  TILE_NOT_HELD (`detail` = the tile id)  TILE_COUNT (`detail` = a tile id)
  NO_LEGAL_MATCH (what fails a log in LogSampleBuilder)  SCORE_CONTINUITY  SCORE_CONSERVATION (validate_logs.py:344-362)

Known limits.  A second or third hora of a multiple ron is not checked against an offer: the kyoku is already over when it arrives.
Settlement amounts are not recomputed: the records carry no ura markers.  Feature encodings are not inspected.  Masked logs
(masked_ok, "?" tiles read as tile 0) trip TILE_COUNT by construction."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, mjai, vecenv
from .streams import StreamLink

NAMES = list(abi.LOGCHECK_NAMES)
CODES = {name: i for i, name in enumerate(NAMES)}


class LogReport:
    """The verdicts of LogSet.validate(), one entry per set log, as tensors on the set's device: code and seat uint8 [M], event / kyoku /
    detail int64 [M], ok = code == OK (bool), counts int64 [16] (the device counters: logs per code).  summary() reads the counters (one
    small transfer); good_ids() and describe() read the verdicts."""

    CODES, NAMES = CODES, NAMES

    def __init__(self, torch, device, code, event, kyoku, seat, detail, counts):
        self.torch, self.device = torch, device
        self.code, self.event, self.kyoku, self.seat, self.detail, self.counts = code, event, kyoku, seat, detail, counts
        self.ok = code == abi.LOGCHECK_OK
        self._host = None

    def __len__(self):
        return int(self.code.shape[0])

    def summary(self):
        """{name: logs with that code}, from the device counters"""
        c = self.counts.cpu().numpy()
        return {name: int(c[i]) for i, name in enumerate(NAMES)}

    def good_ids(self, accept=()):
        """int64 numpy array: the set logs whose code is OK - or one of `accept` (names or numbers, e.g. ("UNFINISHED",)) - in order"""
        codes = [abi.LOGCHECK_OK] + [CODES[a] if isinstance(a, str) else int(a) for a in accept]
        keep = self.torch.isin(self.code, self.torch.tensor(codes, dtype=self.code.dtype, device=self.device))
        return self.torch.nonzero(keep).flatten().cpu().numpy().astype(np.int64)

    def _rows(self):
        if self._host is None:
            self._host = [x.cpu().numpy() for x in (self.code, self.event, self.kyoku, self.seat, self.detail)]
        return self._host

    def describe(self, i):
        """'log 17: TILE_NOT_HELD at event 412 (kyoku 5, seat 2, tile 5mr)'"""
        code, event, kyoku, seat, detail = (int(x[i]) for x in self._rows())
        if code == abi.LOGCHECK_OK:
            return f"log {i}: OK"
        if code == abi.LOGCHECK_PARSE:
            return f"log {i}: PARSE at line {event} ({abi.LOGTEXT_STATUS_NAMES[detail] if detail < len(abi.LOGTEXT_STATUS_NAMES) else detail})"
        where = [f"kyoku {kyoku}"] + ([f"seat {seat}"] if seat != 255 else [])
        if code in (abi.LOGCHECK_TILE_NOT_HELD, abi.LOGCHECK_TILE_COUNT):
            where.append(f"tile {mjai.tid_to_mjai(detail)}")
        return f"log {i}: {NAMES[code]} at event {event} ({', '.join(where)})"


def _empty(torch, device):
    z = lambda dt: torch.zeros((0,), dtype=dt, device=device)   # noqa: E731
    return LogReport(torch, device, z(torch.uint8), z(torch.int64), z(torch.int64), z(torch.uint8), z(torch.int64),
                     torch.zeros((abi.LOGCHECK_COUNTERS,), dtype=torch.int64, device=device))


def validate(logset, game_mode=None, rule=None, n_slots=None, share_stream=True):
    """LogSet.validate: the checking replay of every log of `logset` in n_slots games (default and at most: one per log; memory is per
    slot, the time per event index falls with more of them) -> LogReport.  game_mode defaults from the set's num_players (2: 4p-red-half,
    5: 3p-red-half); rule: None / "tenhou" or "mjsoul", as LogSampleBuilder takes it.  With share_stream the work is issued on torch's
    current stream and the report's tensors are ready in stream order; without, on the library's own stream, which is waited for.
    The set's own kyoku tables feed the two score checks; a set packed from dicts uploads its host tables (the start scores, and
    logset.kyoku_own_end_scores: the end scores every kyoku's own events give - the tables' end column is the next kyoku's start)."""
    torch, L, dev = logset.torch, logset.L, logset.device
    if rule not in (None, "tenhou", "mjsoul"):
        raise ValueError(f"Unknown rule: '{rule}'. Expected 'tenhou' or 'mjsoul'")
    mode = vecenv._mode_id((2 if logset.num_players == 4 else 5) if game_mode is None else game_mode)
    if (3 if mode >= 3 else 4) != logset.num_players:
        raise ValueError("the log set was made for another number of players")
    M = logset.M
    n = M if n_slots is None else int(n_slots)
    if n > M or (M and n < 1):
        raise ValueError(f"n_slots must be between 1 and the number of logs ({M})")
    if M == 0:
        return _empty(torch, dev)
    if not logset.handle:
        raise vecenv.RmjError("the log set is closed")
    bits = abi.RULE_MJSOUL if rule == "mjsoul" else abi.RULE_TENHOU
    env = vecenv.VecRiichiEnv(n, game_mode=mode, seed=0, rule_bits=bits, device=logset.device_index, skip_mjai_logging=True)
    link, h = StreamLink(torch, dev, env), C.c_void_p()
    try:
        stream = torch.cuda.current_stream(dev)
        if share_stream:
            link.bind(stream)
        link.call(L.rmj_logcheck_create, env.h, logset.handle, n, 0, C.byref(h))
        tables = []
        if not logset.owns_tables and logset.n_kyokus:
            from .logset import kyoku_own_end_scores

            own = kyoku_own_end_scores(logset.logs, logset.num_players)
            tables = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev) for a in (logset.start_scores, own)]
            link.call(L.rmj_logcheck_set_scores, h, *tables)
        link.call(L.rmj_logcheck_run_device, h, 0, None)
        v = abi.LogCheckViews()
        vecenv._chk(L.rmj_logcheck_views(h, C.byref(v)))
        wrap = link.wrap
        # clones, in stream order behind the replay (the library's memory goes away with the checker below)
        report = LogReport(torch, dev, wrap(v.code, (M,), "|u1").clone(), wrap(v.event, (M,), "<i4").to(torch.int64), wrap(v.kyoku, (M,), "<i4").to(torch.int64),
                           wrap(v.seat, (M,), "|u1").clone(), wrap(v.detail, (M,), "<i4").to(torch.int64),
                           wrap(v.counts, (abi.LOGCHECK_COUNTERS,), "<i4").to(torch.int64))
        for a in tables:
            a.record_stream(stream)
        return report
    finally:
        # (both destroy calls wait for the handle's stream: the clones above are complete before the memory is freed)
        if h:
            L.rmj_logcheck_destroy(h)
        env.close()
