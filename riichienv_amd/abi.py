"""ctypes mirror of include/riichi_mi355x.h and include/riichi_mi355x_bench.h: the POD structs, the packed-action helpers,
PROTOTYPES - the one table of every function the two headers declare, which vecenv.load_lib() applies - and the wrapper
that hands library-owned device memory to torch (device_tensor).  tests/test_abi.py holds the structs and the table to the
headers: a new C entry is its header declaration plus one row here.

Pure data-layout definitions: no compute, no torch import.  Shared by the product binding (riichienv_amd.vecenv) and by
the test-only oracle binding (oracle/oracle.py).
"""
from __future__ import annotations

import collections
import ctypes as C

NP = 4
MAX_LEGAL = 64
ACTION_SPACE_4P = 82
ACTION_SPACE_3P = 60
MAX_DISCARDS = 32
NO_ACTION = 0xFFFFFFFFFFFFFFFF
TILE_NONE = 0xFF

# ActionType (reference: riichienv-core/src/action.rs:55-68)
DISCARD, CHI, PON, DAIMINKAN, RON, RIICHI, TSUMO, PASS, ANKAN, KAKAN, KYUSHU, KITA = range(12)
ACTION_NAMES = ["DISCARD", "CHI", "PON", "DAIMINKAN", "RON", "RIICHI", "TSUMO", "PASS", "ANKAN", "KAKAN",
                "KYUSHU_KYUHAI", "KITA"]
WAIT_ACT, WAIT_RESPONSE = 0, 1
MELD_CHI, MELD_PON, MELD_DAIMINKAN, MELD_ANKAN, MELD_KAKAN = range(5)
MELD_NAMES = {"chi": 0, "pon": 1, "daiminkan": 2, "ankan": 3, "kakan": 4}

RULE_TENHOU = 64 | 128
RULE_MJSOUL = 1 | 2 | 4 | 8 | 16 | 32 | 128
RULE_REFERENCE_RNG = 256  # not a GameRule field: seed -> wall through the reference's StdRng / shuffle / salt / digest (include/riichi_mi355x.h)


def pack_action(atype: int, tile: int | None = None, consume=()) -> int:
    cons = sorted(consume)
    v = atype & 0xFF
    v |= (TILE_NONE if tile is None else tile) << 8
    v |= len(cons) << 16
    for i, c in enumerate(cons[:4]):
        v |= c << (24 + 8 * i)
    return v


def unpack_action(v: int):
    atype = v & 0xFF
    tile = (v >> 8) & 0xFF
    n = (v >> 16) & 0xFF
    cons = [(v >> (24 + 8 * i)) & 0xFF for i in range(min(n, 4))]
    return atype, (None if tile == TILE_NONE else tile), cons


class MeldView(C.Structure):
    _fields_ = [("meld_type", C.c_uint8), ("n_tiles", C.c_uint8), ("tiles", C.c_uint8 * 4), ("opened", C.c_uint8),
                ("from_who", C.c_int8), ("called_tile", C.c_int16)]


class PlayerView(C.Structure):
    _fields_ = [("hand_len", C.c_uint8), ("hand", C.c_uint8 * 14), ("n_melds", C.c_uint8), ("melds", MeldView * 4),
                ("n_discards", C.c_uint8), ("discards", C.c_uint8 * MAX_DISCARDS),
                ("discard_from_hand_bits", C.c_uint32), ("discard_is_riichi_bits", C.c_uint32),
                ("riichi_declaration_index", C.c_int8), ("score", C.c_int32), ("score_delta", C.c_int32),
                ("riichi_declared", C.c_uint8), ("riichi_stage", C.c_uint8), ("double_riichi_declared", C.c_uint8),
                ("missed_agari_riichi", C.c_uint8), ("missed_agari_doujun", C.c_uint8),
                ("nagashi_eligible", C.c_uint8), ("ippatsu_cycle", C.c_uint8),
                ("pao_daisangen", C.c_int8), ("pao_daisuushi", C.c_int8),
                ("n_forbidden", C.c_uint8), ("forbidden", C.c_uint8 * 2),
                ("riichi_sutehai", C.c_int16), ("last_tedashi", C.c_int16),
                ("n_kita", C.c_uint8), ("kita", C.c_uint8 * 4)]


class StateView(C.Structure):
    _fields_ = [("wall_len", C.c_uint8), ("wall", C.c_uint8 * 136), ("n_dora", C.c_uint8), ("dora", C.c_uint8 * 5),
                ("rinshan_draw_count", C.c_uint8), ("pending_kan_dora_count", C.c_uint8),
                ("drawable_count", C.c_uint8), ("wall_seed", C.c_uint64), ("hand_index", C.c_uint64),
                ("players", PlayerView * NP),
                ("current_player", C.c_uint8), ("is_done", C.c_uint8), ("needs_tsumo", C.c_uint8),
                ("phase", C.c_uint8), ("active_mask", C.c_uint8),
                ("turn_count", C.c_uint32), ("riichi_sticks", C.c_uint32),
                ("last_discard_pid", C.c_int16), ("last_discard_tile", C.c_int16), ("pending_kan_pid", C.c_int16),
                ("pending_kan_action", C.c_uint64),
                ("oya", C.c_uint8), ("honba", C.c_uint8), ("kyoku_idx", C.c_uint8), ("round_wind", C.c_uint8),
                ("is_rinshan_flag", C.c_uint8), ("is_first_turn", C.c_uint8),
                ("riichi_pending_acceptance", C.c_int16), ("drawn_tile", C.c_int16), ("last_error_pid", C.c_int16)]


class Event(C.Structure):
    _fields_ = [("type", C.c_uint8), ("actor", C.c_uint8), ("target", C.c_uint8), ("tile", C.c_uint8),
                ("consumed", C.c_uint8 * 4), ("deltas", C.c_int32 * 4), ("flags", C.c_uint8), ("n_ura", C.c_uint8),
                ("ura", C.c_uint8 * 5), ("pad", C.c_uint8)]


# RMJ_EV_* (include/riichi_mi355x.h)
EV_NONE, EV_START_GAME, EV_START_KYOKU, EV_TSUMO, EV_DAHAI, EV_REACH, EV_REACH_ACCEPTED, EV_CHI, EV_PON, EV_DAIMINKAN, \
    EV_ANKAN, EV_KAKAN, EV_DORA, EV_HORA, EV_RYUKYOKU, EV_END_KYOKU, EV_END_GAME, EV_KITA, EV_TEHAI = range(19)
EVENT_SLOTS = 3  # records per game and call of rmj_apply_events (start_kyoku = START_KYOKU + 2 x TEHAI)
_HONORS = ["E", "S", "W", "N", "P", "F", "C"]


def mjai_to_tid(s: str, masked_ok: bool = False) -> int:
    """parser.rs:336-385 mjai_to_tid: one id per tile name (copy 0; plain 5 = copy 1, red 5 = copy 0).  The reference
    maps an unparsable string (e.g. the masked "?") to tile 0 (parse_mjai_tile, event_handler.rs:8-10); with
    masked_ok the same happens here (bot-side streams: the state of the masked seats is then garbage, as in the
    reference, and only the observing seat's outputs are meaningful), otherwise it raises."""
    if s in _HONORS:
        return 108 + _HONORS.index(s) * 4
    if s in ("5mr", "5pr", "5sr"):
        return {"5mr": 16, "5pr": 52, "5sr": 88}[s]
    if len(s) >= 2 and s[0].isdigit() and s[1] in "mpsz":
        num, suit = int(s[0]), s[1]
        if suit == "z":
            if 1 <= num <= 7:
                return 108 + (num - 1) * 4
        else:
            si = "mps".index(suit)
            if num == 0:
                return si * 36 + 16
            if 1 <= num <= 9:
                base = si * 36 + (num - 1) * 4
                return base + 1 if num == 5 else base
    if masked_ok:
        return 0
    raise ValueError(f"cannot map MJAI tile {s!r} (pass masked_ok=True to ingest masked streams like the reference)")


def event_records_from_mjai(ev: dict, num_players: int = 4, masked_ok: bool = False):
    """MJAI event dict (replay/mjai_replay.rs MjaiEvent) -> up to EVENT_SLOTS binary records for rmj_apply_events /
    the oracle.  Unknown event types map to a NONE record (MjaiEvent::Other: no state change)."""
    recs = (Event * EVENT_SLOTS)()
    ty = ev.get("type")
    e = recs[0]
    actor = int(ev.get("actor", 0) or 0)
    simple = {"start_game": EV_START_GAME, "reach": EV_REACH, "reach_accepted": EV_REACH_ACCEPTED, "hora": EV_HORA,
              "ryukyoku": EV_RYUKYOKU, "end_kyoku": EV_END_KYOKU, "end_game": EV_END_GAME, "kita": EV_KITA}
    if ty in simple:
        e.type, e.actor = simple[ty], actor
    elif ty == "start_kyoku":
        e.type = EV_START_KYOKU
        e.actor = int(ev["oya"])
        e.target = int(ev["kyoku"])
        e.tile = mjai_to_tid(ev["dora_marker"], masked_ok)
        kyotaku = int(ev.get("kyoutaku", ev.get("kyotaku", 0)))
        e.consumed[0] = "ESWN".index(ev["bakaze"]) if ev["bakaze"] in "ESWN" else 0
        e.consumed[1] = int(ev["honba"])
        e.consumed[2], e.consumed[3] = kyotaku & 0xFF, (kyotaku >> 8) & 0xFF
        for i, sc in enumerate(ev["scores"][:4]):
            e.deltas[i] = int(sc)
        tehais = ev["tehais"]
        for half in range(2):
            t = recs[1 + half]
            t.type, t.actor = EV_TEHAI, half
            payload = []
            for q in range(2):
                seat = 2 * half + q
                hand = [mjai_to_tid(x, masked_ok) for x in tehais[seat]] if seat < min(num_players, len(tehais)) else [0] * 13
                if len(hand) != 13:
                    raise ValueError("start_kyoku: every tehai must hold 13 tiles")
                payload += hand
            C.memmove(C.addressof(t) + 4, bytes(payload), 26)
    elif ty in ("tsumo", "dahai", "kakan"):
        e.type = {"tsumo": EV_TSUMO, "dahai": EV_DAHAI, "kakan": EV_KAKAN}[ty]
        e.actor, e.tile = actor, mjai_to_tid(ev["pai"], masked_ok)
        if ty == "dahai":
            e.flags = 1 if ev.get("tsumogiri") else 0
    elif ty in ("pon", "chi", "daiminkan", "kan", "ankan"):
        e.type = {"pon": EV_PON, "chi": EV_CHI, "daiminkan": EV_DAIMINKAN, "kan": EV_DAIMINKAN, "ankan": EV_ANKAN}[ty]
        e.actor = actor
        e.target = int(ev.get("target", 0) or 0)
        if ty != "ankan":
            e.tile = mjai_to_tid(ev["pai"], masked_ok)
        cons = [mjai_to_tid(x, masked_ok) for x in ev["consumed"]][:4]
        for i, c in enumerate(cons):
            e.consumed[i] = c
        e.flags = (len(cons) << 4) & 0xFF
    elif ty == "dora":
        e.type, e.tile = EV_DORA, mjai_to_tid(ev["dora_marker"], masked_ok)
    else:
        e.type = EV_NONE
    return recs


class HandCase(C.Structure):
    _fields_ = [("n_tiles", C.c_uint8), ("tiles", C.c_uint8 * 14), ("n_melds", C.c_uint8), ("melds", MeldView * 4),
                ("win_tile", C.c_uint8), ("n_dora", C.c_uint8), ("dora", C.c_uint8 * 5), ("n_ura", C.c_uint8),
                ("ura", C.c_uint8 * 5),
                ("tsumo", C.c_uint8), ("riichi", C.c_uint8), ("double_riichi", C.c_uint8), ("ippatsu", C.c_uint8),
                ("haitei", C.c_uint8), ("houtei", C.c_uint8), ("rinshan", C.c_uint8), ("chankan", C.c_uint8),
                ("tsumo_first_turn", C.c_uint8), ("player_wind", C.c_uint8), ("round_wind", C.c_uint8),
                ("kita_count", C.c_uint8), ("is_sanma", C.c_uint8), ("honba", C.c_uint32)]


class HandResult(C.Structure):
    _fields_ = [("is_win", C.c_uint8), ("yakuman", C.c_uint8), ("has_win_shape", C.c_uint8), ("n_yaku", C.c_uint8),
                ("yaku", C.c_uint8 * 20), ("han", C.c_uint32), ("fu", C.c_uint32), ("ron_agari", C.c_uint32),
                ("tsumo_agari_oya", C.c_uint32), ("tsumo_agari_ko", C.c_uint32), ("waits", C.c_uint64),
                ("is_tenpai", C.c_uint8), ("is_agari", C.c_uint8), ("pad", C.c_uint8 * 6)]


class WinResult(C.Structure):
    _fields_ = [("is_win", C.c_uint8), ("yakuman", C.c_uint8), ("has_win_shape", C.c_uint8), ("n_yaku", C.c_uint8),
                ("yaku", C.c_uint8 * 20), ("han", C.c_uint32), ("fu", C.c_uint32), ("ron_agari", C.c_uint32),
                ("tsumo_agari_oya", C.c_uint32), ("tsumo_agari_ko", C.c_uint32), ("pao_payer", C.c_int8), ("pad", C.c_uint8 * 3)]


class EventViews(C.Structure):   # RmjEventViews
    _fields_ = [("n_games", C.c_uint32), ("ring", C.c_uint32), ("events", C.c_void_p), ("ev_count", C.c_void_p),
                ("ev_count_stride", C.c_uint32), ("reserved", C.c_uint32), ("lost", C.c_void_p), ("ev_base", C.c_void_p)]


class TextView(C.Structure):     # RmjTextView (rmj_drain_text / rmj_format_events_device)
    _fields_ = [("text", C.c_void_p), ("text_offsets", C.c_void_p), ("bytes", C.c_uint64), ("n_games", C.c_uint32), ("n_events", C.c_uint32),
                ("ms", C.c_double * 3)]


TEXT_ON_DEVICE = 2   # RMJ_TEXT_ON_DEVICE: the view's pointers are device pointers (with DRAIN_PEEK = 1)


class Config(C.Structure):
    _fields_ = [("n_games", C.c_uint32), ("game_mode", C.c_uint8), ("skip_mjai_logging", C.c_uint8),
                ("round_wind", C.c_uint8), ("reserved0", C.c_uint8), ("rule_bits", C.c_uint32),
                ("device", C.c_int32), ("base_seed", C.c_uint64), ("game_offset", C.c_uint64),
                ("seeds", C.POINTER(C.c_uint64)), ("event_ring", C.c_uint32), ("reserved1", C.c_uint32)]


class SeqBuffers(C.Structure):
    _fields_ = [("sparse", C.c_void_p), ("n_sparse", C.c_void_p), ("numeric", C.c_void_p), ("progression", C.c_void_p),
                ("n_progression", C.c_void_p), ("candidates", C.c_void_p), ("n_candidates", C.c_void_p)]


SeqDeltaBuffers = SeqBuffers   # RmjSeqDeltaBuffers: the same fields (the arrays behind progression / n_progression are per seat)

SEQ_SPARSE, SEQ_PROG, SEQ_CAND, SEQ_DELTA_PROG = 25, 256, 64, 64

# feature sets of the observation batches (RMJ_FEATURES_*, rmj_encode_batch_device)
FEATURES_BASE = 0              # Observation.encode(): 74 x W
FEATURES_DISCARD_SHANTEN = 1   # riichienv-ml feat_v2: encode() + decay (4) + shanten efficiency (16, broadcast); 94 x 34, 4P only
FEATURES_EXTENDED = 2          # Observation.encode_extended(): 215 x W
FEATURES = {"base": FEATURES_BASE, "discard_shanten": FEATURES_DISCARD_SHANTEN, "extended": FEATURES_EXTENDED}
FEATURE_CHANNELS = {FEATURES_BASE: 74, FEATURES_DISCARD_SHANTEN: 94, FEATURES_EXTENDED: 215}


class ObsBatch(C.Structure):   # RmjObsBatch
    _fields_ = [("features", C.c_int32), ("compact", C.c_int32), ("row_stride", C.c_uint32), ("capacity", C.c_uint32),
                ("out", C.c_void_p), ("index", C.c_void_p), ("count", C.c_void_p)]


class DeviceViews(C.Structure):   # RmjDeviceViews
    _fields_ = [("n_games", C.c_uint32), ("reserved", C.c_uint32), ("status", C.c_void_p), ("nlegal", C.c_void_p),
                ("legal", C.c_void_p), ("mask", C.c_void_p), ("waits", C.c_void_p), ("stream", C.c_void_p)]


class PpoConfig(C.Structure):   # RmjPpoConfig
    _fields_ = [("features", C.c_int32), ("capacity", C.c_uint32), ("gamma", C.c_double), ("gae_lambda", C.c_double)]


class PpoBatch(C.Structure):    # RmjPpoBatch (rmj_ppo_emit_device)
    _fields_ = [("features", C.c_void_p), ("mask", C.c_void_p), ("action", C.c_void_p), ("log_prob", C.c_void_p), ("advantage", C.c_void_p),
                ("ret", C.c_void_p), ("count", C.c_void_p), ("rows", C.c_uint32), ("reserved", C.c_uint32)]


class PpoViews(C.Structure):    # RmjPpoViews
    _fields_ = [("capacity", C.c_uint32), ("row_stride", C.c_uint32), ("action_space", C.c_uint32), ("reserved", C.c_uint32)] + [
        (k, C.c_void_p) for k in ("features", "mask", "action", "value", "log_prob", "advantage", "ret", "valid", "game", "t", "prev", "seg_len",
                                  "serial", "seg_reward", "counters", "open_len")]


class PpoCounts(C.Structure):   # RmjPpoCounts
    _fields_ = [(k, C.c_uint32) for k in ("fill", "valid", "dropped", "overflowed", "segments", "open")]


class LogsetInfo(C.Structure):       # RmjLogsetInfo
    _fields_ = [(k, C.c_uint32) for k in ("n_logs", "n_events", "n_kyokus", "longest_log")]


class LogsetViews(C.Structure):      # RmjLogsetViews: device pointers (the tables and per-log results are NULL unless the set was parsed from text)
    _fields_ = [(k, C.c_void_p) for k in ("events", "offsets", "kyoku_offsets", "start_scores", "end_scores", "status", "error_line", "decisions")]


# RMJ_LOGTEXT_*: per-line / per-log parse statuses and the flags of rmj_logset_create_from_text
LOGTEXT_OK, LOGTEXT_UNSUPPORTED, LOGTEXT_ERR_JSON, LOGTEXT_ERR_KEY, LOGTEXT_ERR_TEHAI, LOGTEXT_ERR_TILE, LOGTEXT_ERR_VALUE, LOGTEXT_ERR_REPLAY = range(8)
LOGTEXT_STATUS_NAMES = ["OK", "UNSUPPORTED", "ERR_JSON", "ERR_KEY", "ERR_TEHAI", "ERR_TILE", "ERR_VALUE", "ERR_REPLAY"]
LOGTEXT_ON_DEVICE, LOGTEXT_MASKED_OK = 1, 2

LOGREPLAY_INCLUDE_PASS, LOGREPLAY_SKIP_SINGLE_ACTION, LOGREPLAY_HIDDEN, LOGREPLAY_DANGER, LOGREPLAY_DTABLE = 1, 2, 4, 8, 16   # RMJ_LOGREPLAY_*
HIDDEN_PRESENT, HIDDEN_TENPAI, HIDDEN_RIICHI, HIDDEN_FURITEN, HIDDEN_MELDS_SHIFT = 1, 2, 4, 8, 4   # RMJ_HIDDEN_*: the bits of opp_flags


class HiddenOut(C.Structure):        # RmjHiddenOut (rmj_hidden_targets_device)
    _fields_ = [(k, C.c_void_p) for k in ("opp_hand", "opp_shanten", "opp_waits", "opp_flags")]


DANGER_URA, DANGER_KINDS = 1, 37   # RMJ_DANGER_*: the flag of rmj_danger_targets*, the tile kinds of a row (34 types + the three copy-0 fives)


class DangerOut(C.Structure):        # RmjDangerOut (rmj_danger_targets_device)
    _fields_ = [("danger", C.c_void_p)]


DTAB_NONE, DTAB_COLS = 127, 35     # RMJ_DTAB_*: the shanten of an absent column, the columns of a row (34 discards + the hand itself)


class DiscardTableOut(C.Structure):  # RmjDiscardTableOut (rmj_discard_table_device); mask may be NULL
    _fields_ = [(k, C.c_void_p) for k in ("shanten", "accept", "ukeire", "mask")]


# The row targets (index[k] = game * 4 + seat -> fixed-shape rows): the out-struct of the C entries and, in the struct's order, every
# field's name, numpy dtype, shape behind the row axis and the value of a row the call leaves alone.  torch has no arithmetic on uint64:
# there a uint64 field is int64 (torch_dtype).  The one place that states these shapes: VecRiichiEnv, TorchVecEnv, LogSampleBuilder and
# the benchmarks of the targets allocate from it.
RowField = collections.namedtuple("RowField", "name dtype shape fill")
RowTarget = collections.namedtuple("RowTarget", "struct fields")
ROW_TARGETS = {
    "hidden": RowTarget(HiddenOut, (RowField("opp_hand", "uint8", (3, 34), 0), RowField("opp_shanten", "int8", (3,), 0),
                                    RowField("opp_waits", "int64", (3,), 0), RowField("opp_flags", "uint8", (3,), 0))),
    "danger": RowTarget(DangerOut, (RowField("danger", "int32", (3, DANGER_KINDS), 0),)),
    "discard_table": RowTarget(DiscardTableOut, (RowField("shanten", "int8", (DTAB_COLS,), DTAB_NONE), RowField("accept", "uint8", (DTAB_COLS,), 0),
                                                 RowField("ukeire", "uint8", (DTAB_COLS,), 0), RowField("mask", "uint64", (DTAB_COLS,), 0))),
}


def torch_dtype(torch, name):
    """the torch dtype of a RowField's numpy dtype name"""
    return getattr(torch, "int64" if name == "uint64" else name)


def row_arrays(target, k):
    """{field: numpy array [k, ...]} of a row target, every row as a call leaves an absent one"""
    import numpy as np

    return {f.name: np.full((k,) + f.shape, f.fill, f.dtype) for f in ROW_TARGETS[target].fields}


def row_struct(target, arrays):
    """the out-struct of a row target over {field: numpy array or torch tensor}"""
    t = ROW_TARGETS[target]
    return t.struct(*(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data for a in (arrays[f.name] for f in t.fields)))


DET_OK, DET_NOT_ACTING, DET_CHANKAN, DET_DUPLICATE, DET_RIICHI_NOTEN = 0, 1, 2, 3, 16   # RMJ_DET_*: determinize status (RIICHI_NOTEN << r, r = 0, 1, 2)
DET_SWAPPED = 128            # RMJ_DET_SWAPPED: the tenpai repair exchanged at least one tile in the row's world
DETF_RIICHI_TENPAI = 1       # RMJ_DETF_RIICHI_TENPAI (rmj_determinize_ex*)


class Determinize(C.Structure):      # RmjDeterminize (rmj_determinize_device)
    _fields_ = [("seed", C.c_uint64), ("hold", C.c_void_p), ("status", C.c_void_p)]


class LogReplayConfig(C.Structure):  # RmjLogReplayConfig
    _fields_ = [("features", C.c_int32), ("capacity", C.c_uint32), ("flags", C.c_uint32), ("n_powers", C.c_uint32), ("gamma", C.c_double),
                ("gamma_powers", C.c_void_p)]


class LogBatch(C.Structure):         # RmjLogBatch (rmj_logreplay_emit_device)
    _fields_ = [(k, C.c_void_p) for k in ("features", "mask", "action", "packed", "ret", "ret64", "rank", "log", "kyoku", "seat", "t", "count")] + [
        ("rows", C.c_uint32), ("reserved", C.c_uint32)]


class LogReplayViews(C.Structure):   # RmjLogReplayViews
    _fields_ = [(k, C.c_uint32) for k in ("capacity", "row_stride", "action_space", "steps")] + [
        (k, C.c_void_p) for k in ("features", "mask", "action", "packed", "ret", "ret64", "rank", "log", "kyoku", "seat", "t", "log_status", "traj_len",
                                  "traj_broken", "counters")]


class LogHiddenBatch(C.Structure):   # RmjLogHiddenBatch (rmj_logreplay_emit_hidden_device)
    _fields_ = [(k, C.c_void_p) for k in ("opp_hand", "opp_shanten", "opp_waits", "opp_flags", "event")] + [("rows", C.c_uint32), ("reserved", C.c_uint32)]


class LogHiddenViews(C.Structure):   # RmjLogHiddenViews
    _fields_ = [("capacity", C.c_uint32), ("record_bytes", C.c_uint32), ("records", C.c_void_p)]


class LogDangerBatch(C.Structure):   # RmjLogDangerBatch (rmj_logreplay_emit_danger_device)
    _fields_ = [("danger", C.c_void_p), ("rows", C.c_uint32), ("reserved", C.c_uint32)]


class LogDtableBatch(C.Structure):   # RmjLogDtableBatch (rmj_logreplay_emit_dtable_device)
    _fields_ = [(k, C.c_void_p) for k in ("shanten", "accept", "ukeire")] + [("rows", C.c_uint32), ("reserved", C.c_uint32)]


class LogReplayCounts(C.Structure):  # RmjLogReplayCounts
    _fields_ = [(k, C.c_uint32) for k in ("fill", "overflowed", "failed_logs", "complete_logs", "decisions", "events", "steps_done", "steps_left")]


# RMJ_LOGCHECK_*: the verdict codes of rmj_logcheck_* (LogSet.validate), their counters' words, the create flag and its guard words
LOGCHECK_NAMES = ["OK", "PARSE", "NO_START_KYOKU", "AFTER_END", "UNFINISHED", "ACTOR", "DRAW_OUT_OF_TURN", "NOT_OFFERED", "TILE_NOT_HELD", "TILE_COUNT",
                  "NO_LEGAL_MATCH", "SCORE_CONTINUITY", "SCORE_CONSERVATION"]
LOGCHECK_OK, LOGCHECK_PARSE, LOGCHECK_NO_START_KYOKU, LOGCHECK_AFTER_END, LOGCHECK_UNFINISHED, LOGCHECK_ACTOR, LOGCHECK_DRAW_OUT_OF_TURN, LOGCHECK_NOT_OFFERED, \
    LOGCHECK_TILE_NOT_HELD, LOGCHECK_TILE_COUNT, LOGCHECK_NO_LEGAL_MATCH, LOGCHECK_SCORE_CONTINUITY, LOGCHECK_SCORE_CONSERVATION = range(13)
LOGCHECK_COUNTERS, LOGCHECK_GUARDS, LOGCHECK_GUARD_WORDS, LOGCHECK_GUARD_WORD = 16, 1, 64, 0xA5C3F00D


class LogCheckViews(C.Structure):    # RmjLogCheckViews: device pointers to the verdicts
    _fields_ = [("n_logs", C.c_uint32), ("steps", C.c_uint32)] + [(k, C.c_void_p) for k in ("code", "seat", "kyoku", "event", "detail", "counts")]


class GrpOut(C.Structure):           # RmjGrpOut (rmj_logset_grp_device): device pointers, any may be NULL (x needs meta)
    _fields_ = [(k, C.c_void_p) for k in ("meta", "x", "rank", "log_of")]


# RMJ_PLAYSTAT_*: the columns of rmj_logset_playstats_device's rows [n_kyokus][4][PLAYSTAT_COLUMNS] int32
PLAYSTAT_NAMES = ["WIN", "WIN_TSUMO", "DEAL_IN", "RIICHI", "RIICHI_ACCEPTED", "RIICHI_TURN", "CALLS", "CHI", "PON", "KANS", "KITA", "DISCARDS",
                  "TSUMOGIRI", "WIN_TURN", "DEALER", "END"]
PLAYSTAT_COLUMNS = len(PLAYSTAT_NAMES)
PLAYSTAT_WIN, PLAYSTAT_WIN_TSUMO, PLAYSTAT_DEAL_IN, PLAYSTAT_RIICHI, PLAYSTAT_RIICHI_ACCEPTED, PLAYSTAT_RIICHI_TURN, PLAYSTAT_CALLS, PLAYSTAT_CHI, \
    PLAYSTAT_PON, PLAYSTAT_KANS, PLAYSTAT_KITA, PLAYSTAT_DISCARDS, PLAYSTAT_TSUMOGIRI, PLAYSTAT_WIN_TURN, PLAYSTAT_DEALER, PLAYSTAT_END = range(16)
PLAYSTAT_END_HORA, PLAYSTAT_END_RYUKYOKU = 1, 2   # the bits of the END column


class BenchResult(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("step_kernel_ms", C.c_double), ("env_steps", C.c_uint64),
                ("launches", C.c_uint32), ("launches_in_flight", C.c_uint32), ("full_path_steps", C.c_uint64),
                ("queued", C.c_uint32), ("reserved", C.c_uint32)]


# "RmjX" -> the class that mirrors the header's struct RmjX: every Structure of this module, under the name it has here
STRUCTS = {"Rmj" + k: v for k, v in list(globals().items()) if isinstance(v, type) and issubclass(v, C.Structure)}

# Every function the two headers declare, in the headers' order: (name, argtypes[, restype when it is not int]).  Handles and
# raw buffers are c_void_p.  Return codes stay plain ints: vecenv._chk is the one place that raises.
P, vp, cint, u32, u64, f64 = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
PROTOTYPES = [
    # ======== include/riichi_mi355x.h
    # ---- lifecycle
    ("rmj_version", [], C.c_char_p),
    ("rmj_last_error", [], C.c_char_p),
    ("rmj_device_count", []),
    ("rmj_create", [P(Config), P(vp)]),
    ("rmj_destroy", [vp]),
    ("rmj_reset", [vp] * 8),
    ("rmj_clone", [vp, P(vp)]),
    ("rmj_copy_games", [vp, vp, vp, vp, u32]),
    ("rmj_copy_games_device", [vp, vp, vp, vp, u32]),
    ("rmj_step", [vp, vp]),
    ("rmj_step_device", [vp, vp]),
    ("rmj_step_random", [vp, u64, u32, cint]),
    ("rmj_step_greedy", [vp, u64, u32, cint, u32]),
    ("rmj_random_actions", [vp, u64, vp]),
    ("rmj_random_actions_device", [vp, u64, vp]),
    # ---- observations
    ("rmj_get_status", [vp, vp, vp, vp]),
    ("rmj_get_legal", [vp, vp, vp]),
    ("rmj_get_legal_compact", [vp, vp, vp, vp, u32, u32, P(u32), P(u32)]),
    ("rmj_get_mask", [vp, vp]),
    ("rmj_get_waits", [vp, vp]),
    ("rmj_get_scores", [vp, vp]),
    ("rmj_get_ranks", [vp, vp]),
    ("rmj_get_step_counts", [vp, vp]),
    ("rmj_total_steps", [vp, P(u64)]),
    ("rmj_get_wall_digest", [vp, u32, C.c_char_p, C.c_char_p]),
    ("rmj_get_wall_digests", [vp, u32, u32, vp, vp]),
    ("rmj_peek_state", [vp, u32, P(StateView)]),
    ("rmj_peek_outputs", [vp, u32, vp, vp, vp, vp, P(u32)]),
    ("rmj_poke_state", [vp, u32, P(StateView)]),
    ("rmj_get_win_results", [vp, u32, P(WinResult), P(C.c_uint8)]),
    ("rmj_get_event_counts", [vp, vp]),
    ("rmj_get_events", [vp, u32, u32, u32, P(Event), P(u32)]),
    ("rmj_format_event", [P(Event), u32, cint, C.c_char_p, u32]),
    ("rmj_get_log_positions", [vp, vp, vp]),
    ("rmj_drain_events", [vp, vp, vp, u32, vp, P(u32), u32]),
    ("rmj_format_events", [vp, vp, u32, cint, vp, u64, vp, P(u64)]),
    ("rmj_drain_format", [vp, vp, cint, vp, u64, vp, P(u64), P(u32), vp, u32]),
    ("rmj_event_views", [vp, P(EventViews)]),
    ("rmj_get_events_lost", [vp, vp]),
    ("rmj_drain_text", [vp, vp, cint, u32, P(TextView)]),
    ("rmj_format_events_device", [vp, vp, vp, u32, cint, u32, P(TextView)]),
    # ---- batched hand math (kernel gate)
    ("rmj_eval_hands", [cint, P(HandCase), u32, P(HandResult)]),
    ("rmj_agari_counts", [cint, vp, u32, vp, vp, vp]),
    ("rmj_calculate_score", [cint] + [vp] * 6 + [u32, vp]),
    ("rmj_encode", [vp, cint, vp]),
    ("rmj_set_encode_row_stride", [vp, u32]),
    ("rmj_encode_device", [vp, cint, vp]),
    ("rmj_step_random_encode", [vp, u64, u32, cint, cint, vp]),
    ("rmj_encode_compact_device", [vp, vp, vp, u32, vp]),
    ("rmj_step_random_encode_compact", [vp, u64, u32, cint, vp, vp, u32, vp]),
    ("rmj_encode_extended", [vp, cint, vp]),
    ("rmj_encode_extended_device", [vp, cint, vp]),
    ("rmj_encode_batch_device", [vp, P(ObsBatch)]),
    ("rmj_encode_batch", [vp, P(ObsBatch)]),
    ("rmj_step_ids_encode_batch_device", [vp, vp, cint, P(ObsBatch)]),
    ("rmj_step_sample_encode_batch_device", [vp, vp, u32, u64, cint, vp, P(ObsBatch)]),
    ("rmj_hidden_targets_device", [vp, vp, u32, vp, P(HiddenOut)]),
    ("rmj_hidden_targets", [vp, vp, u32, P(HiddenOut)]),
    ("rmj_danger_targets_device", [vp, vp, u32, vp, u32, P(DangerOut)]),
    ("rmj_danger_targets", [vp, vp, u32, u32, P(DangerOut)]),
    ("rmj_discard_table_device", [vp, vp, u32, vp, u32, P(DiscardTableOut)]),
    ("rmj_discard_table", [vp, vp, u32, u32, P(DiscardTableOut)]),
    ("rmj_discard_table_hands", [cint, vp, vp, u32, cint, P(DiscardTableOut)]),
    ("rmj_determinize_device", [vp, vp, u32, vp, P(Determinize)]),
    ("rmj_determinize", [vp, vp, u32, P(Determinize)]),
    ("rmj_determinize_order", [u64, u64, u32, u32, vp]),
    ("rmj_determinize_ex_device", [vp, vp, u32, vp, P(Determinize), u32]),
    ("rmj_determinize_ex", [vp, vp, u32, P(Determinize), u32]),
    ("rmj_determinize_swap_key", [u64, u64, u32, u32, u32, u32, u32, vp]),
    ("rmj_shanten", [cint, vp, u32, cint, vp]),
    ("rmj_effective_tiles", [cint, vp, u32, cint, vp]),
    ("rmj_best_ukeire", [cint, vp, vp, u32, cint, vp]),
    # ---- trainer-side device interface
    ("rmj_device_views", [vp, P(DeviceViews)]),
    ("rmj_step_ids_device", [vp, vp, cint]),
    ("rmj_step_ids_encode_device", [vp, vp, cint, vp]),
    ("rmj_step_sample_encode_device", [vp, vp, u32, u64, cint, vp, vp]),
    ("rmj_sample_ids_device", [vp, vp, u32, u64, vp]),
    ("rmj_select_ids_device", [vp, vp, u32, u64, vp, vp]),
    # ---- PPO transition collector
    ("rmj_ppo_create", [vp, P(PpoConfig), P(vp)]),
    ("rmj_ppo_destroy", [vp]),
    ("rmj_ppo_record_device", [vp, P(ObsBatch), vp, vp, vp, u32, vp]),
    ("rmj_ppo_close_device", [vp, vp, vp]),
    ("rmj_ppo_emit_device", [vp, P(PpoBatch)]),
    ("rmj_ppo_views", [vp, P(PpoViews)]),
    ("rmj_ppo_counts", [vp, P(PpoCounts)]),
    ("rmj_ppo_clear", [vp]),
    # ---- log sample builder
    ("rmj_logset_create", [cint, vp, vp, u32, P(vp)]),
    ("rmj_logset_destroy", [vp]),
    ("rmj_logset_info", [vp, P(LogsetInfo), vp]),
    ("rmj_logset_create_from_text", [cint, vp, vp, u32, u32, u32, P(vp)]),
    ("rmj_logset_views", [vp, P(LogsetViews)]),
    ("rmj_logset_status", [vp, vp, vp, vp, vp]),
    ("rmj_grp_rows_device", [cint, vp, vp, vp, u32, u32, vp, vp]),
    ("rmj_logset_grp_device", [vp, u32, vp, vp, P(GrpOut), vp]),
    ("rmj_logset_playstats_device", [vp, u32, vp, vp]),
    ("rmj_logreplay_assign", [vp, u32, u32, vp, vp, vp, P(u32)]),
    ("rmj_logreplay_create", [vp, vp, P(LogReplayConfig), P(vp)]),
    ("rmj_logreplay_destroy", [vp]),
    ("rmj_logreplay_run_device", [vp, u32, P(u32)]),
    ("rmj_logreplay_finalize_device", [vp, vp, vp]),
    ("rmj_logreplay_emit_device", [vp, P(LogBatch)]),
    ("rmj_logreplay_views", [vp, P(LogReplayViews)]),
    ("rmj_logreplay_counts", [vp, P(LogReplayCounts)]),
    ("rmj_logreplay_clear", [vp]),
    ("rmj_logreplay_emit_hidden_device", [vp, P(LogHiddenBatch)]),
    ("rmj_logreplay_hidden_views", [vp, P(LogHiddenViews)]),
    ("rmj_logreplay_emit_danger_device", [vp, P(LogDangerBatch)]),
    ("rmj_logreplay_emit_dtable_device", [vp, P(LogDtableBatch)]),
    # ---- log validation
    ("rmj_logcheck_name", [u32], C.c_char_p),
    ("rmj_logcheck_create", [vp, vp, u32, u32, P(vp)]),
    ("rmj_logcheck_destroy", [vp]),
    ("rmj_logcheck_set_scores", [vp, vp, vp]),
    ("rmj_logcheck_run_device", [vp, u32, P(u32)]),
    ("rmj_logcheck_views", [vp, P(LogCheckViews)]),
    ("rmj_round_track_device", [vp, vp, vp, vp, vp]),
    ("rmj_round_track_reset", [vp]),
    ("rmj_scores_device", [vp, vp, vp]),
    ("rmj_points_device", [vp, cint, vp]),
    ("rmj_get_points", [vp, cint, vp]),
    ("rmj_sync", [vp]),
    ("rmj_set_stream", [vp, vp, cint]),
    # ---- MJAI event ingestion
    ("rmj_apply_events", [vp, vp]),
    ("rmj_encode_aux", [vp, cint, vp]),
    ("rmj_encode_aux_device", [vp, cint, vp]),
    ("rmj_encode_seq_delta", [vp, cint, P(SeqDeltaBuffers)]),
    ("rmj_encode_seq_delta_device", [vp, cint, P(SeqDeltaBuffers)]),
    ("rmj_encode_seq", [vp, cint, P(SeqBuffers)]),
    ("rmj_encode_seq_device", [vp, cint, P(SeqBuffers)]),
    # ---- scheduling
    ("rmj_set_rollout_streams", [vp, cint]),
    # ======== include/riichi_mi355x_bench.h
    ("rmj_bench_rollout", [vp, u64, u32, u32, P(BenchResult)]),
    ("rmj_time_rollout", [vp, u64, u32, P(BenchResult)]),
    ("rmj_time_rollout_encode", [vp, u64, u32, vp, P(BenchResult)]),
    ("rmj_time_rollout_greedy", [vp, u64, u32, u32, P(BenchResult)]),
    ("rmj_bench_rollout_validated", [vp, u64, u32, u32, P(BenchResult)]),
    ("rmj_bench_hand_kernel", [cint, cint, vp, vp, u32, cint, u32, P(f64)]),
    ("rmj_bench_encode", [vp, cint, cint, vp, u32, P(f64)]),
    ("rmj_bench_encode_compact", [vp, vp, vp, u32, vp, u32, P(f64)]),
    ("rmj_bench_device_alloc", [cint, u64, P(vp)]),
    ("rmj_bench_device_free", [cint, vp]),
    ("rmj_bench_device_sync", [cint]),
    ("rmj_total_full_path", [vp, P(u64)]),
]


class _CudaArray:
    """Minimal __cuda_array_interface__ carrier so that torch.as_tensor wraps library-owned device memory in place."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3,
                                         "strides": None}
        self._owner = owner   # keeps the owning object (and with it the allocation) alive


def device_tensor(torch, owner, device, ptr, shape, typestr):
    """A zero-copy torch tensor over library-owned device memory at `ptr`; the tensor keeps `owner` alive.  (torch is passed in: this
    module imports none; functools.partial over the first three arguments gives a view struct's wrapper.)"""
    return torch.as_tensor(_CudaArray(ptr, shape, typestr, owner), device=device)


def hand_case_from_fixture(case: dict) -> HandCase:
    """Build a HandCase from one entry of the reference's agari_*.json fixtures
    (riichienv-core/tests/agari_correctness.rs:29-84)."""
    hc = HandCase()
    tiles = case["tiles_136"]
    hc.n_tiles = len(tiles)
    for i, t in enumerate(tiles):
        hc.tiles[i] = t
    hc.n_melds = len(case["melds"])
    for i, m in enumerate(case["melds"]):
        mv = hc.melds[i]
        mv.meld_type = MELD_NAMES[m["meld_type"]]
        mv.n_tiles = len(m["tiles"])
        for j, t in enumerate(m["tiles"]):
            mv.tiles[j] = t
        mv.opened = 1 if m["opened"] else 0
        mv.from_who = m["from_who"]
        mv.called_tile = -1
    hc.win_tile = case["win_tile_136"]
    hc.n_dora = len(case["dora_indicators"])
    for i, t in enumerate(case["dora_indicators"]):
        hc.dora[i] = t
    hc.n_ura = len(case["ura_indicators"])
    for i, t in enumerate(case["ura_indicators"]):
        hc.ura[i] = t
    c = case["conditions"]
    for k in ("tsumo", "riichi", "double_riichi", "ippatsu", "haitei", "houtei", "rinshan", "chankan",
              "tsumo_first_turn"):
        setattr(hc, k, 1 if c[k] else 0)
    hc.player_wind = c["player_wind"]
    hc.round_wind = c["round_wind"]
    hc.honba = c["honba"]
    hc.kita_count = c.get("kita_count", 0)
    hc.is_sanma = 1 if c.get("is_sanma", False) else 0
    return hc
