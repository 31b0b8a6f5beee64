// One line of MJAI JSONL text -> its EVENT_SLOTS (3) event records, the inverse of rmj_evtext.h, as scalar functions that the host and the
// device share: the device parser of log text (k_lt_parse in rmj_logtext.hip.h: rmj_logset_create_from_text) and the host test that holds
// it to abi.event_records_from_mjai(json.loads(line), num_players, masked_ok) (riichienv_amd/abi.py), which stays the definition.
// Plain C++17 under g++; __host__ __device__ under hipcc.  No HIP intrinsics in this file.
//
//   parse_line(p, len, num_players, masked_ok, recs[3], &side) -> status
//
// reads [p, p + len) and nothing else.  recs receives the packer's three records (all zero = NONE on any status but OK); side receives
// what the per-kyoku score tables need (datasets.kyoku_tables: MjaiReplay.from_events): the event's class, its `scores` / `deltas`
// (alias `delta`), whether it is a decision type (datasets._DECISION_TYPES), the actor, and the status.
//
// Dialect.  One JSON object per line as json.loads reads it (strict: no control bytes in strings, \uXXXX and the eight short escapes,
// UTF-8 well-formed, NaN / Infinity / -Infinity accepted as numbers like Python does), keys in any order, whitespace (space, tab, \r, \n)
// wherever JSON allows it, unknown keys skipped whatever their value (nested containers to a depth of 64).
//
// A line ends in exactly one of three states - never silently different from the packer:
//   RMJ_LOGTEXT_OK           records bit-equal to the packer's;
//   RMJ_LOGTEXT_ERR_*        where json.loads or the packer raises: ERR_JSON (malformed text, top level not an object), ERR_KEY (a
//                            required key is missing), ERR_TEHAI (a tehai of a seat < min(num_players, len(tehais)) without 13 tiles),
//                            ERR_TILE (a tile name mjai_to_tid cannot map, without masked_ok), ERR_VALUE (null where a value is required);
//   RMJ_LOGTEXT_UNSUPPORTED  valid input this parser declines to interpret:
//                              * a backslash escape inside any key, or inside a string value it must interpret (type, tile names, bakaze);
//                              * a byte >= 0x80 inside a tile name or bakaze;
//                              * a value of another JSON kind than the field's (a string actor, a number pai, true as actor, a truthy
//                                tsumogiri that is not `true`, a type that is an array or an object, scores that are not an array);
//                              * a non-integer number (1.5, 1.0, 1e2) in a field it must interpret, or one out of range: outside 0..255
//                                for actor / target / oya / kyoku / honba, outside 0..65535 for kyotaku, outside int32 for scores / deltas;
//                              * a duplicate key of interest (type actor target pai consumed tsumogiri oya kyoku honba kyotaku kyoutaku
//                                bakaze dora_marker scores tehais deltas delta);
//                              * a bakaze that is not one of E S W N;
//                              * containers nested deeper than 64.
// Only the fields the event's type reads are judged: {"type":"hora","pai":5} is a plain hora.
//
// Semantics (event_records_from_mjai): actor / target missing, null or false read as 0; `kyoutaku` wins over `kyotaku`, both optional;
// `kan` is daiminkan; consumed: every name is mapped, the first 4 are kept, flags = n << 4; tsumogiri true -> 1, false / null / missing
// -> 0; scores cut to 4; tehais of seats >= min(num_players, len(tehais)) read as zeros and are not looked at; mjai_to_tid including its
// prefix rule ("1mX" is 1m) and masked_ok (unmappable -> 0); a missing or unknown type gives a NONE record; hora and ryukyoku records
// carry type and actor only.
#pragma once
#include <stdint.h>

#include "../../include/riichi_mi355x.h"

#if defined(__HIPCC__)
#define RMJP_FN __host__ __device__ inline
#else
#define RMJP_FN inline
#endif

namespace rmjp {

// event classes of the kyoku walk (MjaiReplay.from_events / Kyoku._feed)
enum : uint8_t { CLS_OTHER = 0, CLS_START_KYOKU, CLS_HORA, CLS_RYUKYOKU, CLS_REACH, CLS_REACH_ACCEPTED, CLS_END, CLS_DAHAI, CLS_CALL };
enum : uint8_t {
    SF_HAS_SCORES = 1,   // `scores` present and not null
    SF_HAS_DELTAS = 2,   // `deltas` (else `delta`) present and not null
    SF_DECISION = 4,     // the type is one of datasets._DECISION_TYPES
    SF_ACTOR_NONE = 8,   // actor missing or null (Kyoku._feed indexes its seat tables by it)
    SF_NO_TARGET = 16    // chi / pon / kan without `target` (Kyoku._feed reads ev["target"])
};
struct Side {            // 40 bytes
    int32_t scores[4];   // start_kyoku / hora / ryukyoku `scores`, the first n_scores (<= 4) entries
    int32_t deltas[4];
    uint8_t cls, flags;
    uint8_t n_scores;    // entries of `scores`, capped at 255 (start_kyoku: the seats of the kyoku)
    uint8_t n_deltas;    // entries of `deltas`, capped at 4
    uint8_t status;      // RMJ_LOGTEXT_*
    uint8_t actor;
    uint8_t pad[2];
};

struct Cur { const uint8_t* p; const uint8_t* e; };
struct StrInfo { uint64_t k0, k1; uint32_t len; bool esc, high; };   // the first 16 plain bytes, the character count, escapes / bytes >= 0x80 seen

constexpr uint64_t pk(const char* s, int from) {
    uint64_t v = 0;
    int n = 0;
    while (s[n]) n++;
    for (int i = 0; i < 8; i++)
        if (from + i < n) v |= (uint64_t)(uint8_t)s[from + i] << (8 * i);
    return v;
}
constexpr uint32_t sl(const char* s) {
    uint32_t n = 0;
    while (s[n]) n++;
    return n;
}
template <uint64_t A, uint64_t B, uint32_t L> RMJP_FN bool is_(const StrInfo& s) { return s.len == L && s.k0 == A && s.k1 == B; }
#define RMJP_IS(s, lit) (::rmjp::is_<::rmjp::pk(lit, 0), ::rmjp::pk(lit, 8), ::rmjp::sl(lit)>(s))

RMJP_FN int peek(const Cur& c) { return c.p < c.e ? (int)*c.p : -1; }
RMJP_FN void ws(Cur& c) {
    while (c.p < c.e && (*c.p == ' ' || *c.p == '\t' || *c.p == '\r' || *c.p == '\n')) c.p++;
}
RMJP_FN bool lit(Cur& c, const char* s, uint32_t n) {
    if ((uint64_t)(c.e - c.p) < n) return false;
    for (uint32_t i = 0; i < n; i++)
        if (c.p[i] != (uint8_t)s[i]) return false;
    c.p += n;
    return true;
}
#define RMJP_LIT(c, s) ::rmjp::lit(c, s, (uint32_t)sizeof(s) - 1u)

// the body of a string, the cursor behind its opening quote; false: not a JSON string (json.loads raises)
RMJP_FN bool scan_string(Cur& c, StrInfo& s) {
    s.k0 = s.k1 = 0;
    s.len = 0;
    s.esc = s.high = false;
    for (;;) {
        if (c.p >= c.e) return false;
        const uint32_t ch = *c.p++;
        if (ch == '"') return true;
        if (ch < 0x20u) return false;
        if (ch == '\\') {
            s.esc = true;
            if (c.p >= c.e) return false;
            const uint32_t x = *c.p++;
            if (x == 'u') {
                for (int i = 0; i < 4; i++) {
                    if (c.p >= c.e) return false;
                    const uint32_t h = *c.p++;
                    if (!((h >= '0' && h <= '9') || (h >= 'a' && h <= 'f') || (h >= 'A' && h <= 'F'))) return false;
                }
            } else if (!(x == '"' || x == '\\' || x == '/' || x == 'b' || x == 'f' || x == 'n' || x == 'r' || x == 't')) {
                return false;
            }
        } else if (ch >= 0x80u) {   // one well-formed UTF-8 sequence (a bytes line that does not decode never reaches the packer)
            s.high = true;
            int n;
            uint32_t lo = 0x80u, hi = 0xBFu;
            if (ch >= 0xC2u && ch <= 0xDFu) n = 1;
            else if (ch >= 0xE0u && ch <= 0xEFu) { n = 2; if (ch == 0xE0u) lo = 0xA0u; }   // ED A0..BF (surrogates) pass, as in json.loads of bytes
            else if (ch >= 0xF0u && ch <= 0xF4u) { n = 3; if (ch == 0xF0u) lo = 0x90u; if (ch == 0xF4u) hi = 0x8Fu; }
            else return false;
            for (int i = 0; i < n; i++) {
                if (c.p >= c.e) return false;
                const uint32_t b = *c.p++;
                if (b < lo || b > hi) return false;
                lo = 0x80u;
                hi = 0xBFu;
            }
        } else if (s.len < 8u) {
            s.k0 |= (uint64_t)ch << (8u * s.len);
        } else if (s.len < 16u) {
            s.k1 |= (uint64_t)ch << (8u * (s.len - 8u));
        }
        s.len++;
    }
}

// a JSON number (or Python's NaN / Infinity / -Infinity); is_int: the integer form, v its value saturated at +-2^40
RMJP_FN bool scan_number(Cur& c, bool& is_int, int64_t& v) {
    bool neg = false;
    is_int = false;
    v = 0;
    if (peek(c) == '-') { neg = true; c.p++; }
    int ch = peek(c);
    if (ch == 'I') return RMJP_LIT(c, "Infinity");
    if (ch == 'N') return !neg && RMJP_LIT(c, "NaN");
    int64_t mag = 0;
    if (ch == '0') {
        c.p++;
    } else if (ch >= '1' && ch <= '9') {
        while ((ch = peek(c)) >= '0' && ch <= '9') {
            if (mag < ((int64_t)1 << 40)) mag = mag * 10 + (ch - '0');
            c.p++;
        }
    } else {
        return false;
    }
    is_int = true;
    if (peek(c) == '.') {
        c.p++;
        if (!((ch = peek(c)) >= '0' && ch <= '9')) return false;
        while ((ch = peek(c)) >= '0' && ch <= '9') c.p++;
        is_int = false;
    }
    if ((ch = peek(c)) == 'e' || ch == 'E') {
        c.p++;
        if ((ch = peek(c)) == '+' || ch == '-') c.p++;
        if (!((ch = peek(c)) >= '0' && ch <= '9')) return false;
        while ((ch = peek(c)) >= '0' && ch <= '9') c.p++;
        is_int = false;
    }
    v = neg ? -mag : mag;
    return true;
}

enum : uint8_t { SK_OK = 0, SK_BAD = 1, SK_DEEP = 2 };
// any JSON value, validated and skipped (no recursion: a bit per open container, 1 = object)
RMJP_FN uint8_t skip_value(Cur& c) {
    uint64_t stack = 0;
    int depth = 0;
    StrInfo s;
    for (;;) {
        ws(c);
        const int ch = peek(c);
        bool closed = false;   // a value has just ended
        if (ch == '{' || ch == '[') {
            c.p++;
            if (depth >= 64) return SK_DEEP;
            stack = (stack << 1) | (ch == '{' ? 1u : 0u);
            depth++;
            ws(c);
            if (peek(c) == (ch == '{' ? '}' : ']')) {
                c.p++;
                stack >>= 1;
                depth--;
                closed = true;
            } else if (ch == '[') {
                continue;
            }
        } else if (ch == '"') {
            c.p++;
            if (!scan_string(c, s)) return SK_BAD;
            closed = true;
        } else if (ch == 't') {
            if (!RMJP_LIT(c, "true")) return SK_BAD;
            closed = true;
        } else if (ch == 'f') {
            if (!RMJP_LIT(c, "false")) return SK_BAD;
            closed = true;
        } else if (ch == 'n') {
            if (!RMJP_LIT(c, "null")) return SK_BAD;
            closed = true;
        } else {
            bool ii;
            int64_t v;
            if (!scan_number(c, ii, v)) return SK_BAD;
            closed = true;
        }
        for (;;) {
            if (closed) {
                if (depth == 0) return SK_OK;
                ws(c);
                const int d = peek(c);
                if (d < 0) return SK_BAD;
                c.p++;
                if (stack & 1u) {
                    if (d == '}') { stack >>= 1; depth--; continue; }
                    if (d != ',') return SK_BAD;
                } else {
                    if (d == ']') { stack >>= 1; depth--; continue; }
                    if (d != ',') return SK_BAD;
                    break;   // the next element
                }
            }
            // a key of an open object, then its value
            ws(c);
            if (peek(c) != '"') return SK_BAD;
            c.p++;
            if (!scan_string(c, s)) return SK_BAD;
            ws(c);
            if (peek(c) != ':') return SK_BAD;
            c.p++;
            break;
        }
    }
}

// ---------------------------------------------------------------- field values
// what a line holds under a key of interest, judged only when the event's type reads the field
enum : uint8_t { F_ABSENT = 0, F_OK, F_NULL, F_FALSE, F_BAD };   // F_BAD: st says why
struct IntF { int64_t v; uint8_t tag, st; };
struct TileF { uint8_t tag, st, tid; };
struct IntsF { int32_t v[4]; uint8_t tag, st, n; };
struct TilesF { uint8_t t[4]; uint8_t tag, st, n; };

// value readers return 0, or RMJ_LOGTEXT_ERR_JSON / RMJ_LOGTEXT_UNSUPPORTED (nesting) for the whole line
RMJP_FN uint8_t skip_st(Cur& c) {
    const uint8_t r = skip_value(c);
    return r == SK_OK ? (uint8_t)RMJ_LOGTEXT_OK : r == SK_DEEP ? (uint8_t)RMJ_LOGTEXT_UNSUPPORTED : (uint8_t)RMJ_LOGTEXT_ERR_JSON;
}
RMJP_FN uint8_t read_int(Cur& c, IntF& f) {
    const int ch = peek(c);
    f.v = 0;
    f.st = RMJ_LOGTEXT_UNSUPPORTED;
    if (ch == '-' || (ch >= '0' && ch <= '9')) {
        bool ii;
        if (!scan_number(c, ii, f.v)) return RMJ_LOGTEXT_ERR_JSON;
        f.tag = ii ? F_OK : F_BAD;
        return 0;
    }
    if (ch == 'n') {
        f.tag = F_NULL;
        return RMJP_LIT(c, "null") ? 0 : RMJ_LOGTEXT_ERR_JSON;
    }
    if (ch == 'f') {
        f.tag = F_FALSE;
        return RMJP_LIT(c, "false") ? 0 : RMJ_LOGTEXT_ERR_JSON;
    }
    f.tag = F_BAD;
    return skip_st(c);
}
// mjai_to_tid of a string (abi.py)
RMJP_FN uint8_t tile_of(const StrInfo& s, bool masked_ok, uint8_t& tid) {
    tid = 0;
    if (s.esc || s.high) return RMJ_LOGTEXT_UNSUPPORTED;
    const uint32_t c0 = (uint32_t)(s.k0 & 0xFFu), c1 = (uint32_t)((s.k0 >> 8) & 0xFFu), c2 = (uint32_t)((s.k0 >> 16) & 0xFFu);
    const int suit = c1 == 'm' ? 0 : c1 == 'p' ? 1 : c1 == 's' ? 2 : -1;
    if (s.len == 1u) {
        const int h = c0 == 'E' ? 0 : c0 == 'S' ? 1 : c0 == 'W' ? 2 : c0 == 'N' ? 3 : c0 == 'P' ? 4 : c0 == 'F' ? 5 : c0 == 'C' ? 6 : -1;
        if (h >= 0) { tid = (uint8_t)(108 + 4 * h); return 0; }
    }
    if (s.len == 3u && c0 == '5' && c2 == 'r' && suit >= 0) { tid = (uint8_t)(suit * 36 + 16); return 0; }
    if (s.len >= 2u && c0 >= '0' && c0 <= '9') {
        const int num = (int)c0 - '0';
        if (c1 == 'z') {
            if (num >= 1 && num <= 7) { tid = (uint8_t)(108 + (num - 1) * 4); return 0; }
        } else if (suit >= 0) {
            if (num == 0) { tid = (uint8_t)(suit * 36 + 16); return 0; }
            tid = (uint8_t)(suit * 36 + (num - 1) * 4 + (num == 5 ? 1 : 0));
            return 0;
        }
    }
    return masked_ok ? (uint8_t)0 : (uint8_t)RMJ_LOGTEXT_ERR_TILE;
}
RMJP_FN uint8_t read_tile(Cur& c, bool masked_ok, uint8_t& st, uint8_t& tid) {
    tid = 0;
    if (peek(c) != '"') {
        st = RMJ_LOGTEXT_UNSUPPORTED;
        return skip_st(c);
    }
    c.p++;
    StrInfo s;
    if (!scan_string(c, s)) return RMJ_LOGTEXT_ERR_JSON;
    st = tile_of(s, masked_ok, tid);
    return 0;
}
RMJP_FN void set4(int32_t* a, uint32_t i, int32_t v) {
    for (uint32_t k = 0; k < 4; k++)
        if (k == i) a[k] = v;
}
RMJP_FN void set4(uint8_t* a, uint32_t i, uint8_t v) {
    for (uint32_t k = 0; k < 4; k++)
        if (k == i) a[k] = v;
}
// `[` seen and consumed: is the array empty (then `]` is consumed too)?
RMJP_FN bool array_empty(Cur& c) {
    ws(c);
    if (peek(c) == ']') { c.p++; return true; }
    return false;
}
// after an element: 1 = another follows, 0 = the array ended, -1 = malformed
RMJP_FN int array_next(Cur& c) {
    ws(c);
    const int d = peek(c);
    if (d < 0) return -1;
    c.p++;
    return d == ',' ? 1 : d == ']' ? 0 : -1;
}
RMJP_FN uint8_t read_ints(Cur& c, IntsF& f) {   // scores / deltas: the first four as int32, the rest skipped
    f.n = 0;
    f.st = 0;
    for (int k = 0; k < 4; k++) f.v[k] = 0;
    const int ch = peek(c);
    if (ch == 'n') {
        f.tag = F_NULL;
        return RMJP_LIT(c, "null") ? 0 : RMJ_LOGTEXT_ERR_JSON;
    }
    if (ch != '[') {
        f.tag = F_BAD;
        f.st = RMJ_LOGTEXT_UNSUPPORTED;
        return skip_st(c);
    }
    c.p++;
    f.tag = F_OK;
    if (array_empty(c)) return 0;
    uint32_t n = 0;
    for (;;) {
        ws(c);
        if (n < 4u) {
            IntF e;
            const uint8_t r = read_int(c, e);
            if (r) return r;
            if (e.tag == F_OK && e.v >= -(int64_t)2147483648LL && e.v <= (int64_t)2147483647LL) set4(f.v, n, (int32_t)e.v);
            else if (!f.st) f.st = RMJ_LOGTEXT_UNSUPPORTED;
        } else {
            const uint8_t r = skip_st(c);
            if (r) return r;
        }
        if (n < 255u) n++;
        const int nx = array_next(c);
        if (nx < 0) return RMJ_LOGTEXT_ERR_JSON;
        if (!nx) break;
    }
    f.n = (uint8_t)n;
    if (f.st) f.tag = F_BAD;
    return 0;
}
// an array of tile names: every one mapped (the first failure is kept), the first `keep` stored to out, *count = the entries (capped at 255)
RMJP_FN uint8_t read_tiles(Cur& c, bool masked_ok, uint8_t* out, uint32_t keep, uint8_t& st, uint32_t& count) {
    st = 0;
    count = 0;
    if (peek(c) != '[') {
        st = RMJ_LOGTEXT_UNSUPPORTED;
        return skip_st(c);
    }
    c.p++;
    if (array_empty(c)) return 0;
    for (;;) {
        ws(c);
        uint8_t est, tid;
        const uint8_t r = read_tile(c, masked_ok, est, tid);
        if (r) return r;
        if (est && !st) st = est;
        if (count < keep) out[count] = tid;
        if (count < 255u) count++;
        const int nx = array_next(c);
        if (nx < 0) return RMJ_LOGTEXT_ERR_JSON;
        if (!nx) break;
    }
    return 0;
}

enum : uint8_t {
    T_NONE = 0, T_START_GAME, T_START_KYOKU, T_TSUMO, T_DAHAI, T_REACH, T_REACH_ACCEPTED, T_CHI, T_PON, T_DAIMINKAN, T_KAN, T_ANKAN, T_KAKAN, T_DORA, T_HORA,
    T_RYUKYOKU, T_END_KYOKU, T_END_GAME, T_KITA, T_UNSUPPORTED
};
RMJP_FN uint8_t type_of(const StrInfo& s) {
    if (s.esc) return T_UNSUPPORTED;
    if (s.high) return T_NONE;
    if (RMJP_IS(s, "tsumo")) return T_TSUMO;
    if (RMJP_IS(s, "dahai")) return T_DAHAI;
    if (RMJP_IS(s, "pon")) return T_PON;
    if (RMJP_IS(s, "chi")) return T_CHI;
    if (RMJP_IS(s, "reach")) return T_REACH;
    if (RMJP_IS(s, "reach_accepted")) return T_REACH_ACCEPTED;
    if (RMJP_IS(s, "start_kyoku")) return T_START_KYOKU;
    if (RMJP_IS(s, "end_kyoku")) return T_END_KYOKU;
    if (RMJP_IS(s, "hora")) return T_HORA;
    if (RMJP_IS(s, "ryukyoku")) return T_RYUKYOKU;
    if (RMJP_IS(s, "dora")) return T_DORA;
    if (RMJP_IS(s, "ankan")) return T_ANKAN;
    if (RMJP_IS(s, "kakan")) return T_KAKAN;
    if (RMJP_IS(s, "daiminkan")) return T_DAIMINKAN;
    if (RMJP_IS(s, "kan")) return T_KAN;
    if (RMJP_IS(s, "kita")) return T_KITA;
    if (RMJP_IS(s, "start_game")) return T_START_GAME;
    if (RMJP_IS(s, "end_game")) return T_END_GAME;
    return T_NONE;
}
enum : int {
    K_TYPE = 0, K_ACTOR, K_TARGET, K_PAI, K_CONSUMED, K_TSUMOGIRI, K_OYA, K_KYOKU, K_HONBA, K_KYOTAKU, K_KYOUTAKU, K_BAKAZE, K_DORA_MARKER, K_SCORES, K_TEHAIS,
    K_DELTAS, K_DELTA, K_UNKNOWN
};
RMJP_FN int key_of(const StrInfo& s) {
    if (s.esc || s.high) return K_UNKNOWN;
    if (RMJP_IS(s, "type")) return K_TYPE;
    if (RMJP_IS(s, "actor")) return K_ACTOR;
    if (RMJP_IS(s, "pai")) return K_PAI;
    if (RMJP_IS(s, "tsumogiri")) return K_TSUMOGIRI;
    if (RMJP_IS(s, "target")) return K_TARGET;
    if (RMJP_IS(s, "consumed")) return K_CONSUMED;
    if (RMJP_IS(s, "oya")) return K_OYA;
    if (RMJP_IS(s, "kyoku")) return K_KYOKU;
    if (RMJP_IS(s, "honba")) return K_HONBA;
    if (RMJP_IS(s, "kyotaku")) return K_KYOTAKU;
    if (RMJP_IS(s, "kyoutaku")) return K_KYOUTAKU;
    if (RMJP_IS(s, "bakaze")) return K_BAKAZE;
    if (RMJP_IS(s, "dora_marker")) return K_DORA_MARKER;
    if (RMJP_IS(s, "scores")) return K_SCORES;
    if (RMJP_IS(s, "tehais")) return K_TEHAIS;
    if (RMJP_IS(s, "deltas")) return K_DELTAS;
    if (RMJP_IS(s, "delta")) return K_DELTA;
    return K_UNKNOWN;
}

// a byte field of the record from an integer value: 0 = fine
RMJP_FN uint8_t byte_opt(const IntF& f, uint8_t& out) {   // actor / target: int(ev.get(k, 0) or 0)
    out = 0;
    if (f.tag == F_ABSENT || f.tag == F_NULL || f.tag == F_FALSE) return 0;
    if (f.tag != F_OK || f.v < 0 || f.v > 255) return RMJ_LOGTEXT_UNSUPPORTED;
    out = (uint8_t)f.v;
    return 0;
}
RMJP_FN uint8_t int_req(const IntF& f, int64_t hi, uint32_t& out) {   // int(ev[k])
    out = 0;
    if (f.tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
    if (f.tag == F_NULL) return RMJ_LOGTEXT_ERR_VALUE;
    if (f.tag != F_OK || f.v < 0 || f.v > hi) return RMJ_LOGTEXT_UNSUPPORTED;
    out = (uint32_t)f.v;
    return 0;
}
RMJP_FN uint8_t tile_req(const TileF& f, uint8_t& out) {   // mjai_to_tid(ev[k])
    out = 0;
    if (f.tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
    if (f.st) return f.st;
    out = f.tid;
    return 0;
}

struct Fields {
    IntF actor, target, oya, kyoku, honba, kyotaku, kyoutaku;
    TileF pai, dora_marker;
    IntsF scores, deltas, delta;
    TilesF consumed;
    uint8_t type, type_st;
    uint8_t tsumogiri, tsumogiri_st;
    uint8_t bakaze, bakaze_tag, bakaze_st;
    uint8_t tehais_tag, tehais_st;
};

RMJP_FN void zero_recs(RmjEvent* recs) {
    uint8_t* b = reinterpret_cast<uint8_t*>(recs);
    for (uint32_t i = 0; i < 3u * (uint32_t)sizeof(RmjEvent); i++) b[i] = 0;
}
RMJP_FN uint8_t* tehai_slot(RmjEvent* recs, uint32_t seat) {   // seat's 13 bytes: payload of TEHAI record 1 + seat / 2
    return reinterpret_cast<uint8_t*>(&recs[1 + (seat >> 1)]) + 4 + 13 * (seat & 1u);
}

// tehais: the hands of the seats < num_players go straight into the payload of records 1 and 2 (cleared again unless the line is a start_kyoku)
RMJP_FN uint8_t read_tehais(Cur& c, uint32_t num_players, bool masked_ok, RmjEvent* recs, uint8_t& st) {
    st = 0;
    if (peek(c) != '[') {
        st = RMJ_LOGTEXT_UNSUPPORTED;
        return skip_st(c);
    }
    c.p++;
    if (array_empty(c)) return 0;
    uint32_t seat = 0;
    for (;;) {
        ws(c);
        if (seat < num_players && seat < 4u) {
            uint8_t est;
            uint32_t n;
            const uint8_t r = read_tiles(c, masked_ok, tehai_slot(recs, seat), 13u, est, n);
            if (r) return r;
            if (!est && n != 13u) est = RMJ_LOGTEXT_ERR_TEHAI;
            if (est && !st) st = est;
        } else {
            const uint8_t r = skip_st(c);
            if (r) return r;
        }
        seat++;
        const int nx = array_next(c);
        if (nx < 0) return RMJ_LOGTEXT_ERR_JSON;
        if (!nx) break;
    }
    return 0;
}

RMJP_FN uint8_t parse_body(Cur& c, uint32_t num_players, bool masked_ok, RmjEvent* recs, Side& side) {
    Fields F;
    F.actor.tag = F.target.tag = F.oya.tag = F.kyoku.tag = F.honba.tag = F.kyotaku.tag = F.kyoutaku.tag = F_ABSENT;
    F.pai.tag = F.dora_marker.tag = F_ABSENT;
    F.pai.st = F.dora_marker.st = 0;
    F.scores.tag = F.deltas.tag = F.delta.tag = F.consumed.tag = F_ABSENT;
    F.scores.n = F.deltas.n = F.delta.n = F.consumed.n = 0;
    F.scores.st = F.deltas.st = F.delta.st = F.consumed.st = 0;
    for (int k = 0; k < 4; k++) F.scores.v[k] = F.deltas.v[k] = F.delta.v[k] = 0, F.consumed.t[k] = 0;
    F.type = T_NONE;
    F.type_st = F.tsumogiri = F.tsumogiri_st = F.bakaze = F.bakaze_st = F.tehais_st = 0;
    F.bakaze_tag = F.tehais_tag = F_ABSENT;
    uint32_t seen = 0;
    bool declined = false;   // an escaped key or a duplicate key of interest

    ws(c);
    if (peek(c) != '{') return RMJ_LOGTEXT_ERR_JSON;
    c.p++;
    ws(c);
    if (peek(c) == '}') {
        c.p++;
    } else {
        for (;;) {
            ws(c);
            if (peek(c) != '"') return RMJ_LOGTEXT_ERR_JSON;
            c.p++;
            StrInfo key;
            if (!scan_string(c, key)) return RMJ_LOGTEXT_ERR_JSON;
            ws(c);
            if (peek(c) != ':') return RMJ_LOGTEXT_ERR_JSON;
            c.p++;
            ws(c);
            if (key.esc) declined = true;
            int id = key_of(key);
            if (id != K_UNKNOWN) {
                if (seen & (1u << id)) { declined = true; id = K_UNKNOWN; }
                seen |= 1u << id;
            }
            uint8_t r = 0;
            switch (id) {
                case K_TYPE: {
                    const int ch = peek(c);
                    if (ch == '"') {
                        c.p++;
                        StrInfo s;
                        if (!scan_string(c, s)) return RMJ_LOGTEXT_ERR_JSON;
                        F.type = type_of(s);
                    } else {
                        F.type = (ch == '[' || ch == '{') ? (uint8_t)T_UNSUPPORTED : (uint8_t)T_NONE;
                        r = skip_st(c);
                    }
                    break;
                }
                case K_ACTOR: r = read_int(c, F.actor); break;
                case K_TARGET: r = read_int(c, F.target); break;
                case K_OYA: r = read_int(c, F.oya); break;
                case K_KYOKU: r = read_int(c, F.kyoku); break;
                case K_HONBA: r = read_int(c, F.honba); break;
                case K_KYOTAKU: r = read_int(c, F.kyotaku); break;
                case K_KYOUTAKU: r = read_int(c, F.kyoutaku); break;
                case K_PAI: F.pai.tag = F_OK; r = read_tile(c, masked_ok, F.pai.st, F.pai.tid); break;
                case K_DORA_MARKER: F.dora_marker.tag = F_OK; r = read_tile(c, masked_ok, F.dora_marker.st, F.dora_marker.tid); break;
                case K_CONSUMED: {
                    uint32_t n;
                    F.consumed.tag = F_OK;
                    r = read_tiles(c, masked_ok, F.consumed.t, 4u, F.consumed.st, n);
                    F.consumed.n = (uint8_t)(n > 4u ? 4u : n);
                    break;
                }
                case K_TSUMOGIRI: {
                    const int ch = peek(c);
                    if (ch == 't') { F.tsumogiri = 1; if (!RMJP_LIT(c, "true")) return RMJ_LOGTEXT_ERR_JSON; }
                    else if (ch == 'f') { if (!RMJP_LIT(c, "false")) return RMJ_LOGTEXT_ERR_JSON; }
                    else if (ch == 'n') { if (!RMJP_LIT(c, "null")) return RMJ_LOGTEXT_ERR_JSON; }
                    else { F.tsumogiri_st = RMJ_LOGTEXT_UNSUPPORTED; r = skip_st(c); }
                    break;
                }
                case K_BAKAZE: {
                    F.bakaze_tag = F_OK;
                    F.bakaze_st = RMJ_LOGTEXT_UNSUPPORTED;
                    if (peek(c) == '"') {
                        c.p++;
                        StrInfo s;
                        if (!scan_string(c, s)) return RMJ_LOGTEXT_ERR_JSON;
                        const uint32_t c0 = (uint32_t)(s.k0 & 0xFFu);
                        const int w = c0 == 'E' ? 0 : c0 == 'S' ? 1 : c0 == 'W' ? 2 : c0 == 'N' ? 3 : -1;
                        if (!s.esc && !s.high && s.len == 1u && w >= 0) { F.bakaze = (uint8_t)w; F.bakaze_st = 0; }
                    } else {
                        r = skip_st(c);
                    }
                    break;
                }
                case K_SCORES: r = read_ints(c, F.scores); break;
                case K_DELTAS: r = read_ints(c, F.deltas); break;
                case K_DELTA: r = read_ints(c, F.delta); break;
                case K_TEHAIS: F.tehais_tag = F_OK; r = read_tehais(c, num_players, masked_ok, recs, F.tehais_st); break;
                default: r = skip_st(c); break;
            }
            if (r) return r;   // malformed, or nested deeper than the skipper follows (the rest of the line is then not judged)
            ws(c);
            const int d = peek(c);
            if (d < 0) return RMJ_LOGTEXT_ERR_JSON;
            c.p++;
            if (d == '}') break;
            if (d != ',') return RMJ_LOGTEXT_ERR_JSON;
        }
    }
    ws(c);
    if (c.p != c.e) return RMJ_LOGTEXT_ERR_JSON;   // json.loads: extra data
    if (declined || F.type == T_UNSUPPORTED) return RMJ_LOGTEXT_UNSUPPORTED;

    // ---- the records (event_records_from_mjai) and the side struct
    const uint8_t ty = F.type;
    if (ty != T_START_KYOKU) {   // a `tehais` of another event is not read by the packer
        uint8_t* b = reinterpret_cast<uint8_t*>(&recs[1]);
        for (uint32_t i = 0; i < 2u * (uint32_t)sizeof(RmjEvent); i++) b[i] = 0;
    }
    RmjEvent& e = recs[0];
    uint8_t actor, st;
    if ((st = byte_opt(F.actor, actor)) != 0) return st;
    side.actor = actor;
    if (F.actor.tag == F_ABSENT || F.actor.tag == F_NULL) side.flags |= SF_ACTOR_NONE;
    if (ty == T_DAHAI || ty == T_CHI || ty == T_PON || ty == T_DAIMINKAN || ty == T_KAN || ty == T_ANKAN || ty == T_KAKAN || ty == T_REACH || ty == T_HORA ||
        ty == T_KITA || ty == T_RYUKYOKU)
        side.flags |= SF_DECISION;
    switch (ty) {
        case T_START_GAME: e.type = RMJ_EV_START_GAME; e.actor = actor; break;
        case T_REACH: e.type = RMJ_EV_REACH; e.actor = actor; side.cls = CLS_REACH; break;
        case T_REACH_ACCEPTED: e.type = RMJ_EV_REACH_ACCEPTED; e.actor = actor; side.cls = CLS_REACH_ACCEPTED; break;
        case T_END_KYOKU: e.type = RMJ_EV_END_KYOKU; e.actor = actor; side.cls = CLS_END; break;
        case T_END_GAME: e.type = RMJ_EV_END_GAME; e.actor = actor; side.cls = CLS_END; break;
        case T_KITA: e.type = RMJ_EV_KITA; e.actor = actor; break;
        case T_HORA:
        case T_RYUKYOKU: {
            e.type = ty == T_HORA ? RMJ_EV_HORA : RMJ_EV_RYUKYOKU;
            e.actor = actor;
            side.cls = ty == T_HORA ? CLS_HORA : CLS_RYUKYOKU;
            if (F.scores.tag == F_BAD) return F.scores.st;
            if (F.scores.tag == F_OK) {
                side.flags |= SF_HAS_SCORES;
                side.n_scores = F.scores.n;
                for (int k = 0; k < 4; k++) side.scores[k] = F.scores.v[k];
            }
            const IntsF& D = F.deltas.tag != F_ABSENT ? F.deltas : F.delta;   // ev.get("deltas", ev.get("delta"))
            if (D.tag == F_BAD) {
                if (!(side.flags & SF_HAS_SCORES)) return D.st;   // read only when `scores` does not decide
            } else if (D.tag == F_OK) {
                side.flags |= SF_HAS_DELTAS;
                side.n_deltas = D.n > 4 ? 4 : D.n;
                for (int k = 0; k < 4; k++) side.deltas[k] = D.v[k];
            }
            break;
        }
        case T_START_KYOKU: {
            uint32_t v;
            e.type = RMJ_EV_START_KYOKU;
            if ((st = int_req(F.oya, 255, v)) != 0) return st;
            e.actor = (uint8_t)v;
            if ((st = int_req(F.kyoku, 255, v)) != 0) return st;
            e.target = (uint8_t)v;
            if ((st = tile_req(F.dora_marker, e.tile)) != 0) return st;
            uint32_t kyotaku = 0;
            if (F.kyoutaku.tag != F_ABSENT) { if ((st = int_req(F.kyoutaku, 65535, kyotaku)) != 0) return st; }
            else if (F.kyotaku.tag != F_ABSENT) { if ((st = int_req(F.kyotaku, 65535, kyotaku)) != 0) return st; }
            if (F.bakaze_tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
            if (F.bakaze_st) return F.bakaze_st;
            e.consumed[0] = F.bakaze;
            if ((st = int_req(F.honba, 255, v)) != 0) return st;
            e.consumed[1] = (uint8_t)v;
            e.consumed[2] = (uint8_t)(kyotaku & 0xFFu);
            e.consumed[3] = (uint8_t)(kyotaku >> 8);
            if (F.scores.tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
            if (F.scores.tag == F_NULL) return RMJ_LOGTEXT_ERR_VALUE;
            if (F.scores.tag == F_BAD) return F.scores.st;
            for (int k = 0; k < 4; k++) e.deltas[k] = side.scores[k] = F.scores.v[k];
            side.n_scores = F.scores.n;
            side.flags |= SF_HAS_SCORES;
            if (F.tehais_tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
            if (F.tehais_st) return F.tehais_st;
            recs[1].type = recs[2].type = RMJ_EV_TEHAI;
            recs[1].actor = 0;
            recs[2].actor = 1;
            side.cls = CLS_START_KYOKU;
            break;
        }
        case T_TSUMO:
        case T_DAHAI:
        case T_KAKAN:
            e.type = ty == T_TSUMO ? RMJ_EV_TSUMO : ty == T_DAHAI ? RMJ_EV_DAHAI : RMJ_EV_KAKAN;
            e.actor = actor;
            if ((st = tile_req(F.pai, e.tile)) != 0) return st;
            if (ty == T_DAHAI) {
                if (F.tsumogiri_st) return F.tsumogiri_st;
                e.flags = F.tsumogiri;
                side.cls = CLS_DAHAI;
            }
            break;
        case T_PON:
        case T_CHI:
        case T_DAIMINKAN:
        case T_KAN:
        case T_ANKAN: {
            e.type = ty == T_PON ? RMJ_EV_PON : ty == T_CHI ? RMJ_EV_CHI : ty == T_ANKAN ? RMJ_EV_ANKAN : RMJ_EV_DAIMINKAN;
            e.actor = actor;
            if ((st = byte_opt(F.target, e.target)) != 0) return st;
            if (ty != T_ANKAN) {
                if ((st = tile_req(F.pai, e.tile)) != 0) return st;
                side.cls = CLS_CALL;
                if (F.target.tag == F_ABSENT) side.flags |= SF_NO_TARGET;
            }
            if (F.consumed.tag == F_ABSENT) return RMJ_LOGTEXT_ERR_KEY;
            if (F.consumed.st) return F.consumed.st;
            for (int k = 0; k < 4; k++) e.consumed[k] = k < F.consumed.n ? F.consumed.t[k] : (uint8_t)0;
            e.flags = (uint8_t)(F.consumed.n << 4);
            break;
        }
        case T_DORA:
            e.type = RMJ_EV_DORA;
            if ((st = tile_req(F.dora_marker, e.tile)) != 0) return st;
            break;
        default: break;   // NONE
    }
    return RMJ_LOGTEXT_OK;
}

// The three records and the side struct of the line [p, p + len); returns side->status.
RMJP_FN uint8_t parse_line(const uint8_t* p, uint32_t len, uint32_t num_players, bool masked_ok, RmjEvent* recs, Side* side) {
    zero_recs(recs);
    Side s;
    for (int k = 0; k < 4; k++) s.scores[k] = s.deltas[k] = 0;
    s.cls = CLS_OTHER;
    s.flags = s.n_scores = s.n_deltas = s.status = s.actor = 0;
    s.pad[0] = s.pad[1] = 0;
    Cur c{p, p + len};
    const uint8_t st = parse_body(c, num_players, masked_ok, recs, s);
    if (st != RMJ_LOGTEXT_OK) {
        zero_recs(recs);
        for (int k = 0; k < 4; k++) s.scores[k] = s.deltas[k] = 0;
        s.cls = CLS_OTHER;
        s.flags = s.n_scores = s.n_deltas = s.actor = 0;
    }
    s.status = st;
    *side = s;
    return st;
}

// ---------------------------------------------------------------- the kyoku walk (MjaiReplay.from_events + datasets.kyoku_tables)
// One log's events in order -> the start / end scores of its kyokus.  feed() takes the side struct of every event; rows are written through
// `put(row, start, end)` when a kyoku's end scores are known (a kyoku's end scores are the next kyoku's start scores; the last kyoku keeps
// what its hora / ryukyoku events gave).  status(): RMJ_LOGTEXT_ERR_REPLAY where Kyoku._feed raises (a dahai / reach / reach_accepted
// whose actor is missing or not a seat of the kyoku, a call without `target`), RMJ_LOGTEXT_UNSUPPORTED where a score leaves int32 or an
// end-of-round `scores` has another length than the kyoku's.
struct KyokuWalk {
    int32_t start[4], end[4];
    // with a row: the end scores the kyoku's own events gave, before the next start_kyoku's scores replace them - own[0..3] as `end` holds
    // them, own[4..7] with a ryukyoku's deltas read as already holding the riichi deposits (logs written by this engine do; log validation
    // accepts either reading)
    int32_t own[8];
    int32_t end2[4];           // the second reading while the kyoku is open
    uint32_t n = 0;            // seats of the open kyoku's scores (min 4)
    uint32_t n_raw = 0;        // len(scores) uncut
    uint32_t kyokus = 0;       // start_kyoku events so far
    bool open = false;         // cur is not None
    bool have = false;         // a kyoku's row is pending (start / end hold it)
    bool prev_hora = false;    // _pending_hule is not empty
    uint8_t reached = 0, accepted = 0;
    uint8_t st = 0;

    RMJP_FN void fail(uint8_t s) { if (!st) st = s; }
    // returns true when the row `kyokus - 2` (the kyoku before the one just opened) is complete: start_out / end_out hold it
    RMJP_FN bool feed(const Side& s, int32_t* start_out, int32_t* end_out) {
        bool emit = false;
        if (s.cls == CLS_START_KYOKU) {
            if (have) {
                for (int k = 0; k < 4; k++) { start_out[k] = start[k]; end_out[k] = s.scores[k]; own[k] = end[k]; own[4 + k] = end2[k]; }
                emit = true;
            }
            for (int k = 0; k < 4; k++) start[k] = end[k] = end2[k] = s.scores[k];
            n_raw = s.n_scores;
            n = n_raw > 4u ? 4u : n_raw;
            kyokus++;
            open = have = true;
            prev_hora = false;
            reached = accepted = 0;
            return emit;
        }
        if (!open) return false;
        if (s.cls == CLS_END) { open = false; prev_hora = false; return false; }
        const bool first = !prev_hora;
        prev_hora = s.cls == CLS_HORA;
        if (s.cls == CLS_DAHAI || s.cls == CLS_REACH || s.cls == CLS_REACH_ACCEPTED) {
            if ((s.flags & SF_ACTOR_NONE) || s.actor >= n_raw) { fail(RMJ_LOGTEXT_ERR_REPLAY); return false; }
            if (s.actor < 4u) {
                if (s.cls == CLS_REACH) reached |= (uint8_t)(1u << s.actor);
                if (s.cls == CLS_REACH_ACCEPTED) accepted |= (uint8_t)(1u << s.actor);
            }
        } else if (s.cls == CLS_CALL) {
            if (s.flags & SF_NO_TARGET) fail(RMJ_LOGTEXT_ERR_REPLAY);
        } else if (s.cls == CLS_HORA || s.cls == CLS_RYUKYOKU) {
            if (s.flags & SF_HAS_SCORES) {
                if ((s.n_scores > 4u ? 4u : s.n_scores) != n) { fail(RMJ_LOGTEXT_UNSUPPORTED); return false; }
                for (int k = 0; k < 4; k++) end[k] = end2[k] = s.scores[k];
            } else if (s.flags & SF_HAS_DELTAS) {
                const uint8_t sticks = s.cls == CLS_HORA ? accepted : reached;
                for (uint32_t k = 0; k < 4u; k++) {
                    if (k >= n || k >= s.n_deltas) continue;
                    int64_t v;
                    if (s.cls == CLS_HORA && !first) v = (int64_t)end[k] + s.deltas[k];
                    else v = (int64_t)start[k] + s.deltas[k] - (((sticks >> k) & 1u) ? 1000 : 0);
                    if (v < -(int64_t)2147483648LL || v > (int64_t)2147483647LL) { fail(RMJ_LOGTEXT_UNSUPPORTED); return false; }
                    end[k] = (int32_t)v;
                    const int64_t v2 = s.cls == CLS_RYUKYOKU ? (int64_t)start[k] + s.deltas[k] : v;
                    end2[k] = (int32_t)(v2 > (int64_t)2147483647LL ? (int64_t)2147483647LL : v2);
                }
            }
        }
        return false;
    }
    // after the last event: true when a last row (`kyokus - 1`) is pending
    RMJP_FN bool finish(int32_t* start_out, int32_t* end_out) {
        if (!have) return false;
        for (int k = 0; k < 4; k++) { start_out[k] = start[k]; end_out[k] = own[k] = end[k]; own[4 + k] = end2[k]; }
        return true;
    }
};

}  // namespace rmjp
