// One MJAI event record -> its JSON text, as scalar functions that the host and the device share: the device formatter of the logs of
// every game (k_text_size / k_text_write in rmj_events.hip.h: rmj_drain_text, rmj_format_events_device) and the host test that holds them to
// rmjh::format_event / format_events (rmj_host.h), which stay the definition.  Plain C++17 under g++; __host__ __device__ under hipcc.
// No HIP intrinsics in this file.
//
// Per record two functions:
//   evt_len   - the bytes the record contributes to its game's log ('\n' included), 0, or RMJT_STOP: the log ends before this record;
//   evt_write - the text of a record whose evt_len is > 0, into a byte sink (anything with put(char)).
//
// The sequential rule of a game's window (rmjh::format_events: skip TEHAI, format an event, a START_KYOKU consumes the two TEHAI records
// behind it, stop at the first event that cannot be formatted) restated per record, so that every record is sized on its own:
//   * a TEHAI record never starts an event;
//   * a START_KYOKU record is a valid head iff the next two records of the window are TEHAI: it contributes its whole string and its
//     two TEHAI records contribute 0 bytes (they would have been skipped as heads anyway, so "consumed" and "skipped" agree);
//   * any other TEHAI record (the tail of a head the window lost) contributes 0 bytes;
//   * the log ends before the first non-TEHAI record that cannot be formatted - an unknown type, or a START_KYOKU that is not a valid
//     head - and every record from there on contributes 0 bytes (the host loop's `break`).
// So a game's text is the concatenation, in record order, of the texts of the records before its first RMJT_STOP.
//
// Semantics (rmjh::format_event): alphabetical keys; np = 3 iff pad == 3; seat < 0 - the full text, otherwise tehais and tsumo tiles of
// the other seats are masked ("?"), a seat >= np sees every tehai masked; n_consumed (flags bits 4..7) clamped to 4, n_ura to 5;
// ryukyoku flags >= 7 - "Error: Illegal Action by Player <actor>"; int32 scores / deltas as exact decimals (INT32_MIN included);
// kyotaku 16 bits; tile names of every byte value as put_tile (parser.rs:301-334; ids >= 136 continue the honour numbering: 255 -> 37z).
#pragma once
#include <stdint.h>

#include "../../include/riichi_mi355x.h"

#if defined(__HIPCC__)
#define RMJT_FN __host__ __device__ inline
#define RMJT_UNROLL _Pragma("unroll")
#else
#define RMJT_FN inline
#define RMJT_UNROLL
#endif

namespace rmjt {

constexpr int32_t RMJT_STOP = -1;
// the longest text one record can give: a START_KYOKU with four 13-tile tehais of 3-character names and four 11-character scores
// (496 bytes); the device writer sizes its per-wave staging by it
constexpr uint32_t RMJT_MAX_EVENT_BYTES = 512;

// ---------------------------------------------------------------- tables
// tile name of every byte value: chars in bits 0..23, length in bits 24..31
constexpr uint32_t tile_code(int t) {
    if (t == 16) return '5' | ('m' << 8) | ('r' << 16) | (3u << 24);
    if (t == 52) return '5' | ('p' << 8) | ('r' << 16) | (3u << 24);
    if (t == 88) return '5' | ('s' << 8) | ('r' << 16) | (3u << 24);
    if (t < 108) return (uint32_t)('1' + (t % 36) / 4) | ((uint32_t)(t < 36 ? 'm' : t < 72 ? 'p' : 's') << 8) | (2u << 24);
    const int num = (t - 108) / 4;
    if (num < 7) {
        const char hon[7] = {'E', 'S', 'W', 'N', 'P', 'F', 'C'};
        return (uint32_t)hon[num] | (1u << 24);
    }
    const int v = num + 1;   // 8 .. 37
    if (v < 10) return (uint32_t)('0' + v) | ('z' << 8) | (2u << 24);
    return (uint32_t)('0' + v / 10) | ((uint32_t)('0' + v % 10) << 8) | ('z' << 16) | (3u << 24);
}
struct TileTable { uint32_t v[256]; };
constexpr TileTable make_tile_table() {
    TileTable T{};
    for (int t = 0; t < 256; t++) T.v[t] = tile_code(t);
    return T;
}
// short strings: length in s[0]
struct Str { char s[24]; };
// meld type names (CHI .. KAKAN: type - RMJ_EV_CHI) and ryukyoku reasons (flags 0..6)
#define RMJT_MELD_NAMES {{{3, 'c', 'h', 'i'}}, {{3, 'p', 'o', 'n'}}, {{9, 'd', 'a', 'i', 'm', 'i', 'n', 'k', 'a', 'n'}}, \
                         {{5, 'a', 'n', 'k', 'a', 'n'}}, {{5, 'k', 'a', 'k', 'a', 'n'}}}
#define RMJT_REASONS {{{15, 'e', 'x', 'h', 'a', 'u', 's', 't', 'i', 'v', 'e', '_', 'd', 'r', 'a', 'w'}},                 \
                      {{13, 'n', 'a', 'g', 'a', 's', 'h', 'i', 'm', 'a', 'n', 'g', 'a', 'n'}},                            \
                      {{13, 'k', 'y', 'u', 's', 'h', 'u', '_', 'k', 'y', 'u', 'h', 'a', 'i'}},                            \
                      {{10, 's', 'u', 'f', 'u', 'u', 'r', 'e', 'n', 't', 'a'}},                                          \
                      {{12, 's', 'u', 'u', 'k', 'a', 'n', 's', 'a', 'n', 's', 'e', 'n'}},                                \
                      {{13, 's', 'u', 'u', 'c', 'h', 'a', '_', 'r', 'i', 'i', 'c', 'h', 'i'}},                            \
                      {{8, 's', 'a', 'n', 'c', 'h', 'a', 'h', 'o'}}}
#define RMJT_POW10 {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u}

#if defined(__HIPCC__)
__constant__ const TileTable d_tiles = make_tile_table();
__constant__ const Str d_meld_names[5] = RMJT_MELD_NAMES;
__constant__ const Str d_reasons[7] = RMJT_REASONS;
__constant__ const uint32_t d_pow10[10] = RMJT_POW10;
#endif
static const TileTable h_tiles = make_tile_table();
static const Str h_meld_names[5] = RMJT_MELD_NAMES;
static const Str h_reasons[7] = RMJT_REASONS;
static const uint32_t h_pow10[10] = RMJT_POW10;
#if defined(__HIP_DEVICE_COMPILE__)
#define RMJT_TAB(name) d_##name
#else
#define RMJT_TAB(name) h_##name
#endif

// ---------------------------------------------------------------- literals (one definition for the length and the writer)
#define RMJT_LEN(lit) ((uint32_t)sizeof(lit) - 1u)
#define RMJT_S_START_GAME "{\"type\":\"start_game\"}"
#define RMJT_S_END_KYOKU "{\"type\":\"end_kyoku\"}"
#define RMJT_S_END_GAME "{\"type\":\"end_game\"}"
#define RMJT_S_SK_BAKAZE "{\"bakaze\":\""
#define RMJT_S_SK_DORA "\",\"dora_marker\":\""
#define RMJT_S_SK_HONBA "\",\"honba\":"
#define RMJT_S_SK_KYOKU ",\"kyoku\":"
#define RMJT_S_SK_KYOTAKU ",\"kyotaku\":"
#define RMJT_S_SK_OYA ",\"oya\":"
#define RMJT_S_SK_SCORES ",\"scores\":"
#define RMJT_S_SK_TEHAIS ",\"tehais\":["
#define RMJT_S_SK_END "],\"type\":\"start_kyoku\"}"
#define RMJT_S_MASKED13 "[\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\",\"?\"]"
#define RMJT_S_ACTOR "{\"actor\":"
#define RMJT_S_PAI ",\"pai\":\""
#define RMJT_S_TSUMO_END "\",\"type\":\"tsumo\"}"
#define RMJT_S_TSUMOGIRI "\",\"tsumogiri\":"
#define RMJT_S_DAHAI_END ",\"type\":\"dahai\"}"
#define RMJT_S_REACH_END ",\"type\":\"reach\"}"
#define RMJT_S_REACH_ACC_END ",\"type\":\"reach_accepted\"}"
#define RMJT_S_CONSUMED ",\"consumed\":"
#define RMJT_S_TARGET "\",\"target\":"
#define RMJT_S_HORA_TARGET ",\"target\":"
#define RMJT_S_TYPE_Q ",\"type\":\""
#define RMJT_S_PAI_TYPE_Q "\",\"type\":\""
#define RMJT_S_QBRACE "\"}"
#define RMJT_S_KITA_END "\",\"type\":\"kita\"}"
#define RMJT_S_DORA "{\"dora_marker\":\""
#define RMJT_S_DORA_END "\",\"type\":\"dora\"}"
#define RMJT_S_DELTAS_A ",\"deltas\":"
#define RMJT_S_TSUMO_TRUE ",\"tsumo\":true"
#define RMJT_S_HORA_URA ",\"type\":\"hora\",\"ura_markers\":"
#define RMJT_S_DELTAS_R "{\"deltas\":"
#define RMJT_S_REASON ",\"reason\":\""
#define RMJT_S_ILLEGAL "Error: Illegal Action by Player "
#define RMJT_S_RYUKYOKU_END "\",\"type\":\"ryukyoku\"}"

// ---------------------------------------------------------------- pieces
RMJT_FN uint32_t u32_len(uint32_t u) {
    uint32_t n = 1;
    for (int i = 1; i < 10; i++) n += u >= RMJT_TAB(pow10)[i] ? 1u : 0u;
    return n;
}
RMJT_FN uint32_t abs32(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }
RMJT_FN uint32_t i32_len(int32_t v) { return u32_len(abs32(v)) + (v < 0 ? 1u : 0u); }
RMJT_FN uint32_t tile_len(uint8_t t) { return RMJT_TAB(tiles).v[t] >> 24; }
// ["a","b",...] of n (0..MAX) tiles.  Loops run to the constant MAX (and unroll on the device): a record held in registers is then
// indexed by constants only, never spilled to scratch for a dynamic index.
template <int MAX> RMJT_FN uint32_t tiles_len(const uint8_t* t, int n) {
    uint32_t s = n > 0 ? 2u + 3u * (uint32_t)n - 1u : 2u;
    RMJT_UNROLL
    for (int i = 0; i < MAX; i++)
        if (i < n) s += tile_len(t[i]);
    return s;
}
// [a,b,...] of np (3 or 4) int32
RMJT_FN uint32_t ints_len(const int32_t* v, int n) {
    uint32_t s = 2u + (uint32_t)n - 1u;
    RMJT_UNROLL
    for (int i = 0; i < 4; i++)
        if (i < n) s += i32_len(v[i]);
    return s;
}

template <class O> RMJT_FN void put_lit(O& o, const char* s, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) o.put(s[i]);
}
#define RMJT_PUT(o, lit) put_lit(o, lit, RMJT_LEN(lit))
template <class O> RMJT_FN void put_str(O& o, const Str& s) {
    const uint32_t n = (uint8_t)s.s[0];
    for (uint32_t i = 0; i < n; i++) o.put(s.s[1 + i]);
}
template <class O> RMJT_FN void put_u32(O& o, uint32_t u) {
    uint32_t p = RMJT_TAB(pow10)[u32_len(u) - 1];
    for (;;) {
        o.put((char)('0' + u / p));
        u %= p;
        if (p == 1u) break;
        p /= 10u;
    }
}
template <class O> RMJT_FN void put_i32(O& o, int32_t v) {
    if (v < 0) o.put('-');
    put_u32(o, abs32(v));
}
template <class O> RMJT_FN void put_tile(O& o, uint8_t t) {
    const uint32_t c = RMJT_TAB(tiles).v[t];
    const uint32_t n = c >> 24;
    o.put((char)(c & 0xFFu));
    if (n > 1) o.put((char)((c >> 8) & 0xFFu));
    if (n > 2) o.put((char)((c >> 16) & 0xFFu));
}
template <int MAX, class O> RMJT_FN void put_tiles(O& o, const uint8_t* t, int n) {
    o.put('[');
    RMJT_UNROLL
    for (int i = 0; i < MAX; i++) {
        if (i >= n) break;
        if (i) o.put(',');
        o.put('"');
        put_tile(o, t[i]);
        o.put('"');
    }
    o.put(']');
}
template <class O> RMJT_FN void put_ints(O& o, const int32_t* v, int n) {
    o.put('[');
    RMJT_UNROLL
    for (int i = 0; i < 4; i++) {
        if (i >= n) break;
        if (i) o.put(',');
        put_i32(o, v[i]);
    }
    o.put(']');
}

RMJT_FN int evt_np(const RmjEvent& e) { return e.pad == 3 ? 3 : 4; }
RMJT_FN int evt_ncons(const RmjEvent& e) { return (e.flags >> 4) > 4 ? 4 : (e.flags >> 4); }
RMJT_FN int evt_nura(const RmjEvent& e) { return e.n_ura > 5 ? 5 : e.n_ura; }
RMJT_FN const uint8_t* tehai_of(const RmjEvent* t1, const RmjEvent* t2, int p) {   // seat p's 13 tiles: payload of TEHAI record 1 + p / 2
    return reinterpret_cast<const uint8_t*>(p < 2 ? t1 : t2) + 4 + 13 * (p & 1);
}
RMJT_FN bool seat_sees(int seat, int p) { return seat < 0 || seat == p; }

// ---------------------------------------------------------------- the two per-record functions
// e: the record; t1, t2: the next two records of the window (nullptr past its end) - read only for a START_KYOKU.
RMJT_FN int32_t evt_len(const RmjEvent& e, const RmjEvent* t1, const RmjEvent* t2, int seat) {
    const int np = evt_np(e);
    uint32_t n;
    switch (e.type) {
        case RMJ_EV_TEHAI: return 0;
        case RMJ_EV_START_GAME: n = RMJT_LEN(RMJT_S_START_GAME); break;
        case RMJ_EV_END_KYOKU: n = RMJT_LEN(RMJT_S_END_KYOKU); break;
        case RMJ_EV_END_GAME: n = RMJT_LEN(RMJT_S_END_GAME); break;
        case RMJ_EV_START_KYOKU: {
            if (!t1 || !t2 || t1->type != RMJ_EV_TEHAI || t2->type != RMJ_EV_TEHAI) return RMJT_STOP;
            n = RMJT_LEN(RMJT_S_SK_BAKAZE) + 1u + RMJT_LEN(RMJT_S_SK_DORA) + tile_len(e.tile) + RMJT_LEN(RMJT_S_SK_HONBA) + u32_len(e.consumed[1]) +
                RMJT_LEN(RMJT_S_SK_KYOKU) + u32_len(e.target) + RMJT_LEN(RMJT_S_SK_KYOTAKU) + u32_len(e.consumed[2] | ((uint32_t)e.consumed[3] << 8)) +
                RMJT_LEN(RMJT_S_SK_OYA) + u32_len(e.actor) + RMJT_LEN(RMJT_S_SK_SCORES) + ints_len(e.deltas, np) + RMJT_LEN(RMJT_S_SK_TEHAIS) +
                (uint32_t)(np - 1) + RMJT_LEN(RMJT_S_SK_END);
            for (int p = 0; p < 4; p++) {
                if (p >= np) break;
                n += seat_sees(seat, p) ? tiles_len<13>(tehai_of(t1, t2, p), 13) : RMJT_LEN(RMJT_S_MASKED13);
            }
            break;
        }
        case RMJ_EV_TSUMO:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_PAI) + (seat_sees(seat, e.actor) ? tile_len(e.tile) : 1u) +
                RMJT_LEN(RMJT_S_TSUMO_END);
            break;
        case RMJ_EV_DAHAI:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_PAI) + tile_len(e.tile) + RMJT_LEN(RMJT_S_TSUMOGIRI) +
                ((e.flags & 1) ? 4u : 5u) + RMJT_LEN(RMJT_S_DAHAI_END);
            break;
        case RMJ_EV_REACH: n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_REACH_END); break;
        case RMJ_EV_REACH_ACCEPTED: n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_REACH_ACC_END); break;
        case RMJ_EV_CHI:
        case RMJ_EV_PON:
        case RMJ_EV_DAIMINKAN:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_CONSUMED) + tiles_len<4>(e.consumed, evt_ncons(e)) + RMJT_LEN(RMJT_S_PAI) +
                tile_len(e.tile) + RMJT_LEN(RMJT_S_TARGET) + u32_len(e.target) + RMJT_LEN(RMJT_S_TYPE_Q) +
                (uint8_t)RMJT_TAB(meld_names)[e.type - RMJ_EV_CHI].s[0] + RMJT_LEN(RMJT_S_QBRACE);
            break;
        case RMJ_EV_ANKAN:
        case RMJ_EV_KAKAN:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_CONSUMED) + tiles_len<4>(e.consumed, evt_ncons(e)) + RMJT_LEN(RMJT_S_PAI) +
                tile_len(e.tile) + RMJT_LEN(RMJT_S_PAI_TYPE_Q) + (uint8_t)RMJT_TAB(meld_names)[e.type - RMJ_EV_CHI].s[0] + RMJT_LEN(RMJT_S_QBRACE);
            break;
        case RMJ_EV_KITA:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_PAI) + tile_len(e.tile) + RMJT_LEN(RMJT_S_KITA_END);
            break;
        case RMJ_EV_DORA: n = RMJT_LEN(RMJT_S_DORA) + tile_len(e.tile) + RMJT_LEN(RMJT_S_DORA_END); break;
        case RMJ_EV_HORA:
            n = RMJT_LEN(RMJT_S_ACTOR) + u32_len(e.actor) + RMJT_LEN(RMJT_S_DELTAS_A) + ints_len(e.deltas, np) + RMJT_LEN(RMJT_S_HORA_TARGET) +
                u32_len(e.target) + ((e.flags & 1) ? RMJT_LEN(RMJT_S_TSUMO_TRUE) : 0u) + RMJT_LEN(RMJT_S_HORA_URA) + tiles_len<5>(e.ura, evt_nura(e)) + 1u;
            break;
        case RMJ_EV_RYUKYOKU:
            n = RMJT_LEN(RMJT_S_DELTAS_R) + ints_len(e.deltas, np) + RMJT_LEN(RMJT_S_REASON) +
                (e.flags < 7 ? (uint8_t)RMJT_TAB(reasons)[e.flags].s[0] : RMJT_LEN(RMJT_S_ILLEGAL) + u32_len(e.actor)) + RMJT_LEN(RMJT_S_RYUKYOKU_END);
            break;
        default: return RMJT_STOP;
    }
    return (int32_t)(n + 1u);   // + '\n'
}

// The text of a record whose evt_len is > 0 (same arguments), '\n' included.
template <class O> RMJT_FN void evt_write(O& o, const RmjEvent& e, const RmjEvent* t1, const RmjEvent* t2, int seat) {
    const int np = evt_np(e);
    switch (e.type) {
        case RMJ_EV_START_GAME: RMJT_PUT(o, RMJT_S_START_GAME); break;
        case RMJ_EV_END_KYOKU: RMJT_PUT(o, RMJT_S_END_KYOKU); break;
        case RMJ_EV_END_GAME: RMJT_PUT(o, RMJT_S_END_GAME); break;
        case RMJ_EV_START_KYOKU: {
            RMJT_PUT(o, RMJT_S_SK_BAKAZE);
            o.put("ESWN"[e.consumed[0] & 3]);
            RMJT_PUT(o, RMJT_S_SK_DORA); put_tile(o, e.tile);
            RMJT_PUT(o, RMJT_S_SK_HONBA); put_u32(o, e.consumed[1]);
            RMJT_PUT(o, RMJT_S_SK_KYOKU); put_u32(o, e.target);
            RMJT_PUT(o, RMJT_S_SK_KYOTAKU); put_u32(o, e.consumed[2] | ((uint32_t)e.consumed[3] << 8));
            RMJT_PUT(o, RMJT_S_SK_OYA); put_u32(o, e.actor);
            RMJT_PUT(o, RMJT_S_SK_SCORES); put_ints(o, e.deltas, np);
            RMJT_PUT(o, RMJT_S_SK_TEHAIS);
            for (int p = 0; p < 4; p++) {
                if (p >= np) break;
                if (p) o.put(',');
                if (seat_sees(seat, p)) put_tiles<13>(o, tehai_of(t1, t2, p), 13);
                else RMJT_PUT(o, RMJT_S_MASKED13);
            }
            RMJT_PUT(o, RMJT_S_SK_END);
            break;
        }
        case RMJ_EV_TSUMO:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_PAI);
            if (seat_sees(seat, e.actor)) put_tile(o, e.tile);
            else o.put('?');
            RMJT_PUT(o, RMJT_S_TSUMO_END);
            break;
        case RMJ_EV_DAHAI:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_PAI); put_tile(o, e.tile); RMJT_PUT(o, RMJT_S_TSUMOGIRI);
            if (e.flags & 1) RMJT_PUT(o, "true");
            else RMJT_PUT(o, "false");
            RMJT_PUT(o, RMJT_S_DAHAI_END);
            break;
        case RMJ_EV_REACH: RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_REACH_END); break;
        case RMJ_EV_REACH_ACCEPTED: RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_REACH_ACC_END); break;
        case RMJ_EV_CHI:
        case RMJ_EV_PON:
        case RMJ_EV_DAIMINKAN:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_CONSUMED); put_tiles<4>(o, e.consumed, evt_ncons(e));
            RMJT_PUT(o, RMJT_S_PAI); put_tile(o, e.tile); RMJT_PUT(o, RMJT_S_TARGET); put_u32(o, e.target); RMJT_PUT(o, RMJT_S_TYPE_Q);
            put_str(o, RMJT_TAB(meld_names)[e.type - RMJ_EV_CHI]); RMJT_PUT(o, RMJT_S_QBRACE);
            break;
        case RMJ_EV_ANKAN:
        case RMJ_EV_KAKAN:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_CONSUMED); put_tiles<4>(o, e.consumed, evt_ncons(e));
            RMJT_PUT(o, RMJT_S_PAI); put_tile(o, e.tile); RMJT_PUT(o, RMJT_S_PAI_TYPE_Q); put_str(o, RMJT_TAB(meld_names)[e.type - RMJ_EV_CHI]);
            RMJT_PUT(o, RMJT_S_QBRACE);
            break;
        case RMJ_EV_KITA:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_PAI); put_tile(o, e.tile); RMJT_PUT(o, RMJT_S_KITA_END);
            break;
        case RMJ_EV_DORA: RMJT_PUT(o, RMJT_S_DORA); put_tile(o, e.tile); RMJT_PUT(o, RMJT_S_DORA_END); break;
        case RMJ_EV_HORA:
            RMJT_PUT(o, RMJT_S_ACTOR); put_u32(o, e.actor); RMJT_PUT(o, RMJT_S_DELTAS_A); put_ints(o, e.deltas, np);
            RMJT_PUT(o, RMJT_S_HORA_TARGET); put_u32(o, e.target);
            if (e.flags & 1) RMJT_PUT(o, RMJT_S_TSUMO_TRUE);
            RMJT_PUT(o, RMJT_S_HORA_URA); put_tiles<5>(o, e.ura, evt_nura(e)); o.put('}');
            break;
        case RMJ_EV_RYUKYOKU:
            RMJT_PUT(o, RMJT_S_DELTAS_R); put_ints(o, e.deltas, np); RMJT_PUT(o, RMJT_S_REASON);
            if (e.flags < 7) put_str(o, RMJT_TAB(reasons)[e.flags]);
            else { RMJT_PUT(o, RMJT_S_ILLEGAL); put_u32(o, e.actor); }
            RMJT_PUT(o, RMJT_S_RYUKYOKU_END);
            break;
        default: return;
    }
    o.put('\n');
}

// evt_len of record k of a contiguous window w[0 .. n)
RMJT_FN int32_t evt_len_at(const RmjEvent* w, uint32_t k, uint32_t n, int seat) {
    return evt_len(w[k], k + 1 < n ? &w[k + 1] : nullptr, k + 2 < n ? &w[k + 2] : nullptr, seat);
}

}  // namespace rmjt
