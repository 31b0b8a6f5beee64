// Host-only pieces of the C-ABI that touch no HIP API: state record <-> RmjStateView (rmj_peek_state / rmj_poke_state), the MJAI
// formatter of binary event records (rmj_format_event / rmj_format_events).  Plain C++17 on purpose: rmj_api.hip includes it, and so
// does the sanitizer translation unit (tests/host_san/host_san.cpp, built with -fsanitize=address,undefined by scripts/run_sanitizers.sh -
// GPU-side sanitizers do not exist on this pool, the host side of the boundary can be checked on the CPU).
//
// Reference: GameState / PlayerState (state/mod.rs:31-91, state/player.rs:6-39), MJAI strings with alphabetical keys
// (state/mod.rs:2094-2148), tile names (parser.rs:301-334).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/riichi_mi355x.h"
#include "rmj_state.h"

namespace rmjh {

// ---------------------------------------------------------------- state peek / poke
inline void to_view(const GState& S, const uint8_t* W, RmjStateView* v) {
    memset(v, 0, sizeof(*v));
    int len = (int)S.live_end - (int)S.rinshan_count;
    if (len < 0) len = 0;
    v->wall_len = (uint8_t)len;
    for (int i = 0; i < len && i < 136 && S.rinshan_count + i < RMJ_WALL_STRIDE; i++) v->wall[i] = W[S.rinshan_count + i];
    v->n_dora = S.n_dora;
    for (int i = 0; i < 5; i++) v->dora[i] = i < S.n_dora ? S.dora[i] : 0;
    v->rinshan_draw_count = S.rinshan_count;
    v->pending_kan_dora_count = S.pending_kan_dora;
    v->drawable_count = S.drawable_count;
    v->wall_seed = S.wall_seed;
    v->hand_index = S.hand_index;
    for (int p = 0; p < 4; p++) {
        const PState& P = S.p[p];
        RmjPlayerView& q = v->players[p];
        q.hand_len = P.hand_len;
        for (int i = 0; i < P.hand_len && i < 14; i++) q.hand[i] = P.hand[i];
        q.n_melds = P.n_melds;
        for (int m = 0; m < P.n_melds && m < 4; m++) {
            RmjMeldView& mv = q.melds[m];
            mv.meld_type = P.meld_type[m];
            mv.n_tiles = P.meld_type[m] >= RMJ_MELD_DAIMINKAN ? 4 : 3;
            for (int k = 0; k < mv.n_tiles; k++) mv.tiles[k] = P.meld_tiles[m][k];
            mv.opened = P.meld_type[m] != RMJ_MELD_ANKAN;
            mv.from_who = P.meld_from[m] == 0xFF ? -1 : (int8_t)P.meld_from[m];
            mv.called_tile = P.meld_called[m] == 0xFF ? -1 : (int16_t)P.meld_called[m];
        }
        q.n_discards = P.n_discards;
        for (int i = 0; i < P.n_discards && i < RMJ_MAX_DISCARDS; i++) q.discards[i] = P.discards[i];
        q.discard_from_hand_bits = P.discard_from_hand_bits;
        q.discard_is_riichi_bits = P.discard_is_riichi_bits;
        q.riichi_declaration_index = P.riichi_decl_idx == 0xFF ? -1 : (int8_t)P.riichi_decl_idx;
        q.score = P.score;
        q.score_delta = P.score_delta;
        q.riichi_declared = (P.flags & PF_RIICHI_DECLARED) != 0;
        q.riichi_stage = (P.flags & PF_RIICHI_STAGE) != 0;
        q.double_riichi_declared = (P.flags & PF_DOUBLE_RIICHI) != 0;
        q.missed_agari_riichi = (P.flags & PF_MISSED_RIICHI) != 0;
        q.missed_agari_doujun = (P.flags & PF_MISSED_DOUJUN) != 0;
        q.nagashi_eligible = (P.flags & PF_NAGASHI) != 0;
        q.ippatsu_cycle = (P.flags & PF_IPPATSU) != 0;
        q.pao_daisangen = P.pao37 == 0xFF ? -1 : (int8_t)P.pao37;
        q.pao_daisuushi = P.pao50 == 0xFF ? -1 : (int8_t)P.pao50;
        q.n_forbidden = P.n_forbidden;
        for (int i = 0; i < P.n_forbidden && i < 2; i++) q.forbidden[i] = P.forbidden[i];
        q.riichi_sutehai = P.riichi_sutehai == 0xFF ? -1 : (int16_t)P.riichi_sutehai;
        q.last_tedashi = P.last_tedashi == 0xFF ? -1 : (int16_t)P.last_tedashi;
        q.n_kita = P.n_kita;
        for (int i = 0; i < P.n_kita && i < 4; i++) q.kita[i] = P.kita[i];
    }
    v->current_player = S.current_player;
    v->is_done = S.is_done;
    v->needs_tsumo = S.needs_tsumo;
    v->phase = S.phase;
    v->active_mask = S.active_mask;
    v->turn_count = S.turn_count;
    v->riichi_sticks = S.riichi_sticks;
    v->last_discard_pid = S.last_discard_pid == 0xFF ? -1 : (int16_t)S.last_discard_pid;
    v->last_discard_tile = S.last_discard_pid == 0xFF ? -1 : (int16_t)S.last_discard_tile;
    v->pending_kan_pid = S.pending_kan_pid == 0xFF ? -1 : (int16_t)S.pending_kan_pid;
    v->pending_kan_action = S.pending_kan_pid == 0xFF ? 0 : S.pending_kan_action;
    v->oya = S.oya;
    v->honba = S.honba;
    v->kyoku_idx = S.kyoku_idx;
    v->round_wind = S.round_wind;
    v->is_rinshan_flag = S.is_rinshan;
    v->is_first_turn = S.is_first_turn;
    v->riichi_pending_acceptance = S.riichi_pending == 0xFF ? -1 : (int16_t)S.riichi_pending;
    v->drawn_tile = S.drawn_tile == 0xFF ? -1 : (int16_t)S.drawn_tile;
    v->last_error_pid = S.last_error_pid == 0xFF ? -1 : (int16_t)S.last_error_pid;
}

// The view written over a record (S, W as fetched from the device): what the reference's Python setters do (env.rs:134-622).
// Returns 0, or a message for RMJ_ERR_ARG.  Derived caches (wait cache, stale claim counts) are invalidated.
inline const char* from_view(GState& S, uint8_t* W, const RmjStateView* v) {
    S.rinshan_count = v->rinshan_draw_count;
    const int len = v->wall_len;
    if (S.rinshan_count + len > 136) return "wall too long";
    for (int p = 0; p < 4; p++) S.stale_n[p] = 0;
    for (int i = 0; i < len; i++) W[S.rinshan_count + i] = v->wall[i];
    S.live_end = (uint8_t)(S.rinshan_count + len);
    S.n_dora = v->n_dora > 5 ? 5 : v->n_dora;
    for (int i = 0; i < S.n_dora; i++) S.dora[i] = v->dora[i];
    S.pending_kan_dora = v->pending_kan_dora_count;
    S.drawable_count = v->drawable_count;
    S.hand_index = (uint32_t)v->hand_index;
    for (int p = 0; p < 4; p++) {
        const RmjPlayerView& q = v->players[p];
        if (q.hand_len > 14 || q.n_melds > 4 || q.n_discards > RMJ_MAX_DISCARDS) return "player view out of range";
    }
    for (int p = 0; p < 4; p++) {
        PState& P = S.p[p];
        const RmjPlayerView& q = v->players[p];
        P.hand_len = q.hand_len;
        for (int i = 0; i < q.hand_len; i++) P.hand[i] = q.hand[i];
        P.n_melds = q.n_melds;
        for (int m = 0; m < q.n_melds; m++) {
            const RmjMeldView& mv = q.melds[m];
            P.meld_type[m] = mv.meld_type;
            uint8_t t[4] = {0, 0, 0, 0};
            const int nt = mv.n_tiles > 4 ? 4 : mv.n_tiles;
            for (int k = 0; k < nt; k++) t[k] = mv.tiles[k];
            std::sort(t, t + nt);
            for (int k = 0; k < 4; k++) P.meld_tiles[m][k] = t[k];
            P.meld_from[m] = mv.from_who < 0 ? 0xFF : (uint8_t)mv.from_who;
            P.meld_called[m] = mv.called_tile < 0 ? 0xFF : (uint8_t)mv.called_tile;
        }
        P.n_discards = q.n_discards;
        P.discard_type_mask = 0;
        for (int i = 0; i < q.n_discards; i++) {
            P.discards[i] = q.discards[i];
            P.discard_type_mask |= 1ull << ((q.discards[i] >> 2) & 63);
        }
        P.discard_from_hand_bits = q.discard_from_hand_bits;
        P.discard_is_riichi_bits = q.discard_is_riichi_bits;
        P.riichi_decl_idx = q.riichi_declaration_index < 0 ? 0xFF : (uint8_t)q.riichi_declaration_index;
        P.score = q.score;
        P.score_delta = q.score_delta;
        P.flags = (uint8_t)((q.riichi_declared ? PF_RIICHI_DECLARED : 0) | (q.riichi_stage ? PF_RIICHI_STAGE : 0) |
                            (q.double_riichi_declared ? PF_DOUBLE_RIICHI : 0) | (q.missed_agari_riichi ? PF_MISSED_RIICHI : 0) |
                            (q.missed_agari_doujun ? PF_MISSED_DOUJUN : 0) | (q.nagashi_eligible ? PF_NAGASHI : 0) |
                            (q.ippatsu_cycle ? PF_IPPATSU : 0));
        P.pao37 = q.pao_daisangen < 0 ? 0xFF : (uint8_t)q.pao_daisangen;
        P.pao50 = q.pao_daisuushi < 0 ? 0xFF : (uint8_t)q.pao_daisuushi;
        P.n_forbidden = q.n_forbidden > 2 ? 2 : q.n_forbidden;
        for (int i = 0; i < P.n_forbidden; i++) P.forbidden[i] = q.forbidden[i];
        P.riichi_sutehai = q.riichi_sutehai < 0 ? 0xFF : (uint8_t)q.riichi_sutehai;
        P.last_tedashi = q.last_tedashi < 0 ? 0xFF : (uint8_t)q.last_tedashi;
        P.n_kita = q.n_kita > 4 ? 4 : q.n_kita;
        for (int i = 0; i < P.n_kita; i++) P.kita[i] = q.kita[i];
    }
    S.current_player = v->current_player;
    S.is_done = v->is_done;
    S.needs_tsumo = v->needs_tsumo;
    S.phase = v->phase;
    S.active_mask = v->active_mask;
    S.turn_count = v->turn_count;
    S.riichi_sticks = v->riichi_sticks;
    S.last_discard_pid = v->last_discard_pid < 0 ? 0xFF : (uint8_t)v->last_discard_pid;
    S.last_discard_tile = v->last_discard_pid < 0 ? 0 : (uint8_t)v->last_discard_tile;
    S.pending_kan_pid = v->pending_kan_pid < 0 ? 0xFF : (uint8_t)v->pending_kan_pid;
    S.pending_kan_action = v->pending_kan_pid < 0 ? 0 : v->pending_kan_action;
    S.oya = v->oya;
    S.honba = v->honba;
    S.kyoku_idx = v->kyoku_idx;
    S.round_wind = v->round_wind;
    S.is_rinshan = v->is_rinshan_flag;
    S.is_first_turn = v->is_first_turn;
    S.riichi_pending = v->riichi_pending_acceptance < 0 ? 0xFF : (uint8_t)v->riichi_pending_acceptance;
    S.drawn_tile = v->drawn_tile < 0 ? 0xFF : (uint8_t)v->drawn_tile;
    S.last_error_pid = v->last_error_pid < 0 ? 0xFF : (uint8_t)v->last_error_pid;
    return nullptr;
}

// ---------------------------------------------------------------- MJAI formatting
// Bounded appender: never writes past `end`, remembers how many bytes the text needs.
struct Out {
    char* p;
    char* end;
    uint64_t need;
    void put(char c) {
        if (p < end) *p++ = c;
        need++;
    }
    void str(const char* s) {
        while (*s) put(*s++);
    }
    void num(int64_t v) {
        char t[24];
        int n = 0;
        uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1u : (uint64_t)v;
        do { t[n++] = (char)('0' + u % 10u); u /= 10u; } while (u);
        if (v < 0) put('-');
        while (n) put(t[--n]);
    }
};
inline void put_tile(Out& o, uint8_t tid) {   // parser.rs:301-334
    if (tid == 16) { o.str("5mr"); return; }
    if (tid == 52) { o.str("5pr"); return; }
    if (tid == 88) { o.str("5sr"); return; }
    if (tid < 108) {
        static const char sc[3] = {'m', 'p', 's'};
        o.put((char)('1' + (tid % 36) / 4));
        o.put(sc[tid / 36]);
        return;
    }
    static const char* hon[7] = {"E", "S", "W", "N", "P", "F", "C"};
    const int num = (tid - 108) / 4;
    if (num < 7) { o.str(hon[num]); return; }
    o.num(num + 1);
    o.put('z');
}
inline void put_tiles(Out& o, const uint8_t* t, int n) {
    o.put('[');
    for (int i = 0; i < n; i++) {
        if (i) o.put(',');
        o.put('"');
        put_tile(o, t[i]);
        o.put('"');
    }
    o.put(']');
}
inline void put_ints(Out& o, const int32_t* v, int n) {
    o.put('[');
    for (int i = 0; i < n; i++) {
        if (i) o.put(',');
        o.num(v[i]);
    }
    o.put(']');
}
// One event (START_KYOKU consumes the two TEHAI records behind it) appended to `o` without a terminator.  Returns the records
// consumed, or a negative RMJ_ERR_*.  seat < 0: the full log string; 0..3: the seat's masked view (_push_mjai_event).
inline int format_event(Out& o, const RmjEvent* ev, uint32_t n_avail, int seat) {
    if (!ev || n_avail == 0) return RMJ_ERR_ARG;
    int used = 1;
    const RmjEvent& e = ev[0];
    int ncons = e.flags >> 4;
    if (ncons > 4) ncons = 4;
    const int np = (e.pad == 3) ? 3 : 4;  // seats, written into the pad byte by the device
    switch (e.type) {
        case RMJ_EV_START_GAME: o.str("{\"type\":\"start_game\"}"); break;
        case RMJ_EV_END_KYOKU: o.str("{\"type\":\"end_kyoku\"}"); break;
        case RMJ_EV_END_GAME: o.str("{\"type\":\"end_game\"}"); break;
        case RMJ_EV_START_KYOKU: {
            if (n_avail < 3 || ev[1].type != RMJ_EV_TEHAI || ev[2].type != RMJ_EV_TEHAI) return RMJ_ERR_ARG;
            used = 3;
            static const char* winds[4] = {"E", "S", "W", "N"};
            const uint32_t kyotaku = e.consumed[2] | ((uint32_t)e.consumed[3] << 8);
            o.str("{\"bakaze\":\""); o.str(winds[e.consumed[0] & 3]); o.str("\",\"dora_marker\":\""); put_tile(o, e.tile);
            o.str("\",\"honba\":"); o.num(e.consumed[1]); o.str(",\"kyoku\":"); o.num(e.target); o.str(",\"kyotaku\":"); o.num(kyotaku);
            o.str(",\"oya\":"); o.num(e.actor); o.str(",\"scores\":"); put_ints(o, e.deltas, np); o.str(",\"tehais\":[");
            for (int p = 0; p < np; p++) {
                const uint8_t* pl = reinterpret_cast<const uint8_t*>(&ev[1 + p / 2]) + 4 + 13 * (p & 1);
                if (p) o.put(',');
                if (seat < 0 || seat == p) put_tiles(o, pl, 13);
                else {
                    o.put('[');
                    for (int k = 0; k < 13; k++) o.str(k ? ",\"?\"" : "\"?\"");
                    o.put(']');
                }
            }
            o.str("],\"type\":\"start_kyoku\"}");
            break;
        }
        case RMJ_EV_TSUMO:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"pai\":\"");
            if (seat < 0 || seat == e.actor) put_tile(o, e.tile); else o.put('?');
            o.str("\",\"type\":\"tsumo\"}");
            break;
        case RMJ_EV_DAHAI:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"pai\":\""); put_tile(o, e.tile); o.str("\",\"tsumogiri\":");
            o.str((e.flags & 1) ? "true" : "false"); o.str(",\"type\":\"dahai\"}");
            break;
        case RMJ_EV_REACH: o.str("{\"actor\":"); o.num(e.actor); o.str(",\"type\":\"reach\"}"); break;
        case RMJ_EV_REACH_ACCEPTED: o.str("{\"actor\":"); o.num(e.actor); o.str(",\"type\":\"reach_accepted\"}"); break;
        case RMJ_EV_CHI:
        case RMJ_EV_PON:
        case RMJ_EV_DAIMINKAN:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"consumed\":"); put_tiles(o, e.consumed, ncons); o.str(",\"pai\":\""); put_tile(o, e.tile);
            o.str("\",\"target\":"); o.num(e.target); o.str(",\"type\":\"");
            o.str(e.type == RMJ_EV_CHI ? "chi" : (e.type == RMJ_EV_PON ? "pon" : "daiminkan")); o.str("\"}");
            break;
        case RMJ_EV_ANKAN:
        case RMJ_EV_KAKAN:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"consumed\":"); put_tiles(o, e.consumed, ncons); o.str(",\"pai\":\""); put_tile(o, e.tile);
            o.str("\",\"type\":\""); o.str(e.type == RMJ_EV_ANKAN ? "ankan" : "kakan"); o.str("\"}");
            break;
        case RMJ_EV_KITA:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"pai\":\""); put_tile(o, e.tile); o.str("\",\"type\":\"kita\"}");
            break;
        case RMJ_EV_DORA: o.str("{\"dora_marker\":\""); put_tile(o, e.tile); o.str("\",\"type\":\"dora\"}"); break;
        case RMJ_EV_HORA:
            o.str("{\"actor\":"); o.num(e.actor); o.str(",\"deltas\":"); put_ints(o, e.deltas, np); o.str(",\"target\":"); o.num(e.target);
            if (e.flags & 1) o.str(",\"tsumo\":true");
            o.str(",\"type\":\"hora\",\"ura_markers\":"); put_tiles(o, e.ura, e.n_ura > 5 ? 5 : e.n_ura); o.put('}');
            break;
        case RMJ_EV_RYUKYOKU: {
            static const char* reasons[7] = {"exhaustive_draw", "nagashimangan", "kyushu_kyuhai", "sufuurenta", "suukansansen", "suucha_riichi",
                                             "sanchaho"};
            o.str("{\"deltas\":"); put_ints(o, e.deltas, np); o.str(",\"reason\":\"");
            if (e.flags < 7) o.str(reasons[e.flags]);
            else { o.str("Error: Illegal Action by Player "); o.num(e.actor); }
            o.str("\",\"type\":\"ryukyoku\"}");
            break;
        }
        default: return RMJ_ERR_ARG;
    }
    return used;
}

// The records of game g are ev[offsets[g] .. offsets[g + 1]); its log = the events' strings, one per line ('\n' after each), written
// at buf + text_offsets[g].  Two passes over the games by a pool of threads: sizes, then text (a record run that starts inside a
// start_kyoku triple or ends inside one is formatted up to the last complete event).  Returns the bytes needed in all;
// the text is written only when it fits `cap`.
inline uint64_t format_events(const RmjEvent* ev, const uint32_t* offsets, uint32_t n_games, int seat, char* buf, uint64_t cap, uint64_t* text_offsets,
                              int threads) {
    if (threads <= 0) {
        threads = (int)std::thread::hardware_concurrency();
        if (threads <= 0) threads = 1;
        if (threads > 32) threads = 32;
    }
    if ((uint32_t)threads > n_games) threads = n_games ? (int)n_games : 1;
    auto one = [&](uint32_t g, char* dst, uint64_t room) -> uint64_t {
        Out o{dst, dst ? dst + room : dst, 0};
        const uint32_t lo = offsets[g], hi = offsets[g + 1];
        for (uint32_t i = lo; i < hi;) {
            if (ev[i].type == RMJ_EV_TEHAI) { i++; continue; }   // the tail of a triple whose head was lost: skipped
            const uint64_t mark = o.need;
            char* const pm = o.p;
            const int used = format_event(o, ev + i, hi - i, seat);
            if (used <= 0) { o.need = mark; o.p = pm; break; }
            o.put('\n');
            i += (uint32_t)used;
        }
        return o.need;
    };
    auto run = [&](auto&& body) {
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; t++) pool.emplace_back(body, t);
        body(0);
        for (auto& th : pool) th.join();
    };
    std::vector<uint64_t> sz(n_games);
    run([&](int t) {
        for (uint32_t g = (uint32_t)t; g < n_games; g += (uint32_t)threads) sz[g] = one(g, nullptr, 0);
    });
    uint64_t total = 0;
    for (uint32_t g = 0; g < n_games; g++) {
        text_offsets[g] = total;
        total += sz[g];
    }
    text_offsets[n_games] = total;
    if (buf && total <= cap)
        run([&](int t) {
            for (uint32_t g = (uint32_t)t; g < n_games; g += (uint32_t)threads) one(g, buf + text_offsets[g], sz[g]);
        });
    return total;
}

// ---------------------------------------------------------------- layouts of one allocation
// The arrays of a pool or of a scratch area, each named once: add() records where the array's typed pointer lives and how many bytes it
// needs and returns its offset, bytes() is the size of the allocation, bind() points every registered pointer into it.  The area behind
// an array ends at a multiple of the step (256 bytes unless the call says otherwise), where the next one begins.  Owns no memory.
struct DevLayout {
    explicit DevLayout(size_t step = 256) : step_(step) {}
    template <class T>
    size_t add(T** slot, size_t bytes) { return add(slot, bytes, step_); }
    template <class T>
    size_t add(T** slot, size_t bytes, size_t step) {
        const size_t o = total_;
        items_.push_back(Item{(void*)slot, o});
        total_ = (o + bytes + step - 1) / step * step;
        return o;
    }
    // a guard region of `guard` bytes that ends where the array begins: the array's offset (the guard's joins guards())
    template <class T>
    size_t add_guarded(T** slot, size_t bytes, size_t guard) {
        total_ = (total_ + guard + step_ - 1) / step_ * step_;
        guards_.push_back(total_ - guard);
        return add(slot, bytes);
    }
    size_t guard(size_t bytes) {   // a guard region behind the last array: its offset
        const size_t o = total_;
        guards_.push_back(o);
        total_ = (o + bytes + step_ - 1) / step_ * step_;
        return o;
    }
    size_t bytes() const { return total_; }
    const std::vector<size_t>& guards() const { return guards_; }
    void bind(void* base) const {
        for (const Item& it : items_) {
            char* p = (char*)base + it.off;
            memcpy(it.slot, &p, sizeof(p));   // (the slot is a T* of some T: written as the bytes of a pointer)
        }
    }

private:
    struct Item { void* slot; size_t off; };
    std::vector<Item> items_;
    std::vector<size_t> guards_;
    size_t total_ = 0, step_;
};

// ---------------------------------------------------------------- device-policy rollouts: what a handle is tuned to, how one runs
// smallest batch that a multi-step device rollout splits over several streams of a handle (rmj_step_random)
#define RMJ_SPLIT_MIN_GAMES 16384u
#define RMJ_SPLIT_MIN_PART 8192u   // games per part at least
#define RMJ_MAX_ROLLOUT_STREAMS 8
// games per wave by batch size (STEP_F_ROWS_SHIFT; profiles/r04_rows_sweep.txt, fused 4p-red-single rollouts, M env.step/s at 4 | 2 | 1 games
// per wave: 2 048 games 226 | 254 | 278, 4 096: 435 | 478 | 456, 8 192: 814 | 770 | 522, 16 384: 1 288 | 882 | 599; round 5, profiles/r05_rows_sweep.txt:
// 2 048: 236 | 272 | 301, 3 072: 345 | 373 | 416, 4 096: 455 | 505 | 492, 6 144: 632 | 692 | 589, 8 192: 845 | 823 | 567)
#define RMJ_ROWS1_MAX_GAMES 3584u
#define RMJ_ROWS2_MAX_GAMES 7168u
inline uint32_t rows_for_batch(uint32_t n_games) { return n_games <= RMJ_ROWS1_MAX_GAMES ? 1u : (n_games <= RMJ_ROWS2_MAX_GAMES ? 2u : 4u); }
// the step flags that tell a four-games-per-wave kernel its games per wave (bit position: STEP_F_ROWS_SHIFT of the step kernels)
constexpr uint32_t kStepRowsShift = 20;
inline uint32_t rows_flag_bits(uint32_t rows) { return (rows == 4u ? 0u : rows) << kStepRowsShift; }
// Is the per-step launch over games [g0, g1) of a batch one that may run in heavy-first order (HeavyOrder)?  Whole-batch launches of
// at least 2 048 units (waves) only.
inline bool heavy_first_eligible(uint32_t n_games, uint32_t rows, uint32_t g0, uint32_t g1) {
    return g0 == 0u && g1 == n_games && (g1 - g0 + rows - 1u) / rows >= 2048u;
}

// What rmj_create reads from the environment (and rmj_set_rollout_streams sets): a clone takes its source's with one assignment.
struct RolloutTuning {
    int want_streams = 4;      // parts a multi-step device rollout is cut into (rmj_set_rollout_streams; RMJ_STEP_STREAMS at create)
    int quad = 2;              // device-policy steps: 0 = one game per wave (k_step), 1 = four games per wave (k_step4), 2 = and a
                               // rollout of >= 2 steps is ONE launch in which every wave steps its own games (k_step4<true>); RMJ_STEP4 at create
    // long fused rollouts hand the work out in (quad, chunk) tickets to a grid that fits the chip once (k_step4_queue)
    int queue_chunk = 32;      // calls per ticket (round 5: a ticket is a number of calls of the step function, profiles/r05_ticket_schedule_sweep.txt); RMJ_QUEUE_CHUNK at create, 0 = off (every wave keeps one quad for the rollout)
    int queue_force = 0;       // RMJ_QUEUE_FORCE at create (tests): tickets for every batch of >= 64 quads
    int queue_min_chunk = 5;   // shortest ticket (steps): a rollout of >= 2 tickets per quad runs as tickets; RMJ_QUEUE_MIN_CHUNK at create
    int queue_tail = 0;        // ticket lengths descend towards the expected end of a quad's rollout (q_ticket_plan); RMJ_QUEUE_TAIL=0: equal tickets
    uint32_t queue_skip_xcds = 0;   // test hook: XCDs whose waves leave the queue kernel at once (RMJ_QUEUE_TEST_SKIP_XCDS at create)
    uint32_t rows_pw = 4;      // games per wave of the non-ticket four-games-per-wave kernels: 4, or 2 / 1 for batches that leave the chip
                               // latency bound (chosen at create from the batch size; RMJ_ROWS overrides)
    int heavy_first = 1;       // RMJ_HEAVY_FIRST at create (0: plain block order)
    int enc_fused = 1;         // RMJ_ENC_FUSED at create: the step + encode rollout as ONE launch (k_step4_enc / k_step4_queue_enc); 0 = parts on streams
};

// How one device-policy rollout runs, decided once (rollout_plan): the entry point executes it, the timers report from it.
struct RolloutPlan {
    enum How { PER_STEP, FUSED, TICKETS };
    How how = PER_STEP;        // one launch per step on k streams | ONE launch (k_step4<true> / k_step4_enc) | one launch handed out as tickets + its fix-up
    bool need_slots = false;   // every condition for tickets that does not ask for the ticket kernel's resident waves holds, and they
                               // are unknown: the caller asks the runtime and plans again (what stands here is the rollout without them)
    int pol = 0;               // 0 = RandomAgent, 1 = the greedy policy: the instantiation of the step kernels
    int k = 1;                 // streams of a per-step rollout; part i of the batch is games [part(i), part(i + 1))
    uint32_t n_games = 0;
    uint32_t rows = 4, row_flags = 0;   // games per wave of the k_step4 launches (fused and per step) and the flag bits that say so
    uint32_t chunk = 0;        // steps per ticket
    uint32_t grid_tickets = 0, grid_fixup = 0, grid_plain = 0;   // blocks of the ticket launch (0 unless TICKETS), its fix-up, the fused launch
    bool heavy = false;        // per step: the launches cover the whole batch and may run in heavy-first order
    uint32_t launches = 0, launches_in_flight = 0, queued = 0;   // what RmjBenchResult reports of the rollout
    uint32_t part(int i) const { return (uint32_t)((uint64_t)n_games * i / k); }
};
// pol: 1 = greedy (step rollout only); encode: the step + encode rollout (rmj_step_random_encode) with its only_active; slots: waves of
// the rollout's ticket kernel the device holds at once, 0 = not known; max_xcc_id: the largest XCC id the device reported at create.
inline RolloutPlan rollout_plan(const RolloutTuning& t, uint32_t n_games, uint32_t n_steps, int pol, bool encode, int only_active, uint32_t slots,
                                uint32_t max_xcc_id) {
    RolloutPlan p;
    p.pol = !encode && pol == 1 ? 1 : 0;
    p.n_games = n_games;
    p.rows = t.rows_pw;
    p.row_flags = rows_flag_bits(t.rows_pw);
    const uint32_t quads = (n_games + 3u) / 4u;
    {   // steps per ticket: the configured chunk, shorter for a short rollout (its tail is one chunk long: at least 16 chunks per quad)
        uint32_t cap = (uint32_t)t.queue_chunk;
        const uint32_t lo = (uint32_t)t.queue_min_chunk, fine = n_steps / 16u < lo ? lo : n_steps / 16u;
        if (cap < (n_steps + 39u) / 40u) cap = (n_steps + 39u) / 40u;   // at most 64 tickets per quad (q_ticket_plan)
        p.chunk = fine < cap ? fine : cap;
    }
    p.grid_plain = encode ? quads : (n_games + p.rows - 1u) / p.rows;
    p.grid_fixup = encode ? quads : (quads + 63u) / 64u;   // (k_step4_fixup looks at 64 quads per wave, k_step4_fixup_enc at one)
    // (rmj_set_rollout_streams(h, 1): one launch per step, one stream)
    if (t.quad >= 2 && n_steps >= 2 && t.want_streams >= 2 && (!encode || (t.enc_fused && only_active == 2))) {
        p.how = RolloutPlan::FUSED;
        // Tickets are worth it when the batch is more than one and fewer than eight chip-fulls of waves: below, every quad is resident
        // at once and there is no tail; far above, the tail is a small share and the chunk hand-overs cost more than it (524 288
        // games: -2 %).  Never with more XCC ids than queues: no single L2 per queue (see rmj_create).
        // RMJ_QUEUE_FORCE=1 (tests): any batch with a quad per XCD queue to spare.
        const bool wanted = t.queue_chunk > 0 && n_steps >= 2u * p.chunk && max_xcc_id <= 7u && (!t.queue_force || quads >= 64u);
        p.need_slots = wanted && slots == 0u;
        if (wanted && slots != 0u && (t.queue_force || (quads > slots && quads < 8u * slots))) {
            p.how = RolloutPlan::TICKETS;
            p.grid_tickets = quads < slots ? quads : slots;
        }
    } else if (t.want_streams >= 2 && n_steps >= 2 && n_games >= RMJ_SPLIT_MIN_GAMES) {
        const int fit = (int)(n_games / RMJ_SPLIT_MIN_PART);
        p.k = t.want_streams > RMJ_MAX_ROLLOUT_STREAMS ? RMJ_MAX_ROLLOUT_STREAMS : t.want_streams;
        if (p.k > fit) p.k = fit;
    }
    p.heavy = p.how == RolloutPlan::PER_STEP && t.quad && t.heavy_first && heavy_first_eligible(n_games, p.rows, p.part(0), p.part(1));
    // the step + encode rollout reports a step and an encode launch per step and one launch in flight, on its split path too
    p.launches = p.how != RolloutPlan::PER_STEP ? 1u : (encode ? 2u * n_steps : n_steps * (uint32_t)p.k);
    p.launches_in_flight = encode ? 1u : (uint32_t)p.k;
    p.queued = p.how == RolloutPlan::TICKETS ? 1u : 0u;
    return p;
}

// ---------------------------------------------------------------- chains of logs in replay slots
// the assignment of logs to slots (see the head of rmj_logreplay.hip.h)
inline uint32_t lr_assign(const uint32_t* off, uint32_t M, uint32_t n, uint32_t* slot_of_log, uint32_t* slot_logs, uint32_t* slot_first) {
    std::vector<uint64_t> busy(n, 0);          // the step at which the slot is free again
    std::vector<std::vector<uint32_t>> lists(n);
    for (uint32_t l = 0; l < M; l++) {
        uint32_t best = 0;
        for (uint32_t s = 1; s < n; s++)
            if (busy[s] < busy[best]) best = s;
        busy[best] += off[l + 1] - off[l];
        lists[best].push_back(l);
        if (slot_of_log) slot_of_log[l] = best;
    }
    uint64_t steps = 0;
    uint32_t at = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (slot_first) slot_first[s] = at;
        for (uint32_t l : lists[s]) {
            if (slot_logs) slot_logs[at] = l;
            at++;
        }
        if (busy[s] > steps) steps = busy[s];
    }
    if (slot_first) slot_first[n] = at;
    return (uint32_t)steps;
}
// What a replay (sample builder, checker) keeps of its assignment on the host: slot s replays slot_logs[slot_first[s] .. slot_first[s + 1]),
// a whole replay is `steps` event steps (the longest chain's events), `step` of them are taken.
struct SlotChain {
    std::vector<uint32_t> slot_first, slot_logs;   // [n + 1], [max(M, 1)]
    uint32_t steps = 0, step = 0;
    void assign(const uint32_t* off, uint32_t M, uint32_t n) {
        slot_first.assign((size_t)n + 1, 0u);
        slot_logs.assign(M ? M : 1u, 0u);
        steps = lr_assign(off, M, n, nullptr, slot_logs.data(), slot_first.data());
        step = 0;
    }
    // where every slot starts: pos[s] = its first entry of slot_logs, cur[s] = that log's first event.  A slot may be left without a
    // log (a log of no events keeps its slot free for the next one): its cur stays 0 and slot_logs is not read at pos[s].
    void start_cursors(const uint32_t* off, uint32_t* pos, uint32_t* cur) const {
        for (size_t s = 0; s + 1 < slot_first.size(); s++) {
            pos[s] = slot_first[s];
            cur[s] = pos[s] < slot_first[s + 1] ? off[slot_logs[pos[s]]] : 0u;
        }
    }
};

}  // namespace rmjh
