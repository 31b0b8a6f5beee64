// Log validation (rmj_logcheck_*; riichienv-ml validates a public corpus one log at a time through Python, scripts/validate_logs.py): a
// checking replay of every log of a log set, which leaves for every log its FIRST finding - a code RMJ_LOGCHECK_*, the index of the
// offending event in the log, the kyoku, the seat and a detail word - and records no sample.  Included from rmj_api.hip behind
// rmj_logreplay.hip.h: the slots and their chains of logs are the sample builder's (lr_assign), the decision matching is lr_select,
// the Ron on a robbed kan is recognised by lr_robbed_kan_tile, and the event itself is applied by the variant's k_log_apply.
//
// One event index is two launches: k_log_check (one wave per slot, four slots per block) and k_log_apply.  The checking pass reads the
// event at the slot's cursor, what the last apply published for the slot's game (E.status / E.nlegal / E.legal), the game's hands
// (E.core[g]) and a few words of its own per slot: the kyoku's phase (none started / open / over), the seat due to draw, the previous
// start_kyoku's kyotaku and seen[40], the counts of the kyoku's dealt tiles, dora markers and draws by tile name.  A finding is written
// to the log's record by the one wave that walks the log (no atomics but the counters); the slot then takes its next log in the same
// launch and checks that log's first event too, from a clean start: the slot's words are reset, and the game is rewritten by the log's
// own start events before anything reads it (everything else ahead of the first start_kyoku is a finding).
//
// The lane work: hand membership is a ballot over the lanes below hand_len, the multiset test its popcount against the copies needed;
// the tile counters are lane = tile name (0..33 the types, 34..36 the red fives, lr_name).  No 64-bit value is shifted by a lane's
// amount (scripts/lint_isa_last_vgpr.py).
//
// Limits.  A second or third hora of a multiple ron is not checked against an offer (the kyoku is over when it arrives).  Settlement
// amounts are not recomputed (the records carry no ura markers).  Feature encodings are not inspected.  A masked log ("?" tiles read
// as tile 0) trips TILE_COUNT by construction.
#pragma once

enum { LC_NONE = 0, LC_OPEN = 1, LC_OVER = 2 };   // the kyoku's phase: no start_kyoku yet, started and not over, over
#define LC_NO_SEAT 0xFFu
#define LC_SEEN 40u            /* bytes of tile counts per slot (37 names) */

struct LogCheck {
    // the log set
    const RmjEvent* ev;
    const uint32_t *off, *koff;
    const uint8_t* status;            // [M] RMJ_LOGTEXT_* (NULL: a set packed from dicts)
    const uint32_t* errline;          // [M]
    const int32_t *start, *end;       // kyoku score tables: the start scores [K][4], and the end scores every kyoku's OWN events gave [K][8]
    // the assignment (lr_assign)
    const uint32_t *slot_first, *slot_logs;
    // per slot
    uint32_t *pos, *cur, *kcount;     // as in LogRun
    uint32_t* word;                   // [n] phase | seat due to draw << 8 | previous kyotaku << 16
    uint8_t* seen;                    // [n][LC_SEEN]
    uint32_t* apply_at;               // [games of the handle] the event k_log_apply applies in this step, LR_NO_EVENT = none
    // per log
    uint8_t *code, *seat;
    uint32_t *kyoku, *event, *detail;
    uint32_t* counts;                 // [16] logs per code
    uint32_t n, M, NP, sanma;
};

// the verdicts before the walk: OK everywhere, PARSE for the logs the set keeps with a text status (they are not replayed)
__global__ __launch_bounds__(256) void k_logcheck_init(LogCheck R) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= R.M) return;
    const bool bad = R.status && R.status[l] != RMJ_LOGTEXT_OK;
    R.code[l] = bad ? RMJ_LOGCHECK_PARSE : RMJ_LOGCHECK_OK;
    R.seat[l] = LC_NO_SEAT;
    R.kyoku[l] = 0u;
    R.event[l] = bad ? R.errline[l] : 0u;
    R.detail[l] = bad ? (uint32_t)R.status[l] : 0u;
    if (bad) atomicAdd(&R.counts[RMJ_LOGCHECK_PARSE], 1u);
}

// does `tile` (a 136-id) count under the tile name `name` (lane = name): its type, and the red five's own name
__device__ __forceinline__ uint32_t lc_counts_as(uint32_t name, uint32_t tile) {
    return name < 34u ? ((tile >> 2) == name ? 1u : 0u) : (tile == 16u + 36u * (name - 34u) ? 1u : 0u);
}
__device__ __forceinline__ bool lc_over_limit(uint32_t name, uint32_t cnt) { return name < 37u && cnt > (name < 34u ? 4u : 1u); }

// The checking pass of one event index (see the head of this file).  settle_only: the last call of a run - only the logs that just ended
// get their verdict.
__global__ __launch_bounds__(256) void k_log_check(Env E, LogCheck R, int settle_only) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slot >= R.n) return;
    uint32_t pos = R.pos[slot], cur = R.cur[slot], kc = R.kcount[slot];
    const uint32_t w = R.word[slot];
    uint32_t st = w & 0xFFu, due = (w >> 8) & 0xFFu, kyotaku = w >> 16;
    const uint32_t last = R.slot_first[slot + 1];
    const bool sanma = R.sanma != 0u;
    const uint32_t n = R.NP, g = slot;
    uint8_t* seen = R.seen + (size_t)slot * LC_SEEN;
    uint32_t apply = LR_NO_EVENT;
    for (;;) {
        if (pos >= last) break;
        const uint32_t log = R.slot_logs[pos];
        const uint32_t lo = R.off[log], end = R.off[log + 1];
        uint32_t code = RMJ_LOGCHECK_OK, fseat = LC_NO_SEAT, detail = 0u, fevent = cur - lo, fkyoku = kc;
        bool count_ok = false;
        if (R.code[log] != RMJ_LOGCHECK_OK) {
            // a PARSE log: its verdict stands, nothing is replayed
        } else if (cur >= end) {   // the log is over
            if (st == LC_OPEN) code = RMJ_LOGCHECK_UNFINISHED;
            else count_ok = true;
        } else if (settle_only) {
            break;
        } else {
            const RmjEvent* e = R.ev + (size_t)cur * 3;
            const uint32_t ty = e->type, actor = e->actor, a = actor & 3u;
            const bool structural = ty == RMJ_EV_START_GAME || ty == RMJ_EV_START_KYOKU || ty == RMJ_EV_END_KYOKU || ty == RMJ_EV_END_GAME || ty == RMJ_EV_NONE;
            if (st == LC_NONE && !structural) code = RMJ_LOGCHECK_NO_START_KYOKU;
            else if (st == LC_OVER && !structural && ty != RMJ_EV_HORA) code = RMJ_LOGCHECK_AFTER_END;
            else if (st == LC_OPEN && (ty == RMJ_EV_START_KYOKU || ty == RMJ_EV_START_GAME || ty == RMJ_EV_END_GAME)) code = RMJ_LOGCHECK_UNFINISHED;
            else if (!structural) {
                const bool claim = ty == RMJ_EV_CHI || ty == RMJ_EV_PON || ty == RMJ_EV_DAIMINKAN;
                const bool has_actor = ty == RMJ_EV_TSUMO || ty == RMJ_EV_DAHAI || ty == RMJ_EV_REACH || ty == RMJ_EV_REACH_ACCEPTED || claim || ty == RMJ_EV_ANKAN ||
                                       ty == RMJ_EV_KAKAN || ty == RMJ_EV_HORA || (sanma && ty == RMJ_EV_KITA);
                const bool decision = ty == RMJ_EV_DAHAI || claim || ty == RMJ_EV_ANKAN || ty == RMJ_EV_KAKAN || ty == RMJ_EV_REACH || ty == RMJ_EV_HORA || ty == RMJ_EV_KITA;
                if (has_actor || decision) fseat = actor;
                if ((has_actor && actor >= n) || (claim && ((uint32_t)e->target >= n || (uint32_t)e->target == actor))) {
                    code = RMJ_LOGCHECK_ACTOR;
                } else if (st == LC_OPEN) {   // (a hora behind the kyoku's end - a multiple ron - is not checked further)
                    const uint32_t stw = E.status[g];
                    const bool done = ((stw >> 16) & 0xFFu) != 0u;
                    const uint32_t am = done ? 0u : (stw & 0xFu);
                    const uint32_t cnt = (*reinterpret_cast<const uint32_t*>(E.nlegal + (size_t)g * 4) >> (8u * a)) & 0xFFu;
                    const bool listed = ((am >> a) & 1u) != 0u;
                    const bool robbed = ty == RMJ_EV_HORA && !done && !listed && lr_robbed_kan_tile(R.ev, lo, cur, e) != RMJ_TILE_NONE;
                    if (ty == RMJ_EV_TSUMO && actor != due) {
                        code = RMJ_LOGCHECK_DRAW_OUT_OF_TURN;
                    } else if (decision && !(listed && cnt) && !robbed) {
                        code = RMJ_LOGCHECK_NOT_OFFERED;
                    } else {
                        // the tiles the event takes from the actor's concealed hand, as a multiset of ids
                        const uint32_t en = (uint32_t)(e->flags >> 4) & 15u;
                        uint32_t need = 0u;
                        if (ty == RMJ_EV_DAHAI || ty == RMJ_EV_KAKAN) need = 1u;
                        else if (ty == RMJ_EV_CHI || ty == RMJ_EV_PON) need = min(en, 2u);
                        else if (ty == RMJ_EV_DAIMINKAN) need = min(en, 3u);
                        else if (ty == RMJ_EV_ANKAN) need = min(en, 4u);
                        if (need) {
                            const PState& P = E.core[g].p[a];
                            const uint32_t hl = min((uint32_t)P.hand_len, 14u);
                            const uint32_t mine = (uint32_t)lane < hl ? (uint32_t)P.hand[lane] : 0x100u;
                            const bool own = ty == RMJ_EV_DAHAI || ty == RMJ_EV_KAKAN;
                            for (uint32_t i = 0; i < need && code == RMJ_LOGCHECK_OK; i++) {
                                const uint32_t t = own ? (uint32_t)e->tile : (uint32_t)e->consumed[i];
                                uint32_t copies = 0u;
                                for (uint32_t j = 0; j < need; j++) copies += (own ? (uint32_t)e->tile : (uint32_t)e->consumed[j]) == t ? 1u : 0u;
                                if ((uint32_t)__popcll(__ballot(mine == t)) < copies) { code = RMJ_LOGCHECK_TILE_NOT_HELD; detail = t; }
                            }
                        }
                        if (code == RMJ_LOGCHECK_OK && (ty == RMJ_EV_TSUMO || ty == RMJ_EV_DORA)) {
                            const uint32_t cnt1 = ((uint32_t)lane < 37u ? (uint32_t)seen[lane] : 0u) + lc_counts_as((uint32_t)lane, e->tile);
                            if ((uint32_t)lane < 37u) seen[lane] = (uint8_t)min(cnt1, 255u);
                            if (__ballot(lc_over_limit((uint32_t)lane, cnt1))) { code = RMJ_LOGCHECK_TILE_COUNT; detail = e->tile; }
                        }
                        if (code == RMJ_LOGCHECK_OK && decision && !robbed) {
                            const uint32_t drawn = ty == RMJ_EV_DAHAI ? (uint32_t)E.core[g].drawn_tile : (uint32_t)RMJ_TILE_NONE;
                            const uint64_t* lg = E.legal + ((size_t)g * 4 + a) * RMJ_MAX_LEGAL;
                            if (lr_select(lg, cnt, e, false, drawn, sanma, lane) == RMJ_NO_ACTION) code = RMJ_LOGCHECK_NO_LEGAL_MATCH;
                        }
                    }
                }
            } else if (ty == RMJ_EV_START_KYOKU) {
                fkyoku = kc + 1u;
                // the dealt tiles (two TEHAI records of 26: seats 0 1, seats 2 3) and the dora marker, counted by name
                const uint8_t *h0 = reinterpret_cast<const uint8_t*>(e + 1) + 4, *h1 = reinterpret_cast<const uint8_t*>(e + 2) + 4;
                uint32_t c = lc_counts_as((uint32_t)lane, e->tile);
                for (uint32_t i = 0; i < 26u; i++) c += lc_counts_as((uint32_t)lane, h0[i]);
                for (uint32_t i = 0; i < (n == 3u ? 13u : 26u); i++) c += lc_counts_as((uint32_t)lane, h1[i]);
                if ((uint32_t)lane < 37u) seen[lane] = (uint8_t)c;
                const uint64_t over = __ballot(lc_over_limit((uint32_t)lane, c));
                const uint32_t krow = R.koff[log] + kc;
                if (actor >= n) {   // (the record's actor is the oya)
                    code = RMJ_LOGCHECK_ACTOR;
                } else if (over) {
                    const uint32_t name = (uint32_t)__ffsll((long long)over) - 1u;
                    code = RMJ_LOGCHECK_TILE_COUNT;
                    detail = name < 34u ? name * 4u : 16u + 36u * (name - 34u);
                } else if (kc && R.start && krow < R.koff[log + 1]) {   // the scores between kyoku kc and kyoku kc + 1
                    // (R.end: what kyoku kc's own events gave, in both readings of a ryukyoku's deltas; the tables' end column IS the next
                    // start, so the sum over it is taken from the starts)
                    const int32_t *pe = R.end + (size_t)(krow - 1u) * 8, *ps = R.start + (size_t)(krow - 1u) * 4, *pn = R.start + (size_t)krow * 4;
                    const uint64_t differ = __ballot((uint32_t)lane < n && pe[lane & 3] != pn[lane & 3]);
                    const uint64_t differ2 = __ballot((uint32_t)lane < n && pe[4 + (lane & 3)] != pn[lane & 3]);
                    int64_t moved = 0;
                    for (uint32_t s = 0; s < n; s++) moved += (int64_t)pn[s] - (int64_t)ps[s];
                    const uint32_t now = (uint32_t)e->consumed[2] | ((uint32_t)e->consumed[3] << 8);
                    if (differ && differ2) { code = RMJ_LOGCHECK_SCORE_CONTINUITY; fseat = (uint32_t)__ffsll((long long)differ) - 1u; }
                    else if (moved != -1000ll * ((int64_t)now - (int64_t)kyotaku)) { code = RMJ_LOGCHECK_SCORE_CONSERVATION; detail = (uint32_t)(int32_t)moved; }
                }
            }
            if (code == RMJ_LOGCHECK_OK) { apply = cur; break; }
        }
        // the log is left: with a finding, at its end, or because it was never to be replayed
        if (lane == 0) {
            if (code != RMJ_LOGCHECK_OK) {
                R.code[log] = (uint8_t)code; R.seat[log] = (uint8_t)fseat; R.kyoku[log] = fkyoku; R.event[log] = fevent; R.detail[log] = detail;
                atomicAdd(&R.counts[code], 1u);
            } else if (count_ok) {
                atomicAdd(&R.counts[RMJ_LOGCHECK_OK], 1u);
            }
        }
        pos++;
        if (pos < last) cur = R.off[R.slot_logs[pos]];
        kc = 0u; st = LC_NONE; due = LC_NO_SEAT; kyotaku = 0u;
    }
    if (apply != LR_NO_EVENT) {   // what the event means for the next check
        const RmjEvent* e = R.ev + (size_t)apply * 3;
        const uint32_t ty = e->type, actor = e->actor;
        if (ty == RMJ_EV_START_KYOKU) {
            kc++; st = LC_OPEN; due = actor;   // (the record's actor is the oya)
            kyotaku = (uint32_t)e->consumed[2] | ((uint32_t)e->consumed[3] << 8);
        } else if (ty == RMJ_EV_HORA || ty == RMJ_EV_RYUKYOKU || ty == RMJ_EV_END_KYOKU) {
            if (st == LC_OPEN) st = LC_OVER;
        } else if (ty == RMJ_EV_DAHAI) {
            due = (actor + 1u) % n;
        } else if (ty == RMJ_EV_DAIMINKAN || ty == RMJ_EV_ANKAN || ty == RMJ_EV_KAKAN || (sanma && ty == RMJ_EV_KITA)) {
            due = actor;
        } else if (ty == RMJ_EV_TSUMO || ty == RMJ_EV_CHI || ty == RMJ_EV_PON) {
            due = LC_NO_SEAT;
        }
        cur++;
    }
    if (lane == 0) {
        R.pos[slot] = pos; R.cur[slot] = cur; R.kcount[slot] = kc;
        R.word[slot] = st | (due << 8) | (kyotaku << 16);
        R.apply_at[slot] = settle_only ? LR_NO_EVENT : apply;
    }
}
