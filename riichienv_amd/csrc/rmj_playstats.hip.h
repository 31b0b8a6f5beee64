// Play statistics of every (kyoku, seat) of a log set (rmj_logset_playstats_device): int32 rows[n_kyokus][4][RMJ_PLAYSTAT_COLUMNS], the
// columns RMJ_PLAYSTAT_* of include/riichi_mi355x.h, in table order kyoku_offsets[log] + kyoku - 1.
//
//   k_playstats   one wave per log, 64 events per pass, a lane per event: type and actor from the first four bytes of the event's first
//                 record, flags from byte 24 - nothing else is read.  An event whose actor is no seat (>= n) reads as NONE; a START_KYOKU
//                 carries its oya there and always counts.
//
//                 The accumulator is the wave: lane seat * 16 + column holds one word of the open kyoku's row, so a kyoku is flushed with one
//                 coalesced 256-byte store, without atomics and without a zeroing pass.  Per pass one ballot per event kind and one per
//                 seat; a count column of seat s is popcount(kind & seat[s] & segment), the segment being the lanes of the pass that belong
//                 to the open kyoku.  A pass may hold many START_KYOKU records: the segments are walked in a wave-uniform loop that flushes,
//                 resets and reopens at every boundary.
//
//                 RIICHI_TURN / WIN_TURN: the seat's DAHAI ballot below its first REACH / HORA of the segment, plus the seat's discards
//                 carried from earlier passes; a flag per seat keeps only the first.
//                 Tsumo wins and deal-ins: every HORA lane takes the highest set bit of the tile-event ballot (TSUMO DAHAI KAKAN ANKAN KITA)
//                 below itself and inside its own kyoku, and reads that lane's (type, actor) with one shuffle; a hora in the pass's first
//                 segment with no such lane takes the (kind, actor) carried from earlier passes.  All carries reset at a START_KYOKU.
//
//                 Lane masks are built from 32-bit halves and segment masks in scalar registers: no 64-bit shift by a vector register
//                 (scripts/lint_isa_last_vgpr.py).  Rows are written only below koff[l + 1], whatever the stream holds; every row of a log
//                 whose status is not OK is -1 in all 64 words.
#pragma once

namespace rmjstat {

constexpr uint32_t PS_BLOCK = 256;

// the lanes below `lane`, without a 64-bit vector shift
__device__ __forceinline__ uint64_t ps_below(uint32_t lane) {
    const uint32_t lo = lane >= 32u ? 0xFFFFFFFFu : (1u << lane) - 1u;
    const uint32_t hi = lane > 32u ? (1u << (lane - 32u)) - 1u : 0u;
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t ps_top(uint64_t m) { return 63u - (uint32_t)__clzll((long long)m); }   // m != 0
__device__ __forceinline__ uint32_t ps_low(uint64_t m) { return (uint32_t)__ffsll((long long)m) - 1u; }   // m != 0

__global__ __launch_bounds__(PS_BLOCK) void k_playstats(const RmjEvent* __restrict__ ev, const uint32_t* __restrict__ off, const uint32_t* __restrict__ koff, uint32_t M,
                                                        const uint8_t* __restrict__ status, uint32_t n, int32_t* __restrict__ rows) {
    const uint32_t lane = threadIdx.x & 63u, l = blockIdx.x * (PS_BLOCK / 64u) + (threadIdx.x >> 6);
    if (l >= M) return;   // wave-uniform: a wave is one log
    const uint32_t e0 = off[l], e1 = off[l + 1], r0 = koff[l], r1 = koff[l + 1];
    if (r0 >= r1) return;   // a log without a kyoku has no row
    if (status && status[l] != RMJ_LOGTEXT_OK) {
        for (uint32_t r = r0; r < r1; r++) rows[(size_t)r * 64u + lane] = -1;
        return;
    }
    const uint32_t seat = lane >> 4, col = lane & 15u;
    int32_t acc = 0;
    uint32_t row = r0;
    bool open = false;                       // a START_KYOKU has been seen: acc is the row `row`
    uint32_t dc[4] = {0u, 0u, 0u, 0u};       // the seat's DAHAI events of the open kyoku so far
    uint32_t reached = 0u, won = 0u;         // bit s: seat s has its RIICHI_TURN / WIN_TURN
    uint32_t last_kind = 0u, last_actor = 0u;   // the last tile event of the open kyoku: 0 none, 1 a TSUMO, 2 another tile event
    for (uint32_t i0 = e0; i0 < e1; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint32_t w0 = 0u, w6 = 0u;
        if (i < e1) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(ev + (size_t)i * 3u);
            w0 = p[0];   // type actor target tile
            w6 = p[6];   // flags n_ura ura[0..1]
        }
        uint32_t ty = w0 & 0xFFu;
        const uint32_t actor = (w0 >> 8) & 0xFFu;
        if (ty != (uint32_t)RMJ_EV_START_KYOKU && actor >= n) ty = RMJ_EV_NONE;
        const bool is_hora = ty == RMJ_EV_HORA, is_dahai = ty == RMJ_EV_DAHAI, is_tsumo = ty == RMJ_EV_TSUMO;
        const bool is_tile = is_tsumo || is_dahai || ty == RMJ_EV_KAKAN || ty == RMJ_EV_ANKAN || ty == RMJ_EV_KITA;
        const uint64_t SK = __ballot(ty == RMJ_EV_START_KYOKU), T = __ballot(is_tile);
        // the last tile event before this lane inside its own kyoku
        const uint64_t lt = ps_below(lane), sb = SK & lt;
        const bool first_seg = sb == 0ull;   // no START_KYOKU of this pass lies below: the carries of earlier passes hold
        const uint64_t tb = T & lt & ~(first_seg ? 0ull : ps_below(ps_top(sb)));
        const uint32_t src = tb ? ps_top(tb) : lane;
        const uint32_t lw = (uint32_t)__shfl((int)(is_tsumo ? 1u | (actor << 8) : 2u | (actor << 8)), (int)src);   // every lane takes part
        uint32_t lkind = 0u, lactor = 0u;
        if (tb) {
            lkind = lw & 0xFFu;
            lactor = lw >> 8;
        } else if (first_seg) {
            lkind = last_kind;
            lactor = last_actor;
        }
        const bool tsumo_win = is_hora && lkind == 1u && lactor == actor;
        const bool deal_in = is_hora && lkind != 0u && lactor != actor;
        // ballots: per seat, per kind
        uint64_t A[4], DI[4], D[4];
#pragma unroll
        for (uint32_t s = 0; s < 4u; s++) {
            A[s] = __ballot(ty != RMJ_EV_NONE && actor == s);
            DI[s] = __ballot(deal_in && lactor == s);
        }
        const uint64_t H = __ballot(is_hora), HT = __ballot(tsumo_win), RY = __ballot(ty == RMJ_EV_RYUKYOKU), R = __ballot(ty == RMJ_EV_REACH),
                       RA = __ballot(ty == RMJ_EV_REACH_ACCEPTED), CH = __ballot(ty == RMJ_EV_CHI), PO = __ballot(ty == RMJ_EV_PON),
                       DK = __ballot(ty == RMJ_EV_DAIMINKAN), AK = __ballot(ty == RMJ_EV_ANKAN), KK = __ballot(ty == RMJ_EV_KAKAN),
                       KI = __ballot(ty == RMJ_EV_KITA), DA = __ballot(is_dahai), DT = __ballot(is_dahai && (w6 & 1u)), TS = __ballot(is_tsumo);
#pragma unroll
        for (uint32_t s = 0; s < 4u; s++) D[s] = DA & A[s];
        // this lane's count column: popcount(X & Y & segment)
        const uint64_t As = seat == 0u ? A[0] : seat == 1u ? A[1] : seat == 2u ? A[2] : A[3];
        const uint64_t DIs = seat == 0u ? DI[0] : seat == 1u ? DI[1] : seat == 2u ? DI[2] : DI[3];
        uint64_t X = As, Y = 0ull;
        switch (col) {
            case RMJ_PLAYSTAT_WIN: Y = H; break;
            case RMJ_PLAYSTAT_WIN_TSUMO: Y = HT; break;
            case RMJ_PLAYSTAT_DEAL_IN: X = DIs; Y = ~0ull; break;
            case RMJ_PLAYSTAT_RIICHI: Y = R; break;
            case RMJ_PLAYSTAT_RIICHI_ACCEPTED: Y = RA; break;
            case RMJ_PLAYSTAT_CALLS: Y = CH | PO | DK; break;
            case RMJ_PLAYSTAT_CHI: Y = CH; break;
            case RMJ_PLAYSTAT_PON: Y = PO; break;
            case RMJ_PLAYSTAT_KANS: Y = DK | AK | KK; break;
            case RMJ_PLAYSTAT_KITA: Y = KI; break;
            case RMJ_PLAYSTAT_DISCARDS: Y = DA; break;
            case RMJ_PLAYSTAT_TSUMOGIRI: Y = DT; break;
            default: break;   // RIICHI_TURN, WIN_TURN, DEALER, END: set below
        }
        X &= Y;
        // the segments of the pass (wave-uniform): the lanes below the first START_KYOKU continue the open kyoku, every START_KYOKU flushes
        // it and opens the next
        uint64_t sk = SK, done = 0ull;   // done: the lanes of earlier segments
        for (;;) {
            const uint32_t j = sk ? ps_low(sk) : 64u;                            // the boundary that ends this segment
            const uint64_t seg = (j < 64u ? (1ull << j) - 1ull : ~0ull) & ~done;   // scalar shifts: j is uniform
            if (open) {
                acc += (int32_t)__popcll(X & seg);
                if (col == RMJ_PLAYSTAT_END && seat < n) acc |= ((H & seg) ? 1 : 0) | ((RY & seg) ? 2 : 0);
#pragma unroll
                for (uint32_t s = 0; s < 4u; s++) {
                    const uint64_t d = D[s] & seg, r = R & A[s] & seg, h = H & A[s] & seg;
                    if (r && !((reached >> s) & 1u)) {
                        reached |= 1u << s;
                        const uint32_t v = 1u + dc[s] + (uint32_t)__popcll(d & ((1ull << ps_low(r)) - 1ull));
                        if (lane == s * 16u + RMJ_PLAYSTAT_RIICHI_TURN) acc = (int32_t)v;
                    }
                    if (h && !((won >> s) & 1u)) {
                        won |= 1u << s;
                        const uint32_t v = dc[s] + (uint32_t)__popcll(d & ((1ull << ps_low(h)) - 1ull));
                        if (lane == s * 16u + RMJ_PLAYSTAT_WIN_TURN) acc = (int32_t)v;
                    }
                    dc[s] += (uint32_t)__popcll(d);
                }
                const uint64_t tl = T & seg;
                if (tl) {
                    const uint32_t t = ps_top(tl);
                    last_kind = ((TS >> t) & 1ull) ? 1u : 2u;
                    last_actor = ((A[1] >> t) & 1ull) ? 1u : ((A[2] >> t) & 1ull) ? 2u : ((A[3] >> t) & 1ull) ? 3u : 0u;
                }
            }
            if (!sk) break;
            // lane j holds a START_KYOKU
            if (open) {
                if (row < r1) rows[(size_t)row * 64u + lane] = acc;
                row++;
            }
            open = true;
            const uint32_t oya = ((uint32_t)__shfl((int)w0, (int)j) >> 8) & 0xFFu;
            acc = (col == RMJ_PLAYSTAT_DEALER && seat < n && seat == oya) ? 1 : 0;
            dc[0] = dc[1] = dc[2] = dc[3] = 0u;
            reached = won = last_kind = last_actor = 0u;
            done = (1ull << j) - 1ull;   // lane j itself counts nothing
            sk &= sk - 1ull;
        }
    }
    if (open) {
        if (row < r1) rows[(size_t)row * 64u + lane] = acc;
        row++;
    }
    for (; row < r1; row++) rows[(size_t)row * 64u + lane] = 0;   // every word is written once, even if the stream held fewer kyokus than the table
}

}  // namespace rmjstat
