// MJAI JSONL text -> the resident record array of a log set and its per-kyoku score tables (rmj_logset_create_from_text): the inverse of
// k_text_size / k_text_write.  The scalar work per line is rmj_evparse.h (shared with the host test); this file is the data movement.
//
//   k_lt_lines<false>  line census: one wave per log streams the log's bytes with 16-byte loads (byte loads for the ragged head and tail),
//                      every lane reduces its 16 bytes to one element of the monoid "state of the line scanner" (has a newline / saw a
//                      non-blank byte), a wave scan gives every lane the state it starts in, and the log's non-blank lines are counted.
//   k_lt_scan          exclusive scan of the per-log counts (one block): offsets[M + 1] as rmj_logset_create takes them, the 64-event chunk
//                      offsets of the parse grid, later the kyoku offsets.
//   k_lt_lines<true>   line index: the same walk writes every event's first non-blank byte, its end and its line number.
//   k_lt_parse         one wave per 64 consecutive events of one log: their text is contiguous, it is staged into LDS with coalesced wide
//                      loads (a span over LT_LDS_TEXT bytes is parsed out of global memory instead), one line per lane runs
//                      rmjp::parse_line out of LDS into records in LDS, and the wave stores the records with 16-byte vector stores.  The side
//                      structs go to a temporary array; kyoku / decision counts and the first failing line go to per-log words by atomics.
//   k_lt_tables        one wave per log walks the side structs in order (rmjp::KyokuWalk, uniform across the wave; only the events that
//                      matter are broadcast) and writes start / end scores, status and error line - and `own` [K][8], the end scores
//                      every kyoku's own events gave in two readings (rmjp::KyokuWalk::own; the `end` of a kyoku before the last is the next
//                      start_kyoku's scores: log validation compares the two).
// start_kyoku lines (~450 bytes, about 1 in 500) stay with their lane: see DESIGN.md.
#pragma once
#include "rmj_evparse.h"

namespace rmjlt {

constexpr uint32_t LT_LDS_TEXT = 16384;   // bytes of text a parse wave stages (64 lines of ~40 bytes and a start_kyoku need ~3 KB)

__device__ inline uint32_t lt_byte(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }
__device__ inline bool lt_blank(uint32_t ch) { return ch == ' ' || ch == '\t' || ch == '\r'; }

// An event is a line with a byte that is not space, tab, '\r': it runs from its first such byte to its '\n' (or the end of the log).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_lt_lines(const uint8_t* __restrict__ text, const uint64_t* __restrict__ ranges, uint32_t M, uint32_t* __restrict__ counts,
                                                  const uint32_t* __restrict__ off, uint32_t* __restrict__ ev_start, uint32_t* __restrict__ ev_end,
                                                  uint32_t* __restrict__ ev_line) {
    const uint32_t lane = threadIdx.x & 63u, l = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (l >= M) return;
    const uint8_t* base = text + ranges[2 * (size_t)l];
    const uint32_t n = (uint32_t)(ranges[2 * (size_t)l + 1] - ranges[2 * (size_t)l]);
    const uintptr_t a0 = (uintptr_t)base & ~(uintptr_t)15;
    const uint32_t head = (uint32_t)((uintptr_t)base - a0);
    const uint64_t nchunks = ((uint64_t)head + n + 15u) / 16u;
    const uint32_t e0 = WRITE ? off[l] : 0u, e1 = WRITE ? off[l + 1] : 0u;
    uint32_t S = 0, events = 0, newlines = 0;   // carried from tile to tile: inside a non-blank line, events begun, '\n' seen
    for (uint64_t c0 = 0; c0 < nchunks; c0 += 64u) {
        const uint64_t c = c0 + lane;
        const int64_t rel0 = (int64_t)(c * 16u) - (int64_t)head;   // position in the log of this lane's first byte
        uint32_t w[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};   // bytes outside the log read as spaces: no effect
        if (c < nchunks) {
            if (rel0 >= 0 && rel0 + 16 <= (int64_t)n) {
                const uint4 v = *reinterpret_cast<const uint4*>(a0 + c * 16u);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                for (int j = 0; j < 16; j++) {
                    const int64_t r = rel0 + j;
                    if (r >= 0 && r < (int64_t)n) w[j >> 2] = (w[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | ((uint32_t)base[r] << (8 * (j & 3)));
                }
            }
        }
        // this lane's 16 bytes as a function of the scanner state: with a newline the state behind them is known (val), without one it
        // is (state before) | val
        uint32_t nl = 0, val = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t ch = lt_byte(w, j);
            if (ch == '\n') { nl = 1; val = 0; }
            else if (!lt_blank(ch)) val = 1;
        }
        uint32_t inl = nl, ival = val;   // inclusive scan of the composition
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t pn = __shfl_up(inl, d), pv = __shfl_up(ival, d);
            if (lane >= d && !inl) { inl = pn; ival |= pv; }
        }
        uint32_t en = __shfl_up(inl, 1u), ev = __shfl_up(ival, 1u);
        if (lane == 0) en = ev = 0;
        const uint32_t s_in = en ? ev : (S | ev);
        uint32_t s = s_in, cnt = 0, nlc = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t ch = lt_byte(w, j);
            if (ch == '\n') { s = 0; nlc++; }
            else if (!lt_blank(ch)) { cnt += s ^ 1u; s = 1; }
        }
        uint32_t inc = cnt | (nlc << 16);   // both prefix sums at once (at most 1024 of either in a tile)
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t p = __shfl_up(inc, d);
            if (lane >= d) inc += p;
        }
        if (WRITE) {
            const uint32_t exc = inc - (cnt | (nlc << 16));
            uint32_t k = events + (exc & 0xFFFFu), line = newlines + (exc >> 16);
            s = s_in;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t ch = lt_byte(w, j);
                const uint32_t r = (uint32_t)(rel0 + j);
                if (ch == '\n') {
                    if (s && k >= 1u && e0 + k - 1u < e1) ev_end[e0 + k - 1u] = r;
                    s = 0;
                    line++;
                } else if (!lt_blank(ch)) {
                    if (!s) {
                        if (e0 + k < e1) { ev_start[e0 + k] = r; ev_line[e0 + k] = line + 1u; }
                        k++;
                    }
                    s = 1;
                }
            }
        }
        const uint32_t tot = __shfl(inc, 63), ln = __shfl(inl, 63), lv = __shfl(ival, 63);
        events += tot & 0xFFFFu;
        newlines += tot >> 16;
        S = ln ? lv : (S | lv);
    }
    if (lane == 0) {
        if (!WRITE) counts[l] = events;
        else if (S && events >= 1u && e0 + events - 1u < e1) ev_end[e0 + events - 1u] = n;   // the last line lacks its '\n'
    }
}

// out[i] = sum of ceil(counts[j] / div) over j < i, out[M] and *total the whole sum (64 bits: the caller checks the range), *max_out the largest count
__global__ __launch_bounds__(1024) void k_lt_scan(const uint32_t* __restrict__ counts, uint32_t M, uint32_t div, uint32_t* __restrict__ out,
                                                  unsigned long long* __restrict__ total, uint32_t* __restrict__ max_out) {
    __shared__ unsigned long long sh[1024];
    const uint32_t tid = threadIdx.x, per = (M + 1023u) / 1024u;
    const uint64_t lo = (uint64_t)tid * per, hi = lo + per < M ? lo + per : M;
    unsigned long long sum = 0;
    uint32_t mx = 0;
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t v = counts[i];
        sum += (v + (div - 1u)) / div;
        mx = v > mx ? v : mx;
    }
    sh[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const unsigned long long p = tid >= d ? sh[tid - d] : 0ull;
        __syncthreads();
        sh[tid] += p;
        __syncthreads();
    }
    unsigned long long run = tid ? sh[tid - 1] : 0ull;
    for (uint64_t i = lo; i < hi; i++) {
        out[i] = (uint32_t)run;
        run += (counts[i] + (div - 1u)) / div;
    }
    if (tid == 1023u) {
        out[M] = (uint32_t)sh[1023];
        *total = sh[1023];
    }
    if (max_out && mx) atomicMax(max_out, mx);
}

__global__ __launch_bounds__(64) void k_lt_parse(const uint8_t* __restrict__ text, const uint64_t* __restrict__ ranges, uint32_t M, const uint32_t* __restrict__ off,
                                                 const uint32_t* __restrict__ choff, const uint32_t* __restrict__ ev_start, const uint32_t* __restrict__ ev_end,
                                                 const uint32_t* __restrict__ ev_line, uint32_t num_players, uint32_t masked_ok, RmjEvent* __restrict__ events,
                                                 rmjp::Side* __restrict__ sides, uint32_t* __restrict__ kcount, uint32_t* __restrict__ decisions,
                                                 unsigned long long* __restrict__ first_err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[LT_LDS_TEXT + 32];
    __shared__ __attribute__((aligned(16))) RmjEvent s_recs[64 * 3];
    const uint32_t chunk = blockIdx.x, lane = threadIdx.x;
    uint32_t lo = 0, hi = M;   // choff[lo] <= chunk < choff[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (choff[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    const uint32_t l = lo, e0 = off[l] + (chunk - choff[l]) * 64u, e1 = off[l + 1];
    if (e0 >= e1) return;
    const uint32_t nev = e1 - e0 < 64u ? e1 - e0 : 64u;
    const bool valid = lane < nev;
    const uint32_t n = (uint32_t)(ranges[2 * (size_t)l + 1] - ranges[2 * (size_t)l]);
    uint32_t mys = valid ? ev_start[e0 + lane] : 0u, mye = valid ? ev_end[e0 + lane] : 0u;
    if (mye > n) mye = n;
    if (mys > mye) mys = mye;
    const uint32_t first = __shfl(mys, 0), last = __shfl(mye, (int)(nev - 1u));
    const uint8_t* base = text + ranges[2 * (size_t)l];
    const uint8_t* p = base + mys;
    if (last >= first && last - first <= LT_LDS_TEXT) {   // (wave-uniform) stage [first, last) with the alignment it has in memory
        const uint32_t span = last - first;
        const uint8_t* src = base + first;
        const uintptr_t a0 = (uintptr_t)src & ~(uintptr_t)15;
        const uint32_t head = (uint32_t)((uintptr_t)src - a0), nch = (head + span + 15u) / 16u;
        for (uint32_t c = lane; c < nch; c += 64u) {
            const int32_t rel0 = (int32_t)(c * 16u) - (int32_t)head;
            if (rel0 >= 0 && (uint32_t)rel0 + 16u <= span) {
                *reinterpret_cast<uint4*>(s_text + c * 16u) = *reinterpret_cast<const uint4*>(a0 + c * 16u);
            } else {
                for (int j = 0; j < 16; j++) {
                    const int32_t r = rel0 + j;
                    if (r >= 0 && (uint32_t)r < span) s_text[c * 16u + (uint32_t)j] = src[r];
                }
            }
        }
        __syncthreads();
        p = s_text + head + (mys - first);
    }
    rmjp::Side side;
    side.cls = rmjp::CLS_OTHER;
    side.flags = side.status = 0;
    if (valid) {
        rmjp::parse_line(p, mye - mys, num_players, masked_ok != 0u, &s_recs[lane * 3u], &side);
        sides[e0 + lane] = side;
        if (side.status) atomicMin(&first_err[l], ((unsigned long long)ev_line[e0 + lane] << 8) | side.status);
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(events + (size_t)e0 * 3u);
    const uint4* srcq = reinterpret_cast<const uint4*>(s_recs);
    for (uint32_t q = lane; q < nev * 6u; q += 64u) dst[q] = srcq[q];
    const uint32_t k = (uint32_t)__popcll(__ballot(valid && side.cls == rmjp::CLS_START_KYOKU));
    const uint32_t d = (uint32_t)__popcll(__ballot(valid && (side.flags & rmjp::SF_DECISION)));
    if (lane == 0) {
        if (k) atomicAdd(&kcount[l], k);
        if (d) atomicAdd(&decisions[l], d);
    }
}

__global__ __launch_bounds__(256) void k_lt_tables(const rmjp::Side* __restrict__ sides, const uint32_t* __restrict__ off, const uint32_t* __restrict__ koff, uint32_t M,
                                                   const unsigned long long* __restrict__ first_err, int32_t* __restrict__ start, int32_t* __restrict__ end,
                                                   int32_t* __restrict__ own, uint8_t* __restrict__ status, uint32_t* __restrict__ error_line) {
    const uint32_t lane = threadIdx.x & 63u, l = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (l >= M) return;
    rmjp::KyokuWalk walk;
    const uint32_t e0 = off[l], e1 = off[l + 1], r1 = koff[l + 1];
    uint32_t row = koff[l];
    uint32_t prev_cls = rmjp::CLS_OTHER;   // class of the event before this tile
    int32_t so[4], eo[4];
    for (uint32_t i0 = e0; i0 < e1; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint32_t w[10];
#pragma unroll
        for (int k = 0; k < 10; k++) w[k] = 0u;
        if (i < e1) {
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(&sides[i]);
#pragma unroll
            for (int k = 0; k < 10; k++) w[k] = sp[k];
        }
        const uint32_t cls = w[8] & 0xFFu, flags = (w[8] >> 8) & 0xFFu, actor = (w[9] >> 8) & 0xFFu;
        uint32_t before = __shfl_up(cls, 1u);
        if (lane == 0) before = prev_cls;
        // what the walk must see: every class but a dahai of a seat every kyoku has, and whatever follows a hora (it ends the batch of horas).
        // A kyoku with fewer than three scores has no such seat: while one is open, or opens in this tile, every dahai is fed.
        const bool narrow = (walk.open && walk.n_raw < 3u) || __ballot(cls == rmjp::CLS_START_KYOKU && ((w[8] >> 16) & 0xFFu) < 3u) != 0ull;
        const bool plain = cls == rmjp::CLS_OTHER || (cls == rmjp::CLS_DAHAI && !(flags & rmjp::SF_ACTOR_NONE) && actor < 3u && !narrow);
        unsigned long long m = __ballot(i < e1 && (!plain || before == rmjp::CLS_HORA));
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1ull;
            rmjp::Side t;
            uint32_t* tp = reinterpret_cast<uint32_t*>(&t);
#pragma unroll
            for (int k = 0; k < 10; k++) tp[k] = __shfl(w[k], j);
            if (walk.feed(t, so, eo)) {
                if (lane == 0 && row < r1) {
                    for (int k = 0; k < 4; k++) { start[(size_t)row * 4 + k] = so[k]; end[(size_t)row * 4 + k] = eo[k]; own[(size_t)row * 8 + k] = walk.own[k]; own[(size_t)row * 8 + 4 + k] = walk.own[4 + k]; }
                }
                row++;
            }
        }
        prev_cls = __shfl(cls, 63);
    }
    if (walk.finish(so, eo)) {
        if (lane == 0 && row < r1) {
            for (int k = 0; k < 4; k++) { start[(size_t)row * 4 + k] = so[k]; end[(size_t)row * 4 + k] = eo[k]; own[(size_t)row * 8 + k] = walk.own[k]; own[(size_t)row * 8 + 4 + k] = walk.own[4 + k]; }
        }
    }
    if (lane == 0) {
        const unsigned long long fe = first_err[l];
        if (fe != ~0ull) { status[l] = (uint8_t)(fe & 0xFFu); error_line[l] = (uint32_t)(fe >> 8); }
        else { status[l] = walk.st; error_line[l] = 0u; }
    }
}

}  // namespace rmjlt
