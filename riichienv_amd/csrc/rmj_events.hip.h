// What a trainer reads out of the event rings between steps, on the device: the round tracker (k_round_track), the bulk drain of the
// rings (k_ev_*) and the MJAI text formatter (TextSrc, k_text_*; the per-record functions are rmj_evtext.h).  The kernels have C names
// (they were written inside the C ABI's extern "C" block, and the code object keeps their symbols).  Included from rmj_api.hip last.
#pragma once
extern "C" {
// ---- per-round rewards for a trainer on the same GPU -------------------------------------------
// What riichienv-ml's PPO worker derives on the host between steps (trainers/_ppo_worker.py:100-116, 240-266, 283-291): when a
// round has ended, the seats' score deltas over that round and the round's opening facts (the GRP features chang / ju / ben /
// liqibang); when the game has ended, its final scores (rank rewards).  A tracker per handle remembers where every game's current
// round began; one small launch after a step compares: the wall's hand index moves with every deal (state/wall.rs:36-40), is_done
// with the end of the game.  ended: 0 = the round goes on, 1 = a round ended and the next one was dealt, 2 = the round and the game
// ended; a finished game that was restarted (auto-reset, rmj_reset) re-opens silently.
struct RoundTrack {            // device arrays of the tracker (rmj_env::d_track)
    uint32_t* hand_index;      // [n] hand index when the game's current round was dealt
    uint8_t* was_done;         // [n]
    int32_t* start_scores;     // [n][4]
    int32_t* start_meta;       // [n][4] round_wind, oya, honba, riichi_sticks at the deal
    uint8_t* mark;             // [n] set by rmj_reset / rmj_poke_state for the games they touch: the tracker takes the new state as its baseline
};

__global__ void k_round_track(const GState* __restrict__ core, uint32_t n, RoundTrack T, int baseline, uint8_t* __restrict__ ended, int32_t* __restrict__ delta,
                              int32_t* __restrict__ meta, uint8_t* __restrict__ kyoku_idx) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const GState& S = core[g];
    const uint32_t hi = S.hand_index;
    const bool done = S.is_done != 0;
    int32_t sc[4];
    for (int p = 0; p < 4; p++) sc[p] = S.p[p].score;
    uint8_t e = 0;
    bool rebase = baseline != 0;
    const bool marked = T.mark[g] != 0;   // rmj_reset / rmj_poke_state touched the game since the last call: no round of THIS game ended
    if (marked) { T.mark[g] = 0; rebase = true; }
    if (!baseline && !marked) {
        const bool wd = T.was_done[g] != 0;
        if (wd && !done) rebase = true;                                  // restarted: a new game opens
        else if (done && !wd) e = 2;                                     // the round that ended the game
        else if (!done && hi != T.hand_index[g]) { e = 1; rebase = true; }
    }
    if (ended) ended[g] = e;
    if (kyoku_idx) kyoku_idx[g] = S.kyoku_idx;
    for (int p = 0; p < 4; p++) {
        if (delta) delta[(size_t)g * 4 + p] = e ? sc[p] - T.start_scores[(size_t)g * 4 + p] : 0;
        if (meta) meta[(size_t)g * 4 + p] = e ? T.start_meta[(size_t)g * 4 + p] : 0;
    }
    if (rebase) {
        T.hand_index[g] = hi;
        for (int p = 0; p < 4; p++) T.start_scores[(size_t)g * 4 + p] = sc[p];
        T.start_meta[(size_t)g * 4 + 0] = S.round_wind; T.start_meta[(size_t)g * 4 + 1] = S.oya;
        T.start_meta[(size_t)g * 4 + 2] = S.honba; T.start_meta[(size_t)g * 4 + 3] = (int32_t)S.riichi_sticks;
    }
    T.was_done[g] = done ? 1 : 0;
}

// ---- bulk drain of the event rings ----------------------------------------------------------
// RiichiEnv.mjai_log / per-seat logs of EVERY game (riichienv-python/src/env.rs:729-739, state/mod.rs:2094-2148): the records each
// game slot wrote since the caller's cursor, gathered on the device into one dense buffer (two-level scan of the counts, one wave per
// game copies its window of the ring) and brought down with one copy.  Cursors are positions in the slot's record stream
// (GState::ev_count never goes back: a restart moves ev_base), so a window may hold the end of one game and the start of the next.
// A slot whose ring was lapped since its cursor lost its oldest records: the window starts at the oldest record still there; the loss is
// booked per slot (RmjEventViews.lost, cumulative) by the drain that hands the window over, not by peeks or failed calls.
__global__ __launch_bounds__(LC_BLOCK) void k_ev_count(const GState* __restrict__ core, uint32_t n, uint32_t ring, const uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ first, uint32_t* __restrict__ pre, uint32_t* __restrict__ blk) {
    __shared__ uint32_t sc[LC_BLOCK];
    const uint32_t g = blockIdx.x * LC_BLOCK + threadIdx.x;
    uint32_t c = 0;
    if (g < n) {
        const uint32_t total = core[g].ev_count;
        uint32_t behind = total - cursor[g];           // wrap-safe distance; a cursor "ahead" of the stream (not this slot's) reads as nothing new
        if (behind > 0x80000000u) behind = 0u;
        const uint32_t take = behind > ring ? ring : behind;
        first[g] = total - take;
        c = take;
    }
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < LC_BLOCK; off <<= 1) {
        uint32_t a = 0;
        if ((int)threadIdx.x >= off) a = sc[threadIdx.x - off];
        __syncthreads();
        sc[threadIdx.x] += a;
        __syncthreads();
    }
    if (g < n) pre[g] = sc[threadIdx.x] - c;
    if (threadIdx.x == LC_BLOCK - 1) blk[blockIdx.x] = sc[threadIdx.x];
}
__global__ void k_ev_scan(uint32_t* blk, uint32_t blocks, uint32_t* total) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t r = 0;
    for (uint32_t b = 0; b < blocks; b++) { const uint32_t c = blk[b]; blk[b] = r; r += c; }
    total[0] = r;
}
// one wave per game: lane = (record, half) - 16 bytes per lane, 32 records per pass.  newcur[g] = the position behind the window
// (the window = [first[g], ev_count): the size call of rmj_drain_format keeps what it gathered staged, so no second gather needs a stop position)
__global__ __launch_bounds__(256) void k_ev_gather(const GState* __restrict__ core, const RmjEvent* __restrict__ events, uint32_t n, uint32_t ring,
                                                   const uint32_t* __restrict__ first, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                   uint32_t cap, RmjEvent* __restrict__ out, uint32_t* __restrict__ offs, uint32_t* __restrict__ newcur) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n) return;
    const uint32_t total = core[g].ev_count, lo = first[g], base = blk[g / LC_BLOCK] + pre[g], cnt = total - lo;
    const uint4* src = reinterpret_cast<const uint4*>(events + (size_t)g * ring);
    uint4* dst = reinterpret_cast<uint4*>(out);
    for (uint32_t k = (uint32_t)(lane >> 1); k < cnt; k += 32u) {
        const uint32_t o = base + k;
        if (o < cap) dst[2 * (size_t)o + (lane & 1)] = src[2 * (size_t)((lo + k) & (ring - 1u)) + (lane & 1)];
    }
    if (lane == 0) {
        offs[g] = base;
        if (g == n - 1u) offs[n] = base + cnt;
        newcur[g] = total;
    }
}
// the drain is handed over: what its windows skipped is lost
__global__ void k_ev_book(const uint32_t* __restrict__ cursor, const uint32_t* __restrict__ first, uint32_t n, uint32_t* __restrict__ lost) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t skipped = first[g] - cursor[g];
    if (skipped && skipped <= 0x80000000u) lost[g] += skipped;
}
// ---- MJAI text on the device (rmj_drain_text / rmj_format_events_device) -------------------------
// The host formatter's text (rmjh::format_events), byte for byte, written by the GPU with the per-record functions of rmj_evtext.h (the
// host test holds them to the host formatter).  A game's window is either a run of its ring - stream positions [first[g], ev_count), as
// k_ev_count computes them, read in place: no dense gather - or a run of caller records ev[offsets[g] .. offsets[g + 1]).
//   k_text_size   one wave per game, a record per lane: evt_len; the game's stop = the min over its failing indices (the first set bit
//                 of the first failing chunk's ballot); the game's bytes; the position behind the window (the new cursor).
//   k_text_scan1 / k_text_scan2   the games' bytes to uint64 bases: an exclusive scan inside blocks of 256 games, then the block sums
//                 by one workgroup of 1 024 (any number of blocks - 524 288 games are 2 048).
//   k_text_write  one wave per game: chunks of up to 64 records - as many as fit the wave's LDS staging - are sized again and scanned in
//                 the wave, each lane writes its record's text into the staging, and the staging goes out as aligned 16-byte stores;
//                 only the unaligned head and tail bytes of the game's span are stored narrow.
// The per-record rule (rmj_evtext.h): a TEHAI record gives 0 bytes, a START_KYOKU is a head iff the next two records of the window are
// TEHAI, the log ends before the first other record that cannot be formatted.  A head in front of the stop has its two TEHAI records in
// front of it too (the stop is not a TEHAI), so the write pass bounds the window by the stop.
struct TextSrc {
    const RmjEvent* ev;     // ring mode: the rings [n][ring]; records mode: the caller's records
    uint32_t ring;          // ring size (a power of two); 0 = records mode
    uint32_t rec_bytes;     // sizeof(RmjEvent), as an argument: record addresses are 32 x 32 -> 64-bit multiplies, not 64-bit shifts
    const uint32_t* lo;     // ring mode: first[g] (a stream position); records mode: offsets [n + 1]
    const GState* core;     // ring mode: core[g].ev_count ends the window
};
__device__ inline uint32_t text_end(const TextSrc& s, uint32_t g) { return s.ring ? s.core[g].ev_count : s.lo[g + 1]; }
__device__ inline const RmjEvent* text_rec(const TextSrc& s, uint32_t g, uint32_t pos) {
    const char* b = reinterpret_cast<const char*>(s.ev);
    if (s.ring) return reinterpret_cast<const RmjEvent*>(b + (uint64_t)g * (s.ring * s.rec_bytes) + (pos & (s.ring - 1u)) * s.rec_bytes);
    return reinterpret_cast<const RmjEvent*>(b + (uint64_t)pos * s.rec_bytes);
}
__device__ inline RmjEvent text_load(const RmjEvent* p) {   // one record in two 16-byte loads
    union { uint4 q[2]; RmjEvent e; } u;
    const uint4* q = reinterpret_cast<const uint4*>(p);
    u.q[0] = q[0];
    u.q[1] = q[1];
    return u.e;
}
__device__ inline uint32_t text_incl_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}
__global__ __launch_bounds__(256) void k_text_size(TextSrc s, uint32_t n, int seat, uint32_t* __restrict__ nrec, uint32_t* __restrict__ bytes,
                                                   uint32_t* __restrict__ newcur) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n) return;
    const uint32_t lo = s.lo[g], cnt = text_end(s, g) - lo;
    uint32_t total = 0, stop = cnt;
    for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {
        const uint32_t k = k0 + (uint32_t)lane;
        int32_t len = 0;
        if (k < cnt) {
            const RmjEvent e = text_load(text_rec(s, g, lo + k));
            len = rmjt::evt_len(e, k + 1u < cnt ? text_rec(s, g, lo + k + 1u) : nullptr, k + 2u < cnt ? text_rec(s, g, lo + k + 2u) : nullptr, seat);
        }
        const unsigned long long bad = __ballot(len < 0);
        if (bad) {
            const uint32_t f = (uint32_t)__ffsll(bad) - 1u;
            stop = k0 + f;
            if ((uint32_t)lane >= f) len = 0;
        }
        total += (uint32_t)__shfl((int)text_incl_scan((uint32_t)len, lane), 63, 64);
        if (bad) break;
    }
    if (lane == 0) {
        nrec[g] = stop;
        bytes[g] = total;
        if (newcur) newcur[g] = lo + cnt;
    }
}
__global__ __launch_bounds__(256) void k_text_scan1(const uint32_t* __restrict__ bytes, uint32_t n, uint64_t* __restrict__ pre, uint64_t* __restrict__ blk) {
    __shared__ uint64_t sc[256];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint64_t c = g < n ? bytes[g] : 0u;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint64_t a = 0;
        if ((int)threadIdx.x >= off) a = sc[threadIdx.x - off];
        __syncthreads();
        sc[threadIdx.x] += a;
        __syncthreads();
    }
    if (g < n) pre[g] = sc[threadIdx.x] - c;
    if (threadIdx.x == 255) blk[blockIdx.x] = sc[255];
}
// blk[0 .. blocks) -> exclusive bases; the total -> offs[n]
__global__ __launch_bounds__(1024) void k_text_scan2(uint64_t* __restrict__ blk, uint32_t blocks, uint64_t* __restrict__ offs, uint32_t n,
                                                     uint64_t* __restrict__ total) {
    __shared__ uint64_t sc[1024];
    const uint32_t per = (blocks + 1023u) / 1024u, b0 = threadIdx.x * per;
    uint64_t c = 0;
    for (uint32_t i = 0; i < per; i++)
        if (b0 + i < blocks) c += blk[b0 + i];
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        uint64_t a = 0;
        if ((int)threadIdx.x >= off) a = sc[threadIdx.x - off];
        __syncthreads();
        sc[threadIdx.x] += a;
        __syncthreads();
    }
    uint64_t r = sc[threadIdx.x] - c;
    for (uint32_t i = 0; i < per; i++)
        if (b0 + i < blocks) {
            const uint64_t v = blk[b0 + i];
            blk[b0 + i] = r;
            r += v;
        }
    if (threadIdx.x == 1023) {
        offs[n] = sc[1023];
        total[0] = sc[1023];
    }
}
#define TEXT_STAGE 4096u   // bytes of LDS staging per wave: 64 records of the longest kind do not fit, so a chunk takes what does (>= 1)
static_assert(TEXT_STAGE >= 16u + rmjt::RMJT_MAX_EVENT_BYTES, "a record must fit behind a partial block");
struct LdsSink {
    char* p;
    __device__ void put(char c) { *p++ = c; }
};
__global__ __launch_bounds__(64) void k_text_write(TextSrc s, uint32_t n, int seat, const uint32_t* __restrict__ nrec, const uint32_t* __restrict__ bytes,
                                                   const uint64_t* __restrict__ pre, const uint64_t* __restrict__ blk, uint64_t* __restrict__ offs,
                                                   char* __restrict__ text) {
    __shared__ uint4 stage4[TEXT_STAGE / 16u];
    char* const stage = reinterpret_cast<char*>(stage4);
    const uint32_t g = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t base = blk[g >> 8] + pre[g];
    if (lane == 0) offs[g] = base;
    const uint32_t lo = s.lo[g], m = nrec[g], span = bytes[g];
    char* gp = text + (base & ~(uint64_t)15);    // the global address of stage[0]: 16-byte aligned
    uint32_t fill = (uint32_t)base & 15u;        // bytes staged (the first `skip` of them are not this game's)
    uint32_t skip = fill, done = 0;              // done: bytes of the span staged so far (never more than the size pass gave)
    for (uint32_t k0 = 0; k0 < m;) {
        const uint32_t k = k0 + (uint32_t)lane;
        uint32_t len = 0;
        RmjEvent e;
        const RmjEvent *t1 = nullptr, *t2 = nullptr;
        if (k < m) {
            e = text_load(text_rec(s, g, lo + k));
            if (e.type == RMJ_EV_START_KYOKU) {
                t1 = k + 1u < m ? text_rec(s, g, lo + k + 1u) : nullptr;
                t2 = k + 2u < m ? text_rec(s, g, lo + k + 2u) : nullptr;
            }
            const int32_t l = rmjt::evt_len(e, t1, t2, seat);
            len = l > 0 ? (uint32_t)l : 0u;
        }
        const uint32_t incl = text_incl_scan(len, lane);
        const bool fits = k < m && fill + incl <= TEXT_STAGE && done + incl <= span;
        const uint32_t take = (uint32_t)__popcll(__ballot(fits));   // the lanes that fit are a prefix of the chunk
        if (take == 0) break;                                         // (only if the records changed since the size pass)
        if (fits && len) {
            LdsSink o{stage + fill + incl - len};
            rmjt::evt_write(o, e, t1, t2, seat);
        }
        const uint32_t chunk = (uint32_t)__shfl((int)incl, (int)take - 1, 64);
        fill += chunk;
        done += chunk;
        k0 += take;
        __syncthreads();
        const uint32_t nb = fill >> 4;
        for (uint32_t b = (uint32_t)lane; b < nb; b += 64u) {
            if (b == 0 && skip) {   // the span's unaligned head: the block's first bytes belong to the game before
                for (uint32_t j = skip; j < 16u; j++) gp[j] = stage[j];
            } else {
                *reinterpret_cast<uint4*>(gp + b * 16u) = stage4[b];
            }
        }
        const uint32_t rem = fill & 15u;
        if (nb) {   // the partial block moves to the front of the staging
            const char c = (uint32_t)lane < rem ? stage[nb * 16u + lane] : 0;
            __syncthreads();
            if ((uint32_t)lane < rem) stage[lane] = c;
            __syncthreads();
            gp += nb * 16u;
            fill = rem;
            skip = 0;
        }
    }
    if ((uint32_t)lane < fill && (uint32_t)lane >= skip) gp[lane] = stage[lane];   // the unaligned tail
}
}  // extern "C"
