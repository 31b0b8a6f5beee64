// Observation encoders of a handle's games: encode() (k_encode_base), encode_extended() (k_encode_ext), the feature-set batches of the
// trainer path (k_obs_offsets, encode_batch_row, k_encode_batch) and the auxiliary encoders (k_encode_aux).  The per-seat encoding
// itself is rmj_encode.hip.h.  rmj_ppo.hip.h and rmj_logreplay.hip.h are included behind it (obs_block_prefix, encode_batch_row).
#pragma once
// Observation.encode() / encode_extended() for every (game, seat): one wave (= one block) per (game, seat).
// out[g][seat][C][W] f32, C = 74 or 215.  The tensor is assembled in an 84-channel LDS staging buffer (11 KB: 13 blocks per
// CU) and streamed out group by group: base channels, then the two extended groups (rmj_encode.hip.h).
// only_active: 0 = every seat, 1 = acting seats (other rows zeroed), 2 = acting seats (other rows untouched).
template <int W>
__device__ __forceinline__ void enc_stream_out(float* dst, const float* buf, int n_floats, int lane) {
    // both even: 16-byte rows are not guaranteed (215 x 27 is odd), 8-byte pairs are when the offset and count are even
    if ((n_floats & 1) == 0 && ((reinterpret_cast<uintptr_t>(dst) & 7u) == 0)) {
        for (int i = lane; i < n_floats / 2; i += 64) reinterpret_cast<float2*>(dst)[i] = reinterpret_cast<const float2*>(buf)[i];
    } else {
        for (int i = lane; i < n_floats; i += 64) dst[i] = buf[i];
    }
}
// n_floats floats from LDS to global memory in 16-byte stores: `dst` is 8-byte aligned (every row of the tensors is an even
// number of floats from a 16-byte aligned base), so at most two floats precede the first 16-byte boundary and at most
// three follow the last; the body goes out as dwordx4 (the epilogue of a wave is store-issue bound: half the instructions
// of the 8-byte version).  The LDS side is read as two 8-byte halves (its offset is only 8-byte aligned after the head).
__device__ __forceinline__ void enc_stream_out16(float* dst, const float* buf, int n_floats, int lane) {
    const int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);  // 0 or 2
    const int body = (n_floats - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) dst[lane] = buf[lane];
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int i = lane; i < body; i += 64) {
        const float2 lo = *reinterpret_cast<const float2*>(buf + head + 4 * i), hi = *reinterpret_cast<const float2*>(buf + head + 4 * i + 2);
        d4[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
    if (lane < n_floats - tail0) dst[tail0 + lane] = buf[tail0 + lane];
}
__device__ __forceinline__ void enc_zero16(float* dst, int n_floats, int lane) {
    const int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
    const int body = (n_floats - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) dst[lane] = 0.0f;
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int i = lane; i < body; i += 64) d4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < n_floats - tail0) dst[tail0 + lane] = 0.0f;
}
// Slots of the compact observation batch, level one: a block of 1024 threads scans the acting-seat counts of its 1024 games
// (finished games have none): offs[g] = acting seats in the block's games before g, totals[block] = the block's sum.  The
// encoder adds the totals of the blocks before its game's block (at most 512 numbers, one wave reduction).
#define OBS_SCAN_BLOCK 1024
__global__ __launch_bounds__(OBS_SCAN_BLOCK) void k_obs_offsets(const uint32_t* __restrict__ status, uint32_t n, uint32_t* __restrict__ offs,
                                                               uint32_t* __restrict__ totals) {
    __shared__ uint32_t wsum[OBS_SCAN_BLOCK / 64];
    const uint32_t t = threadIdx.x, g = blockIdx.x * OBS_SCAN_BLOCK + t, lane = t & 63u, wv = t >> 6;
    uint32_t c = 0u;
    if (g < n) {
        const uint32_t w = status[g];
        c = ((w >> 16) & 0xFFu) ? 0u : (uint32_t)__popc(w & 0xFu);
    }
    uint32_t inc = c;   // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d, 64);
        if ((int)lane >= d) inc += v;
    }
    if (lane == 63u) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t k = 0; k < wv; k++) before += wsum[k];
    if (g < n) offs[g] = before + inc - c;
    if (t == OBS_SCAN_BLOCK - 1) totals[blockIdx.x] = before + inc;
}
// sum of totals[0 .. nb) by one wave (nb <= 512 for 524 288 games)
__device__ __forceinline__ uint32_t obs_block_prefix(const uint32_t* __restrict__ totals, uint32_t nb, int lane) {
    uint32_t s = 0u;
    for (uint32_t k = (uint32_t)lane; k < nb; k += 64u) s += totals[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d, 64);
    return s;
}
// Observation.encode() of the games [g0, g0 + gridDim.x): ONE block (= one wave) per game, which walks the seats it has to
// encode - with only_active that is the acting seat (one, rarely two or three), so the launch has a quarter of the blocks of
// a (game, seat) grid and no early-exit blocks.  The tensor of a seat is staged as one byte per cell (EncByteSink: 2.5 KB,
// 4.9 KB of LDS per block with the record, the histograms and the value table) and leaves as a stream of 16-byte stores.
// Round 6: four waves per SIMD.  Left alone the kernel takes 100 VGPR (four waves) under the default flags and 60 (seven) under -disable-machine-licm; alone
// it runs the same either way (3P 0.1347 -> 0.1378 ms, occupancy 5 -> 8 changed nothing in round 5), but next to step and sampler kernels of other
// shards on other streams the seven-wave form crowds them out: the trainer loop as 4 shards on 4 streams 304 -> 345 M env.step/s, 2 shards 290 -> 315 M,
// compact batch 305 -> 334 M with the cap (five waves: 336 / 292 / 320; round-5 binary: 340-350 / 312-320 / 311-316).
#define RMJ_ENC_WAVES 4
// `offs` != nullptr: compact output (rmj_encode_compact_device) - the observations of the acting seats, one after the other in
// (game, seat) order: observation offs[g] + j is the j-th acting seat of game g, `index` receives game * 4 + seat.
template <bool SANMA, bool COMPACT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RMJ_ENC_WAVES, RMJ_ENC_WAVES))) void k_encode_base(Env E, int only_active, float* __restrict__ out, uint32_t g0,
                                                               const uint32_t* __restrict__ offs, int32_t* __restrict__ index, uint32_t capacity,
                                                               const uint32_t* __restrict__ totals, uint32_t* __restrict__ count) {
    constexpr int W = SANMA ? ENC_W3 : ENC_W4, NPP = SANMA ? 3 : 4;
    __shared__ GState st;
    __shared__ __attribute__((aligned(16))) uint8_t raw[(ENC_CH * W + 4 + 15) / 16 * 16];
    __shared__ float lut[ENC_LUT];
    __shared__ uint32_t hist[ENC_HIST_WORDS];
    const int lane = threadIdx.x & 63;
    const uint32_t g = g0 + blockIdx.x;
    // the record is requested together with the status word (nearly every game has a seat to act): one memory round trip
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (lane < (int)(sizeof(GState) / 16)) rec = reinterpret_cast<const uint4*>(E.core + g)[lane];
    const uint32_t stw = E.status[g];
    const uint32_t am = ((stw >> 16) & 0xFFu) ? 0u : (stw & 0xFu);
    const size_t RS = E.enc_stride;   // row stride in floats (>= 74 x W; rows padded to a multiple of 256 B leave at 1.3-1.4 x the rate)
    float* base = out + (size_t)g * 4 * RS;
    uint32_t slot = 0u;
    if (COMPACT) {
        if (blockIdx.x == 0) {   // the size of the batch: all block totals
            const uint32_t all = obs_block_prefix(totals, (E.n_games + OBS_SCAN_BLOCK - 1) / OBS_SCAN_BLOCK, lane);
            if (lane == 0) *count = all;
        }
        if (am == 0u) return;
        slot = offs[g] + obs_block_prefix(totals, g / OBS_SCAN_BLOCK, lane);
    } else if (only_active && am == 0u) {
        if (only_active == 1)
            for (int z = 0; z < 4; z++) enc_zero16(base + (size_t)z * RS, ENC_CH * W, lane);
        return;
    }
    enc_lut_init(lut, lane);
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(&st)[lane] = rec;
    wave_sync();
    const GState& S = st;
    for (int seat = 0; seat < 4; seat++) {
        float* dst = base + (size_t)seat * RS;
        const bool acts = (am >> seat) & 1u;
        if (COMPACT) {
            if (seat >= NPP || !acts) continue;
            if (slot >= capacity) return;                  // (the count tells the caller that the buffer was too small)
            dst = out + (size_t)slot * RS;
            if (lane == 0) index[slot] = (int32_t)(g * 4u + (uint32_t)seat);
            slot += 1u;
        } else if (seat >= NPP || (only_active && !acts)) {
            if (only_active != 2) enc_zero16(dst, ENC_CH * W, lane);
            continue;
        }
        const int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);  // 0 or 2 floats
        EncByteSink<W> o{raw + ((4 - head) & 3), lut, lane, -1.0f};
        encode_seat_to<SANMA>(S, seat, lane, hist, o, true);
        enc_emit_bytes<W>(dst, o.cells, lut, lane, head, o.big);
        wave_sync();
    }
}
// n floats computed per element into 16-byte stores (4-byte aligned dst: up to three floats before the first boundary)
template <class F>
__device__ __forceinline__ void enc_emit_fn(float* dst, int n_floats, int lane, F f) {
    int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
    if (head > n_floats) head = n_floats;
    const int body = (n_floats - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) dst[lane] = f(lane);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int i = lane; i < body; i += 64) {
        const int e = head + 4 * i;
        d4[i] = make_float4(f(e), f(e + 1), f(e + 2), f(e + 3));
    }
    if (lane < n_floats - tail0) dst[tail0 + lane] = f(tail0 + lane);
}
// encode_extended() of every (game, seat): one wave per seat.  The 215 x W tensor leaves in three groups that share one
// staging area of bytes: the 74 base channels (EncByteSink), the extended scalars (four per-column channels as floats and a
// table of the 53 channels that are one value per row) and the 84 meld-overview channels (a 0/1 pattern).  6 KB of LDS per
// block instead of 12 KB: the kernel waits on table lookups (the ukeire walk), and its duration is inversely proportional to
// the resident waves (measured by capping them: 13 / 8 / 5 / 3 blocks per CU -> 1.05 / 1.63 / 2.24 / 3.67 ms).
#define RMJ_ENCX_WAVES 6   /* 3P (85 VGPR left alone = five waves): six waves 691 -> 661 us, seven 667, eight 755; 4P (63 VGPR) the same at any */
template <bool SANMA>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RMJ_ENCX_WAVES, RMJ_ENCX_WAVES))) void k_encode_ext(Env E, int only_active, const float* __restrict__ decay, float* __restrict__ out) {
    constexpr int W = SANMA ? ENC_W3 : ENC_W4;
    constexpr int CH = ENC_EXT_CH;
    __shared__ GState st;
    __shared__ __attribute__((aligned(16))) uint8_t raw[(ENC_EXT_C_SLOTS * W + 4 + 15) / 16 * 16];
    __shared__ float lut[ENC_LUT];
    __shared__ float tab[ENC_EXT_B_SLOTS];
    __shared__ float col4[4 * W];
    __shared__ uint32_t hist[ENC_HIST_WORDS];
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x >> 2;
    const int seat = blockIdx.x & 3;
    float* dst = out + ((size_t)g * 4 + seat) * CH * W;
    if (only_active) {  // cheap early-out from the 4-byte status word, before the record is fetched
        const uint32_t stw = E.status[g];
        const bool acts = ((stw >> seat) & 1u) && !((stw >> 16) & 0xFFu);
        if (!acts || seat >= (SANMA ? 3 : 4)) {
            if (only_active == 1)
                for (int i = lane; i < CH * W; i += 64) dst[i] = 0.0f;
            return;
        }
    }
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(&st)[lane] = reinterpret_cast<const uint4*>(E.core + g)[lane];
    enc_lut_init(lut, lane);
    wave_sync();
    const GState& S = st;
    if (seat >= (SANMA ? 3 : 4)) {
        for (int i = lane; i < CH * W; i += 64) dst[i] = 0.0f;
        return;
    }
    auto head_of = [](const float* p) { return (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2); };
    {   // channels 0..73 (encode_base_into: its own tiles-left count, see encode_seat_to)
        const int head = head_of(dst);
        EncByteSink<W> o{raw + ((4 - head) & 3), lut, lane, -1.0f};
        encode_seat_to<SANMA>(S, seat, lane, hist, o, true, true);
        enc_emit_bytes<W>(dst, o.cells, lut, lane, head, o.big);
        wave_sync();
    }
    {   // channels 74..93 and 178..214
        const int n_legal = (((S.active_mask >> seat) & 1u) && !S.is_done) ? (int)E.nlegal[(size_t)g * 4 + seat] : 0;
        encode_ext_scalars<SANMA>(S, seat, tab, col4, lane, E.sh, decay, E.legal + ((size_t)g * 4 + seat) * RMJ_MAX_LEGAL, n_legal);
        enc_emit_fn(dst + 74 * W, 20 * W, lane, [&](int e) { return e < 4 * W ? col4[e] : tab[e / W]; });
        enc_emit_fn(dst + 178 * W, 37 * W, lane, [&](int e) { return tab[20 + e / W]; });
        wave_sync();
    }
    {   // channels 94..177
        float* d = dst + 94 * W;
        const int head = head_of(d);
        uint8_t* cells = raw + ((4 - head) & 3);
        for (int i = lane; i < (int)sizeof(raw) / 16; i += 64) reinterpret_cast<uint4*>(raw)[i] = make_uint4(0u, 0u, 0u, 0u);
        wave_sync();
        encode_ext_melds<SANMA>(S, seat, cells, lane);
        enc_emit_bytes<W, ENC_EXT_C_SLOTS>(d, cells, lut, lane, head);
    }
}
// Observation batches (rmj_encode_batch_device): the acting seats' rows of one feature set, FEAT = RMJ_FEATURES_*:
//   BASE             encode()                                   74 x W  (channels 0..73, ext_base = false)
//   DISCARD_SHANTEN  encode() + encode_extended()'s 74..93      94 x W  (riichienv-ml feat_v2; 4P only)
//   EXTENDED         encode_extended()                          215 x W (k_encode_ext's rows, byte for byte)
// in one of two layouts: dense out[n][4][RS] (rows of seats that do not act untouched) or, COMPACT, out[capacity][RS] in (game, seat)
// order with index[slot] = game * 4 + seat and *count = the number of acting seats.  k_encode_ext's grid of one wave per (game, seat)
// and its occupancy cap: the extended rows wait on the ukeire walk, and a wave per seat keeps the two or three claimants of a discard
// in parallel.  A seat that does not act leaves on the 4-byte status word.  The compact slot is k_obs_offsets' offset of the game,
// plus the totals of the scan blocks before it, plus the acting seats of the game below this one.
// one row of a feature set: seat `seat` of game `g` into dst (4-byte aligned), by one wave that is a block of its own (the staging areas are the block's LDS)
template <bool SANMA, int FEAT>
__device__ __forceinline__ void encode_batch_row(const Env& E, uint32_t g, int seat, const float* __restrict__ decay, float* __restrict__ dst, int lane) {
    constexpr int W = SANMA ? ENC_W3 : ENC_W4;
    constexpr bool EXT = FEAT == RMJ_FEATURES_EXTENDED;
    constexpr int SLOTS = EXT ? ENC_EXT_C_SLOTS : ENC_CH;
    __shared__ GState st;
    __shared__ __attribute__((aligned(16))) uint8_t raw[(SLOTS * W + 4 + 15) / 16 * 16];
    __shared__ float lut[ENC_LUT];
    __shared__ float tab[ENC_EXT_B_SLOTS];
    __shared__ float col4[4 * W];
    __shared__ uint32_t hist[ENC_HIST_WORDS];
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(&st)[lane] = reinterpret_cast<const uint4*>(E.core + g)[lane];
    enc_lut_init(lut, lane);
    wave_sync();
    const GState& S = st;
    auto head_of = [](const float* p) { return (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2); };
    {   // channels 0..73: encode() (channel 30 counts every meld tile) or encode_extended()'s base block
        const int head = head_of(dst);
        EncByteSink<W> o{raw + ((4 - head) & 3), lut, lane, -1.0f};
        encode_seat_to<SANMA>(S, seat, lane, hist, o, true, EXT);
        enc_emit_bytes<W>(dst, o.cells, lut, lane, head, o.big);
        wave_sync();
    }
    if constexpr (FEAT != RMJ_FEATURES_BASE) {   // channels 74..93 (and 178..214 for EXTENDED)
        const int n_legal = EXT && ((S.active_mask >> seat) & 1u) && !S.is_done ? (int)E.nlegal[(size_t)g * 4 + seat] : 0;
        encode_ext_scalars<SANMA, EXT>(S, seat, tab, col4, lane, E.sh, decay, E.legal + ((size_t)g * 4 + seat) * RMJ_MAX_LEGAL, n_legal);
        enc_emit_fn(dst + 74 * W, 20 * W, lane, [&](int e) { return e < 4 * W ? col4[e] : tab[e / W]; });
        if (EXT) enc_emit_fn(dst + 178 * W, 37 * W, lane, [&](int e) { return tab[20 + e / W]; });
        wave_sync();
    }
    if constexpr (EXT) {   // channels 94..177
        float* d = dst + 94 * W;
        const int head = head_of(d);
        uint8_t* cells = raw + ((4 - head) & 3);
        for (int i = lane; i < (int)sizeof(raw) / 16; i += 64) reinterpret_cast<uint4*>(raw)[i] = make_uint4(0u, 0u, 0u, 0u);
        wave_sync();
        encode_ext_melds<SANMA>(S, seat, cells, lane);
        enc_emit_bytes<W, ENC_EXT_C_SLOTS>(d, cells, lut, lane, head);
    }
}
template <bool SANMA, int FEAT, bool COMPACT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RMJ_ENCX_WAVES, RMJ_ENCX_WAVES))) void k_encode_batch(Env E, const float* __restrict__ decay, float* __restrict__ out, uint32_t RS,
                                                                  const uint32_t* __restrict__ offs, const uint32_t* __restrict__ totals,
                                                                  int32_t* __restrict__ index, uint32_t capacity, uint32_t* __restrict__ count) {
    constexpr int NPP = SANMA ? 3 : 4;
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x >> 2;
    const int seat = blockIdx.x & 3;
    if (COMPACT && blockIdx.x == 0) {   // the size of the batch: all block totals
        const uint32_t all = obs_block_prefix(totals, (E.n_games + OBS_SCAN_BLOCK - 1) / OBS_SCAN_BLOCK, lane);
        if (lane == 0) *count = all;
    }
    const uint32_t stw = E.status[g];
    const uint32_t am = ((stw >> 16) & 0xFFu) ? 0u : (stw & 0xFu);   // the seats k_obs_offsets counts
    if (seat >= NPP || !((am >> seat) & 1u)) return;
    float* dst;
    if (COMPACT) {
        const uint32_t slot = offs[g] + obs_block_prefix(totals, g / OBS_SCAN_BLOCK, lane) + (uint32_t)__popc(am & ((1u << seat) - 1u));
        if (slot >= capacity) return;                  // (the count tells the caller that the buffer was too small)
        if (lane == 0) index[slot] = (int32_t)(g * 4u + (uint32_t)seat);
        dst = out + (size_t)slot * RS;
    } else {
        dst = out + ((size_t)g * 4 + seat) * RS;
    }
    encode_batch_row<SANMA, FEAT>(E, g, seat, decay, dst, lane);
}

// ---- auxiliary encoders (row N3): kawa overview, yaku possibility, furiten-ron possibility ----------------------
// One wave per game; absolute seat order, public information only (the same for every observing seat).
//   which 0  Observation.encode_kawa_overview           (observation/python.rs:881-925, observation_3p/python.rs:759-810)
//   which 1  Observation.encode_yaku_possibility        (observation/python.rs:327-455 over yaku_checker.rs:27-412)
//   which 2  Observation.encode_furiten_ron_possibility (observation/python.rs:251-293)
template <bool SANMA>
__global__ __launch_bounds__(64) void k_encode_aux(Env E, int which, float* __restrict__ out) {
    constexpr int W = SANMA ? ENC_W3 : ENC_W4, NP = SANMA ? 3 : 4;
    __shared__ GState st;
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x;
    if (which == 2) {  // tsumogiri_flags is never filled by the reference (observation/mod.rs:105): every row stays 1.0
        for (int i = lane; i < NP * 21; i += 64) out[(size_t)g * NP * 21 + i] = 1.0f;
        return;
    }
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(&st)[lane] = reinterpret_cast<const uint4*>(E.core + g)[lane];
    wave_sync();
    const GState& S = st;
    if (which == 0) {
        // lane = tile column.  Channel k (< 4) is set iff the seat has discarded more than k tiles of the type; channels 4..6 are
        // the red-five flags with the reference's ids and columns (20 / 24 / 28; 4P column 5 + 9 i, 3P (5, 6) and (6, 15))
        float* dst = out + (size_t)g * NP * 7 * W;
        for (int p = 0; p < NP; p++) {
            const PState& P = S.p[p];
            int cnt = 0;
            bool aka0 = false, aka1 = false, aka2 = false;
            for (int k = 0; k < P.n_discards; k++) {
                const int t = P.discards[k];
                cnt += (lane < W && enc_col<SANMA>(t >> 2) == lane);
                aka0 |= t == 20;
                aka1 |= t == 24;
                aka2 |= t == 28;
            }
            if (lane < W) {
                for (int k = 0; k < 4; k++) dst[(p * 7 + k) * W + lane] = cnt > k ? 1.0f : 0.0f;
                if (!SANMA) {
                    dst[(p * 7 + 4) * W + lane] = (aka0 && lane == 5) ? 1.0f : 0.0f;
                    dst[(p * 7 + 5) * W + lane] = (aka1 && lane == 14) ? 1.0f : 0.0f;
                    dst[(p * 7 + 6) * W + lane] = (aka2 && lane == 23) ? 1.0f : 0.0f;
                } else {
                    dst[(p * 7 + 4) * W + lane] = 0.0f;
                    dst[(p * 7 + 5) * W + lane] = (aka1 && lane == 6) ? 1.0f : 0.0f;
                    dst[(p * 7 + 6) * W + lane] = (aka2 && lane == 15) ? 1.0f : 0.0f;
                }
            }
        }
        return;
    }
    // which == 1.  lane = tile type: visible[type] = own discards + dora indicators (yaku_checker.rs:42-58); the meld facts
    // are wave-uniform loops over <= 4 melds x <= 4 tiles.
    float* dst = out + (size_t)g * NP * 21 * 2;
    for (int p = 0; p < NP; p++) {
        const PState& P = S.p[p];
        int vis = 0;
        for (int k = 0; k < P.n_discards; k++) vis += (P.discards[k] >> 2) == lane;
        for (int k = 0; k < S.n_dora; k++) vis += (S.dora[k] >> 2) == lane;
        const uint64_t vis2 = __ballot(lane < 34 && vis >= 2), vis3 = __ballot(lane < 34 && vis >= 3), vis4 = __ballot(lane < 34 && vis >= 4);
        uint64_t set_types = 0;  // types with a meld of >= 3 tiles starting with that type (yaku_checker.rs:68-75)
        bool any_yaochu = false, simple_tile = false, any_number = false, any_honor = false, any_non_terminal = false;
        bool suit0 = false, suit1 = false, suit2 = false, has_run = false, no_yaochu_meld = false, junchan_bad = false;
        const int nm = P.n_melds;
        for (int m = 0; m < nm; m++) {
            const int len = (P.meld_type[m] == RMJ_MELD_CHI || P.meld_type[m] == RMJ_MELD_PON) ? 3 : 4;
            const int t0 = P.meld_tiles[m][0] >> 2, t1 = P.meld_tiles[m][1] >> 2, t2 = P.meld_tiles[m][2] >> 2;
            set_types |= 1ull << t0;
            if (len == 3 && t0 + 1 == t1 && t1 + 1 == t2 && t0 < 27) has_run = true;
            bool m_yaochu = false, m_terminal = false, m_honor = false;
            for (int k = 0; k < len; k++) {
                const int tt = P.meld_tiles[m][k] >> 2;
                const bool honor = tt >= 27, terminal = !honor && (tt % 9 == 0 || tt % 9 == 8);
                m_yaochu |= honor || terminal;
                m_terminal |= terminal;
                m_honor |= honor;
                any_number |= !honor;
                any_non_terminal |= !terminal;
                simple_tile |= !honor && !terminal;
                if (!honor) { suit0 |= tt < 9; suit1 |= tt >= 9 && tt < 18; suit2 |= tt >= 18; }
            }
            any_yaochu |= m_yaochu;
            any_honor |= m_honor;
            if (!m_yaochu) no_yaochu_meld = true;
            if (m_honor || !m_terminal) junchan_bad = true;
        }
        const int ns = (int)suit0 + (int)suit1 + (int)suit2;
        const int round_t = 27 + S.round_wind, seat_t = 27 + (p + NP - S.oya) % NP;
        auto yakuhai_imp = [&](int tt) { return !((set_types >> tt) & 1ull) && ((vis3 >> tt) & 1ull); };
        const uint64_t koku_req = 0x101ull | (0x101ull << 9) | (0x101ull << 18) | (0x7Full << 27);
        bool imp = false;
        switch (lane) {
            case 0: imp = any_yaochu; break;
            case 1: imp = yakuhai_imp(31); break;
            case 2: imp = yakuhai_imp(32); break;
            case 3: imp = yakuhai_imp(33); break;
            case 4: imp = yakuhai_imp(round_t); break;
            case 5: imp = yakuhai_imp(seat_t); break;
            case 6: imp = nm > 0 && ns >= 2; break;
            case 7: imp = nm > 0 && (ns >= 2 || (ns == 1 && any_honor)); break;
            case 8: imp = has_run; break;
            case 9: imp = nm > 0; break;
            case 10: imp = ((vis4 >> 31) & 7ull) != 0ull; break;
            case 11: imp = (((vis2 & ~set_types) >> 31) & 7ull) != 0ull; break;
            case 12: imp = any_number; break;
            case 13: imp = any_non_terminal; break;
            case 14: imp = simple_tile; break;
            case 15: imp = nm > 0 || (vis4 & koku_req) != 0ull; break;
            case 16: imp = no_yaochu_meld; break;
            case 17: imp = junchan_bad; break;
            case 19: imp = nm > 0; break;
            default: break;  // 18 sanshoku, 20 ittsu: never impossible
        }
        if (lane < 21) {
            const float v = imp ? 0.0f : 1.0f;
            reinterpret_cast<float2*>(dst)[p * 21 + lane] = make_float2(v, v);
        }
    }
}
