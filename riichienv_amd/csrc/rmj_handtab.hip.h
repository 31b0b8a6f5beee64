// Batched hand API, the table-driven half (rmj_shanten, rmj_effective_tiles, rmj_best_ukeire, rmj_calculate_score): one thread or one
// wave per hand over the shanten tables (rmj_shanten.hip.h, rmj_ukeire.hip.h) and the score table.  The evaluating half is rmj_handapi.hip.h.
#pragma once
// shanten.rs:244-261 / :470-484 (calculate_shanten / calculate_shanten_3p over raw histograms): one thread per hand
// one thread per hand; the block's 256 hands (8 704 contiguous bytes) are fetched as coalesced 16-byte loads into LDS first
// (round 2: every thread read its own 34 bytes at a 34-byte stride)
__global__ __launch_bounds__(256) void k_shanten(ShantenTables T, const uint8_t* counts, uint32_t n, int sanma, int8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[256 * 34 + 16];
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t here = n - base < 256u ? n - base : 256u;
    const size_t off0 = (size_t)base * 34;                       // 8 704 * block: 16-byte aligned when `counts` is
    const uint32_t bytes = here * 34u;
    if ((reinterpret_cast<uintptr_t>(counts) & 15u) == 0u) {
        for (uint32_t i = threadIdx.x; i * 16u < bytes; i += 256u) {
            if (i * 16u + 16u <= bytes) reinterpret_cast<uint4*>(tile)[i] = reinterpret_cast<const uint4*>(counts + off0)[i];
            else for (uint32_t b = i * 16u; b < bytes; b++) tile[b] = counts[off0 + b];
        }
    } else {
        for (uint32_t b = threadIdx.x; b < bytes; b += 256u) tile[b] = counts[off0 + b];
    }
    __syncthreads();
    const uint32_t i = base + threadIdx.x;
    if (i >= n) return;
    PH h = {0, 0, 0, 0};
    int total = 0;
    const uint8_t* mine = tile + threadIdx.x * 34;
#pragma unroll
    for (int t = 0; t < 34; t++) {
        const uint32_t c = mine[t];
        total += (int)c;
        const int s = t_suit(t);
        ph_addv(h, s, (c & 7u) << (3 * (t - 9 * s)));
    }
    out[i] = (int8_t)sh_shanten(h, total / 3, sanma != 0, T);
}
// (round 4's walk: 82 VGPRs = five waves per SIMD left alone; compiled for six: +5 %, eight: the same.  Round 5's pair-dense walk, 74 VGPRs left alone:
//  five waves 0.388, six 0.412, seven 0.425, eight 0.430 G hands/s of best ukeire on random hands)
#define RMJ_UKE_WAVES 8
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RMJ_UKE_WAVES, RMJ_UKE_WAVES))) void k_ukeire(ShantenTables T, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma,
                                                int mode, uint32_t* out) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const bool sm = sanma != 0;
    const int t = lane;                                       // tile type of this lane
    const uint32_t my_cnt = t < 34 ? counts[(size_t)i * 34 + t] : 0u;
    const uint32_t my_vis = (t < 34 && visible) ? visible[(size_t)i * 34 + t] : 0u;
    // wave-uniform histogram: lane t contributes its field, the four words are OR-reduced over the wave
    PH h = {0, 0, 0, 0};
    {
        const int s = t < 34 ? t_suit(t) : 0;
        uint32_t f = t < 34 ? (my_cnt & 7u) << (3 * (t - 9 * s)) : 0u;
        uint32_t w[4] = {s == 0 ? f : 0u, s == 1 ? f : 0u, s == 2 ? f : 0u, s == 3 ? f : 0u};
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) w[k] |= (uint32_t)__shfl_xor((int)w[k], off, 64);
        }
        h.a = w[0]; h.b = w[1]; h.c = w[2]; h.d = w[3];
    }
    const uint32_t res = sh_ukeire_wave(T, h, my_cnt, my_vis, sm, mode, lane);
    if (lane == 0) out[i] = res;
}

__global__ void k_score(const uint8_t* han, const uint8_t* fu, const uint8_t* oya, const uint8_t* tsumo, const uint32_t* honba,
                        const uint8_t* np, uint32_t n, uint32_t* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ScoreOut s = calc_score(han[i], fu[i], oya[i] != 0, tsumo[i] != 0, honba[i], np[i]);
    out[4 * i] = s.total; out[4 * i + 1] = s.ron; out[4 * i + 2] = s.tsumo_oya; out[4 * i + 3] = s.tsumo_ko;
}
