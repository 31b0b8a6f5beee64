// GRP rank-model rows (rmj_grp_rows_device, rmj_logset_grp_device): the input of riichienv-ml's rank model for every (kyoku, seat) -
// GrpReplayDataset._encode_features / RewardPredictor.calc_all_player_rewards - and GrpReplayDataset's label, from what a log set or the
// round tracker already holds on the device.
//
//   k_grp_rows<FROM_END>  one thread per 16 bytes of x: the row of (kyoku, seat p), n = 3 or 4 players, is 4n + 4 floats
//                           init[0..n) / S, end[0..n) / S, delta[0..n) / 12000, chang / 3, ju / 3, ben / 4, liqibang / 4, onehot(p)[0..n)
//                         with S = 25000 (4P) / 35000 (3P).  Every quotient is the float64 division of the integer by the constant, rounded
//                         once to float32 - Python's int / float followed by np.float32 - so no reciprocal and no float32 divide.  The second
//                         table is the end scores (FROM_END, log sets: delta = end - init) or the deltas (the round tracker: end = init +
//                         delta); either sum is formed in 64 bits, like Python's integers.  4n + 4 is a multiple of 4: a thread's four floats
//                         lie in one seat's row and the stores of a wave are contiguous.
//   k_grp_logs            one wave per log.  The seat ranks of the log's LAST kyoku's end scores (_compute_rank: stable, ties to the lower
//                         seat; 255 for a log whose status is not OK) and the log's index go to all of its kyoku rows, lane-strided.  Then the
//                         wave walks the log's events, a lane per event: only the first 16 bytes of an event's first record are read (type,
//                         oya, kyoku, bakaze, honba, both kyotaku bytes all lie there), a ballot of the START_KYOKU lanes and its prefix
//                         count number the kyokus, and the lanes that hold one write its meta row with one 16-byte store.
#pragma once

namespace rmjgrp {

constexpr uint32_t GRP_BLOCK = 256;

__device__ inline float grp_q(long long v, double d) { return (float)((double)v / d); }   // IEEE float64 divide, one rounding to float32

// element c of the row of seat p
__device__ inline float grp_elem(uint32_t c, uint32_t p, uint32_t n, const long long* ini, const long long* end, const long long* dl, const int32_t* mt, double S) {
    if (c < n) return grp_q(ini[c], S);
    if (c < 2u * n) return grp_q(end[c - n], S);
    if (c < 3u * n) return grp_q(dl[c - 2u * n], 12000.0);
    const uint32_t k = c - 3u * n;
    if (k < 2u) return grp_q(mt[k], 3.0);
    if (k < 4u) return grp_q(mt[k], 4.0);
    return k - 4u == p ? 1.0f : 0.0f;
}

template <bool FROM_END>
__global__ __launch_bounds__(GRP_BLOCK) void k_grp_rows(const int32_t* __restrict__ init, const int32_t* __restrict__ second, const int32_t* __restrict__ meta,
                                                        uint32_t rows, uint32_t n, float* __restrict__ x) {
    const uint32_t per_seat = n + 1u, per_row = n * per_seat;   // float4s
    const uint64_t total = (uint64_t)rows * per_row;
    for (uint64_t q = (uint64_t)blockIdx.x * GRP_BLOCK + threadIdx.x; q < total; q += (uint64_t)gridDim.x * GRP_BLOCK) {
        const uint64_t row = q / per_row;
        const uint32_t in_row = (uint32_t)(q - row * per_row), p = in_row / per_seat, c0 = (in_row - p * per_seat) * 4u;
        const int4 a = reinterpret_cast<const int4*>(init)[row], b = reinterpret_cast<const int4*>(second)[row], m = reinterpret_cast<const int4*>(meta)[row];
        const long long ini[4] = {a.x, a.y, a.z, a.w}, sec[4] = {b.x, b.y, b.z, b.w};
        const int32_t mt[4] = {m.x, m.y, m.z, m.w};
        long long end[4], dl[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            end[k] = FROM_END ? sec[k] : ini[k] + sec[k];
            dl[k] = FROM_END ? sec[k] - ini[k] : sec[k];
        }
        const double S = n == 3u ? 35000.0 : 25000.0;
        float4 o;
        o.x = grp_elem(c0, p, n, ini, end, dl, mt, S);
        o.y = grp_elem(c0 + 1u, p, n, ini, end, dl, mt, S);
        o.z = grp_elem(c0 + 2u, p, n, ini, end, dl, mt, S);
        o.w = grp_elem(c0 + 3u, p, n, ini, end, dl, mt, S);
        reinterpret_cast<float4*>(x)[q] = o;
    }
}

__global__ __launch_bounds__(GRP_BLOCK) void k_grp_logs(const RmjEvent* __restrict__ ev, const uint32_t* __restrict__ off, const uint32_t* __restrict__ koff, uint32_t M,
                                                        const uint8_t* __restrict__ status, const int32_t* __restrict__ end, uint32_t n, int32_t* __restrict__ meta,
                                                        uint8_t* __restrict__ rank, uint32_t* __restrict__ log_of) {
    const uint32_t lane = threadIdx.x & 63u, l = blockIdx.x * (GRP_BLOCK / 64u) + (threadIdx.x >> 6);
    if (l >= M) return;
    const uint32_t e0 = off[l], e1 = off[l + 1], r0 = koff[l], r1 = koff[l + 1];
    if (r0 >= r1) return;   // a log without a kyoku has no row
    if (rank || log_of) {
        uint8_t rk[4] = {255, 255, 255, 255};
        if (rank && (!status || status[l] == RMJ_LOGTEXT_OK)) {
            const int4 f = reinterpret_cast<const int4*>(end)[r1 - 1u];
            const int32_t sc[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (uint32_t p = 0; p < 4u; p++) {
                uint32_t above = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) above += (q < n && (sc[q] > sc[p] || (sc[q] == sc[p] && q < p))) ? 1u : 0u;
                rk[p] = (uint8_t)above;
            }
        }
        for (uint32_t row = r0 + lane; row < r1; row += 64u) {
            if (log_of) log_of[row] = l;
            if (rank)
                for (uint32_t p = 0; p < n; p++) rank[(size_t)row * n + p] = rk[p];
        }
    }
    if (!meta) return;
    uint32_t row = r0;
    for (uint32_t i0 = e0; i0 < e1; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < e1) v = *reinterpret_cast<const uint4*>(ev + (size_t)i * 3u);   // type actor target tile | consumed[4] | deltas[0..1]
        const bool hit = i < e1 && (v.x & 0xFFu) == (uint32_t)RMJ_EV_START_KYOKU;
        const unsigned long long m = __ballot(hit);
        const uint32_t mine = row + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (hit && mine < r1)
            reinterpret_cast<int4*>(meta)[mine] = make_int4((int32_t)(v.y & 0xFFu), (int32_t)((v.x >> 16) & 0xFFu) - 1, (int32_t)((v.y >> 8) & 0xFFu), (int32_t)(v.y >> 16));
        row += (uint32_t)__popcll(m);
    }
}

static inline dim3 grp_rows_grid(uint32_t rows, uint32_t n) {
    const uint64_t blocks = ((uint64_t)rows * n * (n + 1u) + GRP_BLOCK - 1u) / GRP_BLOCK;
    return dim3((uint32_t)(blocks < 2048u ? (blocks ? blocks : 1u) : 2048u));
}

}  // namespace rmjgrp
