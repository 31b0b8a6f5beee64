// PPO transition collector (riichienv-ml trainers/_ppo_worker.py:129-391 collect_episodes, :393-466 evaluate_episodes) on the device:
// the hero / opponent action selector, the trajectory pool, the per-kyoku GAE and the flattening into the trainer's arrays.
// Included from rmj_api.hip behind rmj_obs.hip.h (sample_ids_row comes from rmj_policy.hip.h, obs_block_prefix from rmj_obs.hip.h).
//
// The pool is a flat array of `capacity` transitions.  Slots are handed out in (call, game) order: a record call scans the games that
// record (k_ppo_scan: block prefix counts, like k_obs_offsets), every recording game takes slot fill + its prefix (k_ppo_record) and
// the fill moves on by the call's total (k_ppo_advance) - no atomic ticket, so the order does not depend on the schedule.  A game's
// transitions of one open segment (a kyoku of its hero) are chained backwards through `prev`; k_ppo_close walks that chain.
#pragma once

#define PPO_SCAN_BLOCK 1024
enum { PPO_C_FILL = 0, PPO_C_VALID = 1, PPO_C_DROPPED = 2, PPO_C_OVERFLOWED = 3, PPO_C_SEGMENTS = 4, PPO_C_WORDS = 8 };

struct PpoPool {
    // per slot
    float* feat;          // [capacity][row_floats]
    uint8_t* mask;        // [capacity][A]
    int32_t* action;      // [capacity]
    float* value;
    float* logp;
    float* adv;
    float* ret;
    int32_t* game;
    uint32_t* serial;     // the game's segment serial
    int32_t* t;           // position in the segment
    int32_t* prev;        // slot of the game's previous transition of the same open segment, -1 = first
    uint8_t* valid;       // the slot's segment was closed complete: advantage / return are there
    int32_t* seg_len;     // at the LAST slot of a closed segment: its length (0 elsewhere)
    float* seg_reward;    // at the same slot: the segment's reward
    // per game
    int32_t* tail;        // slot of the last transition of the open segment, -1 = none
    uint32_t* open_len;
    uint32_t* g_serial;
    uint8_t* broken;      // the open segment lost a transition (pool full, or no observation row): never emitted
    // scratch of one record call (per game) and of one emit call (per slot)
    int32_t* rowof;       // observation row of the game's hero, -1 = does not record
    uint32_t* offs;       // [max(n, capacity)] exclusive prefix inside the scan block
    uint32_t* totals;     // [blocks] the scan blocks' sums
    uint32_t* ctr;        // [PPO_C_WORDS] device counters
    uint32_t capacity, row_floats, feat_floats, A;
};

// Action ids of one step when ONE seat per game learns (rmj_select_ids_device): the hero seat hero[g] of game g draws like
// rmj_sample_ids_device (the same keyed Gumbel draw: sample_ids_row restricted to that seat), every other seat that is to act takes
// the arg-max of its logits over its legal ids (_ppo_worker.py:227-228 `opp_logits.masked_fill(~mask, -1e9).argmax`): ties to the lowest
// id; a NaN or -inf logit loses to any finite or +inf one; if there is none, the lowest legal id.  hero[g] = 255: every seat takes the
// arg-max (evaluate_episodes); hero = NULL: every seat samples.  Four games per wave, one 16-lane row each, lane r judges ids r, r + 16, ...
__global__ __launch_bounds__(256) void k_select_ids(Env E, const float* __restrict__ logits, uint32_t stride, uint64_t seed, const uint8_t* __restrict__ hero,
                                                    int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = lane & 15;
    const uint32_t g = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (uint32_t)(lane >> 4);
    const bool in = g < E.n_games;
    const uint32_t gi = in ? g : 0u;
    const uint32_t hs = hero ? (uint32_t)hero[gi] : 0xFFFFu;                       // (0xFFFF: no hero array - all seats sample)
    const uint32_t draw = !hero ? 0xFu : (hs < 4u ? (1u << hs) : 0u);              // seats that draw
    int32_t res = sample_ids_row(E.status, E.core, E.nlegal, E.mask, E.game_offset, E.game_mode, g, in, logits, stride, seed, lane, draw);
    const uint32_t st = in ? E.status[gi] : 0x10000u;
    const uint32_t am = ((st >> 16) & 0xFFu ? 0u : (st & 0xFu)) & ~draw;
    const int A = E.game_mode >= 3 ? RMJ_ACTION_SPACE_3P : RMJ_ACTION_SPACE_4P;
    const uint32_t nl4 = in ? *reinterpret_cast<const uint32_t*>(E.nlegal + (size_t)gi * 4) : 0u;
    for (int p = 0; p < 4; p++) {
        const bool act = ((am >> p) & 1u) && ((nl4 >> (8 * p)) & 0xFFu) != 0u;   // (row-uniform)
        if (!__ballot(act)) continue;
        const uint8_t* m = E.mask + ((size_t)gi * 4 + p) * 82;
        const float* lg = logits ? logits + ((size_t)gi * 4 + p) * stride : nullptr;
        float best = -INFINITY;
        int bid = -1;
        if (act) {
            for (int id = r; id < A; id += 16) {
                if (m[id]) {
                    const float v = lg ? lg[id] : 0.0f;
                    const float key = __builtin_isnan(v) ? -INFINITY : v;
                    if (key > best || bid < 0) { best = key; bid = id; }
                }
            }
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bid, off, 64);
            if (oi >= 0 && (bid < 0 || ob > best || (ob == best && oi < bid))) { best = ob; bid = oi; }
        }
        if (act && r == p) res = bid;
    }
    if (in && r < 4) out[(size_t)g * 4 + r] = res;
}

// inclusive scan of one value per thread over a block of PPO_SCAN_BLOCK threads; returns the exclusive prefix, *total = the block's sum
__device__ __forceinline__ uint32_t ppo_block_scan(uint32_t c, uint32_t* wsum, uint32_t* total) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d, 64);
        if ((int)lane >= d) inc += v;
    }
    if (lane == 63u) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t k = 0; k < PPO_SCAN_BLOCK / 64; k++) {
        if (k < wv) before += wsum[k];
        all += wsum[k];
    }
    *total = all;
    return before + inc - c;
}

// Record, step one: which games record in this call (their hero is to act: ids[g][hero[g]] >= 0), the observation row each of them
// reads (dense: g * 4 + hero; compact: the slot whose index entry is g * 4 + hero - the index is sorted, a binary search over the
// first min(count, rows) entries), and the games' prefix counts inside their scan block.  A hero that acts without an observation row
// (a compact batch that was too small) loses the transition: counted as overflowed, the open segment is broken.
__global__ __launch_bounds__(PPO_SCAN_BLOCK) void k_ppo_scan(PpoPool P, uint32_t n, const uint8_t* __restrict__ hero, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ index, uint32_t rows, const uint32_t* __restrict__ count) {
    __shared__ uint32_t wsum[PPO_SCAN_BLOCK / 64];
    const uint32_t g = blockIdx.x * PPO_SCAN_BLOCK + threadIdx.x;
    int32_t row = -1;
    if (g < n) {
        const uint32_t hs = hero[g];
        if (hs < 4u && ids[(size_t)g * 4 + hs] >= 0) {
            const int32_t want = (int32_t)(g * 4u + hs);
            if (!index) row = want;
            else {
                uint32_t lo = 0u, hi = min(*count, rows);
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (index[mid] < want) lo = mid + 1u; else hi = mid;
                }
                if (lo < min(*count, rows) && index[lo] == want) row = (int32_t)lo;
            }
            if (row < 0) {
                atomicAdd(&P.ctr[PPO_C_OVERFLOWED], 1u);
                P.broken[g] = 1;
            }
        }
        P.rowof[g] = row;
    }
    uint32_t total;
    const uint32_t ex = ppo_block_scan(row >= 0 ? 1u : 0u, wsum, &total);
    if (g < n) P.offs[g] = ex;
    if (threadIdx.x == 0) P.totals[blockIdx.x] = total;
}

// `n` floats from src to dst by one wave, in the widest units both addresses allow (16, 8 or 4 bytes), four units in flight per lane
template <typename V>
__device__ __forceinline__ void ppo_copy_units(const float* __restrict__ src, float* __restrict__ dst, uint32_t n, int lane) {
    constexpr uint32_t F = sizeof(V) / 4;
    const uint32_t nu = n / F;
    const V* s = reinterpret_cast<const V*>(src);
    V* d = reinterpret_cast<V*>(dst);
    uint32_t i = (uint32_t)lane;
    for (; i + 192u < nu; i += 256u) {
        const V a = s[i], b = s[i + 64u], c = s[i + 128u], e = s[i + 192u];
        d[i] = a; d[i + 64u] = b; d[i + 128u] = c; d[i + 192u] = e;
    }
    for (; i < nu; i += 64u) d[i] = s[i];
    const uint32_t done = nu * F;
    if (done + (uint32_t)lane < n) dst[done + lane] = src[done + lane];   // (F <= 4: at most three floats left)
}
__device__ __forceinline__ void ppo_copy_row(const float* __restrict__ src, float* __restrict__ dst, uint32_t n, int lane) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst);
    if ((a & 15u) == 0u) ppo_copy_units<uint4>(src, dst, n, lane);
    else if ((a & 7u) == 0u) ppo_copy_units<uint2>(src, dst, n, lane);
    else ppo_copy_units<uint32_t>(src, dst, n, lane);
}

// log_softmax(masked_fill(logits, ~mask, -1e9))[action] (_ppo_worker.py:175-182) of one row by a 16-lane row: lane r holds ids r, r + 16, ...
// - the maximum and the sum of exp(x - max) are reduced over the row, the result is (x[a] - max) - log(sum) like torch's kernel.
__device__ __forceinline__ float ppo_log_prob(const uint8_t* __restrict__ m, const float* __restrict__ lg, int A, int a, int lane) {
    const int r = lane & 15;
    float x[6];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int id = r + 16 * k;
        x[k] = -INFINITY;   // (no such id)
        if (id < A) x[k] = m[id] ? lg[id] : -1e9f;
        mx = fmaxf(mx, x[k]);
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++)
        if (r + 16 * k < A) s += expf(x[k] - mx);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float xa = a < A && m[a] ? lg[a] : -1e9f;
    return (xa - mx) - logf(s);
}

// Record, step two: one wave per recording game (grid-stride over the games).  Slot = the pool's fill + the recording games before
// this one; behind the pool's end nothing is written: the transition is counted as overflowed and the game's open segment is broken.
__global__ __launch_bounds__(256) void k_ppo_record(PpoPool P, uint32_t n, const uint8_t* __restrict__ game_mask, const uint8_t* __restrict__ hero,
                                                    const int32_t* __restrict__ ids, const float* __restrict__ obs, uint32_t obs_stride,
                                                    const float* __restrict__ logits, uint32_t logit_stride, const float* __restrict__ values) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t fill = P.ctr[PPO_C_FILL];
    for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < n; g += waves) {
        const int32_t row = P.rowof[g];
        if (row < 0) continue;
        const uint32_t slot = fill + obs_block_prefix(P.totals, g / PPO_SCAN_BLOCK, lane) + P.offs[g];
        if (slot >= P.capacity) {
            if (lane == 0) {
                atomicAdd(&P.ctr[PPO_C_OVERFLOWED], 1u);
                P.broken[g] = 1;
            }
            continue;
        }
        const uint32_t hs = hero[g];
        const int32_t a = ids[(size_t)g * 4 + hs];
        ppo_copy_row(obs + (size_t)row * obs_stride, P.feat + (size_t)slot * P.row_floats, P.feat_floats, lane);
        const uint8_t* m = game_mask + ((size_t)g * 4 + hs) * 82;
        for (uint32_t i = (uint32_t)lane; i < P.A; i += 64u) P.mask[(size_t)slot * P.A + i] = m[i];
        const float lp = ppo_log_prob(m, logits + (size_t)row * logit_stride, (int)P.A, a, lane);
        if (lane == 0) {
            P.action[slot] = a;
            P.value[slot] = values[row];
            P.logp[slot] = lp;
            P.game[slot] = (int32_t)g;
            P.serial[slot] = P.g_serial[g];
            P.t[slot] = (int32_t)P.open_len[g];
            P.prev[slot] = P.tail[g];
            P.valid[slot] = 0;
            P.seg_len[slot] = 0;
            P.seg_reward[slot] = 0.0f;
            P.tail[g] = (int32_t)slot;
            P.open_len[g] += 1u;
        }
    }
}
// Record, step three: the fill moves on by the number of games that recorded (and stops at the pool's end)
__global__ __launch_bounds__(64) void k_ppo_advance(PpoPool P, uint32_t nb) {
    const uint32_t all = obs_block_prefix(P.totals, nb, (int)threadIdx.x);
    if (threadIdx.x == 0) {
        const uint64_t f = (uint64_t)P.ctr[PPO_C_FILL] + all;
        P.ctr[PPO_C_FILL] = f > P.capacity ? P.capacity : (uint32_t)f;
    }
}

// Close: one thread per game whose hero's segment ends here (_ppo_worker.py:240-281).  The generalised advantage estimate of
// :314-326, walked backwards through `prev`: float64 over the f32 values and the f32 reward, in the worker's order of operations and
// WITHOUT fused multiply-adds (the worker computes in Python floats), rounded to f32 once at the end (:350-351) - the worker's bits.
// A broken segment is dropped (its slots never become valid); an empty one is skipped (:307-308).
__global__ __launch_bounds__(256) void k_ppo_close(PpoPool P, uint32_t n, const uint8_t* __restrict__ ended, const float* __restrict__ reward,
                                                   double gamma, double gamma_lambda) {
#pragma clang fp contract(off)   // (this function only: the build's -O3 contracts a * b + c by default)
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || !ended[g]) return;
    const uint32_t len = P.open_len[g];
    const bool br = P.broken[g] != 0;
    if (!len && !br) return;
    const int32_t last = P.tail[g];
    if (br) {
        if (len) atomicAdd(&P.ctr[PPO_C_DROPPED], len);
    } else {
        const float r = reward[g];
        double gae = 0.0, next_value = 0.0, rew = (double)r;
        for (int32_t s = last; s >= 0; s = P.prev[s]) {
            const double v = (double)P.value[s];
            const double delta = rew + gamma * next_value - v;
            gae = delta + gamma_lambda * gae;
            P.adv[s] = (float)gae;
            P.ret[s] = (float)(gae + v);
            P.valid[s] = 1;
            next_value = v;
            rew = 0.0;
        }
        P.seg_len[last] = (int32_t)len;
        P.seg_reward[last] = r;
        atomicAdd(&P.ctr[PPO_C_VALID], len);
        atomicAdd(&P.ctr[PPO_C_SEGMENTS], 1u);
    }
    P.tail[g] = -1;
    P.open_len[g] = 0u;
    P.broken[g] = 0;
    P.g_serial[g] += 1u;
}

// Emit, step one: prefix counts of the valid slots (blocks of PPO_SCAN_BLOCK slots below the fill)
__global__ __launch_bounds__(PPO_SCAN_BLOCK) void k_ppo_emit_scan(PpoPool P) {
    __shared__ uint32_t wsum[PPO_SCAN_BLOCK / 64];
    const uint32_t s = blockIdx.x * PPO_SCAN_BLOCK + threadIdx.x;
    const bool in = s < P.ctr[PPO_C_FILL];
    uint32_t total;
    const uint32_t ex = ppo_block_scan(in && P.valid[s] ? 1u : 0u, wsum, &total);
    if (s < P.capacity) P.offs[s] = ex;
    if (threadIdx.x == 0) P.totals[blockIdx.x] = total;
}
struct PpoOut {
    float* features;     // [rows][feat_floats]
    uint8_t* mask;       // [rows][A]
    int64_t* action;
    float* log_prob;
    float* advantage;
    float* ret;
    uint32_t* count;     // [2]: valid transitions (may exceed rows: only the first `rows` were written), slots left out (open or broken)
    uint32_t rows;
};
// Emit, step two: the valid slots, in pool order, into the caller's arrays - one wave per slot (grid-stride), rows behind the
// caller's capacity are not written
__global__ __launch_bounds__(256) void k_ppo_emit(PpoPool P, PpoOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u, w0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t fill = P.ctr[PPO_C_FILL];
    if (w0 == 0u) {
        const uint32_t all = obs_block_prefix(P.totals, (P.capacity + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK, lane);
        if (lane == 0) { O.count[0] = all; O.count[1] = fill - all; }
    }
    for (uint32_t s = w0; s < fill; s += waves) {
        if (!P.valid[s]) continue;
        const uint32_t d = obs_block_prefix(P.totals, s / PPO_SCAN_BLOCK, lane) + P.offs[s];
        if (d >= O.rows) continue;
        ppo_copy_row(P.feat + (size_t)s * P.row_floats, O.features + (size_t)d * P.feat_floats, P.feat_floats, lane);
        for (uint32_t i = (uint32_t)lane; i < P.A; i += 64u) O.mask[(size_t)d * P.A + i] = P.mask[(size_t)s * P.A + i];
        if (lane == 0) {
            O.action[d] = (int64_t)P.action[s];
            O.log_prob[d] = P.logp[s];
            O.advantage[d] = P.adv[s];
            O.ret[d] = P.ret[s];
        }
    }
}
