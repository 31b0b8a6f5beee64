// Read-out kernels: what the host entry points fetch from the game records between steps - step and full-path counters, compact legal
// lists (rmj_get_legal_compact), points and scores, log positions, wall digests - and the XCC probe of rmj_create.
#pragma once
// largest raw HW_REG_XCC_ID[3:0] over the waves of the launch (rmj_create: is the per-XCD queue assumption of k_step4_queue valid?)
__global__ void k_probe_xcc(unsigned long long* out) {
    const unsigned long long id = (unsigned long long)((uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u);
    if ((threadIdx.x & 63u) == 0u) atomicMax(out, id);
}
__global__ void k_sum_steps(const GState* core, uint32_t n, unsigned long long* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0;
    for (; i < n; i += gridDim.x * blockDim.x) v += core[i].step_count;
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}
__global__ void k_sum_full(const GState* core, uint32_t n, unsigned long long* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0;
    for (; i < n; i += gridDim.x * blockDim.x) v += core[i].full_count;
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}
__global__ void k_gather_steps(const GState* core, uint32_t n, uint64_t* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = core[i].step_count;
}
// ---- compact legal lists for a host agent loop (rmj_get_legal_compact): rows = the seats that are to act, in (game, seat) order,
// entries = their lists one after the other.  Pass 1: per game the rows / entries it contributes, block prefix sums; pass 2: the
// block totals scanned by one block; pass 3: every game writes its rows.  Deterministic order, no atomics.
#define LC_BLOCK 256
__device__ __forceinline__ uint32_t lc_rows_of(uint32_t status, const uint8_t* nl, uint32_t& entries) {
    const uint32_t am = (status >> 16) & 1u ? 0u : (status & 0xFu);
    uint32_t rows = 0;
    entries = 0;
    for (int p = 0; p < 4; p++)
        if (((am >> p) & 1u) && nl[p]) { rows++; entries += nl[p]; }
    return rows;
}
__global__ __launch_bounds__(LC_BLOCK) void k_lc_count(const uint32_t* __restrict__ status, const uint8_t* __restrict__ nlegal, uint32_t n, uint32_t* __restrict__ pre /*[n][2]*/,
                                                       uint32_t* __restrict__ blk /*[blocks][2]*/) {
    __shared__ uint32_t sr[LC_BLOCK], se[LC_BLOCK];
    const uint32_t g = blockIdx.x * LC_BLOCK + threadIdx.x;
    uint32_t e = 0, r = 0;
    if (g < n) r = lc_rows_of(status[g], nlegal + (size_t)g * 4, e);
    sr[threadIdx.x] = r; se[threadIdx.x] = e;
    __syncthreads();
    for (int off = 1; off < LC_BLOCK; off <<= 1) {     // inclusive Hillis-Steele scan
        uint32_t ar = 0, ae = 0;
        if ((int)threadIdx.x >= off) { ar = sr[threadIdx.x - off]; ae = se[threadIdx.x - off]; }
        __syncthreads();
        sr[threadIdx.x] += ar; se[threadIdx.x] += ae;
        __syncthreads();
    }
    if (g < n) { pre[2 * (size_t)g] = sr[threadIdx.x] - r; pre[2 * (size_t)g + 1] = se[threadIdx.x] - e; }
    if (threadIdx.x == LC_BLOCK - 1) { blk[2 * blockIdx.x] = sr[threadIdx.x]; blk[2 * blockIdx.x + 1] = se[threadIdx.x]; }
}
__global__ void k_lc_scan(uint32_t* blk, uint32_t blocks, uint32_t* totals /*[2]*/) {   // one thread: a few thousand blocks at most
    if (blockIdx.x || threadIdx.x) return;
    uint32_t r = 0, e = 0;
    for (uint32_t b = 0; b < blocks; b++) {
        const uint32_t cr = blk[2 * b], ce = blk[2 * b + 1];
        blk[2 * b] = r; blk[2 * b + 1] = e;
        r += cr; e += ce;
    }
    totals[0] = r; totals[1] = e;
}
__global__ __launch_bounds__(LC_BLOCK) void k_lc_gather(const uint32_t* __restrict__ status, const uint8_t* __restrict__ nlegal, const uint64_t* __restrict__ legal, uint32_t n,
                                                        const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk, uint32_t cap_rows, uint32_t cap_entries,
                                                        uint32_t* __restrict__ index, uint32_t* __restrict__ offs, uint64_t* __restrict__ entries) {
    const uint32_t g = blockIdx.x * LC_BLOCK + threadIdx.x;
    if (g >= n) return;
    const uint32_t st = status[g];
    const uint32_t am = (st >> 16) & 1u ? 0u : (st & 0xFu);
    uint32_t row = blk[2 * blockIdx.x] + pre[2 * (size_t)g], ent = blk[2 * blockIdx.x + 1] + pre[2 * (size_t)g + 1];
    for (int p = 0; p < 4; p++) {
        const uint32_t k = nlegal[(size_t)g * 4 + p];
        if (!((am >> p) & 1u) || !k) continue;
        if (row < cap_rows) { index[row] = g * 4u + (uint32_t)p; offs[row] = ent; offs[row + 1] = ent + k; }   // (the next row writes the same value at row + 1)
        for (uint32_t j = 0; j < k; j++)
            if (ent + j < cap_entries) entries[ent + j] = legal[((size_t)g * 4 + p) * RMJ_MAX_LEGAL + j];
        row++;
        ent += k;
    }
}
// RiichiEnv.points (env.rs:691-727) with ranks (env.rs:673-689: by score, ties by seat) for every game: f64 like the reference
__global__ void k_points(const GState* core, uint32_t n, int np, double weight, double base, double u0, double u1, double u2, double u3, double* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t sc[4];
    for (int p = 0; p < 4; p++) sc[p] = core[i].p[p].score;
    for (int p = 0; p < 4; p++) {
        double v = 0.0;
        if (p < np) {
            int rank = 0;   // seats ahead: a higher score, or the same score and a lower seat index
            for (int o = 0; o < np; o++) rank += (sc[o] > sc[p]) || (sc[o] == sc[p] && o < p);
            const double uma = rank == 0 ? u0 : (rank == 1 ? u1 : (rank == 2 ? u2 : u3));
            v = ((double)sc[p] - base) / 1000.0 * weight + uma;
        }
        out[(size_t)i * 4 + p] = v;
    }
}
__global__ void k_gather_scores(const GState* core, uint32_t n, int32_t* out, uint32_t* evc) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        for (int p = 0; p < 4; p++) out[(size_t)i * 4 + p] = core[i].p[p].score;
        if (evc) evc[i] = core[i].ev_count - core[i].ev_base;   // len(mjai_log) of the current game
    }
}
__global__ void k_track_mark(uint8_t* mark, const uint8_t* __restrict__ select, uint32_t first, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (!select || select[first + i])) mark[first + i] = 1;
}
__global__ void k_log_positions(const GState* core, uint32_t n, uint32_t* base, uint32_t* pos) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { base[i] = core[i].ev_base; pos[i] = core[i].ev_count; }
}

// WallState.salt / wall_digest (state/wall.rs:15-16, 48-55) of games [first, first + n): out[i] = {valid, salt (u64), SHA-256 (8 x u32, big
// endian words)} as 11 dwords; one lane per game.  valid = GState::wall_meta (RMJ_RULE_REFERENCE_RNG shuffles only).
__global__ __launch_bounds__(64) void k_wall_digest(const GState* __restrict__ core, const uint8_t* __restrict__ wall, const uint32_t* __restrict__ frozen,
                                                    uint32_t first, uint32_t n, int tiles, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = first + i;
    const uint8_t* W = wall + (size_t)g * RMJ_WALL_STRIDE;
    uint32_t* o = out + (size_t)i * 11;
    const uint32_t valid = core[g].wall_meta;
    uint64_t salt = 0;
    uint32_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (valid) {
        for (int k = 0; k < 8; k++) salt |= (uint64_t)W[136 + k] << (8 * k);
        if (valid == 2) { for (int k = 0; k < 8; k++) dg[k] = frozen[(size_t)g * 8 + k]; }   // the wall it belonged to is gone
        else sha256_wall(W, tiles, salt, dg);
    }
    o[0] = valid; o[1] = (uint32_t)salt; o[2] = (uint32_t)(salt >> 32);
    for (int k = 0; k < 8; k++) o[3 + k] = dg[k];
}
