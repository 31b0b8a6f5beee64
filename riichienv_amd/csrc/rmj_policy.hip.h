// What the step kernels' headers (rmj_step.hip.h, rmj_kernels.hip.h, rmj_step4.hip.h) take from the translation unit that includes
// them - the step flags, a block's LDS record, the state load / store, the reset arguments - and the device policies that do not step:
// the RandomAgent's actions (k_random_actions) and the trainer-side masked categorical sampler (sample_ids_row, k_sample_ids).
// Included from rmj_api.hip before the step headers (behind `using namespace rmj`).
#pragma once
#define WPB 4
#define STEP_F_RANDOM 1u
#define STEP_F_AUTORESET 2u
#define STEP_F_IDS 4u /* `actions` holds int32 action ids [n][4] (Observation.find_action semantics) */
#define STEP_F_QUIET 0x10000u   /* fused rollouts, every step but the last: no mask rows, no nlegal / waits / status words (nobody can read them) */
#define STEP_F_ALLROWS 0x20000u /* fused rollouts, last step: all four mask rows are rewritten (the quiet steps left them stale) */
#define STEP_F_CONT_RYU 0x40000u /* ol_step_full: continue at the exhaustive draw on the record k_step4's tier 0 left in LDS (no reload, no replay of the discard) */
#define STEP_F_CONT_FIN 0x80000u /* ol_step_full: the step is complete on the record in LDS, only the observation outputs are produced */
#define STEP_F_CONT_CLAIMS 0x400000u /* ol_step_full: continue behind the dahai event of the discard made on the record in LDS (claim generation, then the rest of _resolve_discard) */
#define STEP_F_GREEDY 8u /* with STEP_F_RANDOM: the greedy policy (rmj_step_greedy, r4_policy_greedy) instead of the RandomAgent; bits 8..15 = call rate / 256 */

template <int N>
struct BlockSharedT {
    GState st[N];
    WaveScratch x[N];
};
typedef BlockSharedT<WPB> BlockShared;
#define RMJ_STEP_WPB 1 /* games (= waves) per block of the step kernel: single-wave blocks release their LDS as soon as the game is done (a block of four waited for its slowest game) */

__device__ __forceinline__ void load_state(GState& S, const GState* src, int lane) {
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(&S)[lane] = reinterpret_cast<const uint4*>(src)[lane];
    wave_sync();
}
__device__ __forceinline__ void store_state(const GState& S, GState* dst, int lane) {
    wave_sync();
    if (lane < (int)(sizeof(GState) / 16)) reinterpret_cast<uint4*>(dst)[lane] = reinterpret_cast<const uint4*>(&S)[lane];
}

// fast path of k_step: the 128 B of globals and the PState quarters named by `dirty` (bit = seat)
__device__ __forceinline__ void store_state_partial(const GState& S, GState* dst, int lane, uint32_t dirty) {
    wave_sync();
    if (lane < (int)(sizeof(GState) / 16) && (lane >= 32 || ((dirty >> (lane >> 3)) & 1u)))
        reinterpret_cast<uint4*>(dst)[lane] = reinterpret_cast<const uint4*>(&S)[lane];
}

// Device policy without stepping (rmj_random_actions)
__global__ void k_random_actions(Env E, uint64_t policy_seed, uint64_t* out) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const GState& S = E.core[g];
    uint64_t gs = sm64(policy_seed + E.game_offset + g);
    for (int p = 0; p < 4; p++) {
        uint64_t a = RMJ_NO_ACTION;
        int n = E.nlegal[(size_t)g * 4 + p];
        if (((S.active_mask >> p) & 1u) && n > 0 && !S.is_done) {
            const uint32_t ch = policy_pick(policy_key32(gs, S.step_count, (uint32_t)p), (uint32_t)n);
            a = E.legal[((size_t)g * 4 + p) * RMJ_MAX_LEGAL + ch];
        }
        out[(size_t)g * 4 + p] = a;
    }
}

// Trainer-side masked categorical sampler (rmj_sample_ids_device): one wave per game; for every seat that is to act the
// lanes hold ids lane and lane + 64 of the seat's mask row, add Gumbel noise to the policy's logits (Gumbel-max = a draw
// from softmax(logits) restricted to the legal ids; no logits = uniform over the legal ids) and a wave arg-max picks the id.
// The noise is counter-based: splitmix64(seed, global game, the game's step count, seat, id).
// Round 5: four games per wave (one 16-lane row each; lane r of a row judges the ids r, r + 16, ...), like the step kernels - the keyed Gumbel
// draw of an id costs the same wherever it runs, but a wave per game left 64 lanes to 82 ids of (mostly) one seat.  The same keys, the same
// arg-max rule (ties to the lower id) as the wave-per-game kernel of rounds 3-4: identical ids.
// One id per acting seat of the row's game g (in: the row has a game): lane p of the row returns seat p's id, -1 where nobody acts.
// Non-finite logits: a -inf or NaN logit is never drawn while a finite one is legal; if every legal id is -inf or NaN the lowest legal
// id is drawn; among several +inf logits the lowest id wins.  tests/sampler_ref.py restates the draw in float64.
__device__ __forceinline__ int32_t sample_ids_row(const uint32_t* status, const GState* core, const uint8_t* nlegal, const uint8_t* mask, uint64_t game_offset,
                                                  int game_mode, uint32_t g, bool in, const float* __restrict__ logits, uint32_t stride, uint64_t seed, int lane,
                                                  uint32_t seats = 0xFu) {   // seats: the seats that draw (k_select_ids draws for one)
    const int r = lane & 15;
    const uint32_t gi = in ? g : 0u;
    const uint32_t st = in ? status[gi] : 0x10000u;
    const uint32_t am = ((st >> 16) & 0xFFu ? 0u : (st & 0xFu)) & seats;   // done games have nobody to act
    const int A = game_mode >= 3 ? RMJ_ACTION_SPACE_3P : RMJ_ACTION_SPACE_4P;
    const uint64_t base = sm64(seed ^ sm64(game_offset + gi)) + ((uint64_t)core[gi].step_count << 10);
    const uint32_t nl4 = in ? *reinterpret_cast<const uint32_t*>(nlegal + (size_t)gi * 4) : 0u;   // the four list lengths of the game
    int32_t res = -1;
    for (int p = 0; p < 4; p++) {
        const bool act = ((am >> p) & 1u) && ((nl4 >> (8 * p)) & 0xFFu) != 0u;   // (row-uniform)
        if (!__ballot(act)) continue;
        const uint8_t* m = mask + ((size_t)gi * 4 + p) * 82;
        const float* lg = logits ? logits + ((size_t)gi * 4 + p) * stride : nullptr;
        float best = -INFINITY;
        int bid = -1;
        if (act) {
            for (int id = r; id < A; id += 16) {
                if (m[id]) {
                    const uint64_t h = sm64(base + ((uint64_t)p << 8) + (uint64_t)id);
                    // u in (0, 1), 24 bits: 0xFFFFFF + 0.5f rounds to 2^24 (u = 1, a +inf key whatever the logit), so the top value is
                    // clamped to the largest float below 1 - the only hash value whose u this changes
                    const float u = fminf(((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
                    const float k = (lg ? lg[id] : 0.0f) - __logf(-__logf(u));
                    const float key = __builtin_isnan(k) ? -INFINITY : k;   // a NaN logit is drawn like -inf (the arg-max stays a function of the keys)
                    if (key > best || bid < 0) { best = key; bid = id; }
                }
            }
        }
        // row arg-max (ties to the lower id)
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bid, off, 64);
            if (oi >= 0 && (bid < 0 || ob > best || (ob == best && oi < bid))) { best = ob; bid = oi; }
        }
        if (act && r == p) res = bid;
    }
    return res;
}
__global__ __launch_bounds__(256) void k_sample_ids(Env E, const float* __restrict__ logits, uint32_t stride, uint64_t seed,
                                                    int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = lane & 15;
    const uint32_t g = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (uint32_t)(lane >> 4);
    const bool in = g < E.n_games;
    const int32_t res = sample_ids_row(E.status, E.core, E.nlegal, E.mask, E.game_offset, E.game_mode, g, in, logits, stride, seed, lane);
    if (in && r < 4) out[(size_t)g * 4 + r] = res;
}

struct ResetArgs {
    const uint8_t* select;
    const uint8_t* walls;       // [n][136] reference orientation (draw order)
    const uint8_t* oya;
    const uint8_t* round_wind;
    const int32_t* scores;      // [n][4]
    const uint8_t* honba;
    const uint32_t* kyotaku;
    const uint64_t* seeds;      // ctor only
    uint64_t base_seed;
    uint32_t is_ctor;
};
