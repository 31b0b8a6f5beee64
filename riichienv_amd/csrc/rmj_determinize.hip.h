// Determinize: re-deal what a seat cannot see.  For a (game g, viewpoint seat a) pair the kernel permutes the hidden tiles of the game in
// place - the concealed hands of the opponents and the part of the wall that can still be drawn or revealed - and republishes lists, masks,
// waits and status for the new record, so that the game is a position seat a could not tell from the one it was and any existing call steps
// it on (PIMC move evaluation, determinized tree search, value targets on sampled worlds).  Included from rmj_api.hip behind every other
// subsystem, so the code object keeps the kernels it had where they were; the step kernels are not touched.
//
// The hidden pool, in CANONICAL ORDER, in terms of RmjStateView (rmj_peek_state), NP = 4 or 3 seats:
//   for r = 0, 1, 2 with r + 1 < NP and bit r of `hold` clear:  players[(a + 1 + r) mod NP].hand[0 .. hand_len)   by hand slot
//   then wall[j] for j = 0 .. wall_len ascending, except the revealed dora indicators: j + rinshan_draw_count = D + 2 k, k < n_dora, with
//   D = 4 (4P) or 8 (3P; the step kernels read 3P's indicators at 8 + 2 k and its ura indicators at 9 + 2 k).
// wall[] of the view is the wall row between the kan-replacement cursor and live_end: the live wall, the rinshan tiles not yet drawn,
// the dora indicators not yet revealed and every ura indicator.  Not in the pool: the revealed indicators, everything drawn, seat a's own
// hand with its drawn tile, melds, discards, kita.  m <= 3 * 14 + 122 tiles.
//
// The permutation (det_mix / det_key / det_rank below are the definition, for the kernel and for rmj_determinize_order alike):
//   mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (mod 2^64)
//   base  = mix(seed + global game)                      the global game as the device policies count it: RmjConfig.game_offset + g
//   key_i = mix(base + (a * 256 + i) * 0x9E3779B97F4A7C15)     i = canonical index
//   perm  = the indices 0 .. m - 1 sorted by (key_i, i);  the new tile at canonical position r is the old tile at canonical position perm[r]
// i.e. a sort by 64-bit keys: every lane ranks its two or three pool slots against the keys in LDS (m <= 164), no serial Fisher-Yates loop.
// Keys are compared as 64-bit integers; nothing is shifted by a per-lane amount (scripts/lint_isa_last_vgpr.py).
//
// After the re-deal the record is left as a step leaves one: re-dealt hands are sorted; a re-dealt seat that is the current player and
// holds a drawn tile (drawn_tile set, hand_len = 2 mod 3) keeps its last slot last, the slots before it are sorted and drawn_tile names
// the tile now in it; PF_WAITS_VALID is cleared for the re-dealt seats, tp_seat is void; in RMJ_WAIT_RESPONSE the claims of every seat but the discarder
// are rebuilt from the new hands (finalize_outputs alone would rebuild only the seats that were active) and active_mask / ron_offer_mask
// are what the rebuild finds - seat a's own list depends on its own hand only, so it stays and the set is never empty; the player flags
// stay what they were (the rebuild marks no missed win, like the poke of a view into the reference) and the claim lists kept from before
// an accepted call (stale_n) are dropped, as a poke drops them; with wall_meta == 1 the digest of
// the wall that goes away is frozen first (wall_meta = 2), so salt and digest answer what they answered, as rmj_poke_state does.
// NOT rewritten: the event ring.  The MJAI log of a determinized game still tells the true deal - it no longer describes the opponents'
// tiles or the draws to come.
// The sample is uniform over placements of the pool's tiles, NOT over worlds consistent with what the opponents did: in particular a seat
// that has declared riichi may get 13 tiles that are not tenpai - status bits 4..6 report it per opponent, and the caller rejects the
// world, resamples with another seed, holds that hand or asks for the repair below.
//
// RMJ_DETF_RIICHI_TENPAI (k_determinize<V, true>; the definition is in include/riichi_mi355x.h): between the permutation and the sort the
// hand of every re-dealt riichi seat with hand_len = 1 mod 3 walks to tenpai by exchanges of one hand slot with one PARTNER - a canonical
// index whose location is no hand slot of a riichi seat: the pool's wall entries and the hands of the re-dealt opponents not in riichi.
// A step (at most DET_FIX_STEPS per seat, while the shanten number is above 0) judges every (hand slot i, tile type t held by a partner)
// with one per-lane shanten each (hid_shanten over the hand's histogram minus the slot's type plus t, lane = pair, verdicts in LDS),
// takes the step down if a pair gives it and a sideways step otherwise, and among the concrete (slot, partner) pairs with that verdict
// picks the least (det_swap_key, i, j) by a wave reduction.  The result is the nearest tenpai hand by fewest exchanges from a uniform
// deal with seeded ties - not a posterior: no furiten consistency, no weighting by discards or calls, the event ring stays, and a riichi
// seat with hand_len = 2 mod 3 is left to its NOTEN bit.  k_determinize<V, false> is the kernel as it was: no LDS, no code of the repair.
//
// Two launches: k_determinize_claim (one thread per row) judges every row from the untouched records, writes the status of the rows that
// are not carried out and lets the eligible rows of a game compete for the game's claim word (atomic max of epoch << 32 | ~row: the lowest
// row wins, whatever the timing; the epoch - one per call - makes last call's words lose without a memset); k_determinize (one wave per
// row) carries out the rows that hold their game's word.
#pragma once

#define DET_POOL_CAP 192u   // slots of the pool's LDS arrays: three passes of the wave (m <= 164 on any record the step kernels produce)

__host__ __device__ __forceinline__ uint64_t det_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t det_base(uint64_t seed, uint64_t global_game) { return det_mix(seed + global_game); }
__host__ __device__ __forceinline__ uint64_t det_key(uint64_t base, uint32_t seat, uint32_t i) {
    return det_mix(base + (uint64_t)(seat * 256u + i) * 0x9E3779B97F4A7C15ull);
}
// the position of (key, i) in the order by (key, index): how many of keys[0 .. m) come before it
__host__ __device__ __forceinline__ uint32_t det_rank(const uint64_t* keys, uint32_t m, uint64_t key, uint32_t i) {
    uint32_t r = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint64_t kj = keys[j];
        r += (kj < key || (kj == key && j < i)) ? 1u : 0u;
    }
    return r;
}
// the key of the exchange (hand slot i, partner j) in step k of opponent r's walk: offset 1024 keeps it off the permutation's keys
__host__ __device__ __forceinline__ uint64_t det_swap_key(uint64_t base, uint32_t seat, uint32_t r, uint32_t k, uint32_t i, uint32_t j) {
    return det_mix(base + (uint64_t)(1024u + ((((seat * 4u + r) * 16u + k) * 16u + i) * 256u + j)) * 0x9E3779B97F4A7C15ull);
}
__host__ __device__ __forceinline__ unsigned long long det_claim_word(uint32_t epoch, uint32_t row) { return ((unsigned long long)epoch << 32) | (0xFFFFFFFFu - row); }

// what the kernel takes from the variant's step header (rmj4:: / rmj3::)
struct DetV4 {
    typedef rmj4::Ctx Ctx;
    static constexpr uint32_t NP = 4u, DORA0 = 4u;
    static constexpr int TILES = 136;
    static __device__ __forceinline__ void sort(Ctx& c, PState& P, int n) { rmj4::sort_hand(c, P, n); }
    static __device__ __forceinline__ uint64_t waits(Ctx& c, int s) { return rmj4::seat_waits(c, s); }
    static __device__ __forceinline__ bool claims(Ctx& c, int i, int pid, int tile) { return rmj4::gen_claims(c, i, pid, tile, false); }
    static __device__ __forceinline__ void publish(Ctx& c) { rmj4::finalize_outputs<false>(c, true, false); }
    static __device__ __forceinline__ void freeze(const uint8_t* W, uint32_t* out) { rmj4::freeze_wall_digest(W, TILES, out); }
};
struct DetV3 {
    typedef rmj3::Ctx Ctx;
    static constexpr uint32_t NP = 3u, DORA0 = 8u;
    static constexpr int TILES = 108;
    static __device__ __forceinline__ void sort(Ctx& c, PState& P, int n) { rmj3::sort_hand(c, P, n); }
    static __device__ __forceinline__ uint64_t waits(Ctx& c, int s) { return rmj3::seat_waits(c, s); }
    static __device__ __forceinline__ bool claims(Ctx& c, int i, int pid, int tile) { return rmj3::gen_claims(c, i, pid, tile, false); }
    static __device__ __forceinline__ void publish(Ctx& c) { rmj3::finalize_outputs<false>(c, true, false); }
    static __device__ __forceinline__ void freeze(const uint8_t* W, uint32_t* out) { rmj3::freeze_wall_digest(W, TILES, out); }
};

struct DetArgs {
    const int32_t* index;
    const uint32_t* count;
    const uint8_t* hold;
    uint8_t* status;
    unsigned long long* claim;   // [n_games]
    uint64_t seed;
    uint32_t rows, epoch;
};
__device__ __forceinline__ uint32_t det_rows(const DetArgs& A) {
    uint32_t lim = A.rows;
    if (A.count) { const uint32_t c = *A.count; lim = c < lim ? c : lim; }
    return lim;
}

// one thread per row: the status of the rows that are not carried out, and the claim of the rows that could be
__global__ __launch_bounds__(256) void k_determinize_claim(Env E, DetArgs A) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= det_rows(A)) return;
    const uint32_t ix = (uint32_t)A.index[row];   // (a negative index is a large one)
    const uint32_t NP = E.game_mode >= 3u ? 3u : 4u;
    uint32_t st = RMJ_DET_NOT_ACTING;
    if (ix < E.n_games * 4u) {
        const uint32_t g = ix >> 2, a = ix & 3u;
        const GState& S = E.core[g];
        if (a < NP && !S.is_done && (((uint32_t)S.active_mask >> a) & 1u)) {
            // the claims on a robbed kan / kita cannot be rebuilt (k_refresh leaves such a record alone as well), nor those on no discard at all
            if (S.pending_kan_pid != 0xFF || (S.phase == RMJ_WAIT_RESPONSE && S.last_discard_pid == 0xFF)) {
                st = RMJ_DET_CHANKAN;
            } else {
                st = RMJ_DET_DUPLICATE;   // unless k_determinize finds the game's word to be this row's
                atomicMax(A.claim + g, det_claim_word(A.epoch, row));
            }
        }
    }
    if (A.status) A.status[row] = (uint8_t)st;
}

struct DetPool {
    uint64_t key[DET_POOL_CAP];
    uint8_t loc[DET_POOL_CAP];   // where canonical slot i lives: seat * 16 + hand slot, or 64 + wall position
};

// ---- RMJ_DETF_RIICHI_TENPAI: the walk of the re-dealt riichi hands to tenpai
#define DET_FIX_STEPS 12u
#define DET_FIX_NONE 0xFFFFFFFFu
struct DetFix {
    uint8_t ver[14 * 34];   // shanten of the hand with slot i's tile replaced by type t, at i * 34 + t; 99 = no such pair
    uint8_t qh[36];         // the partners' tiles by type (34 counts; updated a 32-bit word at a time)
};
// the histogram of P.hand[0 .. n), wave-uniform
__device__ __forceinline__ PH det_hand_ph(const PState& P, uint32_t n) {
    PH h{0u, 0u, 0u, 0u};
    for (uint32_t i = 0; i < n; i++) ph_add(h, (int)min((uint32_t)P.hand[i] >> 2, 33u));
    return h;
}
// All 64 lanes call with wave-uniform arguments, behind the permutation and a wave_sync; true if a tile was exchanged.
template <class V>
__device__ __forceinline__ bool det_repair(typename V::Ctx& c, GState& S, const DetPool& D, DetFix& F, const ShantenTables& T, uint64_t base,
                                           uint32_t a, uint32_t hold, uint32_t m, int lane) {
    constexpr bool sanma = V::NP == 3u;
    uint32_t riichi = 0;
    for (uint32_t s = 0; s < V::NP; s++) riichi |= (rmj4::U((int)S.p[s].flags) & PF_RIICHI_DECLARED) ? 1u << s : 0u;
    riichi = (uint32_t)__builtin_amdgcn_readfirstlane((int)riichi);   // (the same in every lane: scalar from here on, like n and cur below)
    bool swapped = false;
    for (uint32_t r = 0; r + 1u < V::NP; r++) {
        const uint32_t x = a + 1u + r, s = x >= V::NP ? x - V::NP : x;
        if (((hold >> r) & 1u) || !((riichi >> s) & 1u)) continue;
        PState& P = S.p[s];
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)min((uint32_t)rmj4::U((int)P.hand_len), 14u));
        if (n % 3u != 1u) continue;
        PH h = det_hand_ph(P, n);
        int cur = __builtin_amdgcn_readfirstlane(hid_shanten(h, (int)(n / 3u), sanma, T));
        for (uint32_t k = 0; k < DET_FIX_STEPS && cur > 0; k++) {
            // the partners of this lane (canonical indices lane, lane + 64, lane + 128) and the types they hold
            uint32_t pt[3];
            if (lane < 36) F.qh[lane] = 0;
            wave_sync();
#pragma unroll
            for (uint32_t q = 0; q < 3u; q++) {
                const uint32_t j = (uint32_t)lane + 64u * q;
                pt[q] = DET_FIX_NONE;
                if (j < m) {
                    const uint32_t l = D.loc[j];
                    if (l >= 64u || !((riichi >> (l >> 4)) & 1u)) {
                        pt[q] = min((l < 64u ? (uint32_t)S.p[l >> 4].hand[l & 15u] : (uint32_t)c.X.tiles[l - 64u]) >> 2, 33u);
                        atomicAdd(reinterpret_cast<uint32_t*>(F.qh) + (pt[q] >> 2), 1u << (8u * (pt[q] & 3u)));   // (at most 4 of a type: no carry)
                    }
                }
            }
            wave_sync();
            // the verdict of every (slot, type) pair, lane = pair
            bool down = false, side = false;
            for (uint32_t p = (uint32_t)lane; p < n * 34u; p += 64u) {
                const uint32_t i = p / 34u, t = p - i * 34u, d = min((uint32_t)P.hand[i] >> 2, 33u);
                int v = 99;
                if (d != t && F.qh[t] != 0) {
                    PH y = h;
                    ph_sub(y, (int)d);
                    ph_add(y, (int)t);
                    v = hid_shanten(y, (int)(n / 3u), sanma, T);
                }
                F.ver[p] = (uint8_t)v;
                down |= v == cur - 1;
                side |= v == cur;
            }
            wave_sync();
            const bool dn = __ballot(down) != 0ull;
            if (!dn && __ballot(side) == 0ull) break;
            const int want = dn ? cur - 1 : cur;
            // the least (key, i, j) over the concrete pairs with that verdict
            uint64_t bk = ~0ull;
            uint32_t bij = DET_FIX_NONE;
#pragma unroll
            for (uint32_t q = 0; q < 3u; q++) {
                if (pt[q] == DET_FIX_NONE) continue;
                const uint32_t j = (uint32_t)lane + 64u * q;
                for (uint32_t i = 0; i < n; i++) {
                    if ((int)F.ver[i * 34u + pt[q]] != want) continue;
                    const uint64_t key = det_swap_key(base, a, r, k, i, j);
                    const uint32_t ij = i * 256u + j;
                    if (key < bk || (key == bk && ij < bij)) { bk = key; bij = ij; }
                }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const uint64_t ok = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(bk >> 32), off, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)bk, off, 64);
                const uint32_t oij = (uint32_t)__shfl_xor((int)bij, off, 64);
                if (ok < bk || (ok == bk && oij < bij)) { bk = ok; bij = oij; }
            }
            bij = (uint32_t)__builtin_amdgcn_readfirstlane((int)bij);
            if (bij == DET_FIX_NONE) break;   // (a verdict without a pair: cannot happen, and nothing is touched if it does)
            const uint32_t i = min(bij >> 8, n - 1u), l = D.loc[min(bij & 255u, DET_POOL_CAP - 1u)];
            wave_sync();
            if (lane == 0) {
                const uint8_t mine = P.hand[i];
                if (l < 64u) { P.hand[i] = S.p[l >> 4].hand[l & 15u]; S.p[l >> 4].hand[l & 15u] = mine; }
                else { P.hand[i] = c.X.tiles[l - 64u]; c.X.tiles[l - 64u] = mine; }
            }
            wave_sync();
            h = det_hand_ph(P, n);
            cur = want;
            swapped = true;
        }
    }
    return swapped;
}

template <class V, bool FIX = false>
__global__ __launch_bounds__(256, 4) void k_determinize(const Env* __restrict__ Ep, DetArgs A) {   // (the bounds of k_apply_event: the out-of-line functions both reach keep the register budget they had)
    CEnv& E = *(CEnv*)Ep;
    __shared__ BlockShared sh;
    __shared__ DetPool pool[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * WPB + (uint32_t)wave;
    if (row >= det_rows(A)) return;
    const uint32_t ix = (uint32_t)__builtin_amdgcn_readfirstlane(A.index[row]);
    if (ix >= E.n_games * 4u) return;
    const uint32_t g = ix >> 2, a = ix & 3u;
    if (A.claim[g] != det_claim_word(A.epoch, row)) return;   // not eligible, or another row of this call has the game
    const uint32_t hold = A.hold ? (uint32_t)__builtin_amdgcn_readfirstlane((int)A.hold[row]) : 0u;
    GState& S = sh.st[wave];
    DetPool& D = pool[wave];
    load_state(S, E.core + g, lane);
    typename V::Ctx c{S, E, sh.x[wave], g, lane, E.wall + (size_t)g * RMJ_WALL_STRIDE, E.legal + (size_t)g * 4 * RMJ_MAX_LEGAL};
    if (lane < RMJ_WALL_STRIDE / 4) reinterpret_cast<uint32_t*>(c.X.tiles)[lane] = reinterpret_cast<const uint32_t*>(c.W)[lane];

    // ---- the pool in canonical order: D.loc
    uint32_t m = 0, redeal = 0;
    for (uint32_t r = 0; r + 1u < V::NP; r++) {
        if ((hold >> r) & 1u) continue;
        const uint32_t x = a + 1u + r, s = x >= V::NP ? x - V::NP : x;
        const uint32_t hl = min((uint32_t)rmj4::U((int)S.p[s].hand_len), 14u);
        if ((uint32_t)lane < hl) D.loc[m + lane] = (uint8_t)(s * 16u + lane);
        m += hl;
        redeal |= 1u << s;
    }
    {
        const uint32_t rc = (uint32_t)rmj4::U((int)S.rinshan_count), le = min((uint32_t)rmj4::U((int)S.live_end), 136u);
        const uint32_t nd = min((uint32_t)rmj4::U((int)S.n_dora), 5u);
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t p = (uint32_t)lane + 64u * k;
            const bool shown = p >= V::DORA0 && ((p - V::DORA0) & 1u) == 0u && (p - V::DORA0) / 2u < nd;
            const bool in = p >= rc && p < le && !shown;
            const uint64_t b = __ballot(in);
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (in) D.loc[m + before] = (uint8_t)(64u + p);
            m += (uint32_t)__popcll(b);
        }
    }
    wave_sync();

    // ---- keys, ranks, and every old tile to its new place
    const uint64_t base = det_base(A.seed, E.game_offset + g);
    uint64_t key[3];
    uint32_t old[3];
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        const uint32_t i = (uint32_t)lane + 64u * k;
        key[k] = 0ull; old[k] = 0u;
        if (i < m) {
            const uint32_t l = D.loc[i];
            old[k] = l < 64u ? (uint32_t)S.p[l >> 4].hand[l & 15u] : (uint32_t)c.X.tiles[l - 64u];
            key[k] = det_key(base, a, i);
            D.key[i] = key[k];
        }
    }
    wave_sync();
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        const uint32_t i = (uint32_t)lane + 64u * k;
        if (i < m) {
            const uint32_t l = D.loc[det_rank(D.key, m, key[k], i)];
            if (l < 64u) S.p[l >> 4].hand[l & 15u] = (uint8_t)old[k];
            else c.X.tiles[l - 64u] = (uint8_t)old[k];
        }
    }
    wave_sync();

    bool swapped = false;
    if constexpr (FIX) {   // ---- RMJ_DETF_RIICHI_TENPAI: re-dealt riichi hands walk to tenpai before anything is sorted
        __shared__ __attribute__((aligned(4))) DetFix fix[WPB];
        const ShantenTables T = sh_tables_of(E);
        swapped = det_repair<V>(c, S, D, fix[wave], T, base, a, hold, m, lane);
    }

    // ---- the record as a step keeps it
    const uint32_t cp = (uint32_t)rmj4::U((int)S.current_player);
    for (uint32_t s = 0; s < V::NP; s++) {
        if (!((redeal >> s) & 1u)) continue;
        PState& P = S.p[s];
        const int hl = min(rmj4::U((int)P.hand_len), 14);
        const bool drawn = s == cp && rmj4::U((int)S.drawn_tile) != 0xFF && hl % 3 == 2;
        V::sort(c, P, drawn ? hl - 1 : hl);
        if (drawn) S.drawn_tile = P.hand[hl - 1];
        P.flags &= ~PF_WAITS_VALID;
    }
    if (rmj4::U((int)S.wall_meta) == 1) {   // salt and digest stay those of the shuffled wall (state/wall.rs:69-80): the digest is evaluated now
        if (lane == 0) V::freeze(c.W, E.wall_dg + (size_t)g * 8);
        S.wall_meta = 2;
    }
    wave_sync();
    if (lane < RMJ_WALL_STRIDE / 4) reinterpret_cast<uint32_t*>(c.W)[lane] = reinterpret_cast<const uint32_t*>(c.X.tiles)[lane];
    wave_sync();

    // ---- status bits 4..6: a re-dealt seat in riichi whose 13 tiles wait on nothing
    uint32_t st = swapped ? RMJ_DET_SWAPPED : RMJ_DET_OK;
    for (uint32_t r = 0; r + 1u < V::NP; r++) {
        const uint32_t x = a + 1u + r, s = x >= V::NP ? x - V::NP : x;
        if (!((redeal >> s) & 1u) || (hold >> r) & 1u) continue;
        if ((rmj4::U((int)S.p[s].flags) & PF_RIICHI_DECLARED) && V::waits(c, (int)s) == 0ull) st |= RMJ_DET_RIICHI_NOTEN << r;
    }

    // ---- claims of every seat but the discarder from the new hands, then the publication.  Claim lists kept from before an accepted call
    // (GState::stale_n) name tiles of the old hands: dropped for every seat, as a poke drops them.
    if (lane < 4) S.stale_n[lane] = 0;
    wave_sync();
    if (rmj4::U((int)S.phase) == RMJ_WAIT_RESPONSE) {
        const int pid = rmj4::U((int)S.last_discard_pid), tile = rmj4::U((int)S.last_discard_tile);
        uint32_t got = 0;
        S.ron_offer_mask = 0;
        for (int i = 0; i < 4; i++) {
            c.X.nl[i] = 0;
            c.X.wout[i] = 0;
            if (i >= (int)V::NP || i == pid) continue;
            if (V::claims(c, i, pid, tile)) got |= 1u << i;
        }
        S.active_mask = (uint8_t)got;
    }
    V::publish(c);
    store_state(S, E.core + g, lane);
    if (A.status && lane == 0) A.status[row] = (uint8_t)st;
}
