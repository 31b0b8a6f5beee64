// Hidden-hand targets: what the three opponents of a (game, hero seat) pair hold and how far their hands are - the second half of a
// training sample (auxiliary heads for opponent tenpai / waits / hand, the input of a perfect-information critic).  The state of every
// game is complete on the device (E.core[g] carries all four hands); this file reads it for the seats the observation hides.
// Included from rmj_api.hip behind every other subsystem, so the code object keeps the kernels it had where they were (LogRun and lr_emits
// come from rmj_logreplay.hip.h, obs_block_prefix from rmj_obs.hip.h).
//
// The row of (g, a): opponent r = 0, 1, 2 is seat s = (a + 1 + r) mod NP - shimocha, toimen, kamicha; in 3P r = 2 is absent (all zero).
//   hand    [34] u8   concealed tiles of s by tile type (red fives count as fives)
//   shanten     i8    calculate_shanten / calculate_shanten_3p of that histogram with total / 3 groups (shanten.rs:244-261 / :470-484)
//   waits       u64   bit t: HandEvaluator(hand, melds).get_waits() holds type t (hand_evaluator.rs:196-213): empty unless concealed +
//                     3 x melds = 13, a type held four times is skipped
//   flags       u8    HID_PRESENT | HID_TENPAI (waits != 0) | HID_RIICHI (riichi_declared) | HID_FURITEN (the waits meet a type of the seat's
//                     discards, or missed_agari_doujun, or missed_agari_riichi) | n_melds << 4
// One wave per row.  The three histograms and wait masks are wave-cooperative and wave-uniform (build_ph_wave, wave_waits: lane = tile
// type); the three shanten numbers are one pass of the table walk with lane r < 3 on opponent r's histogram.  The state is only read: the
// waits13 cache is used where PF_WAITS_VALID proves it current and never written back (sh13 is a lower bound there, not the number).
// No 64-bit value is shifted by a per-lane amount: the furiten test looks the discard's bit up in the 32-bit halves of the mask, and the
// entry of the merged cost vector is taken from a 32-bit window of it (scripts/lint_isa_last_vgpr.py, docs/journal_r06.md section 1).
#pragma once

#define HID_PRESENT 1u
#define HID_TENPAI 2u
#define HID_RIICHI 4u
#define HID_FURITEN 8u
// The pool's record of a sample (log sample builder, RMJ_LOGREPLAY_HIDDEN): three opponents of HID_OPP_BYTES - waits u64, hand [34] u8,
// shanten i8, flags u8, 4 spare bytes - then the event index i32 and a spare word: 152 bytes, 8-byte aligned.
#define HID_OPP_BYTES 48u
#define HID_O_WAITS 0u
#define HID_O_HAND 8u
#define HID_O_SHANTEN 42u
#define HID_O_FLAGS 43u
#define HID_O_EVENT (3u * HID_OPP_BYTES)
#define HID_SLOT_BYTES (3u * HID_OPP_BYTES + 8u)

struct HiddenRow {       // a row in the wave's registers
    uint32_t cnt[3];     // lane t < 34: opponent r's concealed tiles of type t
    uint64_t waits[3];   // wave-uniform from here on
    int shanten[3];
    uint32_t flags[3];
};

// sh_shanten (rmj_shanten.hip.h) with the entry (pair, m) read from a 32-bit window of the merged vector: m differs from lane to lane here
__device__ __forceinline__ int hid_shanten(const PH& h, int len_div3, bool sanma, const ShantenTables& T) {
    const PH x = sanma ? sh_relocate_3p(h) : h;
    const uint64_t r = sh_merge(sh_merge(T.suit[sh_rank(x.a, 9, T.rank9)], T.suit[sh_rank(x.b, 9, T.rank9)]),
                                sh_merge(T.suit[sh_rank(x.c, 9, T.rank9)], T.honor[sh_rank(x.d, 7, T.rank7)]));
    const uint32_t pair_half = (uint32_t)(r >> 20);   // entries (pair = 1, m = 0..4), four bits each
    int s = (int)((pair_half >> (4 * (len_div3 > 4 ? 4 : len_div3))) & 15u) - 1;
    if (s <= 0 || len_div3 < 4) return s;
    const int c = sh_chiitoi(h, sanma);
    s = c < s ? c : s;
    if (s > 0) {
        const int k = sh_kokushi(h);
        s = k < s ? k : s;
    }
    return s;
}

// The row of (game g, hero seat `hero`); `ok` = the pair exists (a row asked for with an index out of range is absent as a whole).
// g, hero and ok must be wave-uniform; all 64 lanes call.
__device__ __forceinline__ HiddenRow hidden_row(const Env& E, uint32_t g, uint32_t hero, bool ok, int lane) {
    const bool sanma = E.game_mode >= 3u;
    const uint32_t NP = sanma ? 3u : 4u;
    HiddenRow H;
    PH h[3];
    int total[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        H.cnt[r] = 0u; H.waits[r] = 0ull; H.shanten[r] = 0; H.flags[r] = 0u;
        h[r] = PH{0u, 0u, 0u, 0u};
        total[r] = 0;
        if (!(ok && hero < NP && (uint32_t)r + 1u < NP)) continue;
        const uint32_t x = hero + 1u + (uint32_t)r, s = x >= NP ? x - NP : x;
        const PState& P = E.core[g].p[s];
        h[r] = build_ph_wave(P, lane);
        total[r] = ph_total(h[r]);
        const uint32_t pf = P.flags, nm = min((uint32_t)P.n_melds, 4u);
        uint64_t W = 0ull;
        if ((uint32_t)total[r] + 3u * nm == 13u) W = (pf & PF_WAITS_VALID) ? P.waits13 : wave_waits(h[r], lane);
        // furiten by the seat's own discards: lane j looks up discard j's type in the mask's halves
        bool hit = false;
        if ((uint32_t)lane < min((uint32_t)P.n_discards, 32u)) {
            const uint32_t d = (uint32_t)P.discards[lane] >> 2;
            hit = d < 32u ? (((uint32_t)W >> d) & 1u) != 0u : (((uint32_t)(W >> 32) >> (d - 32u)) & 1u) != 0u;
        }
        const bool furiten = __ballot(hit) != 0ull || (pf & (PF_MISSED_RIICHI | PF_MISSED_DOUJUN)) != 0u;
        H.waits[r] = W;
        H.flags[r] = HID_PRESENT | (W ? HID_TENPAI : 0u) | ((pf & PF_RIICHI_DECLARED) ? HID_RIICHI : 0u) | (furiten ? HID_FURITEN : 0u) | (nm << 4);
        H.cnt[r] = lane < 34 ? (uint32_t)ph_cnt(h[r], lane) : 0u;
    }
    int sh = 0;
    if (lane < 3) {
        const PH mine = lane == 0 ? h[0] : (lane == 1 ? h[1] : h[2]);
        sh = hid_shanten(mine, (lane == 0 ? total[0] : (lane == 1 ? total[1] : total[2])) / 3, sanma, E.sh);
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int v = __builtin_amdgcn_readlane(sh, r);
        H.shanten[r] = (H.flags[r] & HID_PRESENT) ? v : 0;
    }
    return H;
}

// lane r < 3 stores opponent r's scalars: this lane's pick of the three
__device__ __forceinline__ void hidden_pick(const HiddenRow& H, int lane, uint64_t& w, int& sh, uint32_t& fl) {
    w = lane == 0 ? H.waits[0] : (lane == 1 ? H.waits[1] : H.waits[2]);
    sh = lane == 0 ? H.shanten[0] : (lane == 1 ? H.shanten[1] : H.shanten[2]);
    fl = lane == 0 ? H.flags[0] : (lane == 1 ? H.flags[1] : H.flags[2]);
}
// the row as the caller's four arrays hold it (RmjHiddenOut), row `row`
__device__ __forceinline__ void hidden_store(const HiddenRow& H, const RmjHiddenOut& O, size_t row, int lane) {
    if (lane < 34) {
#pragma unroll
        for (int r = 0; r < 3; r++) O.d_opp_hand[(row * 3 + r) * 34 + lane] = (uint8_t)H.cnt[r];
    }
    if (lane < 3) {
        uint64_t w; int sh; uint32_t fl;
        hidden_pick(H, lane, w, sh, fl);
        O.d_opp_waits[row * 3 + lane] = w;
        O.d_opp_shanten[row * 3 + lane] = (int8_t)sh;
        O.d_opp_flags[row * 3 + lane] = (uint8_t)fl;
    }
}

// rmj_hidden_targets_device: one wave per row of the index (index[i] = game * 4 + seat); rows at or behind min(rows, *count) stay untouched
__global__ __launch_bounds__(256) void k_hidden_targets(Env E, const int32_t* __restrict__ index, uint32_t rows, const uint32_t* __restrict__ count, RmjHiddenOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t lim = rows;
    if (count) { const uint32_t c = *count; lim = c < lim ? c : lim; }
    if (row >= lim) return;
    const uint32_t ix = (uint32_t)__builtin_amdgcn_readfirstlane(index[row]);
    const bool ok = ix < E.n_games * 4u;   // (a negative index is a large one)
    hidden_store(hidden_row(E, ok ? ix >> 2 : 0u, ix & 3u, ok, lane), O, row, lane);
}

// ---- log sample builder: the hidden record of every pool slot
// The sibling of k_log_record over the same grid, launched behind it and before the step's k_log_apply: one wave (= block) per decision
// j of slot s, the same pool slot by the same arithmetic, the row of (game = slot, hero = the deciding seat) from the state before the
// event.  A decision that found no pool slot writes nothing here either (k_log_record has counted it).
__global__ __launch_bounds__(64) void k_log_hidden(Env E, LogRun R, uint8_t* __restrict__ hid) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x >> 2, j = blockIdx.x & 3u;
    if (j >= (uint32_t)R.dec_n[slot]) return;
    const uint32_t seat = R.dec_seat[slot * 4u + j] & 3u;
    const uint64_t s64 = (uint64_t)R.ctr[LR_C_FILL] + obs_block_prefix(R.totals, slot / PPO_SCAN_BLOCK, lane) + R.offs[slot] + j;
    if (s64 >= R.capacity) return;
    const HiddenRow H = hidden_row(E, slot, seat, true, lane);
    uint8_t* rec = hid + (size_t)s64 * HID_SLOT_BYTES;
    if (lane < 34) {
#pragma unroll
        for (int r = 0; r < 3; r++) rec[r * HID_OPP_BYTES + HID_O_HAND + lane] = (uint8_t)H.cnt[r];
    }
    if (lane < 3) {
        uint64_t w; int sh; uint32_t fl;
        hidden_pick(H, lane, w, sh, fl);
        uint8_t* o = rec + lane * HID_OPP_BYTES;
        *reinterpret_cast<uint64_t*>(o + HID_O_WAITS) = w;
        o[HID_O_SHANTEN] = (uint8_t)(int8_t)sh;
        o[HID_O_FLAGS] = (uint8_t)fl;
    }
    if (lane == 0) *reinterpret_cast<int32_t*>(rec + HID_O_EVENT) = (int32_t)(R.apply_at[slot] - R.off[R.dec_log[slot]]);
}

// Emit: the hidden records of the slots k_log_emit emits, to the same rows (behind k_log_emit_scan, like k_log_emit)
struct LogHiddenOut {
    RmjHiddenOut rows;
    int32_t* event;
    uint32_t n_rows;
};
__global__ __launch_bounds__(256) void k_log_emit_hidden(LogRun R, const uint8_t* __restrict__ hid, LogHiddenOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u, w0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t fill = R.ctr[LR_C_FILL];
    for (uint32_t s = w0; s < fill; s += waves) {
        if (!lr_emits(R, s)) continue;
        const uint32_t d = obs_block_prefix(R.totals, s / PPO_SCAN_BLOCK, lane) + R.offs[s];
        if (d >= O.n_rows) continue;
        const uint8_t* rec = hid + (size_t)s * HID_SLOT_BYTES;
        if (lane < 34) {
#pragma unroll
            for (int r = 0; r < 3; r++) O.rows.d_opp_hand[((size_t)d * 3 + r) * 34 + lane] = rec[r * HID_OPP_BYTES + HID_O_HAND + lane];
        }
        if (lane < 3) {
            const uint8_t* o = rec + lane * HID_OPP_BYTES;
            O.rows.d_opp_waits[(size_t)d * 3 + lane] = *reinterpret_cast<const uint64_t*>(o + HID_O_WAITS);
            O.rows.d_opp_shanten[(size_t)d * 3 + lane] = (int8_t)o[HID_O_SHANTEN];
            O.rows.d_opp_flags[(size_t)d * 3 + lane] = o[HID_O_FLAGS];
        }
        if (lane == 0) O.event[d] = *reinterpret_cast<const int32_t*>(rec + HID_O_EVENT);
    }
}
