// Discard efficiency table: for a hand, the shanten after every discard, the draws that then lower it and how many of them are live -
// the per-discard numbers the ukeire walk (rmj_shanten.hip.h, rmj_ukeire.hip.h) holds in the discard's type lane before it folds them
// to a maximum.  The label of an efficiency head (next to the hidden and danger rows), the leaf value of a search, the core of a "which
// tile do I cut" tool.  Included from rmj_api.hip behind rmj_danger.hip.h (LogRun, lr_emits, obs_block_prefix as there).
//
// The table of a hand histogram c[34] of n tiles and a visible histogram v[34] (include/riichi_mi355x.h states the same):
//   valid types   all 34 in 4P; type 0 and types 8..33 in 3P (SANMA_VALID_TILE_TYPES, shanten.rs:244-247)
//   sh(x)         calculate_shanten / _3p of x with tiles / 3 groups (rmj_shanten)
//   for x of 3k+1 tiles: A(x) = { t valid : x[t] < 4 and sh(x + t) < sh(x) }, accept(x) = |A(x)|,
//                 ukeire(x) = sum over A of max(0, max(0, 4 - v[t]) - x[t]), mask(x) = the bits of A
//   column t < 34 if n % 3 == 2 and c[t] > 0: x = c - e_t, shanten[t] = sh(x), accept[t], ukeire[t], mask[t] - discards that raise the
//                 shanten included; otherwise shanten[t] = RMJ_DTAB_NONE and the rest 0
//   column 34     shanten = sh(c); n % 3 == 1: accept and mask of c; n % 3 == 2: accept and ukeire are, separately, the maxima over
//                 the t with shanten[t] <= shanten[34] (calculate_effective_tiles_with_discard / calculate_best_ukeire, shanten.rs:304-393),
//                 mask 0; n % 3 == 0: the shanten only.  ukeire[34] of a 3n+1 hand is calculate_best_ukeire of it too, so that column 34
//                 is what rmj_shanten / rmj_effective_tiles / rmj_best_ukeire and channels 78..80 of the extended features say of EVERY
//                 hand: the reference walks the discards of a 3n+1 hand as well - the maximum of ukeire(c - e_d) over the held d with
//                 sh(c - e_d) <= sh(c), the 3n hands judged with (n - 1) / 3 groups - and that is not ukeire(c)
// An absent row (index out of range, seat >= NP, more than 14 tiles or a count above 4 in a raw histogram): every shanten RMJ_DTAB_NONE,
// the rest 0.
//
// One wave per row, lane = tile type for the inputs (held / visible count) and lane = column for the outputs.  The walk is the one of
// sh_ukeire_both with lane = draw and one pass per held type - every held type, not only those that keep the shanten - so that the
// ballot of a pass IS the discard's mask and lands in the discard's lane as two 32-bit halves:
//   * 4P hands and the 3P hands that relocate (three honor slots free, no 2m..8m): a hand of the walk is h - d + t and differs from h
//     in at most two suits, so its replacement number is one entry of a merge of two vectors known before the pair is looked at
//     (sh_ukeire_both's round-4 form: one table lookup per same-suit pair, two lane-parallel merges per discard);
//   * the other 3P hands (raw histograms with 2m..8m, fewer than three free honor slots): the full table walk per (discard, draw).
// No 64-bit value is shifted by a per-lane amount (docs/journal_r06.md section 1): ballots are split by constant shifts, the entry of a
// merged vector is read from a 32-bit window (hid_shanten, sh_entry_pm).  The state is only read; no cache is written back.
#pragma once

// The pool's record of a sample (log sample builder, RMJ_LOGREPLAY_DTABLE): shanten [35] i8, accept [35] u8, ukeire [35] u8, 7 spare
// bytes.  The masks stay out of the pool (280 more bytes per slot that no trainer reads).
#define DT_O_SHANTEN 0u
#define DT_O_ACCEPT 35u
#define DT_O_UKEIRE 70u
#define DT_SLOT_BYTES 112u

struct DtRow {   // lane = column
    int sh;
    uint32_t acc, uke, mlo, mhi;
};

// tiles of a type left to draw: 4 - visible - held, both saturating (shanten.rs:380-389)
__device__ __forceinline__ uint32_t dt_left(uint32_t vis, int held) {
    int r = 4 - (int)vis;
    r = r < 0 ? 0 : r;
    r -= held;
    return (uint32_t)(r < 0 ? 0 : r);
}
// the wave's sum of w (0..4) over the lanes with f
__device__ __forceinline__ uint32_t dt_weight_sum(bool f, uint32_t w) {
    w = f ? w : 0u;
    return (uint32_t)__popcll(__ballot(w & 1u)) + 2u * (uint32_t)__popcll(__ballot(w & 2u)) + 4u * (uint32_t)__popcll(__ballot(w & 4u));
}

// The table of ONE wave-uniform hand of at most 14 tiles, counts at most 4; my_cnt / my_vis = this lane's held / visible count
// (0 for lanes >= 34).  All 64 lanes call.
__device__ inline DtRow dt_walk(const ShantenTables& T, const PH& h, uint32_t my_cnt, uint32_t my_vis, bool sm, int lane) {
    const int t = lane;
    const bool t_in = t < 34;
    const bool t_ok = t_in && (!sm || t == 0 || t >= 8);
    const int total = ph_total(h);
    const bool fast = !sm || (__popc(~(h.d | (h.d >> 1) | (h.d >> 2)) & O7_1) >= 3 && (h.a & ~(7u | (7u << 24))) == 0u);
    const int q = t_in ? ((sm && (t == 0 || t == 8)) ? 3 : t_suit(t)) : 0;   // the suit whose vector the tile type changes
    auto word = [&](const PH& y, int qq) -> uint32_t {                        // suit qq of hand y as the tables see it
        if (!sm) return ph_get(y, qq);
        return qq == 0 ? 0u : (qq == 3 ? sh_relocate_3p(y).d : ph_get(y, qq));
    };
    auto finish = [&](int rep, const PH& x, int len_div3) -> int {            // shanten.rs:228-241 / :454-468
        int s0 = rep - 1;
        if (s0 <= 0 || len_div3 < 4) return s0;
        const int c = sh_chiitoi(x, sm);
        s0 = c < s0 ? c : s0;
        if (s0 > 0) { const int k = sh_kokushi(x); s0 = k < s0 ? k : s0; }
        return s0;
    };
    auto m4 = [](int m) -> int { return m > 4 ? 4 : m; };
    DtRow R{RMJ_DTAB_NONE, 0u, 0u, 0u, 0u};
    const bool drawable = t_ok && my_cnt < 4u;
    PH hp = h;
    if (drawable) ph_add(hp, t);
    ShBase Bh{};
    uint64_t O_mine = 0, vt = 0;
    int cur;
    if (fast) {
        const uint64_t mine = sh_vec(word(h, lane & 3), lane & 3, T);
#pragma unroll
        for (int k = 0; k < 4; k++) Bh.v[k] = sh_rl64(mine, k);
        const bool r0 = (lane >> 4) == 0;
        const uint64_t M = sh_merge_rows(r0 ? Bh.v[0] : Bh.v[2], r0 ? Bh.v[1] : Bh.v[3], lane);
        Bh.ab = sh_rl64(M, 15);
        Bh.cd = sh_rl64(M, 31);
        cur = finish(sh_entry_pm(Bh.ab, Bh.cd, m4(total / 3)), h, total / 3);
        // O_q: the three other suits of h merged (row q computes O_q)
        const int rw = lane >> 4;
        const uint64_t pa = rw == 0 ? Bh.v[1] : (rw == 1 ? Bh.v[0] : (rw == 2 ? Bh.v[3] : Bh.v[2]));
        const uint64_t Om = sh_merge_rows(pa, rw < 2 ? Bh.cd : Bh.ab, lane);
        const uint64_t O0 = sh_rl64(Om, 15), O1 = sh_rl64(Om, 31), O2 = sh_rl64(Om, 47), O3 = sh_rl64(Om, 63);
        O_mine = q == 0 ? O0 : (q == 1 ? O1 : (q == 2 ? O2 : O3));
        if (drawable) vt = sh_vec(word(hp, q), q, T);   // this lane's suit with the lane's type drawn
    } else {
        cur = hid_shanten(h, total / 3, sm, T);
    }
    uint32_t c_acc = 0u, c_uke = 0u;   // column 34, wave-uniform
    uint64_t c_mask = 0ull;
    if (total % 3 == 1) {
        bool f = false;
        if (drawable) {
            const int d3 = (total + 1) / 3;
            f = (fast ? finish(sh_entry_pm(vt, O_mine, m4(d3)), hp, d3) : hid_shanten(hp, d3, sm, T)) < cur;
        }
        c_mask = __ballot(f);
        c_acc = (uint32_t)__popcll(c_mask);
    }
    // the walk over the hand's own discards.  3n+2: the columns, and the maxima of column 34.  3n+1: calculate_best_ukeire walks the
    // discards of such a hand all the same (shanten.rs:352-390, 3n hands judged with (n - 1) / 3 groups) - column 34 takes its maximum,
    // no column t < 34 is written
    const bool cols = total % 3 == 2;
    if (total % 3 != 0 && total > 0) {
        const int d3 = total / 3, s3 = (total - 1) / 3;   // hands of the loop hold total tiles again (h - d + t)
        int nsh_l = RMJ_DTAB_NONE;                        // lane = type: shanten after discarding one tile of it
        uint64_t nv_d = 0;
        if (t_in && my_cnt > 0u) {
            PH sub = h;
            ph_sub(sub, t);
            if (fast) {
                nv_d = sh_vec(word(sub, q), q, T);
                nsh_l = finish(sh_entry_pm(nv_d, O_mine, m4(s3)), sub, s3);
            } else {
                nsh_l = hid_shanten(sub, s3, sm, T);
            }
        }
        if (cols) R.sh = nsh_l;
        uint64_t Pt = 0;   // this lane's suit with the type drawn (+) its partner suit
        if (fast && drawable) Pt = sh_merge(vt, q == 0 ? Bh.v[1] : (q == 1 ? Bh.v[0] : (q == 2 ? Bh.v[3] : Bh.v[2])));
        uint64_t held = __ballot(t_in && my_cnt > 0u);
        while (held) {
            const int d = __ffsll((long long)held) - 1;
            held &= held - 1ull;
            const int nsh = __builtin_amdgcn_readlane(nsh_l, d);
            PH sub = h;
            ph_sub(sub, d);
            const bool can = t_ok && ph_cnt(sub, t) < 4;
            PH x = sub;
            if (can) ph_add(x, t);
            bool f = false;
            if (fast) {
                // t in the suit of d: entry(vec(suit of h - d + t), O_q); in its partner suit: entry(vec(suit of h + t), W_d), W_d = vec(suit of
                // h - d) (+) the other half of h; in the other half: entry(P_t, H_d), H_d = vec(suit of h - d) (+) its partner suit
                const int qd = (sm && (d == 0 || d == 8)) ? 3 : t_suit(d);
                const uint64_t V = sh_rl64(nv_d, d);
                const uint64_t pd = qd == 0 ? Bh.v[1] : (qd == 1 ? Bh.v[0] : (qd == 2 ? Bh.v[3] : Bh.v[2]));
                const uint64_t xd = qd < 2 ? Bh.cd : Bh.ab;
                const uint64_t HW = sh_merge_rows(V, (lane >> 4) == 0 ? pd : xd, lane);   // row 0: H_d, row 1: W_d
                const uint64_t Hd = sh_rl64(HW, 15), Wd = sh_rl64(HW, 31);
                if (can) {
                    uint64_t a, b;
                    if (q == qd) { a = sh_vec(word(x, q), q, T); b = O_mine; }
                    else if ((q ^ 1) == qd) { a = vt; b = Wd; }
                    else { a = Pt; b = Hd; }
                    f = finish(sh_entry_pm(a, b, m4(d3)), x, d3) < nsh;
                }
            } else if (can) {
                f = hid_shanten(x, d3, sm, T) < nsh;
            }
            const uint64_t fb = __ballot(f);
            const uint32_t e = (uint32_t)__popcll(fb);
            const uint32_t u = dt_weight_sum(f, dt_left(my_vis, (int)my_cnt - (t == d ? 1 : 0)));
            if (cols && lane == d) { R.acc = e; R.uke = u; R.mlo = (uint32_t)fb; R.mhi = (uint32_t)(fb >> 32); }
            if (nsh <= cur) {
                if (cols) c_acc = e > c_acc ? e : c_acc;
                c_uke = u > c_uke ? u : c_uke;
            }
        }
    }
    if (lane == 34) { R.sh = cur; R.acc = c_acc; R.uke = c_uke; R.mlo = (uint32_t)c_mask; R.mhi = (uint32_t)(c_mask >> 32); }
    return R;
}

// The row of (game g, seat a): the seat's concealed tiles by type against the histogram the efficiency block of encode_extended counts
// (encode.rs:317-327: every seat's discards, every seat's meld tiles - 4 for kans - and the revealed dora indicators).  `ok` = the pair
// exists.  g, a and ok must be wave-uniform; all 64 lanes call.
__device__ __forceinline__ DtRow dtable_row(const Env& E, uint32_t g, uint32_t a, bool ok, int lane) {
    const bool sanma = E.game_mode >= 3u;
    const uint32_t NP = sanma ? 3u : 4u;
    if (!(ok && a < NP)) return DtRow{RMJ_DTAB_NONE, 0u, 0u, 0u, 0u};
    const GState& S = E.core[g];
    const PH h = build_ph_wave(S.p[a], lane);
    uint32_t my_cnt = 0u, my_vis = 0u;
    if (lane < 34) {
        my_cnt = (uint32_t)ph_cnt(h, lane);
        for (uint32_t s = 0; s < NP; s++) {
            const PState& Q = S.p[s];
            const int nd = min((int)Q.n_discards, 32), nm = min((int)Q.n_melds, 4);
            for (int j = 0; j < nd; j++) my_vis += (Q.discards[j] >> 2) == lane;
            for (int m = 0; m < nm; m++) {
                const int nt = (Q.meld_type[m] >= RMJ_MELD_DAIMINKAN) ? 4 : 3;
                for (int k = 0; k < nt; k++) my_vis += (Q.meld_tiles[m][k] >> 2) == lane;
            }
        }
        const int ndo = min((int)S.n_dora, 5);
        for (int k = 0; k < ndo; k++) my_vis += (S.dora[k] >> 2) == lane;
    }
    return dt_walk(E.sh, h, my_cnt, my_vis, sanma, lane);
}

// the row as the caller's arrays hold it (RmjDiscardTableOut), row `row`; the mask array may be absent
__device__ __forceinline__ void dtable_store(const DtRow& R, const RmjDiscardTableOut& O, size_t row, int lane) {
    if (lane >= RMJ_DTAB_COLS) return;
    const size_t at = row * RMJ_DTAB_COLS + (size_t)lane;
    O.d_shanten[at] = (int8_t)R.sh;
    O.d_accept[at] = (uint8_t)R.acc;
    O.d_ukeire[at] = (uint8_t)R.uke;
    if (O.d_mask) O.d_mask[at] = (uint64_t)R.mlo | ((uint64_t)R.mhi << 32);
}

// The four kernels are templates with an unused parameter: a template kernel is placed in the code object where it is first named, and
// rmj_api.hip names these at its very end (dt_launch_*), behind every other kernel and out-of-line function.  As plain kernels they sat
// where this file is included, in front of the step kernels' instantiations, and moved those 100 096 bytes away from their out-of-line
// callees: bench.py then read 0.15 % lower in six of six alternating pairs with the parent's library.
// rmj_discard_table_device: one wave per row of the index (index[i] = game * 4 + seat); rows at or behind min(rows, *count) stay untouched
template <int PLACED_LAST>
__global__ __launch_bounds__(256) void k_dtable_rows(Env E, const int32_t* __restrict__ index, uint32_t rows, const uint32_t* __restrict__ count, RmjDiscardTableOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t lim = rows;
    if (count) { const uint32_t c = *count; lim = c < lim ? c : lim; }
    if (row >= lim) return;
    const uint32_t ix = (uint32_t)__builtin_amdgcn_readfirstlane(index[row]);
    const bool ok = ix < E.n_games * 4u;   // (a negative index is a large one)
    dtable_store(dtable_row(E, ok ? ix >> 2 : 0u, ix & 3u, ok, lane), O, row, lane);
}

// rmj_discard_table_hands: one wave per raw histogram pair (visible may be absent: all zero)
template <int PLACED_LAST>
__global__ __launch_bounds__(256) void k_dtable_hands(ShantenTables T, const uint8_t* __restrict__ counts, const uint8_t* __restrict__ visible, uint32_t n, int sanma,
                                                      RmjDiscardTableOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n) return;
    const int t = lane;
    const uint32_t my_cnt = t < 34 ? counts[(size_t)i * 34 + t] : 0u;
    const uint32_t my_vis = (t < 34 && visible) ? visible[(size_t)i * 34 + t] : 0u;
    const bool fits = __ballot(my_cnt > 4u) == 0ull;
    // wave-uniform histogram: lane t contributes its field, the four words are OR-reduced over the wave
    PH h = {0, 0, 0, 0};
    {
        const int s = t < 34 ? t_suit(t) : 0;
        const uint32_t f = (t < 34 && fits) ? my_cnt << (3 * (t - 9 * s)) : 0u;
        uint32_t w[4] = {s == 0 ? f : 0u, s == 1 ? f : 0u, s == 2 ? f : 0u, s == 3 ? f : 0u};
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) w[k] |= (uint32_t)__shfl_xor((int)w[k], off, 64);
        }
        h.a = w[0]; h.b = w[1]; h.c = w[2]; h.d = w[3];
    }
    DtRow R{RMJ_DTAB_NONE, 0u, 0u, 0u, 0u};
    if (fits && ph_total(h) <= 14) R = dt_walk(T, h, my_cnt, my_vis, sanma != 0, lane);
    dtable_store(R, O, i, lane);
}

// ---- log sample builder: the table record of every pool slot
// The sibling of k_log_hidden over the same grid: one wave (= block) per decision j of slot s, the same pool slot by the same arithmetic,
// the row of (game = slot, the deciding seat) from the state before the event.
template <int PLACED_LAST>
__global__ __launch_bounds__(64) void k_log_dtable(Env E, LogRun R, uint8_t* __restrict__ dtb) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x >> 2, j = blockIdx.x & 3u;
    if (j >= (uint32_t)R.dec_n[slot]) return;
    const uint32_t seat = R.dec_seat[slot * 4u + j] & 3u;
    const uint64_t s64 = (uint64_t)R.ctr[LR_C_FILL] + obs_block_prefix(R.totals, slot / PPO_SCAN_BLOCK, lane) + R.offs[slot] + j;
    if (s64 >= R.capacity) return;
    const DtRow D = dtable_row(E, slot, seat, true, lane);
    uint8_t* rec = dtb + (size_t)s64 * DT_SLOT_BYTES;
    if (lane < RMJ_DTAB_COLS) {
        rec[DT_O_SHANTEN + lane] = (uint8_t)(int8_t)D.sh;
        rec[DT_O_ACCEPT + lane] = (uint8_t)D.acc;
        rec[DT_O_UKEIRE + lane] = (uint8_t)D.uke;
    }
}

// Emit: the table records of the slots k_log_emit emits, to the same rows (behind k_log_emit_scan, like k_log_emit)
struct LogDtableOut {
    int8_t* shanten;
    uint8_t *accept, *ukeire;
    uint32_t n_rows;
};
template <int PLACED_LAST>
__global__ __launch_bounds__(256) void k_log_emit_dtable(LogRun R, const uint8_t* __restrict__ dtb, LogDtableOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u, w0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t fill = R.ctr[LR_C_FILL];
    for (uint32_t s = w0; s < fill; s += waves) {
        if (!lr_emits(R, s)) continue;
        const uint32_t d = obs_block_prefix(R.totals, s / PPO_SCAN_BLOCK, lane) + R.offs[s];
        if (d >= O.n_rows) continue;
        const uint8_t* rec = dtb + (size_t)s * DT_SLOT_BYTES;
        if (lane < RMJ_DTAB_COLS) {
            const size_t at = (size_t)d * RMJ_DTAB_COLS + (size_t)lane;
            O.shanten[at] = (int8_t)rec[DT_O_SHANTEN + lane];
            O.accept[at] = rec[DT_O_ACCEPT + lane];
            O.ukeire[at] = rec[DT_O_UKEIRE + lane];
        }
    }
}
