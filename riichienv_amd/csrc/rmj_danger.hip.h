// Deal-in danger targets: for a (game, hero seat) pair, every opponent and every tile kind, the points that opponent would win by ron if the
// hero discarded that tile now - the label of a danger head, a folding policy or a search leaf.  A wait mask (rmj_hidden.hip.h) is not that
// label: a furiten wait, a wait whose hand has no yaku and a tile the seat discarded itself cost nothing, a live one anything from 1 000
// points up.  Only the hand evaluator knows; this file brings the row-form evaluator (e4_calc, rmj_eval4.hip.h) to the seats the
// observation hides.  Included from rmj_api.hip behind rmj_hidden.hip.h (LogRun, lr_emits, obs_block_prefix as there).
//
// The row of (g, a): opponent r = 0, 1, 2 is seat s = (a + 1 + r) mod NP (3P: r = 2 absent).  Kind k < 34: tile type k as the non-red id
// 4 k + 1; kinds 34, 35, 36: ids 16, 52, 88, copy 0 of the fives (the red ones where the mode has them; the mode is not consulted).
// danger[r][k] is the ron branch of gen_claims followed by the per-winner part of ol_settle_ron (rmj_step.hip.h), 0 unless
//   * s holds concealed + 3 x melds = 13 (a seat with a drawn tile has no ron) and the type of k is among its waits (waits13 where
//     PF_WAITS_VALID proves it current, wave_waits otherwise; never stored back),
//   * the type is not among s's own discards, no wait of s is (furiten), neither missed_agari flag is set,
//   * the evaluation is a win (a yaku other than dora, or a yakuman);
// then the value is ron_agari under base_cf(s) (riichi, double riichi, ippatsu), CF_HOUTEI when drawable_count == 0 && !is_rinshan, no
// chankan, the seat's and the round's wind, the dora indicators revealed now, kita_count = n_kita in 3P, honba = S.honba, capped like
// cap_double under the handle's rule bits.  Ura indicators (the wall at the indices seat_calc_impl uses) count only under RMJ_DANGER_URA
// and only for a seat in riichi.
// Deviations from what the settlement moves: riichi sticks are not part of the value (the winner takes them, the discarder does not pay
// them); a pao split is not applied (the value is the winner's gain; with a liable third seat the discarder pays less); of several
// simultaneous winners only the nearest takes honba, here every opponent is valued as the only and first winner; the sanchaho draw is
// ignored; a kan-dora indicator pending at the moment of the row (pending_kan_dora > 0) is revealed with the discard itself and not counted.
//
// One wave per row.  Per opponent the 13-tile histogram, the meld aggregate (lane = meld inside every 16-lane row, as r4_seat_eval does),
// the red fives, the indicators' dora types (lane = indicator) and the conditions are built once.  The candidates are the set bits of the
// wait mask plus a red kind for each five among them; e4_calc evaluates one hand per 16-lane DPP row, and here the four rows take FOUR
// DIFFERENT candidates per pass: the E4In differs in hand14, win34, aka and the dora counts only.  Lane k < 37 keeps the value of kind k and
// stores it once.  The state is only read.  No 64-bit value is shifted by a per-lane amount: the candidate mask lives in two 32-bit scalars.
#pragma once

#define DNG_SLOT_BYTES 224u   // the pool's record of a sample (RMJ_LOGREPLAY_DANGER): [3][37] u16 in hundreds of points (every ron value is a multiple of 100) + 2 spare bytes

__device__ __forceinline__ uint32_t dng_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// cap_double (rmj_step.hip.h) of a ron result under the rule bits: a double yakuman whose rule bit is off counts once
__device__ __forceinline__ uint32_t dng_capped_ron(const E4Out& o, uint32_t rule_bits, bool is_oya, uint32_t honba, uint32_t np) {
    uint32_t ron = o.ron;
    if (o.yakuman && o.han > 13) {
        int cap = 0;
        if (((o.ym >> 47) & 1ull) && !(rule_bits & RMJ_RULE_JUNSEI_CHUUREN_DOUBLE)) cap += 13;
        if (((o.ym >> 48) & 1ull) && !(rule_bits & RMJ_RULE_SUUANKOU_TANKI_DOUBLE)) cap += 13;
        if (((o.ym >> 49) & 1ull) && !(rule_bits & RMJ_RULE_KOKUSHI13_DOUBLE)) cap += 13;
        if (((o.ym >> 50) & 1ull) && !(rule_bits & RMJ_RULE_DAISUUSHII_DOUBLE)) cap += 13;
        if (cap > 0) {
            const int h = o.han > cap ? o.han - cap : 0;
            ron = calc_score((uint32_t)(h < 13 ? 13 : h), 0u, is_oya, false, honba, np).ron;
        }
    }
    return ron;
}

// The row of (game g, hero seat `hero`), stored as out[r * 37 + k] = points / DIV (T = int32_t, DIV = 1: the caller's array; T = uint16_t,
// DIV = 100: the pool's record).  `ok` = the pair exists (an index out of range gives an all-zero row).  g, hero, ok and use_ura must be
// wave-uniform; all 64 lanes call.
template <typename T, uint32_t DIV>
__device__ __forceinline__ void danger_row(const Env& E, uint32_t g, uint32_t hero, bool ok, bool use_ura, int lane, T* __restrict__ out) {
    const bool sanma = E.game_mode >= 3u;
    const uint32_t NP = sanma ? 3u : 4u;
    const int r16 = lane & 15, rb = lane & 48, q = lane >> 4;
    const GState& S = E.core[g];
    const uint8_t* Wg = E.wall + (size_t)g * RMJ_WALL_STRIDE;
#pragma unroll 1
    for (uint32_t r = 0; r < 3u; r++) {
        uint32_t val = 0u;   // lane k < 37: the value of kind k
        const uint32_t x = hero + 1u + r, s = (x >= NP ? x - NP : x) & 3u;
        const PState& P = S.p[s];
        bool live = ok && hero < NP && r + 1u < NP;
        PH h13 = PH{0u, 0u, 0u, 0u};
        uint32_t pf = 0u, nm = 0u;
        if (live) {
            h13 = build_ph_wave(P, lane);
            pf = dng_u(P.flags); nm = min(dng_u(P.n_melds), 4u);
            live = (uint32_t)ph_total(h13) + 3u * nm == 13u;
        }
        uint32_t mlo = 0u, mhi = 0u;   // the candidate kinds still to evaluate: bits 0..31 / 32..36
        if (live) {
            const uint64_t W = ((pf & PF_WAITS_VALID) ? P.waits13 : wave_waits(h13, lane)) & 0x3FFFFFFFFull;
            const uint64_t own = P.discard_type_mask;
            const uint32_t wlo = dng_u((uint32_t)W), whi = dng_u((uint32_t)(W >> 32));
            const uint32_t hit = dng_u((uint32_t)(W & own) | (uint32_t)((W & own) >> 32));
            if (hit == 0u && !(pf & (PF_MISSED_RIICHI | PF_MISSED_DOUJUN))) {   // not furiten: every wait is live (none of them is among the own discards)
                mlo = wlo;
                mhi = whi | (((wlo >> 4) & 1u) << 2) | (((wlo >> 13) & 1u) << 3) | (((wlo >> 22) & 1u) << 4);
            }
        }
        if ((mlo | mhi) != 0u) {
            // ---- what every candidate of this opponent shares
            const uint32_t hl = min(dng_u(P.hand_len), 14u);
            int aka13 = __popcll(__ballot((uint32_t)lane < hl && is_aka((int)P.hand[lane < 14 ? lane : 0])));
            uint32_t ma_ = 0, mb_ = 0, mc_ = 0, md_ = 0;   // lane = meld (inside every row): the meld tiles' histogram and the packed words
            E4Meld mp;
            {
                const bool mv = (uint32_t)r16 < nm;
                const int m = r16 & 3;
                const uint32_t type = P.meld_type[m];
                const int nt = type >= RMJ_MELD_DAIMINKAN ? 4 : 3;
                const uint32_t t0 = P.meld_tiles[m][0], t1 = P.meld_tiles[m][1], t2 = P.meld_tiles[m][2], t3 = P.meld_tiles[m][3];
                if (mv) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        int t = (int)(k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : t3))) >> 2;
                        t = t < 34 ? t : 33;
                        if (k < nt) {
                            const int su = t_suit(t);
                            const uint32_t one = 1u << (3 * (t - 9 * su));
                            ma_ += su == 0 ? one : 0u; mb_ += su == 1 ? one : 0u; mc_ += su == 2 ? one : 0u; md_ += su == 3 ? one : 0u;
                        }
                    }
                }
                // (a chi made by an MJAI event keeps [called, consumed...] order: its lowest tile is not always first)
                mp = e4_meld_lane(mv, type, nt, t0, t1, t2, t3, (int)((type == RMJ_MELD_CHI ? min(t0, min(t1, t2)) : t0) >> 2), type != RMJ_MELD_CHI,
                                  type != RMJ_MELD_ANKAN);
            }
            const E4Meld ma = e4_meld_reduce(mp, rb);
            aka13 += e4m_aka(ma);
            PH full13 = h13;
            full13.a += e4_rsum(ma_, rb); full13.b += e4_rsum(mb_, rb); full13.c += e4_rsum(mc_, rb); full13.d += e4_rsum(md_, rb);
            const int kita = sanma ? (int)dng_u(P.n_kita) : 0;
            // lane = indicator (inside every row): the type it makes dora, -1 = none
            const bool riichi = (pf & PF_RIICHI_DECLARED) != 0u;
            int dn = -1, un = -1;
            if (r16 < 5 && (uint32_t)r16 < dng_u(S.n_dora)) {
                const int d = (int)S.dora[r16] >> 2;
                dn = next_dora34(d < 34 ? d : 33, sanma);
                const int idx = sanma ? 9 + 2 * r16 : 5 + 2 * r16;   // _get_ura_indicators; 3P: pre-extracted, no bound
                if (use_ura && riichi && (sanma || idx < (int)S.live_end)) {
                    const int u = (int)Wg[idx] >> 2;
                    un = next_dora34(u < 34 ? u : 33, sanma);
                }
            }
            uint32_t cf = 0u;   // base_cf
            if (pf & PF_RIICHI_DECLARED) cf |= CF_RIICHI;
            if (pf & PF_DOUBLE_RIICHI) cf |= CF_DOUBLE_RIICHI;
            if (pf & PF_IPPATSU) cf |= CF_IPPATSU;
            if (dng_u(S.drawable_count) == 0u && !dng_u(S.is_rinshan)) cf |= CF_HOUTEI;
            const uint32_t oya = dng_u(S.oya) & 3u, honba = dng_u(S.honba);
            const uint32_t sw = s + NP - oya;
            E4In in;
            in.ma = ma;
            in.cf = cf;
            in.nuki = kita;
            in.round_wind34 = 27 + (int)(dng_u(S.round_wind) & 3u);
            in.seat_wind34 = 27 + (int)((sw >= NP ? sw - NP : sw) & 3u);
            in.sanma = sanma;
            in.honba = honba;
            // ---- four candidates per pass, one per 16-lane row
            while ((mlo | mhi) != 0u) {
                int kq[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    kq[j] = mlo ? __ffs((int)mlo) - 1 : (mhi ? 31 + __ffs((int)mhi) : -1);
                    if (mlo) mlo &= mlo - 1u; else mhi &= mhi - 1u;
                }
                const int k = q == 0 ? kq[0] : (q == 1 ? kq[1] : (q == 2 ? kq[2] : kq[3]));
                const bool red = k >= 34;
                const int win34 = k < 0 ? 0 : (red ? 4 + 9 * (k - 34) : k);
                in.on = k >= 0;
                in.win34 = win34;
                in.hand14 = h13;
                ph_add(in.hand14, win34);
                in.aka = aka13 + (red ? 1 : 0);
                PH full = full13;
                ph_add(full, win34);
                int dc = 0, uc = 0;
                if (dn >= 0) dc = ph_cnt(full, dn) + ((sanma && dn == 30) ? kita : 0);   // hand_evaluator_3p.rs:110-116
                if (un >= 0) uc = ph_cnt(full, un) + ((sanma && un == 30) ? kita : 0);
                in.dora = (int)(e4_rsum((uint32_t)dc, rb) & 0xFFu);
                in.ura = (int)(e4_rsum((uint32_t)uc, rb) & 0xFFu);
                const E4Out o = e4_calc(in, r16, rb);
                const uint32_t v = (in.on && o.is_win) ? dng_capped_ron(o, E.rule_bits, s == oya, honba, NP) : 0u;
#pragma unroll
                for (int j = 0; j < 4; j++) {   // gather: row j's value to the lane of its kind
                    const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * j);
                    if (lane == kq[j]) val = vj;
                }
            }
        }
        if (lane < (int)RMJ_DANGER_KINDS) out[r * RMJ_DANGER_KINDS + (uint32_t)lane] = (T)(val / DIV);
    }
}

// rmj_danger_targets_device: one wave per row of the index (index[i] = game * 4 + seat); rows at or behind min(rows, *count) stay untouched.
// (The bounds of k_apply_event: the out-of-line wave_waits it reaches keeps the register budget it had.)
__global__ __launch_bounds__(256, 4) void k_danger_targets(Env E, const int32_t* __restrict__ index, uint32_t rows, const uint32_t* __restrict__ count, uint32_t flags,
                                                           int32_t* __restrict__ danger) {
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t lim = rows;
    if (count) { const uint32_t c = *count; lim = c < lim ? c : lim; }
    if (row >= lim) return;
    const uint32_t ix = (uint32_t)__builtin_amdgcn_readfirstlane(index[row]);
    const bool ok = ix < E.n_games * 4u;   // (a negative index is a large one)
    danger_row<int32_t, 1u>(E, ok ? ix >> 2 : 0u, ix & 3u, ok, (flags & RMJ_DANGER_URA) != 0u, lane, danger + (size_t)row * 3u * RMJ_DANGER_KINDS);
}

// ---- log sample builder: the danger record of every pool slot (RMJ_LOGREPLAY_DANGER)
// A sibling of k_log_record over the same grid like k_log_hidden, launched behind it and before the step's k_log_apply: the row of
// (game = slot, hero = the deciding seat) from the state before the event.  No ura: logs carry no wall.
__global__ __launch_bounds__(256, 4) void k_log_danger(Env E, LogRun R, uint8_t* __restrict__ dng) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x >> 2, j = blockIdx.x & 3u;
    if (j >= (uint32_t)R.dec_n[slot]) return;
    const uint32_t seat = R.dec_seat[slot * 4u + j] & 3u;
    const uint64_t s64 = (uint64_t)R.ctr[LR_C_FILL] + obs_block_prefix(R.totals, slot / PPO_SCAN_BLOCK, lane) + R.offs[slot] + j;
    if (s64 >= R.capacity) return;
    danger_row<uint16_t, 100u>(E, slot, seat, true, false, lane, reinterpret_cast<uint16_t*>(dng + (size_t)s64 * DNG_SLOT_BYTES));
}

// Emit: the danger records of the slots k_log_emit emits, widened to int32 points, to the same rows (behind k_log_emit_scan, like k_log_emit)
__global__ __launch_bounds__(256) void k_log_emit_danger(LogRun R, const uint8_t* __restrict__ dng, int32_t* __restrict__ out, uint32_t n_rows) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u, w0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t fill = R.ctr[LR_C_FILL];
    for (uint32_t s = w0; s < fill; s += waves) {
        if (!lr_emits(R, s)) continue;
        const uint32_t d = obs_block_prefix(R.totals, s / PPO_SCAN_BLOCK, lane) + R.offs[s];
        if (d >= n_rows) continue;
        const uint16_t* rec = reinterpret_cast<const uint16_t*>(dng + (size_t)s * DNG_SLOT_BYTES);
        for (uint32_t i = (uint32_t)lane; i < 3u * RMJ_DANGER_KINDS; i += 64u) out[(size_t)d * 3u * RMJ_DANGER_KINDS + i] = (int32_t)rec[i] * 100;
    }
}
