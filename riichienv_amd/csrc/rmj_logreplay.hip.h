// Log sample builder (riichienv-ml datasets/mjai_logs.py:62-129 MCDataset) on the device: many MJAI logs replayed in lock-step from one
// resident event stream, and what the dataset yields per decision - feature row, mask, action id, return, rank - left in a pool.
// Included from rmj_api.hip behind rmj_ppo.hip.h (encode_batch_row, obs_block_prefix come from rmj_obs.hip.h, ppo_block_scan from rmj_ppo.hip.h).
//
// Slots and logs.  The M logs of a log set are replayed in n <= M game slots.  Which slot replays which logs, in which order, is
// fixed before the replay by lr_assign: the logs are handed out in log order, each to the slot that becomes free first when every
// event takes one step (ties to the lowest slot) - what a work queue would do in lock-step, but a pure function of (M, n, the logs'
// lengths), so that the pool order of two runs is the same.  A log that fails frees its slot early; the lists stay as they are.
//
// One event index is four launches: k_log_decide (the decisions the NEXT event of every slot's log stands for, matched against the
// published legal lists: one wave per slot, lane = list entry), k_log_scan (the slots' prefix counts, so that pool slots are handed
// out in (event index, slot, decision) order without an atomic ticket), k_log_record (one wave per decision: the feature row is
// encoded straight into the pool) and the variant's k_log_apply (the event itself, with the log walker's bookkeeping).
#pragma once

enum { LR_C_FILL = 0, LR_C_OVERFLOWED = 1, LR_C_FAILED = 2, LR_C_PENDING = 3, LR_C_DECISIONS = 4, LR_C_EVENTS = 5, LR_C_COMPLETE = 6, LR_C_WORDS = 8 };
enum { LR_LOG_OPEN = 0, LR_LOG_COMPLETE = 1, LR_LOG_FAILED = 2 };
#define LR_NO_EVENT 0xFFFFFFFFu
#define LR_ROBBED 0x80u   /* dec_seat: the Ron on a robbed kan - the seat's list is that Ron and Pass, not the published one */

struct LogRun {
    // the log set
    const RmjEvent* ev;         // [total][3]
    const uint32_t* off;        // [M + 1] first event of every log
    const uint32_t* koff;       // [M + 1] first kyoku row of every log
    // the assignment: slot s replays slot_logs[slot_first[s] .. slot_first[s + 1])
    const uint32_t* slot_first; // [n + 1]
    const uint32_t* slot_logs;  // [M]
    // per slot
    uint32_t* pos;              // [n] position in slot_logs of the log being replayed (slot_first[s + 1]: none left)
    uint32_t* cur;              // [n] its next event
    uint32_t* kcount;           // [n] start_kyoku events of that log so far
    uint32_t* tcount;           // [n][4] decisions recorded for each seat in the current kyoku
    uint32_t* apply_at;         // [n] the event k_log_apply applies in this step, LR_NO_EVENT = none
    // the decisions of this step
    uint8_t* dec_n;             // [n]
    uint8_t* dec_seat;          // [n][4] seat | LR_ROBBED
    uint64_t* dec_action;       // [n][4]
    uint32_t* dec_t;            // [n][4]
    uint32_t* dec_log;          // [n]
    uint32_t* dec_krow;         // [n]
    // per log, per (kyoku, seat)
    uint8_t* log_status;        // [M] LR_LOG_*
    uint32_t* traj_len;         // [K][4]
    uint8_t* traj_broken;       // [K][4] a decision of the trajectory found no pool slot
    // the pool
    float* feat;                // [capacity][row_floats]
    uint8_t* mask;              // [capacity][A]
    int32_t* action;
    uint64_t* packed;
    int32_t *log, *kyoku, *seat, *t;
    uint32_t* krow;
    float* ret;
    double* ret64;
    int32_t* rank;
    // scan scratch: [max(n, capacity)], its block totals, the counters
    uint32_t* offs;
    uint32_t* totals;
    uint32_t* ctr;
    uint32_t n, M, K, capacity, row_floats, feat_floats, A, NP, include_pass, skip_single, sanma;
};

// ---- host: the assignment of logs to slots (see the head of this file) is rmjh::lr_assign (rmj_host.h: plain C++, also built without HIP)

// ---- decision matching
// the MJAI name of a tile id as a number (parser.rs:301-334 tid_to_mjai): the tile type, the red fives apart
__device__ __forceinline__ uint32_t lr_name(uint32_t t) { return (t == 16u || t == 52u || t == 88u) ? 34u + t / 36u : (t >> 2); }
// the names of up to four consumed tiles as a sorted multiset in one word
__device__ __forceinline__ uint32_t lr_cons_key(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t n) {
    uint32_t k0 = n > 0u ? lr_name(c0) : 0xFFu, k1 = n > 1u ? lr_name(c1) : 0xFFu, k2 = n > 2u ? lr_name(c2) : 0xFFu, k3 = n > 3u ? lr_name(c3) : 0xFFu;
#define LR_CSWAP(a, b) { const uint32_t lo_ = min(a, b), hi_ = max(a, b); a = lo_; b = hi_; }
    LR_CSWAP(k0, k1) LR_CSWAP(k2, k3) LR_CSWAP(k0, k2) LR_CSWAP(k1, k3) LR_CSWAP(k1, k2)
#undef LR_CSWAP
    return k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
}
// Observation.select_action_from_mjai (observation/mjai_select.rs:88-194) over a seat's published list: the first entry, in list order,
// that the event record `e` stands for, RMJ_NO_ACTION if there is none.  Lane = list entry (RMJ_MAX_LEGAL = one wave); the first match
// is the lowest set bit of the ballot (found by counting, nothing is shifted).  `pass`: the message {"type": "none"}.
// The records carry what rmj_apply_events needs, which is less than the MJAI text: a dahai without a tsumogiri field reads as
// tsumogiri = false, a kakan is matched by its tile name alone (one pon per tile type: its consumed tiles follow), kita and reach carry
// no tile.  On logs that a game produced these select the same entry.
__device__ __forceinline__ uint64_t lr_select(const uint64_t* __restrict__ lg, uint32_t n, const RmjEvent* __restrict__ e, bool pass, uint32_t drawn, bool sanma, int lane) {
    const uint64_t a = (uint32_t)lane < n ? lg[lane] : RMJ_NO_ACTION;
    const uint32_t at = a_type(a), tile = a_tile(a);
    const uint32_t ty = pass ? (uint32_t)RMJ_EV_NONE : (uint32_t)e->type;
    const bool tile_eq = tile != RMJ_TILE_NONE && lr_name(tile) == lr_name(e->tile);
    bool hit = false;
    if (pass) hit = at == RMJ_PASS;
    else if (ty == RMJ_EV_HORA) hit = at == RMJ_TSUMO || at == RMJ_RON;
    else if (ty == RMJ_EV_DAHAI) hit = at == RMJ_DISCARD && tile_eq;
    else if (ty == RMJ_EV_REACH) hit = at == RMJ_RIICHI;
    else if (ty == RMJ_EV_RYUKYOKU) hit = at == RMJ_KYUSHU;
    else if (ty == RMJ_EV_KITA) hit = sanma && at == RMJ_KITA;
    else if (ty == RMJ_EV_KAKAN) hit = at == RMJ_KAKAN && tile_eq;
    else if (ty == RMJ_EV_PON || ty == RMJ_EV_CHI || ty == RMJ_EV_DAIMINKAN || ty == RMJ_EV_ANKAN) {
        const uint32_t want = ty == RMJ_EV_PON ? RMJ_PON : (ty == RMJ_EV_CHI ? RMJ_CHI : (ty == RMJ_EV_DAIMINKAN ? RMJ_DAIMINKAN : RMJ_ANKAN));
        const uint32_t en = min((uint32_t)(e->flags >> 4) & 15u, 4u), an = min(a_n(a), 4u);
        hit = at == want && !(sanma && ty == RMJ_EV_CHI) && an == en &&
              lr_cons_key(a_c(a, 0), a_c(a, 1), a_c(a, 2), a_c(a, 3), an) == lr_cons_key(e->consumed[0], e->consumed[1], e->consumed[2], e->consumed[3], en) &&
              (ty == RMJ_EV_ANKAN || tile_eq);
    }
    uint64_t b = __ballot(hit);
    if (!b) return RMJ_NO_ACTION;
    if (!pass && ty == RMJ_EV_DAHAI && drawn != RMJ_TILE_NONE) {   // the tsumogiri flag picks between the drawn tile and its twin in the hand
        const bool tg = (e->flags & 1u) != 0u;
        const uint64_t b2 = __ballot(hit && ((tile == drawn) == tg));
        if (b2) b = b2;
    }
    return lg[__ffsll((long long)b) - 1];
}

// The tile of the kan that the hora `e` at event `cur` of a log (its first event: `lo`) robs, RMJ_TILE_NONE if it robs none: the log's
// previous action - dora events do not count - is a kakan or an ankan by another seat (the record carries no target: on a played log
// that seat is the target).  The caller has seen that the hora's actor is not among the active seats.
__device__ __forceinline__ uint32_t lr_robbed_kan_tile(const RmjEvent* __restrict__ ev, uint32_t lo, uint32_t cur, const RmjEvent* __restrict__ e) {
    uint32_t tile = RMJ_TILE_NONE;
    for (uint32_t j = cur; j > lo;) {
        j--;
        const RmjEvent* q = ev + (size_t)j * 3;
        if (q->type == RMJ_EV_DORA) continue;
        if (q->actor != e->actor) {
            if (q->type == RMJ_EV_KAKAN) tile = q->tile;
            else if (q->type == RMJ_EV_ANKAN && (q->flags >> 4)) tile = q->consumed[0];
        }
        break;
    }
    return tile;
}

// One step of the replay, part one: one wave per slot.  The slot first leaves logs that are over (marking them complete) and takes its
// next one; then the decisions of ReplayBatch._decisions_before for the event at the slot's cursor - see lr_select, plus what the log
// walker yields without a direct match: the Pass of every seat that let a claim go (include_pass), the Ron on a robbed kakan / ankan
// (replay/mod.rs:483-527: not in the published lists, the seat is not even active), and skip_single_action (a decision over a list of
// at most one entry is not a sample and does not count in `t`).  Passes come first, highest seat first, like Kyoku.steps delivers them.
// A decision event whose actor is offered a list that holds no match fails the log (status word, counter): its slot goes on to its
// next log in the same step.  That is the only failure THIS replay detects: apply_event reports nothing, so an event that does not fit the
// state in another way - a decision event by a seat that is not to act, a tsumo out of turn - is applied as rmj_apply_events applies it,
// and the log counts as complete.  The checking replay (rmj_logcheck.hip.h, LogSet.validate()) finds those before samples are built.
// settle_only: only the bookkeeping (the last call of a run: the logs that just ended become complete).
// Wave 0 also adds the samples of the previous step to the pool's fill (nothing reads the fill during this launch).
__global__ __launch_bounds__(256) void k_log_decide(Env E, LogRun R, int settle_only) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slot == 0u) {
        const uint32_t nb = R.ctr[LR_C_PENDING];
        if (nb) {
            const uint32_t all = obs_block_prefix(R.totals, nb, lane);
            if (lane == 0) {
                const uint64_t f = (uint64_t)R.ctr[LR_C_FILL] + all;
                R.ctr[LR_C_FILL] = f > R.capacity ? R.capacity : (uint32_t)f;
                R.ctr[LR_C_PENDING] = 0u;
            }
        }
    }
    if (slot >= R.n) return;
    uint32_t pos = R.pos[slot], cur = R.cur[slot], kc = R.kcount[slot];
    const uint32_t last = R.slot_first[slot + 1];
    const bool sanma = R.sanma != 0u;
    uint32_t apply = LR_NO_EVENT, nd = 0u, log = 0u;
    uint64_t sel[4] = {RMJ_NO_ACTION, RMJ_NO_ACTION, RMJ_NO_ACTION, RMJ_NO_ACTION};
    uint32_t robbed = 0u;
    const uint32_t g = slot;
    for (;;) {
        if (pos >= last) break;
        log = R.slot_logs[pos];
        const uint32_t end = R.off[log + 1];
        if (cur >= end) {   // the log is over
            if (lane == 0) { R.log_status[log] = LR_LOG_COMPLETE; atomicAdd(&R.ctr[LR_C_COMPLETE], 1u); }
            pos++;
            if (pos < last) cur = R.off[R.slot_logs[pos]];
            kc = 0u;
            continue;
        }
        if (settle_only) break;
        const RmjEvent* e = R.ev + (size_t)cur * 3;
        const uint32_t ty = e->type, actor = e->actor & 3u;
        const uint32_t stw = E.status[g];
        const bool done = ((stw >> 16) & 0xFFu) != 0u;
        const uint32_t am = done ? 0u : (stw & 0xFu), phase = (stw >> 8) & 0xFFu;
        const uint32_t nl4 = *reinterpret_cast<const uint32_t*>(E.nlegal + (size_t)g * 4);
        const uint64_t* lg = E.legal + (size_t)g * 4 * RMJ_MAX_LEGAL;
        bool fail = false;
        robbed = 0u;
#pragma unroll
        for (int s = 0; s < 4; s++) sel[s] = RMJ_NO_ACTION;
        bool matched = false;
        if (ty == RMJ_EV_HORA && !done && !((am >> actor) & 1u)) {
            // the Ron on a robbed kan
            const uint32_t tile = lr_robbed_kan_tile(R.ev, R.off[log], cur, e);
            if (tile != RMJ_TILE_NONE) {
                const uint64_t ron = mk_action(RMJ_RON, tile, 0);
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if ((uint32_t)s == actor) sel[s] = ron;
                robbed = 1u << actor;
                matched = true;
            }
        }
        const bool actor_dec = ty == RMJ_EV_DAHAI || ty == RMJ_EV_CHI || ty == RMJ_EV_PON || ty == RMJ_EV_DAIMINKAN || ty == RMJ_EV_ANKAN || ty == RMJ_EV_KAKAN ||
                               ty == RMJ_EV_REACH || ty == RMJ_EV_HORA || ty == RMJ_EV_KITA;
        if (!matched && (actor_dec || (ty == RMJ_EV_RYUKYOKU && am && nl4))) {
            const uint32_t seats = actor_dec ? (1u << actor) : am;   // (a ryukyoku names no seat: whoever is to act may have called it)
            const uint32_t drawn = ty == RMJ_EV_DAHAI ? (uint32_t)E.core[g].drawn_tile : (uint32_t)RMJ_TILE_NONE;
            const bool claim = ty == RMJ_EV_CHI || ty == RMJ_EV_PON || ty == RMJ_EV_DAIMINKAN || ty == RMJ_EV_HORA;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const uint32_t cnt = (nl4 >> (8 * s)) & 0xFFu;
                if (!((am >> s) & 1u) || !cnt) continue;
                if ((seats >> s) & 1u) {
                    sel[s] = lr_select(lg + s * RMJ_MAX_LEGAL, cnt, e, false, drawn, sanma, lane);
                    if (sel[s] == RMJ_NO_ACTION && actor_dec) fail = true;
                } else if (R.include_pass && claim) {   // offered a claim and let it go
                    sel[s] = lr_select(lg + s * RMJ_MAX_LEGAL, cnt, e, true, RMJ_TILE_NONE, sanma, lane);
                }
            }
        } else if (!matched && R.include_pass && ty == RMJ_EV_TSUMO && am && phase == RMJ_WAIT_RESPONSE) {   // everybody passed on the last discard
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const uint32_t cnt = (nl4 >> (8 * s)) & 0xFFu;
                if (((am >> s) & 1u) && cnt) sel[s] = lr_select(lg + s * RMJ_MAX_LEGAL, cnt, e, true, RMJ_TILE_NONE, sanma, lane);
            }
        }
        if (R.skip_single) {
#pragma unroll
            for (int s = 0; s < 4; s++)
                if (!((robbed >> s) & 1u) && ((nl4 >> (8 * s)) & 0xFFu) <= 1u) sel[s] = RMJ_NO_ACTION;
        }
        nd = 0u;
#pragma unroll
        for (int s = 0; s < 4; s++) nd += sel[s] != RMJ_NO_ACTION ? 1u : 0u;
        if (nd && kc == 0u) fail = true;   // a decision before any start_kyoku: no kyoku to file it under
        if (!fail) { apply = cur; break; }
        if (lane == 0) { R.log_status[log] = LR_LOG_FAILED; atomicAdd(&R.ctr[LR_C_FAILED], 1u); }
        nd = 0u;
        pos++;
        if (pos < last) cur = R.off[R.slot_logs[pos]];
        kc = 0u;
    }
    if (settle_only) {
        if (lane == 0) { R.pos[slot] = pos; R.cur[slot] = cur; R.kcount[slot] = kc; R.dec_n[slot] = 0; R.apply_at[slot] = LR_NO_EVENT; }
        return;
    }
    if (lane == 0) {
        uint32_t j = 0u;
        if (apply != LR_NO_EVENT && nd) {
            const uint32_t krow = R.koff[log] + kc - 1u;
            R.dec_log[slot] = log;
            R.dec_krow[slot] = krow;
            // passes first, highest seat first; then the seat that acts (seats ascending)
#pragma unroll
            for (int pass = 1; pass >= 0; pass--) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int s = pass ? 3 - k : k;
                    if (sel[s] == RMJ_NO_ACTION || (a_type(sel[s]) == RMJ_PASS) != (pass != 0)) continue;
                    const uint32_t t = R.tcount[slot * 4u + s];
                    R.tcount[slot * 4u + s] = t + 1u;
                    R.traj_len[(size_t)krow * 4 + s] = t + 1u;
                    R.dec_seat[slot * 4u + j] = (uint8_t)((uint32_t)s | (((robbed >> s) & 1u) ? LR_ROBBED : 0u));
                    R.dec_action[slot * 4u + j] = sel[s];
                    R.dec_t[slot * 4u + j] = t;
                    j++;
                }
            }
            atomicAdd(&R.ctr[LR_C_DECISIONS], j);
        }
        R.dec_n[slot] = (uint8_t)j;
        R.apply_at[slot] = apply;
        if (apply != LR_NO_EVENT) {
            atomicAdd(&R.ctr[LR_C_EVENTS], 1u);
            if (R.ev[(size_t)apply * 3].type == RMJ_EV_START_KYOKU) {
                kc++;
#pragma unroll
                for (int s = 0; s < 4; s++) R.tcount[slot * 4u + s] = 0u;
            }
            cur++;
        }
        R.pos[slot] = pos; R.cur[slot] = cur; R.kcount[slot] = kc;
    }
}

// part two: the slots' decision counts as prefix sums inside blocks of PPO_SCAN_BLOCK slots (like k_ppo_scan); the next k_log_decide
// adds the totals to the fill
__global__ __launch_bounds__(PPO_SCAN_BLOCK) void k_log_scan(LogRun R) {
    __shared__ uint32_t wsum[PPO_SCAN_BLOCK / 64];
    const uint32_t s = blockIdx.x * PPO_SCAN_BLOCK + threadIdx.x;
    uint32_t total;
    const uint32_t ex = ppo_block_scan(s < R.n ? (uint32_t)R.dec_n[s] : 0u, wsum, &total);
    if (s < R.n) R.offs[s] = ex;
    if (threadIdx.x == 0) {
        R.totals[blockIdx.x] = total;
        if (blockIdx.x == 0) R.ctr[LR_C_PENDING] = gridDim.x;
    }
}

// part three: one wave (= block) per decision j of slot s: pool slot = fill + the decisions of the slots before + j; the feature row is
// encoded into the pool (encode_batch_row: the batch encoder's rows, whether the seat is active or not), the mask is the seat's
// published row - or, for the Ron on a robbed kan, the ids of that Ron and of Pass (what get_observation_for_replay builds,
// state/mod.rs:265-325).  Behind the pool's end nothing is written: counted, and the trajectory is marked broken.
template <bool SANMA, int FEAT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RMJ_ENCX_WAVES, RMJ_ENCX_WAVES))) void k_log_record(Env E, LogRun R, const float* __restrict__ decay) {
    const int lane = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x >> 2, j = blockIdx.x & 3u;
    if (j >= (uint32_t)R.dec_n[slot]) return;
    const uint32_t sb = R.dec_seat[slot * 4u + j], seat = sb & 3u;
    const uint32_t krow = R.dec_krow[slot];
    const uint64_t s64 = (uint64_t)R.ctr[LR_C_FILL] + obs_block_prefix(R.totals, slot / PPO_SCAN_BLOCK, lane) + R.offs[slot] + j;
    if (s64 >= R.capacity) {
        if (lane == 0) {
            atomicAdd(&R.ctr[LR_C_OVERFLOWED], 1u);
            R.traj_broken[(size_t)krow * 4 + seat] = 1;
        }
        return;
    }
    const size_t s = (size_t)s64;
    const uint64_t act = R.dec_action[slot * 4u + j];
    const int id = SANMA ? a_encode_3p(act) : a_encode(act);
    encode_batch_row<SANMA, FEAT>(E, slot, (int)seat, decay, R.feat + s * R.row_floats, lane);
    uint8_t* mo = R.mask + s * R.A;
    if (sb & LR_ROBBED) {
        const uint64_t pas = mk_action(RMJ_PASS, RMJ_TILE_NONE, 0);
        const int pid = SANMA ? a_encode_3p(pas) : a_encode(pas);
        for (uint32_t i = (uint32_t)lane; i < R.A; i += 64u) mo[i] = ((int)i == id || (int)i == pid) ? 1 : 0;
    } else {
        const uint8_t* m = E.mask + ((size_t)slot * 4 + seat) * 82;
        for (uint32_t i = (uint32_t)lane; i < R.A; i += 64u) mo[i] = m[i];
    }
    if (lane == 0) {
        const uint32_t log = R.dec_log[slot];
        R.action[s] = id;
        R.packed[s] = act;
        R.log[s] = (int32_t)log;
        R.kyoku[s] = (int32_t)(krow - R.koff[log] + 1u);
        R.seat[s] = (int32_t)seat;
        R.t[s] = (int32_t)R.dec_t[slot * 4u + j];
        R.krow[s] = krow;
    }
}

// Returns and ranks (mjai_logs.py:14-17, :98-118): sample t of a trajectory of T decisions gets reward x P[T - t - 1] - one float64
// multiplication by the host's table P[k] = gamma ** k, so the product has the dataset's bits without a device pow - and the seat's
// rank in the kyoku's end scores (a stable descending sort: ties to the lower seat).  One thread per pool slot.
__global__ __launch_bounds__(256) void k_log_finalize(LogRun R, const double* __restrict__ reward, const int32_t* __restrict__ end_scores, const double* __restrict__ powers,
                                                      uint32_t n_powers) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= R.ctr[LR_C_FILL]) return;
    const size_t row = (size_t)R.krow[s] * 4;
    const uint32_t seat = (uint32_t)R.seat[s], T = R.traj_len[row + seat];
    uint32_t k = T - (uint32_t)R.t[s] - 1u;
    if (k >= n_powers) k = n_powers - 1u;   // (a trajectory is never longer than its log: the table is sized by the longest log)
    const double v = reward[row + seat] * powers[k];
    R.ret64[s] = v;
    R.ret[s] = (float)v;
    const int32_t mine = end_scores[row + seat];
    int32_t rank = 0;
    for (uint32_t p = 0; p < R.NP; p++) {
        const int32_t o = end_scores[row + p];
        rank += (o > mine || (o == mine && p < seat)) ? 1 : 0;
    }
    R.rank[s] = rank;
}

// Emit: the samples of complete logs whose trajectory lost nothing, in pool order (the scan / copy pair of the PPO collector's emit).
// The scan reuses R.offs / R.totals, which between k_log_scan and the next k_log_decide hold the step's counts that are still to join the
// fill: rmj_logreplay_run_device ends every call with a settle launch that folds them in (LR_C_PENDING = 0), so no emit meets them.  A
// caller that emits between the launches of a step would have to settle first.
__device__ __forceinline__ bool lr_emits(const LogRun& R, uint32_t s) {
    return R.log_status[R.log[s]] == LR_LOG_COMPLETE && !R.traj_broken[(size_t)R.krow[s] * 4 + (uint32_t)R.seat[s]];
}
__global__ __launch_bounds__(PPO_SCAN_BLOCK) void k_log_emit_scan(LogRun R) {
    __shared__ uint32_t wsum[PPO_SCAN_BLOCK / 64];
    const uint32_t s = blockIdx.x * PPO_SCAN_BLOCK + threadIdx.x;
    const bool in = s < R.ctr[LR_C_FILL];
    uint32_t total;
    const uint32_t ex = ppo_block_scan(in && lr_emits(R, s) ? 1u : 0u, wsum, &total);
    if (s < R.capacity) R.offs[s] = ex;
    if (threadIdx.x == 0) R.totals[blockIdx.x] = total;
}
struct LogOut {
    float* features;
    uint8_t* mask;
    int64_t* action;
    uint64_t* packed;
    float* ret;
    double* ret64;
    int64_t* rank;
    int32_t *log, *kyoku, *seat, *t;
    uint32_t* count;   // [2]: samples emitted (may exceed rows), slots left out
    uint32_t rows;
};
__global__ __launch_bounds__(256) void k_log_emit(LogRun R, LogOut O) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * 4u, w0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t fill = R.ctr[LR_C_FILL];
    if (w0 == 0u) {
        const uint32_t all = obs_block_prefix(R.totals, (R.capacity + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK, lane);
        if (lane == 0) { O.count[0] = all; O.count[1] = fill - all; }
    }
    for (uint32_t s = w0; s < fill; s += waves) {
        if (!lr_emits(R, s)) continue;
        const uint32_t d = obs_block_prefix(R.totals, s / PPO_SCAN_BLOCK, lane) + R.offs[s];
        if (d >= O.rows) continue;
        ppo_copy_row(R.feat + (size_t)s * R.row_floats, O.features + (size_t)d * R.feat_floats, R.feat_floats, lane);
        for (uint32_t i = (uint32_t)lane; i < R.A; i += 64u) O.mask[(size_t)d * R.A + i] = R.mask[(size_t)s * R.A + i];
        if (lane == 0) {
            O.action[d] = (int64_t)R.action[s];
            O.packed[d] = R.packed[s];
            O.ret[d] = R.ret[s];
            O.ret64[d] = R.ret64[s];
            O.rank[d] = (int64_t)R.rank[s];
            O.log[d] = R.log[s];
            O.kyoku[d] = R.kyoku[s];
            O.seat[d] = R.seat[s];
            O.t[d] = R.t[s];
        }
    }
}
