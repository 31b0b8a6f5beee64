// CPU check of the one place that decides how a device-policy rollout runs (riichienv_amd/csrc/rmj_host.h: rmjh::rollout_plan), built
// with g++ by tests/test_rollout_plan_host.py - once plain, once under AddressSanitizer + UBSan.
//
// (a) The plan is held to a restatement: the expressions the host code carried before there was a plan - rollout_streams,
// rollout_chunk and rollout_queued of the step rollouts, the conditions rmj_step_random_encode spelled inline, and what the two
// timers reported - transcribed here as functions of their own over a stand-in for the handle, and compared field by field over the
// full cross product of the inputs below.  The ticket kernel's resident waves (`slots`) are an input: 0 stands for a query that
// fails.  Two things are stated here rather than transcribed: the old code asked for the slots a little earlier than the plan's
// need_slots does (before it had looked at RMJ_QUEUE_FORCE's 64 quads; the step + encode rollout before any other condition), which
// changes no result when the query succeeds; and the encode timer's report is compared for only_active = 2, the one value it runs with.
// (b) A short table of cases written out by hand, so that a mistake copied into both sides still shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../riichienv_amd/csrc/rmj_host.h"

using rmjh::RolloutPlan;
using rmjh::RolloutTuning;

static uint64_t g_checks = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        g_checks++;                                              \
        if (!(cond)) {                                           \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                                 \
            printf("\n");                                        \
            exit(1);                                             \
        }                                                        \
    } while (0)

// ---- the restatement.  The members of the handle that the old expressions read, under their old names, and the old constants
struct OldEnv {
    struct { uint32_t n_games; } cfg;
    int want_streams, quad, queue_chunk, queue_force, queue_min_chunk, heavy_first, enc_fused;
    uint32_t rows_pw, max_xcc_id, q_slots_pol[2], q_slots_enc;
};
#define OLD_SPLIT_MIN_GAMES 16384u
#define OLD_SPLIT_MIN_PART 8192u
#define OLD_MAX_ROLLOUT_STREAMS 8
#define OLD_STEP_F_ROWS_SHIFT 20

static int old_rollout_streams(const OldEnv* h, uint32_t n_steps) {
    const int want = h->want_streams;
    if (h->quad >= 2 && n_steps >= 2 && want >= 2) return 1;   // the fused rollout: one launch, no parts
    if (want < 2 || n_steps < 2 || h->cfg.n_games < OLD_SPLIT_MIN_GAMES) return 1;
    int k = want > OLD_MAX_ROLLOUT_STREAMS ? OLD_MAX_ROLLOUT_STREAMS : want;
    const int fit = (int)(h->cfg.n_games / OLD_SPLIT_MIN_PART);
    return k > fit ? fit : k;
}
static uint32_t old_rollout_chunk(const OldEnv* h, uint32_t n_steps) {
    uint32_t cap = (uint32_t)h->queue_chunk;
    const uint32_t lo = (uint32_t)h->queue_min_chunk, fine = n_steps / 16u < lo ? lo : n_steps / 16u;
    if (cap < (n_steps + 39u) / 40u) cap = (n_steps + 39u) / 40u;   // at most 64 tickets per quad (q_ticket_plan)
    return fine < cap ? fine : cap;
}
// (query: what the occupancy query yields when it is made, 0 = it fails)
static bool old_rollout_queued(OldEnv* h, uint32_t n_steps, int pol, uint32_t query) {
    const uint32_t quads = (h->cfg.n_games + 3u) / 4u;
    if (!(h->quad >= 2 && n_steps >= 2 && h->want_streams >= 2) || h->queue_chunk <= 0 || n_steps < 2u * old_rollout_chunk(h, n_steps)) return false;
    if (h->max_xcc_id > 7u) return false;   // more XCC ids than queues: no single L2 per queue (see rmj_create)
    pol = pol == 1 ? 1 : 0;
    if (h->q_slots_pol[pol] == 0) {
        if (query == 0) return false;
        h->q_slots_pol[pol] = query;
    }
    const uint32_t slots = h->q_slots_pol[pol];
    if (h->queue_force) return quads >= 64u;   // RMJ_QUEUE_FORCE=1 (tests): any batch with a quad per XCD queue to spare
    return quads > slots && quads < 8u * slots;
}

// what a rollout did, in the plan's terms
struct Ran {
    RolloutPlan::How how = RolloutPlan::PER_STEP;
    bool error = false;   // the step + encode rollout's "occupancy query failed"
    int k = 1;
    uint32_t bound[OLD_MAX_ROLLOUT_STREAMS + 1] = {};
    uint32_t rows = 0, row_flags = 0, chunk = 0, gq = 0, gfix = 0, gplain = 0;
    bool heavy = false;
    uint32_t launches = 0, in_flight = 0, queued = 0;
};
// the whole-batch test of launch_step_range for part [g0, g1)
static bool old_heavy(const OldEnv* h, uint32_t g0, uint32_t g1) {
    if (!h->quad) return false;
    const uint32_t rows = h->rows_pw;
    const uint32_t units = (g1 - g0 + rows - 1u) / rows;
    return h->heavy_first && g0 == 0u && g1 == h->cfg.n_games && units >= 2048u;
}
static void old_parts(const OldEnv* h, int k, Ran* r) {
    const uint32_t n = h->cfg.n_games;
    r->how = RolloutPlan::PER_STEP;
    r->k = k;
    for (int i = 0; i <= k; i++) r->bound[i] = (uint32_t)((uint64_t)n * i / k);
    r->heavy = false;
    for (int i = 0; i < k; i++) r->heavy = r->heavy || old_heavy(h, r->bound[i], r->bound[i + 1]);
}
// step_policy_impl, then bench_rollout_impl's report
static Ran old_step_rollout(OldEnv* h, uint32_t n_steps, int pol, uint32_t query) {
    Ran r;
    const uint32_t n = h->cfg.n_games;
    if (h->quad >= 2 && n_steps >= 2 && h->want_streams >= 2) {
        const uint32_t grid = (n + 3u) / 4u;
        if (old_rollout_queued(h, n_steps, pol, query)) {
            r.how = RolloutPlan::TICKETS;
            r.gq = grid < h->q_slots_pol[pol == 1 ? 1 : 0] ? grid : h->q_slots_pol[pol == 1 ? 1 : 0];
            r.gfix = (grid + 63u) / 64u;
            r.chunk = old_rollout_chunk(h, n_steps);
        } else {
            const uint32_t rows = h->rows_pw;
            r.how = RolloutPlan::FUSED;
            r.gplain = (n + rows - 1u) / rows;
            r.rows = rows;
            r.row_flags = (rows == 4u ? 0u : rows) << OLD_STEP_F_ROWS_SHIFT;
        }
    } else {
        old_parts(h, old_rollout_streams(h, n_steps), &r);
    }
    const uint32_t steps = n_steps;
    const uint32_t fl = (uint32_t)old_rollout_streams(h, steps);
    const bool fused = h->quad >= 2 && steps >= 2 && h->want_streams >= 2;
    r.launches = fused ? 1u : steps * fl;
    r.in_flight = fl;
    r.queued = old_rollout_queued(h, steps, pol, 0u) ? 1u : 0u;   // (after the rollout: the slots are known, or the query has failed)
    return r;
}
// rmj_step_random_encode, then rmj_time_rollout_encode's report (which runs with only_active = 2)
static Ran old_encode_rollout(OldEnv* h, uint32_t n_steps, int only_active, uint32_t query) {
    Ran r;
    const uint32_t n = h->cfg.n_games;
    if (h->enc_fused && h->quad >= 2 && h->want_streams >= 2 && n_steps >= 2 && only_active == 2) {
        const uint32_t grid = (n + 3u) / 4u;
        r.how = RolloutPlan::FUSED;
        if (h->q_slots_enc == 0) {
            if (query == 0) { r.error = true; return r; }
            h->q_slots_enc = query;
        }
        const uint32_t chunk = old_rollout_chunk(h, n_steps);
        const bool queued = h->queue_chunk > 0 && h->max_xcc_id <= 7u && n_steps >= 2u * chunk &&
                            (h->queue_force ? grid >= 64u : (grid > h->q_slots_enc && grid < 8u * h->q_slots_enc));
        r.chunk = chunk;
        if (queued) {
            r.how = RolloutPlan::TICKETS;
            r.gq = grid < h->q_slots_enc ? grid : h->q_slots_enc;
            r.gfix = grid;
        } else {
            r.gplain = grid;
        }
    } else {
        int k = h->want_streams;
        if (k > OLD_MAX_ROLLOUT_STREAMS) k = OLD_MAX_ROLLOUT_STREAMS;
        if ((int)(n / OLD_SPLIT_MIN_PART) < k) k = (int)(n / OLD_SPLIT_MIN_PART);
        if (n_steps < 2 || n < OLD_SPLIT_MIN_GAMES || k < 2) k = 1;
        old_parts(h, k, &r);
    }
    const uint32_t steps = n_steps;
    const bool fused = h->enc_fused && h->quad >= 2 && h->want_streams >= 2 && steps >= 2;
    const uint32_t quads = (h->cfg.n_games + 3u) / 4u, chunk = old_rollout_chunk(h, steps);
    r.launches = fused ? 1u : 2u * steps;
    r.in_flight = 1u;
    r.queued = (fused && h->queue_chunk > 0 && h->max_xcc_id <= 7u && steps >= 2u * chunk && h->q_slots_enc &&
                (h->queue_force ? quads >= 64u : (quads > h->q_slots_enc && quads < 8u * h->q_slots_enc))) ? 1u : 0u;
    return r;
}
// the conditions for tickets that do not ask for the slots, in the old expressions' terms
static bool old_wants_tickets(const OldEnv* h, uint32_t n_steps, bool one_launch) {
    const uint32_t quads = (h->cfg.n_games + 3u) / 4u;
    return one_launch && h->queue_chunk > 0 && n_steps >= 2u * old_rollout_chunk(h, n_steps) && h->max_xcc_id <= 7u && (!h->queue_force || quads >= 64u);
}

static void compare(const RolloutPlan& p, const Ran& r, const OldEnv& h, uint32_t n_steps, bool encode, bool report, const char* what) {
#define CTX "%s: n %u steps %u quad %d want %d chunk %d min %d force %d xcc %u", what, h.cfg.n_games, n_steps, h.quad, h.want_streams, h.queue_chunk, h.queue_min_chunk, h.queue_force, h.max_xcc_id
    CHECK(p.how == r.how, CTX);
    CHECK(p.n_games == h.cfg.n_games, CTX);
    CHECK(p.k == r.k, CTX);
    if (r.how == RolloutPlan::PER_STEP)
        for (int i = 0; i <= r.k; i++) CHECK(p.part(i) == r.bound[i], CTX);
    CHECK(p.part(0) == 0u && p.part(p.k) == h.cfg.n_games, CTX);
    CHECK(p.rows == h.rows_pw && p.row_flags == ((h.rows_pw == 4u ? 0u : h.rows_pw) << OLD_STEP_F_ROWS_SHIFT), CTX);
    CHECK(p.chunk == old_rollout_chunk(&h, n_steps), CTX);
    CHECK(p.heavy == r.heavy, CTX);
    if (r.how == RolloutPlan::TICKETS) {
        CHECK(p.chunk == r.chunk, CTX);
        CHECK(p.grid_tickets == r.gq, CTX);
        CHECK(p.grid_fixup == r.gfix, CTX);
    } else {
        CHECK(p.grid_tickets == 0u, CTX);
    }
    if (r.how == RolloutPlan::FUSED) {
        CHECK(p.grid_plain == r.gplain, CTX);
        if (!encode) CHECK(p.rows == r.rows && p.row_flags == r.row_flags, CTX);
    }
    if (report) {
        CHECK(p.launches == r.launches, CTX);
        CHECK(p.launches_in_flight == r.in_flight, CTX);
        CHECK(p.queued == r.queued, CTX);
    }
#undef CTX
}

static const uint32_t kGames[] = {1, 3, 4, 255, 256, 259, 1001, 3584, 3585, 4099, 7168, 7169, 8191, 8192, 16383, 16384, 24576, 32768, 65536, 524288};
static const uint32_t kSteps[] = {0, 1, 2, 9, 10, 15, 16, 20, 63, 64, 79, 80, 100, 333, 2000, 2561};
static const int kQuad[] = {0, 1, 2}, kWant[] = {1, 2, 4, 8}, kChunk[] = {0, 5, 32, 50, 64, 166}, kMinChunk[] = {1, 5}, kForce[] = {0, 1};
static const uint32_t kXcc[] = {7, 8}, kSlots[] = {0, 5120, 6144};
static const int kPol[] = {0, 1}, kEncFused[] = {0, 1}, kOnlyActive[] = {0, 2};

static uint64_t cross_product() {
    uint64_t combos = 0;
    for (uint32_t n : kGames) for (uint32_t steps : kSteps) for (int quad : kQuad) for (int want : kWant) for (int qc : kChunk)
    for (int qmin : kMinChunk) for (int force : kForce) for (uint32_t xcc : kXcc) for (uint32_t slots : kSlots)
    for (int pol : kPol) for (int ef : kEncFused) for (int oa : kOnlyActive) {
        combos++;
        RolloutTuning t;
        t.want_streams = want; t.quad = quad; t.queue_chunk = qc; t.queue_force = force; t.queue_min_chunk = qmin; t.enc_fused = ef;
        t.rows_pw = rmjh::rows_for_batch(n);
        CHECK(t.rows_pw == (n <= 3584u ? 1u : (n <= 7168u ? 2u : 4u)), "rows of %u games", n);
        OldEnv h{};
        h.cfg.n_games = n;
        h.want_streams = want; h.quad = quad; h.queue_chunk = qc; h.queue_force = force; h.queue_min_chunk = qmin; h.enc_fused = ef;
        h.heavy_first = t.heavy_first; h.rows_pw = t.rows_pw; h.max_xcc_id = xcc;
        {   // the step rollout under policy `pol`
            const bool one_launch = quad >= 2 && steps >= 2 && want >= 2;
            const Ran r = old_step_rollout(&h, steps, pol, slots);
            const RolloutPlan p = rmjh::rollout_plan(t, n, steps, pol, false, 0, slots, xcc);
            compare(p, r, h, steps, false, true, pol ? "greedy" : "random");
            CHECK(p.pol == pol, "policy index");
            CHECK(p.need_slots == (slots == 0u && old_wants_tickets(&h, steps, one_launch)), "need_slots: n %u steps %u", n, steps);
        }
        {   // the step + encode rollout
            const bool one_launch = ef && quad >= 2 && want >= 2 && steps >= 2 && oa == 2;
            const Ran r = old_encode_rollout(&h, steps, oa, slots);
            const RolloutPlan p = rmjh::rollout_plan(t, n, steps, 0, true, oa, slots, xcc);
            CHECK(p.pol == 0, "policy index");
            CHECK(p.need_slots == (slots == 0u && old_wants_tickets(&h, steps, one_launch)), "need_slots (encode): n %u steps %u", n, steps);
            if (r.error) CHECK(p.how == RolloutPlan::FUSED && slots == 0u, "encode without slots: n %u steps %u", n, steps);
            else compare(p, r, h, steps, true, oa == 2, "encode");
        }
    }
    return combos;
}

// ---- (b) cases by hand; 6 144 resident waves of the ticket kernel are assumed, not measured
static RolloutPlan plan_of(RolloutTuning t, uint32_t n, uint32_t steps, int pol = 0, uint32_t slots = 6144, uint32_t xcc = 7) {
    t.rows_pw = rmjh::rows_for_batch(n);
    return rmjh::rollout_plan(t, n, steps, pol, false, 0, slots, xcc);
}
static void by_hand() {
    const RolloutTuning dflt;
    const uint32_t some_steps[] = {2, 9, 10, 15, 20, 100, 200, 2000};
    RolloutPlan p = plan_of(dflt, 32768, 200);
    CHECK(p.how == RolloutPlan::TICKETS && p.chunk == 12 && p.queued == 1 && p.launches == 1 && p.grid_tickets == 6144 && p.grid_fixup == 128, "32768 x 200");
    CHECK(plan_of(dflt, 32768, 100).how == RolloutPlan::TICKETS, "32768 x 100");
    p = plan_of(dflt, 32768, 20);
    CHECK(p.how == RolloutPlan::TICKETS && p.chunk == 5, "32768 x 20");
    CHECK(plan_of(dflt, 32768, 15).how == RolloutPlan::TICKETS, "32768 x 15");
    p = plan_of(dflt, 32768, 9);
    CHECK(p.how == RolloutPlan::FUSED && p.queued == 0 && p.grid_plain == 8192 && p.row_flags == 0, "32768 x 9");
    for (uint32_t steps : some_steps) {
        RolloutTuning t = dflt;
        t.queue_chunk = 0;
        CHECK(plan_of(t, 32768, steps).how == RolloutPlan::FUSED, "queue_chunk 0, %u steps", steps);
        CHECK(plan_of(dflt, 32768, steps, 0, 6144, 8).how == RolloutPlan::FUSED, "max_xcc_id 8, %u steps", steps);
        p = plan_of(dflt, 4096, steps);
        CHECK(p.how == RolloutPlan::FUSED && p.launches == 1 && p.launches_in_flight == 1 && p.rows == 2 && p.grid_plain == 2048, "4096 x %u", steps);
        CHECK(plan_of(dflt, 524288, steps).how == RolloutPlan::FUSED, "524288 x %u", steps);   // 131 072 quads >= 8 x 6 144
    }
    CHECK(plan_of(dflt, 65536, 100, 1, 5120).how == RolloutPlan::TICKETS, "65536 greedy");
    CHECK(plan_of(dflt, 65536, 100, 1, 5120).pol == 1 && plan_of(dflt, 65536, 100, 1, 5120).grid_tickets == 5120, "65536 greedy");
    {
        RolloutTuning t = dflt;
        t.queue_force = 1;
        p = plan_of(t, 256, 20);   // 64 quads
        CHECK(p.how == RolloutPlan::TICKETS && p.grid_tickets == 64 && p.grid_fixup == 1, "forced, 64 quads");
        CHECK(plan_of(t, 252, 20).how == RolloutPlan::FUSED, "forced, 63 quads");
    }
    {
        RolloutTuning t = dflt;
        t.quad = 1;
        p = plan_of(t, 65536, 10);
        CHECK(p.how == RolloutPlan::PER_STEP && p.k == 4 && p.launches == 40 && p.launches_in_flight == 4 && !p.heavy, "quad 1, 65536 x 10");
        for (int i = 0; i <= 4; i++) CHECK(p.part(i) == 16384u * (uint32_t)i, "part %d", i);
        CHECK(plan_of(t, 16384, 10).k == 2, "quad 1, 16384");
        p = plan_of(t, 16383, 10);
        CHECK(p.how == RolloutPlan::PER_STEP && p.k == 1 && p.heavy, "quad 1, 16383");   // 4 096 units on one stream: heavy-first
    }
    {
        RolloutTuning t = dflt;
        t.want_streams = 1;
        p = plan_of(t, 32768, 20);
        CHECK(p.how == RolloutPlan::PER_STEP && p.k == 1 && p.launches == 20 && p.launches_in_flight == 1 && p.queued == 0, "one stream, quad 2");
    }
}

int main() {
    by_hand();
    const uint64_t combos = cross_product();
    printf("rollout plan OK %llu checks over %llu combinations\n", (unsigned long long)g_checks, (unsigned long long)combos);
    return 0;
}
