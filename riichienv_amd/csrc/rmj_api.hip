// C-ABI (include/riichi_mi355x.h) of the MI355X-native batched Riichi step path.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC rmj_api.hip -o libriichi_mi355x.so
//
// Launch geometry: 256-thread workgroups = 4 wavefronts = 4 games; grid = ceil(B/4) (16 384
// workgroups at B = 65 536, i.e. 64 per CU: far above the ">>256 workgroups" rule).  The
// blockIdx -> game map is launch-invariant, so a game is always served by the same XCD
// (block b runs on XCD b % 8) and its 640-byte record is re-read from that XCD's L2 / MALL.
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/riichi_mi355x.h"
#include "../../include/riichi_mi355x_bench.h"
#include "rmj_common.hip.h"
#include "rmj_eval4.hip.h"
#include "rmj_encode.hip.h"
#include "rmj_seq.hip.h"
#include "rmj_host.h"
#include "rmj_evtext.h"

using namespace rmj;

// the device code, by subsystem, in the order the code object keeps its kernels
#include "rmj_policy.hip.h"
#define RMJ_NS rmj4
#define RMJ_SANMA 0
#include "rmj_step.hip.h"
#include "rmj_kernels.hip.h"
#include "rmj_step4.hip.h"
#undef RMJ_NS
#undef RMJ_SANMA
#define RMJ_NS rmj3
#define RMJ_SANMA 1
#include "rmj_step.hip.h"
#include "rmj_kernels.hip.h"
#include "rmj_step4.hip.h"
#undef RMJ_NS
#undef RMJ_SANMA
#include "rmj_readout.hip.h"
#include "rmj_handapi.hip.h"
#include "rmj_obs.hip.h"
#include "rmj_ppo.hip.h"
#include "rmj_logreplay.hip.h"
#include "rmj_logcheck.hip.h"
#include "rmj_logtext.hip.h"
#include "rmj_grp.hip.h"
#include "rmj_playstats.hip.h"
#include "rmj_handtab.hip.h"
#include "rmj_events.hip.h"
#include "rmj_hidden.hip.h"
#include "rmj_determinize.hip.h"
#include "rmj_danger.hip.h"
#include "rmj_dtable.hip.h"
// the launches of the discard table's kernels, defined at the end of this file: there the kernels are named for the first time (rmj_dtable.hip.h)
static void dt_launch_rows(hipStream_t st, const Env& E, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDiscardTableOut& O);
static void dt_launch_hands(const ShantenTables& T, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, const RmjDiscardTableOut& O);
static void dt_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* dtb);
static void hid_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* hid);
static void dng_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* dng);
static void dt_launch_log_emit(hipStream_t st, const LogRun& R, const uint8_t* dtb, const LogDtableOut& O);

// The extra records a log sample builder's pool can keep, in the order a replay step launches their kernels: the RMJ_LOGREPLAY_* flag
// that asks for them (and its name), the bytes of a slot's record, what the messages call them, and the launch of the kernel that
// records a step's rows from the state before the step's event (`records`: [capacity][slot_bytes], an allocation of its own).
struct LogExtra {
    uint32_t flag;
    const char* flag_name;
    size_t slot_bytes;
    const char* noun;
    void (*launch)(hipStream_t st, const Env& E, const LogRun& R, uint8_t* records);
};
enum { LX_HIDDEN, LX_DANGER, LX_DTABLE, LX_COUNT };
static const LogExtra kLogExtras[LX_COUNT] = {{RMJ_LOGREPLAY_HIDDEN, "RMJ_LOGREPLAY_HIDDEN", HID_SLOT_BYTES, "hidden", hid_launch_log},
                                              {RMJ_LOGREPLAY_DANGER, "RMJ_LOGREPLAY_DANGER", DNG_SLOT_BYTES, "danger", dng_launch_log},
                                              {RMJ_LOGREPLAY_DTABLE, "RMJ_LOGREPLAY_DTABLE", DT_SLOT_BYTES, "discard efficiency", dt_launch_log}};

static inline dim3 step_grid(uint32_t n) { return dim3((n + RMJ_STEP_WPB - 1) / RMJ_STEP_WPB); }
static_assert(rmjh::kStepRowsShift == STEP_F_ROWS_SHIFT, "rmj_host.h states the step kernels' rows flag position");

// The step kernels of one player count, as typed pointers: Env and HeavyOrder are shared by rmj3 and rmj4, so an instantiation has the
// same type in both.  A handle points at its player count's table from create on (rmj_env::kern).
struct StepKernels {
    decltype(&rmj4::k_step) step;
    decltype(&rmj4::k_step4<false, 0>) step4[2][2];   // [LOOP][POL]
    decltype(&rmj4::k_step4_queue<0>) queue[2];       // [POL]
    decltype(&rmj4::k_step4_fixup<0>) fixup[2];       // [POL]
    decltype(&rmj4::k_step4_enc<0>) enc;
    decltype(&rmj4::k_step4_queue_enc<0>) queue_enc;
    decltype(&rmj4::k_step4_fixup_enc<0>) fixup_enc;
    decltype(&rmj4::k_step4_act_enc) act_enc;
    decltype(&rmj4::k_step4_sample_enc) sample_enc;
};
// Where a template kernel is first named decides its place in the code object, and two tables filled one after the other cannot name
// rmj3 and rmj4 in turns: this list, which nothing reads, names the instantiations in the order the code object has always kept them.
[[maybe_unused]] static const void* const kStepKernelOrder[] = {
    (void*)rmj3::k_step4<false, 1>, (void*)rmj3::k_step4<false, 0>, (void*)rmj4::k_step4<false, 1>, (void*)rmj4::k_step4<false, 0>,
    (void*)rmj3::k_step4_queue<1>, (void*)rmj4::k_step4_queue<1>, (void*)rmj3::k_step4_queue<0>, (void*)rmj4::k_step4_queue<0>,
    (void*)rmj3::k_step4_fixup<1>, (void*)rmj3::k_step4_fixup<0>, (void*)rmj4::k_step4_fixup<1>, (void*)rmj4::k_step4_fixup<0>,
    (void*)rmj3::k_step4<true, 1>, (void*)rmj3::k_step4<true, 0>, (void*)rmj4::k_step4<true, 1>, (void*)rmj4::k_step4<true, 0>,
    (void*)rmj3::k_step4_queue_enc<0>, (void*)rmj4::k_step4_queue_enc<0>, (void*)rmj3::k_step4_fixup_enc<0>, (void*)rmj4::k_step4_fixup_enc<0>,
    (void*)rmj3::k_step4_enc<0>, (void*)rmj4::k_step4_enc<0>};
#define RMJ_STEP_KERNELS(NS)                                                                                                            \
    {NS::k_step, {{NS::k_step4<false, 0>, NS::k_step4<false, 1>}, {NS::k_step4<true, 0>, NS::k_step4<true, 1>}},                         \
     {NS::k_step4_queue<0>, NS::k_step4_queue<1>}, {NS::k_step4_fixup<0>, NS::k_step4_fixup<1>}, NS::k_step4_enc<0>,                     \
     NS::k_step4_queue_enc<0>, NS::k_step4_fixup_enc<0>, NS::k_step4_act_enc, NS::k_step4_sample_enc}
static const StepKernels kStepKernels3 = RMJ_STEP_KERNELS(rmj3), kStepKernels4 = RMJ_STEP_KERNELS(rmj4);

// ================================================================= host side
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) return fail(RMJ_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// A buffer a handle grows on demand: need() leaves room for `bytes` bytes, by free-then-allocate when it is short.  Device memory is
// freed only after the stream `st` has drained (work queued there may still read it); pinned host memory is freed at once.
// headroom: a grown buffer gets bytes + bytes / 8 + 1 MiB, so that the next call of a similar size fits; always: allocated on first
// use even for 0 bytes (a non-null pointer for the kernels).  The members of rmj_env state which buffer has which rule.
struct Grown {
    enum Kind { DEVICE, PINNED };
    Kind kind;
    bool headroom = false, always = false;
    void* p = nullptr;
    size_t cap = 0;
    Grown(Kind k, bool headroom_ = false, bool always_ = false) : kind(k), headroom(headroom_), always(always_) {}
    hipError_t need(size_t bytes, hipStream_t st = nullptr) {   // st: device memory only
        if (bytes <= cap && (p || !always)) return hipSuccess;
        if (kind == DEVICE) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
        }
        release();
        const size_t want = headroom ? bytes + bytes / 8 + ((size_t)1 << 20) : bytes;
        hipError_t e = kind == DEVICE ? hipMalloc(&p, want) : hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) kind == DEVICE ? (void)hipFree(p) : (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct rmj_env {
    RmjConfig cfg;
    Env d;
    hipStream_t stream = nullptr;      // the stream every entry point works on: own_stream, or the caller's (rmj_set_stream)
    hipStream_t own_stream = nullptr;
    // extra streams of multi-step device rollouts (rmj_step_random): the games are stepped as k parts, one per stream,
    // so that the draining tail of one part's launch overlaps the bodies of the others'.  Forked from and joined back
    // into `stream` inside the call: every other entry point sees one ordered stream.  Measured at 65 536 games:
    // 1 stream 504 M env.step/s, 2: 605 M, 3: 648 M, 4: 678 M, 6: 469 M, 8: 498 M, 16: 343 M.
    hipStream_t xstream[RMJ_MAX_ROLLOUT_STREAMS - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[RMJ_MAX_ROLLOUT_STREAMS - 1] = {};
    Env* d_env = nullptr;  // device-resident copy of `d` (kernels take a pointer, see rmj_kernels.hip.h)
    uint64_t* d_actions = nullptr;
    unsigned long long* d_counter = nullptr;
    uint32_t* d_obs_offs = nullptr;    // [n_games] + [blocks] slots of the compact observation batch (rmj_encode_compact_device)
    uint32_t ring = 0;
    float* d_decay = nullptr;  // expf(-0.2f * age), age 0..31, computed on the host (encode_extended)
    Grown scratch{Grown::DEVICE};   // staging buffer of the host-copy entry points (grown on demand to the exact size, never per call): scratch_for
    rmjh::RolloutTuning tune;          // what the rollouts are tuned to: read from the environment at create, rmj_set_rollout_streams
    const StepKernels* kern = nullptr; // the step kernels of the handle's player count
    hipEvent_t ev_time[2] = {nullptr, nullptr};   // rmj_time_rollout* / rmj_bench_rollout: created with the handle, so that a timed region holds no event create / destroy
    uint32_t* d_qheads = nullptr;   // the ticket rollouts' counter sets and progress words (ticket_counters)
    uint32_t q_slots_pol[2] = {0, 0};   // waves of k_step4_queue<policy> the device holds at once (the greedy instantiation is compiled for fewer)
    void* d_heavy = nullptr;        // heavy-first launch order of whole-batch per-step launches (HeavyOrder): two counters, lists, flag arrays
    uint32_t heavy_phase = 0;       // which half the next launch reads
    uint32_t max_xcc_id = 0;        // largest HW_REG_XCC_ID seen by a probe launch at create: the ticket rollout assumes ids 0..7 (one L2 per queue)
    uint32_t* d_ev_lost = nullptr;  // [n_games] records a game's ring lost to a late drain (rmj_drain_events), cumulative
    std::vector<struct rmj_ppo*> ppo;   // transition collectors bound to this handle (rmj_ppo_create): destroyed with it
    std::vector<struct rmj_logreplay*> logreplay;   // log sample builders bound to this handle (rmj_logreplay_create): destroyed with it
    void* d_track = nullptr;        // round tracker (rmj_round_track_device): hand index / scores / meta where every game's round began
    // staging of rmj_drain_format's size call (the records sit in `pin`): reused by the call that brings the text buffer
    bool stage_valid = false;
    int stage_seat = 0;
    uint32_t stage_events = 0;
    double stage_ms[2] = {0, 0};
    std::vector<uint32_t> stage_cursor;
    Grown pin{Grown::PINNED};       // pinned host staging of the host-buffer entry points (rmj_get_legal_compact, rmj_drain_*), exact size; when it
                                    // moves, the staged size call is gone (stage_valid = false): pin_for
    // buffers of the text calls (rmj_drain_text / rmj_format_events_device): what the last call's RmjTextView points at
    Grown txt{Grown::DEVICE, true, true};   // device text: headroom, and there from the first call on even when that call's text is empty
    Grown txt_offs{Grown::DEVICE};  // device text offsets: [games + 1] slots of 8 bytes
    Grown txt_work{Grown::DEVICE};  // sizes, stops and scan of the text calls (text_format_device lays it out)
    Grown h_txt{Grown::PINNED, true};   // pinned text (host delivery): headroom
    Grown h_txt_offs{Grown::PINNED};    // pinned text offsets [games + 1], then the new cursors
    uint32_t q_slots_enc = 0;       // waves of k_step4_queue_enc the device holds at once
    Grown det_claim{Grown::DEVICE}; // rmj_determinize_device: [n_games] u64 claim words (epoch << 32 | ~row), allocated and cleared by the handle's first call
    uint32_t det_epoch = 0;         // the last call's epoch: a word of an earlier call loses against any word of this one
};
// device staging memory of at least `bytes` bytes, owned by the handle
static int scratch_for(rmj_env* h, size_t bytes, void** out) {
    HIPCHK(h->scratch.need(bytes, h->stream));
    *out = h->scratch.p;
    return RMJ_OK;
}
// the same, laid out: the arrays registered in `L` point into the scratch
static int scratch_for(rmj_env* h, const rmjh::DevLayout& L) {
    void* sp;
    int rc = scratch_for(h, L.bytes(), &sp);
    if (!rc) L.bind(sp);
    return rc;
}

static int ensure_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RMJ_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(RMJ_ERR_NO_DEVICE, "device ordinal out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(RMJ_ERR_NO_DEVICE, "hipSetDevice failed");
    return RMJ_OK;
}
static inline dim3 game_grid(uint32_t n) { return dim3((n + WPB - 1) / WPB); }
// one launch of the handle's variant of KERNEL (rmj3:: for three players, rmj4:: for four) on its stream, the handle's device Env as the
// first argument.  A macro, expanded in place: where a kernel is first named decides its place in the code object.
#define RMJ_LAUNCH_MODE(h, KERNEL, grid, block, ...)                                                                                   \
    do {                                                                                                                                \
        if ((h)->cfg.game_mode >= 3) hipLaunchKernelGGL(rmj3::KERNEL, grid, block, 0, (h)->stream, (const Env*)(h)->d_env, __VA_ARGS__); \
        else hipLaunchKernelGGL(rmj4::KERNEL, grid, block, 0, (h)->stream, (const Env*)(h)->d_env, __VA_ARGS__);                         \
    } while (0)

// Temporary device buffers (and timing events) of one entry point: released on EVERY return path, so that an error
// in the middle of a call (HIPCHK returns at once) strands nothing on the device.
struct DevTmp {
    std::vector<void*> bufs;
    std::vector<hipEvent_t> events;
    ~DevTmp() {
        for (void* q : bufs) if (q) hipFree(q);
        for (hipEvent_t e : events) if (e) hipEventDestroy(e);
    }
    template <typename T>
    hipError_t alloc(T** dst, size_t bytes) {
        *dst = nullptr;
        hipError_t e = hipMalloc((void**)dst, bytes);
        if (e == hipSuccess) bufs.push_back((void*)*dst);
        return e;
    }
    template <typename T>
    int upload(const T* src, size_t count, T** dst) {  // NULL source = optional array not given
        *dst = nullptr;
        if (!src) return RMJ_OK;
        HIPCHK(alloc(dst, count * sizeof(T)));
        HIPCHK(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
        return RMJ_OK;
    }
    hipError_t event(hipEvent_t* e) {
        hipError_t r = hipEventCreate(e);
        if (r == hipSuccess) events.push_back(*e);
        return r;
    }
    void release(void* p) {   // the buffer has an owner that outlives the call: no longer freed here
        for (void*& q : bufs) if (q == p) q = nullptr;
    }
};
// Host-copy twin of a `_device` entry point: `fill` (the twin) writes `bytes` bytes into the handle's scratch, which are waited for and copied to `out`
template <class Fill>
static int fill_and_fetch(rmj_env* h, void* out, size_t bytes, Fill fill) {
    HIPCHK(hipSetDevice(h->cfg.device));
    void* sp;
    int rc = scratch_for(h, bytes, &sp);
    if (rc) return rc;
    if ((rc = fill(sp))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, sp, bytes, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
// The same for the two sequence encoders: the seven arrays of `Buffers` (sz: their bytes) at 256-byte steps of the handle's scratch
template <class Buffers, class Twin>
static int encode_seq_host(rmj_env* h, int game_style, const Buffers* out, const size_t (&sz)[7], Twin twin) {
    HIPCHK(hipSetDevice(h->cfg.device));
    Buffers d{};
    rmjh::DevLayout L;
    L.add(&d.sparse, sz[0]); L.add(&d.n_sparse, sz[1]); L.add(&d.numeric, sz[2]); L.add(&d.progression, sz[3]); L.add(&d.n_progression, sz[4]);
    L.add(&d.candidates, sz[5]); L.add(&d.n_candidates, sz[6]);
    int rc = scratch_for(h, L);
    if (rc) return rc;
    if ((rc = twin(h, game_style, &d))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    void* dst[7] = {out->sparse, out->n_sparse, out->numeric, out->progression, out->n_progression, out->candidates, out->n_candidates};
    const void* src[7] = {d.sparse, d.n_sparse, d.numeric, d.progression, d.n_progression, d.candidates, d.n_candidates};
    for (int i = 0; i < 7; i++) {
        if (!dst[i]) return fail(RMJ_ERR_ARG, "null output array");
        HIPCHK(hipMemcpy(dst[i], src[i], sz[i], hipMemcpyDeviceToHost));
    }
    return RMJ_OK;
}
// The same for the per-row calls (index[i] = game * 4 + seat): the index and the row arrays at 256-byte steps of the handle's scratch.  An
// array is where its device pointer lives, the caller's host array, its bytes per row and whether it goes UP to the device before the call or
// comes DOWN after it; a NULL host array - the entries have refused every one that is not optional - is not staged and its pointer stays NULL.
struct RowArray { void* slot; void* host; size_t row_bytes; enum { DOWN, UP } dir = DOWN; };
template <class Call>
static int row_call_host(rmj_env* h, const int32_t* index, uint32_t rows, std::initializer_list<RowArray> arrays, Call call) {
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t r = rows;
    int32_t* d_index;
    rmjh::DevLayout L;
    L.add(&d_index, r * 4);
    for (const RowArray& a : arrays)
        if (a.host) L.add((char**)a.slot, r * a.row_bytes);
    int rc = scratch_for(h, L);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(d_index, index, r * 4, hipMemcpyHostToDevice));
    for (const RowArray& a : arrays)
        if (a.host && a.dir == RowArray::UP) HIPCHK(hipMemcpy(*(char**)a.slot, a.host, r * a.row_bytes, hipMemcpyHostToDevice));
    if ((rc = call(d_index))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (const RowArray& a : arrays)
        if (a.host && a.dir == RowArray::DOWN) HIPCHK(hipMemcpy(a.host, *(char**)a.slot, r * a.row_bytes, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
// Average ms of one `launch` (returns an RMJ code): a warm-up, then `reps` launches between two events on `st`; settle: the warm-up is waited for
template <class Launch>
static int time_launches(hipStream_t st, uint32_t reps, bool settle, double* avg_ms, Launch launch) {
    DevTmp tmp;
    hipEvent_t e0, e1;
    HIPCHK(tmp.event(&e0));
    HIPCHK(tmp.event(&e1));
    int rc;
    if ((rc = launch())) return rc;  // warm-up
    if (settle) {
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    HIPCHK(hipEventRecord(e0, st));
    for (uint32_t i = 0; i < reps; i++)
        if ((rc = launch())) return rc;
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = (double)ms / reps;
    return RMJ_OK;
}

// a PPO transition collector bound to a handle (rmj_ppo_create): its pool is one device allocation
struct rmj_ppo {
    rmj_env* env = nullptr;
    RmjPpoConfig cfg{};
    double gamma_lambda = 0.0;   // gamma * lambda as the worker forms it (_ppo_worker.py:322), in double
    void* mem = nullptr;
    PpoPool P{};
};
// a set of MJAI logs as one device-resident event stream (rmj_logset_create)
struct rmj_logset {
    int device = 0;
    uint32_t M = 0, total = 0, K = 0, max_len = 0;
    std::vector<uint32_t> off, koff;   // [M + 1] first event / first kyoku row of every log
    RmjEvent* d_ev = nullptr;
    uint32_t *d_off = nullptr, *d_koff = nullptr;
    // a set parsed from text (rmj_logset_create_from_text) also holds its score tables and per-log results
    int32_t *d_start = nullptr, *d_end = nullptr;   // [K][4]
    int32_t* d_own = nullptr;                       // [K][8] the end scores every kyoku's own events gave, in two readings (rmj_logcheck_*)
    uint8_t* d_status = nullptr;                    // [M]
    uint32_t *d_errline = nullptr, *d_dec = nullptr;
};
// a log sample builder bound to a handle and a log set (rmj_logreplay_create): its pool and bookkeeping are one device allocation
struct rmj_logreplay {
    rmj_env* env = nullptr;
    rmj_logset* set = nullptr;
    RmjLogReplayConfig cfg{};
    void* mem = nullptr;
    LogRun R{};
    double* d_powers = nullptr;
    uint8_t* d_extra[LX_COUNT] = {};   // the records of kLogExtras[i], [capacity][slot_bytes] in an allocation of its own; NULL: made without its flag
    uint32_t n_powers = 0;
    rmjh::SlotChain chain;             // which slot replays which logs, the steps of a whole replay and the steps taken
};
// a checking replay bound to a handle and a log set (rmj_logcheck_create): its verdicts and bookkeeping are one device allocation
struct rmj_logcheck {
    rmj_env* env = nullptr;
    rmj_logset* set = nullptr;
    void* mem = nullptr;
    LogCheck R{};
    rmjh::SlotChain chain;
};
// the assignment of a replay on the device: slot_first [n + 1], slot_logs [M]
static hipError_t upload_chain(const rmjh::SlotChain& c, uint32_t M, const uint32_t* d_first, const uint32_t* d_logs) {
    hipError_t e = hipMemcpy((void*)d_first, c.slot_first.data(), c.slot_first.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && M) e = hipMemcpy((void*)d_logs, c.slot_logs.data(), (size_t)M * 4, hipMemcpyHostToDevice);
    return e;
}
// where every slot of a replay starts, on the device (the stream has drained: the copies are not ordered behind it)
static hipError_t upload_start_cursors(const rmjh::SlotChain& c, const rmj_logset* set, uint32_t n, uint32_t* d_pos, uint32_t* d_cur) {
    std::vector<uint32_t> pos(n), cur(n);
    c.start_cursors(set->off.data(), pos.data(), cur.data());
    hipError_t e = hipMemcpy(d_pos, pos.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    return e != hipSuccess ? e : hipMemcpy(d_cur, cur.data(), (size_t)n * 4, hipMemcpyHostToDevice);
}
// the shanten tables on a device, uploaded once (rmj_create: the handle's Env; the hand API)
static int shanten_tables_for(int device, ShantenTables* out) {
    static ShantenTables cache[64];
    static bool have[64] = {false};
    static std::mutex mu;   // handles are created from several host threads (MultiGpuVecEnv: one per shard, shards may share a device)
    if (device < 0 || device >= 64) return fail(RMJ_ERR_ARG, "device ordinal");
    std::lock_guard<std::mutex> lock(mu);
    if (!have[device]) {
        const ShantenHostTables& H = shanten_host_tables();
        uint64_t *ds, *dh;
        uint32_t *r9, *r7;
        HIPCHK(hipMalloc(&ds, H.suit.size() * 8));
        HIPCHK(hipMalloc(&dh, H.honor.size() * 8));
        HIPCHK(hipMalloc(&r9, H.rank9.size() * 4));
        HIPCHK(hipMalloc(&r7, H.rank7.size() * 4));
        HIPCHK(hipMemcpy(ds, H.suit.data(), H.suit.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dh, H.honor.data(), H.honor.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(r9, H.rank9.data(), H.rank9.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(r7, H.rank7.data(), H.rank7.size() * 4, hipMemcpyHostToDevice));
        uint32_t* r2;
        uint64_t* v6;
        HIPCHK(hipMalloc(&r2, H.r2.size() * 4));
        HIPCHK(hipMalloc(&v6, H.v6.size() * 8));
        HIPCHK(hipMemcpy(r2, H.r2.data(), H.r2.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(v6, H.v6.data(), H.v6.size() * 8, hipMemcpyHostToDevice));
        cache[device].suit = ds; cache[device].honor = dh; cache[device].rank9 = r9; cache[device].rank7 = r7;
        cache[device].r2 = r2; cache[device].v6 = v6;
        have[device] = true;
    }
    *out = cache[device];
    return RMJ_OK;
}
// The slabs of a handle's Env, each named once, in the order rmj_create allocates them: where the pointer lives, its bytes for B games
// and an event ring of `ring` records, and when rmj_create zeroes it - NEVER (k_reset writes all of it), AT_ALLOC, or LATE (queued
// behind the XCC probe).  create_impl, rmj_clone and rmj_destroy walk it.
struct EnvSlab { void** p; size_t bytes; enum { NEVER, AT_ALLOC, LATE } zero; };
static std::array<EnvSlab, 10> env_slabs(Env& d, size_t B = 0, size_t ring = 0) {   // (no sizes: for the pointers alone)
    return {{{(void**)&d.core, B * sizeof(GState), EnvSlab::NEVER}, {(void**)&d.wall, B * RMJ_WALL_STRIDE, EnvSlab::NEVER},
             {(void**)&d.legal, B * 4 * RMJ_MAX_LEGAL * sizeof(uint64_t), EnvSlab::LATE}, {(void**)&d.nlegal, B * 4, EnvSlab::LATE},
             {(void**)&d.mask, B * 4 * 82, EnvSlab::LATE}, {(void**)&d.waits, B * 4 * sizeof(uint64_t), EnvSlab::NEVER},
             {(void**)&d.status, B * sizeof(uint32_t), EnvSlab::NEVER}, {(void**)&d.events, B * ring * sizeof(RmjEvent), EnvSlab::LATE},
             {(void**)&d.win, B * 4 * sizeof(RmjWinResult), EnvSlab::AT_ALLOC}, {(void**)&d.wall_dg, B * 32, EnvSlab::AT_ALLOC}}};
}
// A per-step rollout: fn(stream, g0, g1) issues one step of games [g0, g1), n_steps times for each of the plan's k parts.  Games are
// independent: each part advances on a stream of its own (header: rmj_step_random), forked from the handle's and joined back into it.
template <class Fn>
static int run_parts(rmj_env* h, const rmjh::RolloutPlan& p, uint32_t n_steps, Fn fn) {
    // Side streams (and their join events) of the paths that split a batch over k streams - the per-step rollouts of RMJ_STEP4=0/1 builds and the unfused
    // step + encode rollout.  Round 6: created on first use, not in rmj_create: the default paths (fused rollouts, one stream) never touch them, and every live
    // stream makes hipDeviceSynchronize slower - with seven idle side streams the synchronisation behind the driver's 20-step window took ~45 us of a 0.78 ms
    // region (scripts/r06_window_order.py: the same window between stream synchronisations ran at 1.76 G env.step/s, between device synchronisations at 1.66 G).
    for (int i = 0; i < p.k - 1; i++) {
        if (!h->xstream[i]) HIPCHK(hipStreamCreateWithFlags(&h->xstream[i], hipStreamNonBlocking));
        if (!h->ev_join[i]) HIPCHK(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
    }
    if (p.k >= 2) HIPCHK(hipEventRecord(h->ev_fork, h->stream));
    for (int i = 1; i < p.k; i++) HIPCHK(hipStreamWaitEvent(h->xstream[i - 1], h->ev_fork, 0));
    for (uint32_t s = 0; s < n_steps; s++)
        for (int i = 0; i < p.k; i++) fn(i ? h->xstream[i - 1] : h->stream, p.part(i), p.part(i + 1));
    for (int i = 1; i < p.k; i++) {
        HIPCHK(hipEventRecord(h->ev_join[i - 1], h->xstream[i - 1]));
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join[i - 1], 0));
    }
    return RMJ_OK;
}
// The plan of a rollout on this handle (rmjh::rollout_plan is the one place that decides how a rollout runs).  *slots caches the
// waves of the rollout's ticket kernel the device holds at once: asked of the runtime at most once per handle and kernel, and only
// by a call that would otherwise run as tickets.  A query that fails leaves need_slots set in the plan of the rollout without tickets.
template <class Kernel>
static rmjh::RolloutPlan plan_rollout(rmj_env* h, uint32_t n_steps, int pol, bool encode, int only_active, Kernel ticket_kernel, uint32_t* slots) {
    const auto plan = [&] { return rmjh::rollout_plan(h->tune, h->cfg.n_games, n_steps, pol, encode, only_active, *slots, h->max_xcc_id); };
    int per_cu = 0, cus = 0;
    if (plan().need_slots && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ticket_kernel, 64, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) == hipSuccess)
        *slots = (uint32_t)(per_cu > 0 ? per_cu : 1) * (uint32_t)(cus > 0 ? cus : 1);
    return plan();
}
// An emit entry of the extra records `which` (entry: its name): the checks, then `emit(stream, records)` behind the scan k_log_emit runs behind;
// no_array: the batch has rows and lacks an array
template <class Emit>
static int logreplay_emit_extra(rmj_logreplay* r, int which, const char* entry, const void* out, bool no_array, Emit emit) {
    if (!r || !out) return fail(RMJ_ERR_ARG, "null argument");
    const uint8_t* records = r->d_extra[which];
    if (!records) return fail(RMJ_ERR_ARG, std::string(entry) + ": the builder was made without " + kLogExtras[which].flag_name);
    if (no_array) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = r->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_log_emit_scan, dim3((r->R.capacity + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK), dim3(PPO_SCAN_BLOCK), 0, h->stream, r->R);
    emit(h->stream, records);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// (defined in its section: ahead of rmj_step_random_encode it would put k_encode_base before the fused step kernels in the code object)
static void launch_encode_base_range(rmj_env* h, hipStream_t st, int only_active, float* d_out, uint32_t g0, uint32_t g1);

extern "C" {

const char* rmj_version(void) { return "riichi_mi355x 0.1 (gfx950)"; }
const char* rmj_last_error(void) { return g_err.c_str(); }
int rmj_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// body of rmj_create; on any failure the caller destroys the partially built handle (rmj_destroy tolerates null members)
static int create_impl(rmj_env* h, const RmjConfig* cfg, uint64_t** d_seeds_out) {
    uint32_t ring = cfg->event_ring ? cfg->event_ring : 64;
    uint32_t r2 = 64;
    while (r2 < ring) r2 <<= 1;
    h->ring = r2;
    rmjh::RolloutTuning& t = h->tune;
    if (const char* e = getenv("RMJ_STEP_STREAMS")) t.want_streams = atoi(e);
    if (const char* e = getenv("RMJ_STEP4")) t.quad = atoi(e);
    if (const char* e = getenv("RMJ_QUEUE_CHUNK")) t.queue_chunk = atoi(e);
    if (const char* e = getenv("RMJ_QUEUE_FORCE")) t.queue_force = atoi(e);
    if (const char* e = getenv("RMJ_QUEUE_TEST_SKIP_XCDS")) t.queue_skip_xcds = (uint32_t)strtoul(e, nullptr, 0) & 0xFFu;
    if (const char* e = getenv("RMJ_QUEUE_TAIL")) t.queue_tail = atoi(e) != 0;
    if (const char* e = getenv("RMJ_QUEUE_MIN_CHUNK")) t.queue_min_chunk = atoi(e) > 0 ? atoi(e) : 1;
    if (const char* e = getenv("RMJ_HEAVY_FIRST")) t.heavy_first = atoi(e);
    t.rows_pw = rmjh::rows_for_batch(cfg->n_games);
    if (const char* e = getenv("RMJ_ROWS")) { const int r = atoi(e); if (r == 1 || r == 2 || r == 4) t.rows_pw = (uint32_t)r; }
    if (const char* e = getenv("RMJ_ENC_FUSED")) t.enc_fused = atoi(e);
    h->kern = cfg->game_mode >= 3 ? &kStepKernels3 : &kStepKernels4;
    const size_t B = cfg->n_games;
    Env& d = h->d;
    HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    // (the side streams of the split paths are created when such a path first runs: run_parts)
    // the two events of rmj_time_rollout* / rmj_bench_rollout: here, not at their first use - the driver's timed region IS their first use, and two
    // hipEventCreate calls between its host timestamps cost the 20-step window ~4 % (round 6, scripts/r06_window_order.py: first window 1.65-1.69 G, later ones 1.76 G)
    for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&h->ev_time[i]));
    const auto slabs = env_slabs(d, B, r2);
    for (const EnvSlab& s : slabs) {
        HIPCHK(hipMalloc(s.p, s.bytes));
        if (s.zero == EnvSlab::AT_ALLOC) HIPCHK(hipMemsetAsync(*s.p, 0, s.bytes, h->stream));
    }
    HIPCHK(hipMalloc(&h->d_actions, B * 4 * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&h->d_counter, sizeof(unsigned long long)));
    {   // The ticket rollout (k_step4_queue) hands a quad from wave to wave through ONE XCD's L2 and keys its eight queues by
        // HW_REG_XCC_ID & 7: on a part or partition mode that reports ids >= 8 two XCDs would share a queue and the hand-over
        // would cross L2s without a write-back.  A probe launch (more blocks than any dispatcher keeps on one XCD) records the
        // largest id; tickets are used only when it is <= 7 (rmjh::rollout_plan), k_step4<true> otherwise.
        HIPCHK(hipMemsetAsync(h->d_counter, 0, sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(k_probe_xcc, dim3(4096), dim3(64), 0, h->stream, h->d_counter);
        HIPCHK(hipGetLastError());
        unsigned long long m = 0;
        HIPCHK(hipMemcpyAsync(&m, h->d_counter, sizeof(m), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->max_xcc_id = (uint32_t)m;
    }
    HIPCHK(hipMalloc(&h->d_obs_offs, (B + (B + 1023) / 1024) * sizeof(uint32_t)));   // per game + per scan block
    for (const EnvSlab& s : slabs)
        if (s.zero == EnvSlab::LATE) HIPCHK(hipMemsetAsync(*s.p, 0, s.bytes, h->stream));
    d.ring_mask = r2 - 1;
    d.n_games = cfg->n_games;
    d.rule_bits = cfg->rule_bits;
    d.game_mode = cfg->game_mode;
    d.skip_log = cfg->skip_mjai_logging;
    d.ctor_round_wind = cfg->round_wind;
    d.game_offset = cfg->game_offset;
    d.enc_stride = (uint32_t)(ENC_CH * (cfg->game_mode >= 3 ? ENC_W3 : ENC_W4));
    d.pad_ = 0;
    int rc;
    if ((rc = shanten_tables_for(cfg->device, &d.sh))) return rc;
    HIPCHK(hipMalloc(&h->d_env, sizeof(Env)));
    HIPCHK(hipMemcpy(h->d_env, &d, sizeof(Env), hipMemcpyHostToDevice));
    {
        float decay[RMJ_MAX_DISCARDS];
        for (int a = 0; a < RMJ_MAX_DISCARDS; a++) decay[a] = expf(-0.2f * (float)a);  // same call as the reference's f32::exp
        HIPCHK(hipMalloc(&h->d_decay, sizeof(decay)));
        HIPCHK(hipMemcpy(h->d_decay, decay, sizeof(decay), hipMemcpyHostToDevice));
    }
    ResetArgs A;
    memset(&A, 0, sizeof(A));
    A.is_ctor = 1;
    A.base_seed = cfg->base_seed;
    if (cfg->seeds) {
        HIPCHK(hipMalloc(d_seeds_out, B * sizeof(uint64_t)));
        HIPCHK(hipMemcpy(*d_seeds_out, cfg->seeds, B * sizeof(uint64_t), hipMemcpyHostToDevice));
        A.seeds = *d_seeds_out;
    }
    RMJ_LAUNCH_MODE(h, k_reset, game_grid(cfg->n_games), dim3(256), A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}
int rmj_create(const RmjConfig* cfg, rmj_handle* out) {
    if (!cfg || !out || cfg->n_games == 0) return fail(RMJ_ERR_ARG, "bad config");
    if (cfg->game_mode > 5) return fail(RMJ_ERR_ARG, "game_mode must be 0..5");
    int rc = ensure_device(cfg->device);
    if (rc) return rc;
    rmj_env* h = new rmj_env();
    h->cfg = *cfg;
    memset(&h->d, 0, sizeof(h->d));
    uint64_t* d_seeds = nullptr;
    rc = create_impl(h, cfg, &d_seeds);
    if (d_seeds) hipFree(d_seeds);
    h->cfg.seeds = nullptr;
    if (rc) {  // nothing allocated so far outlives a failed constructor (an OOM at 524 288 games would strand GBs)
        const std::string keep = g_err;
        rmj_destroy(h);
        g_err = keep;
        return rc;
    }
    *out = h;
    return RMJ_OK;
}

int rmj_destroy(rmj_handle h) {
    if (!h) return RMJ_OK;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (const EnvSlab& s : env_slabs(h->d)) hipFree(*s.p);
    for (void* p : {(void*)h->d_decay, (void*)h->d_actions, (void*)h->d_counter, (void*)h->d_obs_offs, (void*)h->d_env, (void*)h->d_qheads, (void*)h->d_ev_lost,
                    h->d_track, h->d_heavy})
        hipFree(p);
    while (!h->ppo.empty()) rmj_ppo_destroy(h->ppo.back());
    while (!h->logreplay.empty()) rmj_logreplay_destroy(h->logreplay.back());
    for (Grown* g : {&h->scratch, &h->pin, &h->txt, &h->txt_offs, &h->txt_work, &h->h_txt, &h->h_txt_offs, &h->det_claim}) g->release();
    for (int i = 0; i < 2; i++) if (h->ev_time[i]) hipEventDestroy(h->ev_time[i]);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    for (int i = 0; i < RMJ_MAX_ROLLOUT_STREAMS - 1; i++) {
        if (h->xstream[i]) { hipStreamSynchronize(h->xstream[i]); hipStreamDestroy(h->xstream[i]); }
        if (h->ev_join[i]) hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    delete h;
    return RMJ_OK;
}

int rmj_clone(rmj_handle h, rmj_handle* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));   // (before anything is allocated: an early return below must not strand the copy)
    RmjConfig cfg = h->cfg;
    cfg.seeds = nullptr;
    cfg.event_ring = h->d.ring_mask + 1u;
    rmj_handle c = nullptr;
    int rc = rmj_create(&cfg, &c);
    if (rc) return rc;
    c->tune = h->tune;
    if (h->d.enc_stride != c->d.enc_stride) { int rc2 = rmj_set_encode_row_stride(c, h->d.enc_stride); if (rc2) { rmj_destroy(c); return rc2; } }
    const size_t B = h->cfg.n_games, ring = (size_t)h->d.ring_mask + 1u;
    const auto from = env_slabs(h->d, B, ring), to = env_slabs(c->d, B, ring);
    for (size_t i = 0; i < from.size(); i++) {
        if (hipMemcpyAsync(*to[i].p, *from[i].p, from[i].bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
            rmj_destroy(c);
            return fail(RMJ_ERR_HIP, "rmj_clone: device copy failed");
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        rmj_destroy(c);
        return fail(RMJ_ERR_HIP, "rmj_clone: device copy failed");
    }
    *out = c;
    return RMJ_OK;
}

int rmj_copy_games(rmj_handle dst, const uint32_t* dst_idx, rmj_handle src, const uint32_t* src_idx, uint32_t n) {
    DevTmp tmp;
    if (!dst || !src || (n && (!dst_idx || !src_idx))) return fail(RMJ_ERR_ARG, "null argument");
    if (dst->cfg.device != src->cfg.device || (dst->cfg.game_mode >= 3) != (src->cfg.game_mode >= 3) || dst->d.ring_mask != src->d.ring_mask)
        return fail(RMJ_ERR_ARG, "rmj_copy_games: the handles must share device, player count and event ring size");
    if (n == 0) return RMJ_OK;
    for (uint32_t i = 0; i < n; i++)
        if (dst_idx[i] >= dst->cfg.n_games || src_idx[i] >= src->cfg.n_games) return fail(RMJ_ERR_ARG, "rmj_copy_games: game index out of range");
    HIPCHK(hipSetDevice(dst->cfg.device));
    uint32_t *d_a, *d_b;
    int rc;
    if ((rc = tmp.upload(dst_idx, n, &d_a)) || (rc = tmp.upload(src_idx, n, &d_b))) return rc;
    if (src != dst) HIPCHK(hipStreamSynchronize(src->stream));
    RMJ_LAUNCH_MODE(dst, k_copy_games, dim3(n), dim3(64), (const Env*)src->d_env, d_a, d_b, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(dst->stream));
    return RMJ_OK;
}

int rmj_copy_games_device(rmj_handle dst, const uint32_t* d_dst_idx, rmj_handle src, const uint32_t* d_src_idx, uint32_t n) {
    if (!dst || !src || (n && (!d_dst_idx || !d_src_idx))) return fail(RMJ_ERR_ARG, "null argument");
    if (dst->cfg.device != src->cfg.device || (dst->cfg.game_mode >= 3) != (src->cfg.game_mode >= 3) || dst->d.ring_mask != src->d.ring_mask)
        return fail(RMJ_ERR_ARG, "rmj_copy_games_device: the handles must share device, player count and event ring size");
    if (n == 0) return RMJ_OK;
    HIPCHK(hipSetDevice(dst->cfg.device));
    if (src != dst && src->stream != dst->stream) HIPCHK(hipStreamSynchronize(src->stream));
    RMJ_LAUNCH_MODE(dst, k_copy_games, dim3(n), dim3(64), (const Env*)src->d_env, d_dst_idx, d_src_idx, n);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}

int rmj_reset(rmj_handle h, const uint8_t* select, const uint8_t* walls, const uint8_t* oya, const uint8_t* round_wind,
              const int32_t* scores, const uint8_t* honba, const uint32_t* kyotaku) {
    DevTmp tmp;
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t B = h->cfg.n_games;
    uint8_t *d_sel, *d_walls, *d_oya, *d_rw, *d_honba;
    int32_t* d_sc;
    uint32_t* d_ky;
    int rc;
    if ((rc = tmp.upload(select, B, &d_sel))) return rc;
    if ((rc = tmp.upload(walls, B * 136, &d_walls))) return rc;
    if ((rc = tmp.upload(oya, B, &d_oya))) return rc;
    if ((rc = tmp.upload(round_wind, B, &d_rw))) return rc;
    if ((rc = tmp.upload(scores, B * 4, &d_sc))) return rc;
    if ((rc = tmp.upload(honba, B, &d_honba))) return rc;
    if ((rc = tmp.upload(kyotaku, B, &d_ky))) return rc;
    ResetArgs A;
    memset(&A, 0, sizeof(A));
    A.select = d_sel; A.walls = d_walls; A.oya = d_oya; A.round_wind = d_rw; A.scores = d_sc; A.honba = d_honba; A.kyotaku = d_ky;
    RMJ_LAUNCH_MODE(h, k_reset, game_grid(h->cfg.n_games), dim3(256), A);
    if (h->d_track)   // the round tracker must not read the reset as the end of a round (rmj_round_track_device)
        hipLaunchKernelGGL(k_track_mark, dim3((h->cfg.n_games + 255u) / 256u), dim3(256), 0, h->stream, (uint8_t*)h->d_track + B * 37, (const uint8_t*)d_sel, 0u, h->cfg.n_games);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}

// Whole-batch per-step launches in heavy-first order (HeavyOrder): the previous launch's notes name the units that will end a round,
// restart or may settle a Ron - they get the first blocks.  The order of the handle's next launch of `units` units; without the
// buffer (allocated here on first use), the plain order.
static const HeavyOrder kPlainOrder = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u};
static HeavyOrder next_heavy_order(rmj_env* h, hipStream_t st, uint32_t units) {
    HeavyOrder ho = kPlainOrder;
    const uint32_t front = units / 4u;
    const size_t o_list = 384, o_flag = o_list + 2 * (size_t)front * 4, bytes = o_flag + 2 * (size_t)units;   // three counters, a line each
    if (!h->d_heavy) {
        if (hipMalloc(&h->d_heavy, bytes) == hipSuccess) hipMemsetAsync(h->d_heavy, 0, bytes, st);
        else h->d_heavy = nullptr;
    }
    if (h->d_heavy) {
        uint8_t* b = (uint8_t*)h->d_heavy;
        const uint32_t k = h->heavy_phase, in = k & 1u, out = in ^ 1u;
        ho.in_cnt = (const uint32_t*)(b + 128 * (k % 3u)); ho.out_cnt = (uint32_t*)(b + 128 * ((k + 1u) % 3u)); ho.zero_cnt = (uint32_t*)(b + 128 * ((k + 2u) % 3u));
        ho.in_list = (const uint32_t*)(b + o_list) + (size_t)front * in; ho.out_list = (uint32_t*)(b + o_list) + (size_t)front * out;
        ho.in_flag = b + o_flag + (size_t)units * in; ho.out_flag = b + o_flag + (size_t)units * out;
        ho.front = front;
        h->heavy_phase = (k + 1u) % 6u;   // (period of the counter and the list rotation)
    }
    return ho;
}
// one k_step launch over games [g0, g1) of the handle
static inline void launch_step_range(rmj_env* h, hipStream_t st, const uint64_t* d_actions, uint64_t policy_seed, uint32_t flags,
                                     uint32_t g0, uint32_t g1) {
    if (!h->tune.quad) {
        hipLaunchKernelGGL(h->kern->step, step_grid(g1 - g0), dim3(64 * RMJ_STEP_WPB), 0, st, (const Env*)h->d_env, d_actions, policy_seed, flags, g0, g1);
        return;
    }
    // four games per wave (device policy, packed actions or action ids); small batches: two or one (rows_pw)
    const uint32_t rows = h->tune.rows_pw, units = (g1 - g0 + rows - 1u) / rows;
    const HeavyOrder ho = h->tune.heavy_first && rmjh::heavy_first_eligible(h->cfg.n_games, rows, g0, g1) ? next_heavy_order(h, st, units) : kPlainOrder;
    const int pol = (flags & STEP_F_GREEDY) != 0u;   // (four-games-per-wave kernels only: the callers check tune.quad)
    hipLaunchKernelGGL(h->kern->step4[0][pol], dim3(units + ho.front), dim3(64), 0, st, (const Env*)h->d_env, policy_seed,
                       flags | rmjh::rows_flag_bits(rows), g0, g1, 1u, d_actions, ho);
}
int rmj_step_device(rmj_handle h, const rmj_action_t* d_actions) {
    if (!h || !d_actions) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    launch_step_range(h, h->stream, (const uint64_t*)d_actions, 0ull, 0u, 0u, h->cfg.n_games);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// Trainer-side entry (row N4): the policy's categorical outputs (action ids of the 82- / 60-way space, -1 = no action),
// resident on the device, are mapped to the first legal action with that id (Observation.find_action,
// observation/python.rs:119-122) inside the step kernel.  An id without a legal action is an illegal action (chombo).
int rmj_step_ids_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset) {
    if (!h || !d_action_ids) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t flags = STEP_F_IDS | (auto_reset ? STEP_F_AUTORESET : 0u);
    launch_step_range(h, h->stream, reinterpret_cast<const uint64_t*>(d_action_ids), 0ull, flags, 0u, h->cfg.n_games);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// rmj_step_ids_device + rmj_encode_device(only_active = 2) as ONE launch (k_step4_act_enc): the step of every game under the policy's
// action ids, then Observation.encode() of the seats that are to act next into the resident tensor d_out [n][4][74][W].
int rmj_step_ids_encode_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset, float* d_out) {
    if (!h || !d_action_ids || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    if (!h->tune.quad) return fail(RMJ_ERR_ARG, "rmj_step_ids_encode_device runs in the four-games-per-wave kernels (RMJ_STEP4=0 selects the one-game kernel)");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t flags = STEP_F_IDS | (auto_reset ? STEP_F_AUTORESET : 0u);
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(h->kern->act_enc, dim3((n + 3u) / 4u), dim3(64), 0, h->stream, (const Env*)h->d_env, flags, 0u, n, reinterpret_cast<const uint64_t*>(d_action_ids), d_out);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// the rows of the logits, where the caller gives any, hold the handle's whole action space
static int check_logits_stride(const rmj_env* h, const float* d_logits, uint32_t stride) {
    const uint32_t A = h->cfg.game_mode >= 3 ? RMJ_ACTION_SPACE_3P : RMJ_ACTION_SPACE_4P;
    return d_logits && stride < A ? fail(RMJ_ERR_ARG, "logits row shorter than the action space") : RMJ_OK;
}
// rmj_sample_ids_device + rmj_step_ids_encode_device as ONE launch (k_step4_sample_enc): every wave draws the ids of its own four games
// (the same keyed draw: identical ids, written to d_ids for the caller), steps them and encodes the seats that act next.
int rmj_step_sample_encode_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int auto_reset, int32_t* d_ids, float* d_out) {
    if (!h || !d_ids || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    if (!h->tune.quad) return fail(RMJ_ERR_ARG, "rmj_step_sample_encode_device runs in the four-games-per-wave kernels (RMJ_STEP4=0 selects the one-game kernel)");
    if (int rc = check_logits_stride(h, d_logits, stride)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t flags = STEP_F_IDS | (auto_reset ? STEP_F_AUTORESET : 0u);
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(h->kern->sample_enc, dim3((n + 3u) / 4u), dim3(64), 0, h->stream, (const Env*)h->d_env, flags, 0u, n, d_logits, stride, seed, d_ids, d_out);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_sample_ids_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int32_t* d_ids) {
    if (!h || !d_ids) return fail(RMJ_ERR_ARG, "null argument");
    if (int rc = check_logits_stride(h, d_logits, stride)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_sample_ids, dim3((n + 15) / 16), dim3(256), 0, h->stream, h->d, d_logits, stride, seed, d_ids);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_select_ids_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, const uint8_t* d_hero, int32_t* d_ids) {
    if (!h || !d_ids) return fail(RMJ_ERR_ARG, "null argument");
    if (int rc = check_logits_stride(h, d_logits, stride)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_select_ids, dim3((n + 15) / 16), dim3(256), 0, h->stream, h->d, d_logits, stride, seed, d_hero, d_ids);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_device_views(rmj_handle h, RmjDeviceViews* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    out->n_games = h->cfg.n_games;
    out->status = h->d.status;
    out->nlegal = h->d.nlegal;
    out->legal = h->d.legal;
    out->mask = h->d.mask;
    out->waits = h->d.waits;
    out->stream = (void*)h->stream;
    return RMJ_OK;
}
int rmj_scores_device(rmj_handle h, int32_t* d_scores, uint32_t* d_event_counts) {
    if (!h || !d_scores) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_gather_scores, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d.core, n, d_scores, d_event_counts);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// RiichiEnv.points(rule_name) (env.rs:691-727) of every game on the device: rule 0 = "basic", 1 = "ouza-tyoujyo", 2 = "ouza-normal"
// (3P knows "basic" only, like the reference); d_points [n][4] f64, seats beyond the player count get 0.  Asynchronous on the
// handle's stream: the reward a trainer-side loop reads without leaving the GPU.
int rmj_points_device(rmj_handle h, int rule, double* d_points) {
    if (!h || !d_points) return fail(RMJ_ERR_ARG, "null argument");
    const bool sanma = h->cfg.game_mode >= 3;
    if (rule < 0 || rule > (sanma ? 0 : 2)) return fail(RMJ_ERR_ARG, sanma ? "Unknown preset rule for 3P" : "Unknown preset rule");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    static const double UMA4[3][4] = {{50.0, 10.0, -10.0, -50.0}, {100.0, 40.0, -40.0, -100.0}, {50.0, 20.0, -20.0, -50.0}};
    const double w = sanma ? 1.0 : (rule == 0 ? 1.0 : 0.0), base = sanma ? 35000.0 : 25000.0;
    const double u0 = sanma ? 40.0 : UMA4[rule][0], u1 = sanma ? 0.0 : UMA4[rule][1], u2 = sanma ? -40.0 : UMA4[rule][2], u3 = sanma ? 0.0 : UMA4[rule][3];
    hipLaunchKernelGGL(k_points, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d.core, n, sanma ? 3 : 4, w, base, u0, u1, u2, u3, d_points);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_get_points(rmj_handle h, int rule, double* points) {
    DevTmp tmp;
    if (!h || !points) return fail(RMJ_ERR_ARG, "null argument");
    double* d;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(tmp.alloc(&d, (size_t)h->cfg.n_games * 4 * sizeof(double)));
    int rc = rmj_points_device(h, rule, d);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(points, d, (size_t)h->cfg.n_games * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return RMJ_OK;
}
// Row stride of the base encoder's outputs (rmj_encode(_device), rmj_encode_compact_device, rmj_step_random_encode, rmj_step_ids_encode_device):
// every (game, seat) row - 74 x W floats - starts `floats` floats after the previous one; 0 restores the dense layout (74 x W).  Padding
// the rows to a multiple of 256 B (2 048 floats in 3P, 2 560 in 4P) costs 2 % more memory and lets the acting seats' rows - one row in
// four of the tensor - leave at 1.3-1.4 x the rate: unaligned rows of 7 992 / 10 064 B are written at 3.8 TB/s, aligned ones at 5.0-5.3
// (torch fills of the same pattern, scripts/micro/row_stride_fill.py).  The pad floats are never written.
int rmj_set_encode_row_stride(rmj_handle h, uint32_t floats) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    const uint32_t dense = (uint32_t)(ENC_CH * (h->cfg.game_mode >= 3 ? ENC_W3 : ENC_W4));
    if (floats == 0) floats = dense;
    if (floats < dense || (floats & 1u)) return fail(RMJ_ERR_ARG, "row stride must be an even number of floats >= 74 x W");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->d.enc_stride = floats;
    HIPCHK(hipMemcpy(h->d_env, &h->d, sizeof(Env), hipMemcpyHostToDevice));
    return RMJ_OK;
}
int rmj_set_stream(rmj_handle h, void* stream, int own) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));  // everything issued so far is complete before the order changes hands
    h->stream = own ? h->own_stream : (hipStream_t)stream;  // (a NULL stream is the device's default stream)
    return RMJ_OK;
}
int rmj_sync(rmj_handle h) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}
int rmj_step(rmj_handle h, const rmj_action_t* actions) {
    if (!h || !actions) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_actions, actions, (size_t)h->cfg.n_games * 4 * sizeof(uint64_t), hipMemcpyHostToDevice));
    return rmj_step_device(h, h->d_actions);
}
// The ticket rollouts' counters, one allocation made and zeroed by the handle's first ticket rollout: three sets of ticket counters (one
// line per XCD) + the quads' ticket counts, and behind them the games' step counts of the running rollout, carried from ticket to
// ticket (*prog: written before it is read).  Set 0 is the step rollout's: zeroed once here and re-armed by every k_step4_fixup launch
// behind its ticket launch, so no memset sits between rollouts and a captured rollout can be replayed (round 6; round 5 alternated two
// sets from the host, which a graph replay of one launch found exhausted).  Set 2 is the step + encode rollout's, which memsets it in
// front of every rollout.
static int ticket_counters(rmj_env* h, int set, uint32_t** heads, uint32_t** done, uint32_t** prog) {
    const size_t quads = (h->cfg.n_games + 3u) / 4u, set_words = 8 * RMJ_Q_STRIDE + quads;
    if (!h->d_qheads) {
        HIPCHK(hipMalloc(&h->d_qheads, (3 * set_words + quads * 4) * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(h->d_qheads, 0, 3 * set_words * sizeof(uint32_t), h->stream));
    }
    *heads = h->d_qheads + set * set_words;
    *done = *heads + 8 * RMJ_Q_STRIDE;
    *prog = h->d_qheads + 3 * set_words;
    if (set == 2) HIPCHK(hipMemsetAsync(*heads, 0, set_words * sizeof(uint32_t), h->stream));
    return RMJ_OK;
}
// device-policy rollout: pol 0 = RandomAgent (rmj_step_random), 1 = the greedy policy (rmj_step_greedy); ran: the plan it executed
static int step_policy_impl(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, int pol, uint32_t call_rate, rmjh::RolloutPlan* ran = nullptr) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    uint32_t flags = STEP_F_RANDOM | (auto_reset ? STEP_F_AUTORESET : 0u);
    if (pol == 1) {
        if (!h->tune.quad) return fail(RMJ_ERR_ARG, "the greedy device policy runs in the four-games-per-wave kernels (RMJ_STEP4=0 selects the one-game kernel)");
        flags |= STEP_F_GREEDY | ((call_rate > 255u ? 255u : call_rate) << 8);
    }
    const StepKernels& K = *h->kern;
    const Env* const E = h->d_env;
    const uint32_t n = h->cfg.n_games;
    // (when the occupancy query fails the plan is the plain fused launch)
    const rmjh::RolloutPlan p = plan_rollout(h, n_steps, pol, false, 0, K.queue[pol == 1], &h->q_slots_pol[pol == 1]);
    if (p.how == rmjh::RolloutPlan::TICKETS) {
        // a long rollout of a batch that does not fill the chip a whole number of times, in (quad, chunk) tickets
        uint32_t *heads, *done, *prog;
        if (int rc = ticket_counters(h, 0, &heads, &done, &prog)) return rc;
        hipLaunchKernelGGL(K.queue[p.pol], dim3(p.grid_tickets), dim3(64), 0, h->stream, E, policy_seed, flags, n, n_steps, p.chunk, heads, done, h->tune.queue_skip_xcds, prog, (uint32_t)h->tune.queue_tail);
        hipLaunchKernelGGL(K.fixup[p.pol], dim3(p.grid_fixup), dim3(64), 0, h->stream, E, policy_seed, flags, n, n_steps, done);
    } else if (p.how == rmjh::RolloutPlan::FUSED) {
        // four games per wave, the whole rollout in ONE launch: every wave steps its own games n_steps times (k_step4<true>)
        hipLaunchKernelGGL(K.step4[1][p.pol], dim3(p.grid_plain), dim3(64), 0, h->stream, E, policy_seed, flags | p.row_flags, 0u, n, n_steps, (const uint64_t*)nullptr, kPlainOrder);
    } else if (int rc = run_parts(h, p, n_steps, [&](hipStream_t st, uint32_t g0, uint32_t g1) { launch_step_range(h, st, nullptr, policy_seed, flags, g0, g1); })) {
        return rc;
    }
    HIPCHK(hipGetLastError());
    if (ran) *ran = p;
    return RMJ_OK;
}
int rmj_step_random(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset) {
    return step_policy_impl(h, policy_seed, n_steps, auto_reset, 0, 0u);
}
int rmj_step_greedy(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, uint32_t call_rate_256) {
    return step_policy_impl(h, policy_seed, n_steps, auto_reset, 1, call_rate_256);
}
// The feature-output rollout of BASELINE configs[4]: every step of the device-policy rollout is followed by Observation.encode()
// of the seats that are to act, written into the resident tensor d_out [n][4][74][W] (only_active as in rmj_encode_device).
// Same results as n_steps x (rmj_step_random(h, seed, 1, auto_reset); rmj_encode_device(h, only_active, d_out)); issued like
// rmj_step_random as up to four parts of the batch on as many streams, each part running step, encode, step, encode ...
static int step_encode_impl(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, int only_active, float* d_out, rmjh::RolloutPlan* ran = nullptr) {
    if (!h || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t flags = STEP_F_RANDOM | (auto_reset ? STEP_F_AUTORESET : 0u);
    const StepKernels& K = *h->kern;
    const Env* const E = h->d_env;
    const uint32_t n = h->cfg.n_games;
    const rmjh::RolloutPlan p = plan_rollout(h, n_steps, 0, true, only_active, K.queue_enc, &h->q_slots_enc);
    if (p.need_slots) return fail(RMJ_ERR_HIP, "occupancy query failed");
    if (p.how == rmjh::RolloutPlan::TICKETS) {
        // ... as (quad, chunk) tickets when the batch is between one and eight chip-fulls of waves (k_step4_queue_enc)
        uint32_t *heads, *done, *prog;
        if (int rc = ticket_counters(h, 2, &heads, &done, &prog)) return rc;
        hipLaunchKernelGGL(K.queue_enc, dim3(p.grid_tickets), dim3(64), 0, h->stream, E, policy_seed, flags, n, n_steps, p.chunk, heads, done, h->tune.queue_skip_xcds, d_out);
        hipLaunchKernelGGL(K.fixup_enc, dim3(p.grid_fixup), dim3(64), 0, h->stream, E, policy_seed, flags, n, n_steps, (const uint32_t*)done, d_out);
    } else if (p.how == rmjh::RolloutPlan::FUSED) {
        // Round 3: ONE launch - every wave steps its four games and writes the rows of the seats that are to act, step after step (k_step4_enc)
        hipLaunchKernelGGL(K.enc, dim3(p.grid_plain), dim3(64), 0, h->stream, E, policy_seed, flags, 0u, n, n_steps, d_out);
    } else {
        // The encoder is bound by its stores, the step by instruction issue: parts of the batch on k streams put the step of one
        // part under the encoder of another (measured, 65 536 3P games: one stream 283 M env.step/s, four parts 383 M with the
        // four-game kernel and 323 M with the one-game kernel).
        if (int rc = run_parts(h, p, n_steps, [&](hipStream_t st, uint32_t g0, uint32_t g1) {
                launch_step_range(h, st, nullptr, policy_seed, flags, g0, g1);
                launch_encode_base_range(h, st, only_active, d_out, g0, g1);
            }))
            return rc;
    }
    HIPCHK(hipGetLastError());
    if (ran) *ran = p;
    return RMJ_OK;
}
int rmj_step_random_encode(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, int only_active, float* d_out) {
    return step_encode_impl(h, policy_seed, n_steps, auto_reset, only_active, d_out);
}
int rmj_random_actions(rmj_handle h, uint64_t policy_seed, rmj_action_t* actions) {
    if (!h || !actions) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_random_actions, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, policy_seed, h->d_actions);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(actions, h->d_actions, (size_t)n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RMJ_OK;
}

#define SYNC_FETCH(dst, src, bytes)                                   \
    do {                                                              \
        HIPCHK(hipSetDevice(h->cfg.device));                          \
        HIPCHK(hipStreamSynchronize(h->stream));                      \
        HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));    \
    } while (0)

int rmj_get_status(rmj_handle h, uint8_t* active_mask, uint8_t* phase, uint8_t* done) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    std::vector<uint32_t> st(h->cfg.n_games);
    SYNC_FETCH(st.data(), h->d.status, st.size() * 4);
    for (size_t i = 0; i < st.size(); i++) {
        if (active_mask) active_mask[i] = st[i] & 0xFF;
        if (phase) phase[i] = (st[i] >> 8) & 0xFF;
        if (done) done[i] = (st[i] >> 16) & 0xFF;
    }
    return RMJ_OK;
}
int rmj_get_legal(rmj_handle h, rmj_action_t* legal, uint8_t* counts) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    size_t B = h->cfg.n_games;
    if (legal) SYNC_FETCH(legal, h->d.legal, B * 4 * RMJ_MAX_LEGAL * sizeof(uint64_t));
    if (counts) SYNC_FETCH(counts, h->d.nlegal, B * 4);
    return RMJ_OK;
}
// What a host agent loop reads per step, without the 2 KB per game of the full [n][4][64] list slab: one row per seat that is to
// act, in (game, seat) order - index[row] = game * 4 + seat, its list = entries[offsets[row] .. offsets[row + 1]) - gathered on the
// device and brought down through pinned staging memory (~110 B per game instead of 2 055).  n_rows / n_entries report the totals;
// when they exceed the capacities only the first cap_rows rows / cap_entries entries were written (call again with more room).
int rmj_get_legal_compact(rmj_handle h, uint32_t* index, uint32_t* offsets /*[cap_rows + 1]*/, rmj_action_t* entries, uint32_t cap_rows, uint32_t cap_entries,
                          uint32_t* n_rows, uint32_t* n_entries) {
    if (!h || !index || !offsets || !entries || !n_rows || !n_entries) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games, blocks = (n + LC_BLOCK - 1) / LC_BLOCK;
    // device scratch: pre [n][2] | blk [blocks][2] | totals [2] | index [cap_rows] | offs [cap_rows] | entries [cap_entries]
    const size_t o_blk = (size_t)n * 8, o_tot = o_blk + (size_t)blocks * 8, o_idx = o_tot + 16, o_off = o_idx + (size_t)cap_rows * 4;
    const size_t o_ent = (o_off + ((size_t)cap_rows + 1) * 4 + 15) & ~(size_t)15, total = o_ent + (size_t)cap_entries * 8;
    void* sp;
    int rc = scratch_for(h, total, &sp);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)sp;
    uint32_t *pre = (uint32_t*)base, *blk = (uint32_t*)(base + o_blk), *tot = (uint32_t*)(base + o_tot), *d_idx = (uint32_t*)(base + o_idx), *d_off = (uint32_t*)(base + o_off);
    uint64_t* d_ent = (uint64_t*)(base + o_ent);
    hipLaunchKernelGGL(k_lc_count, dim3(blocks), dim3(LC_BLOCK), 0, h->stream, (const uint32_t*)h->d.status, (const uint8_t*)h->d.nlegal, n, pre, blk);
    hipLaunchKernelGGL(k_lc_scan, dim3(1), dim3(64), 0, h->stream, blk, blocks, tot);
    hipLaunchKernelGGL(k_lc_gather, dim3(blocks), dim3(LC_BLOCK), 0, h->stream, (const uint32_t*)h->d.status, (const uint8_t*)h->d.nlegal, (const uint64_t*)h->d.legal, n,
                       (const uint32_t*)pre, (const uint32_t*)blk, cap_rows, cap_entries, d_idx, d_off, d_ent);
    HIPCHK(hipGetLastError());
    const size_t need_pin = 16 + (size_t)cap_rows * 8 + 4 + (size_t)cap_entries * 8;
    h->stage_valid = false;   // (the pinned staging is shared with rmj_drain_format's size call)
    HIPCHK(h->pin.need(need_pin));
    uint8_t* pin = (uint8_t*)h->pin.p;
    HIPCHK(hipMemcpyAsync(pin, tot, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const uint32_t rows = ((uint32_t*)pin)[0], ents = ((uint32_t*)pin)[1];
    *n_rows = rows; *n_entries = ents;
    const uint32_t wr = rows < cap_rows ? rows : cap_rows, we = ents < cap_entries ? ents : cap_entries;
    uint8_t *p_idx = pin + 16, *p_off = p_idx + (size_t)cap_rows * 4, *p_ent = p_off + ((size_t)cap_rows + 1) * 4;
    if (wr) {
        HIPCHK(hipMemcpyAsync(p_idx, d_idx, (size_t)wr * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(p_off, d_off, ((size_t)wr + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (we) HIPCHK(hipMemcpyAsync(p_ent, d_ent, (size_t)we * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(index, p_idx, (size_t)wr * 4);
    if (wr) memcpy(offsets, p_off, ((size_t)wr + 1) * 4);   // offsets[wr] = the end of the last row written
    else offsets[0] = 0u;
    memcpy(entries, p_ent, (size_t)we * 8);
    return RMJ_OK;
}
int rmj_get_mask(rmj_handle h, uint8_t* mask) {
    if (!h || !mask) return fail(RMJ_ERR_ARG, "null argument");
    SYNC_FETCH(mask, h->d.mask, (size_t)h->cfg.n_games * 4 * 82);
    return RMJ_OK;
}
int rmj_get_waits(rmj_handle h, uint64_t* waits) {
    if (!h || !waits) return fail(RMJ_ERR_ARG, "null argument");
    SYNC_FETCH(waits, h->d.waits, (size_t)h->cfg.n_games * 4 * sizeof(uint64_t));
    return RMJ_OK;
}
static int fetch_scores(rmj_handle h, std::vector<int32_t>& sc, std::vector<uint32_t>& evc) {
    uint32_t n = h->cfg.n_games;
    int32_t* d_sc;
    uint32_t* d_ev;
    HIPCHK(hipSetDevice(h->cfg.device));
    void* sp;
    int rcs = scratch_for(h, (size_t)n * 20, &sp);
    if (rcs) return rcs;
    d_sc = (int32_t*)sp;
    d_ev = (uint32_t*)((char*)sp + (size_t)n * 16);
    hipLaunchKernelGGL(k_gather_scores, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d.core, n, d_sc, d_ev);
    sc.resize((size_t)n * 4);
    evc.resize(n);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(sc.data(), d_sc, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(evc.data(), d_ev, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_get_scores(rmj_handle h, int32_t* scores) {
    if (!h || !scores) return fail(RMJ_ERR_ARG, "null argument");
    std::vector<int32_t> sc;
    std::vector<uint32_t> ev;
    int rc = fetch_scores(h, sc, ev);
    if (rc) return rc;
    memcpy(scores, sc.data(), sc.size() * 4);
    return RMJ_OK;
}
// state.wall.salt / state.wall.wall_digest of the reference (state/wall.rs:15-16): 17 / 65 bytes per game, NUL-terminated; both empty for a
// wall without them (no RMJ_RULE_REFERENCE_RNG, or after a start_kyoku event: event_handler.rs:81-82)
int rmj_get_wall_digests(rmj_handle h, uint32_t first, uint32_t n, char* salts /*[n][17]*/, char* digests /*[n][65]*/) {
    if (!h || !salts || !digests) return fail(RMJ_ERR_ARG, "null argument");
    if (first > h->cfg.n_games || n > h->cfg.n_games - first) return fail(RMJ_ERR_RANGE, "game range out of bounds");
    if (n == 0) return RMJ_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    void* sp;
    int rcs = scratch_for(h, (size_t)n * 44, &sp);
    if (rcs) return rcs;
    hipLaunchKernelGGL(k_wall_digest, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->d.core, h->d.wall, h->d.wall_dg, first, n,
                       h->cfg.game_mode >= 3 ? 108 : 136, (uint32_t*)sp);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> host((size_t)n * 11);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host.data(), sp, (size_t)n * 44, hipMemcpyDeviceToHost));
    static const char* HX = "0123456789abcdef";
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* o = host.data() + (size_t)i * 11;
        char* s = salts + (size_t)i * 17;
        char* d = digests + (size_t)i * 65;
        if (!o[0]) { s[0] = 0; d[0] = 0; continue; }
        const uint64_t salt = (uint64_t)o[1] | ((uint64_t)o[2] << 32);
        for (int k = 0; k < 16; k++) s[k] = HX[(salt >> (60 - 4 * k)) & 15];   // format!("{:016x}")
        s[16] = 0;
        for (int k = 0; k < 64; k++) d[k] = HX[(o[3 + (k >> 3)] >> (28 - 4 * (k & 7))) & 15];   // format!("{:x}", hasher.finalize())
        d[64] = 0;
    }
    return RMJ_OK;
}
int rmj_get_wall_digest(rmj_handle h, uint32_t game, char* salt /*[17]*/, char* digest /*[65]*/) {
    if (!h) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    return rmj_get_wall_digests(h, game, 1, salt, digest);
}
int rmj_get_ranks(rmj_handle h, uint8_t* ranks) {  // env.rs:673-689
    if (!h || !ranks) return fail(RMJ_ERR_ARG, "null argument");
    std::vector<int32_t> sc;
    std::vector<uint32_t> ev;
    int rc = fetch_scores(h, sc, ev);
    if (rc) return rc;
    const int np = h->cfg.game_mode >= 3 ? 3 : 4;
    for (uint32_t g = 0; g < h->cfg.n_games; g++)
        for (int a = 0; a < 4; a++) {
            int r = 1;
            for (int b = 0; b < np; b++)
                if (sc[g * 4 + b] > sc[g * 4 + a] || (sc[g * 4 + b] == sc[g * 4 + a] && b < a)) r++;
            ranks[g * 4 + a] = a < np ? (uint8_t)r : 0;
        }
    return RMJ_OK;
}
int rmj_get_event_counts(rmj_handle h, uint32_t* counts) {
    if (!h || !counts) return fail(RMJ_ERR_ARG, "null argument");
    std::vector<int32_t> sc;
    std::vector<uint32_t> ev;
    int rc = fetch_scores(h, sc, ev);
    if (rc) return rc;
    memcpy(counts, ev.data(), ev.size() * 4);
    return RMJ_OK;
}
int rmj_get_step_counts(rmj_handle h, uint64_t* steps) {
    if (!h || !steps) return fail(RMJ_ERR_ARG, "null argument");
    uint32_t n = h->cfg.n_games;
    uint64_t* d;
    HIPCHK(hipSetDevice(h->cfg.device));
    void* sp;
    int rcs = scratch_for(h, (size_t)n * 8, &sp);
    if (rcs) return rcs;
    d = (uint64_t*)sp;
    hipLaunchKernelGGL(k_gather_steps, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d.core, n, d);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(steps, d, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_total_steps(rmj_handle h, uint64_t* total) {
    if (!h || !total) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipMemsetAsync(h->d_counter, 0, 8, h->stream));
    hipLaunchKernelGGL(k_sum_steps, dim3(512), dim3(256), 0, h->stream, h->d.core, h->cfg.n_games, h->d_counter);
    unsigned long long v = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(&v, h->d_counter, 8, hipMemcpyDeviceToHost));
    *total = v;
    return RMJ_OK;
}

int rmj_get_win_results(rmj_handle h, uint32_t game, RmjWinResult* out, uint8_t* seat_mask) {
    if (!h || !out || !seat_mask) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    GState st;
    SYNC_FETCH(&st, h->d.core + game, sizeof(GState));
    HIPCHK(hipMemcpy(out, h->d.win + (size_t)game * 4, 4 * sizeof(RmjWinResult), hipMemcpyDeviceToHost));
    *seat_mask = st.win_mask;
    for (int p = 0; p < 4; p++)
        if (!((st.win_mask >> p) & 1u)) memset(&out[p], 0, sizeof(RmjWinResult));
    return RMJ_OK;
}
int rmj_get_events(rmj_handle h, uint32_t game, uint32_t first, uint32_t max_events, RmjEvent* out, uint32_t* n_out) {
    if (!h || !out || !n_out) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    GState st;
    SYNC_FETCH(&st, h->d.core + game, sizeof(GState));
    // `first` counts from the current game's first record (GameState.mjai_log: a reset starts it again); the ring runs on stream positions
    const uint32_t total = st.ev_count - st.ev_base;
    const uint32_t lo = total > h->ring ? total - h->ring : 0;
    if (first < lo) return fail(RMJ_ERR_RANGE, "requested events already overwritten in the ring (create with a larger event_ring)");
    uint32_t n = 0;
    std::vector<RmjEvent> ring(h->ring);
    HIPCHK(hipMemcpy(ring.data(), h->d.events + (size_t)game * h->ring, (size_t)h->ring * sizeof(RmjEvent), hipMemcpyDeviceToHost));
    for (uint32_t i = first; i < total && n < max_events; i++) out[n++] = ring[(st.ev_base + i) & (h->ring - 1)];
    *n_out = n;
    return RMJ_OK;
}

// ---- state peek / poke (conversions: rmj_host.h) -------------------------------------------
int rmj_peek_state(rmj_handle h, uint32_t game, RmjStateView* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    GState st;
    uint8_t W[RMJ_WALL_STRIDE];
    SYNC_FETCH(&st, h->d.core + game, sizeof(GState));
    HIPCHK(hipMemcpy(W, h->d.wall + (size_t)game * RMJ_WALL_STRIDE, RMJ_WALL_STRIDE, hipMemcpyDeviceToHost));
    rmjh::to_view(st, W, out);
    return RMJ_OK;
}

int rmj_poke_state(rmj_handle h, uint32_t game, const RmjStateView* v) {
    if (!h || !v) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    GState S;
    uint8_t W[RMJ_WALL_STRIDE];
    SYNC_FETCH(&S, h->d.core + game, sizeof(GState));
    HIPCHK(hipMemcpy(W, h->d.wall + (size_t)game * RMJ_WALL_STRIDE, RMJ_WALL_STRIDE, hipMemcpyDeviceToHost));
    if (S.wall_meta == 1) {   // the view may carry another wall: salt and digest stay those of the shuffled one (state/wall.rs:69-80)
        void* sp;
        int rcs = scratch_for(h, 44, &sp);
        if (rcs) return rcs;
        hipLaunchKernelGGL(k_wall_digest, dim3(1), dim3(64), 0, h->stream, h->d.core, h->d.wall, h->d.wall_dg, game, 1u,
                           h->cfg.game_mode >= 3 ? 108 : 136, (uint32_t*)sp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h->d.wall_dg + (size_t)game * 8, (const uint32_t*)sp + 3, 32, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        S.wall_meta = 2;
    }
    if (const char* err = rmjh::from_view(S, W, v)) return fail(RMJ_ERR_ARG, err);
    HIPCHK(hipMemcpy(h->d.core + game, &S, sizeof(GState), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d.wall + (size_t)game * RMJ_WALL_STRIDE, W, RMJ_WALL_STRIDE, hipMemcpyHostToDevice));
    RMJ_LAUNCH_MODE(h, k_refresh, dim3(1), dim3(64), game);
    if (h->d_track) hipLaunchKernelGGL(k_track_mark, dim3(1), dim3(64), 0, h->stream, (uint8_t*)h->d_track + (size_t)h->cfg.n_games * 37, (const uint8_t*)nullptr, game, 1u);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}

// ---- MJAI formatting (state/mod.rs:2094-2148; parser.rs:301-334; formatter: rmj_host.h) -----
int rmj_format_event(const RmjEvent* ev, uint32_t n_avail, int seat, char* buf, uint32_t cap) {
    if (!ev || !buf || n_avail == 0 || cap == 0) return RMJ_ERR_ARG;
    rmjh::Out o{buf, buf + (cap - 1), 0};
    const int used = rmjh::format_event(o, ev, n_avail, seat);
    if (used < 0) return used;
    if (o.need + 1 > cap) return RMJ_ERR_RANGE;
    *o.p = 0;
    return used;
}
int rmj_format_events(const RmjEvent* ev, const uint32_t* offsets, uint32_t n_games, int seat, char* buf, uint64_t cap, uint64_t* text_offsets,
                      uint64_t* needed) {
    if (!ev || !offsets || !text_offsets || !needed) return RMJ_ERR_ARG;
    *needed = rmjh::format_events(ev, offsets, n_games, seat, buf, cap, text_offsets, 0);
    return (buf && *needed <= cap) ? RMJ_OK : RMJ_ERR_RANGE;
}

// ---- bulk drain of the event rings (k_ev_*: rmj_events.hip.h) ---------------------------------------------
// the device part of a drain: the handle's scratch holds [cursor | first | pre | blk | total | offsets | new cursor | records]
struct DrainPlan { uint32_t *d_cur, *d_first, *d_pre, *d_blk, *d_tot, *d_off, *d_new; RmjEvent* d_ev; uint32_t cap; };
static int drain_device(rmj_env* h, const uint32_t* cursor, uint32_t cap_events, DrainPlan* P, uint32_t* n_events) {
    const uint32_t n = h->cfg.n_games, blocks = (n + LC_BLOCK - 1) / LC_BLOCK;
    if (!h->d_ev_lost) {
        HIPCHK(hipMalloc(&h->d_ev_lost, (size_t)n * 4));
        HIPCHK(hipMemsetAsync(h->d_ev_lost, 0, (size_t)n * 4, h->stream));
    }
    // packed words, the records behind them at a multiple of 32 bytes: a first pass sizes them (the scan total), the buffer is sized by
    // the caller's cap or, when it passes 0, by the total
    rmjh::DevLayout L(4);
    L.add(&P->d_cur, (size_t)n * 4); L.add(&P->d_first, (size_t)n * 4); L.add(&P->d_pre, (size_t)n * 4); L.add(&P->d_blk, (size_t)blocks * 4);
    L.add(&P->d_tot, 16); L.add(&P->d_off, ((size_t)n + 1) * 4); L.add(&P->d_new, (size_t)n * 4, 32);
    L.add(&P->d_ev, (size_t)cap_events * sizeof(RmjEvent), 1);
    int rc = scratch_for(h, L);
    if (rc) return rc;
    P->cap = cap_events;
    HIPCHK(hipMemcpyAsync(P->d_cur, cursor, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ev_count, dim3(blocks), dim3(LC_BLOCK), 0, h->stream, (const GState*)h->d.core, n, h->ring, (const uint32_t*)P->d_cur, P->d_first, P->d_pre, P->d_blk);
    hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(64), 0, h->stream, P->d_blk, blocks, P->d_tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n_events, P->d_tot, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}
static void drain_gather(rmj_env* h, const DrainPlan& P) {
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_ev_gather, dim3((n + 3u) / 4u), dim3(256), 0, h->stream, (const GState*)h->d.core, (const RmjEvent*)h->d.events, n, h->ring,
                       (const uint32_t*)P.d_first, (const uint32_t*)P.d_pre, (const uint32_t*)P.d_blk, P.cap, P.d_ev, P.d_off, P.d_new);
}
static void drain_book(rmj_env* h, const DrainPlan& P) {
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_ev_book, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, (const uint32_t*)P.d_cur, (const uint32_t*)P.d_first, n, h->d_ev_lost);
}
static int pin_for(rmj_env* h, size_t bytes) {
    if (bytes > h->pin.cap) h->stage_valid = false;
    HIPCHK(h->pin.need(bytes));
    return RMJ_OK;
}
int rmj_get_log_positions(rmj_handle h, uint32_t* base, uint32_t* pos) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    void* sp;
    int rc = scratch_for(h, (size_t)n * 8, &sp);
    if (rc) return rc;
    uint32_t* d = (uint32_t*)sp;
    hipLaunchKernelGGL(k_log_positions, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, (const GState*)h->d.core, n, d, d + n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (base) HIPCHK(hipMemcpy(base, d, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (pos) HIPCHK(hipMemcpy(pos, d + n, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_drain_events(rmj_handle h, uint32_t* cursor, RmjEvent* out, uint32_t cap_events, uint32_t* offsets, uint32_t* n_events, uint32_t flags) {
    if (!h || !cursor || !offsets || !n_events || (!out && cap_events)) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    h->stage_valid = false;
    DrainPlan P;
    int rc = drain_device(h, cursor, cap_events, &P, n_events);
    if (rc) return rc;
    if (*n_events > cap_events) return fail(RMJ_ERR_RANGE, "rmj_drain_events: more records than cap_events (n_events holds the number; nothing was drained)");
    drain_gather(h, P);
    if (!(flags & RMJ_DRAIN_PEEK)) drain_book(h, P);
    HIPCHK(hipGetLastError());
    rc = pin_for(h, ((size_t)n * 2 + 1) * 4 + (size_t)*n_events * sizeof(RmjEvent));
    if (rc) return rc;
    uint8_t* pin = (uint8_t*)h->pin.p;
    HIPCHK(hipMemcpyAsync(pin, P.d_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(pin + ((size_t)n + 1) * 4, P.d_new, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (*n_events) HIPCHK(hipMemcpyAsync(out, P.d_ev, (size_t)*n_events * sizeof(RmjEvent), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(offsets, pin, ((size_t)n + 1) * 4);
    if (!(flags & RMJ_DRAIN_PEEK)) memcpy(cursor, pin + ((size_t)n + 1) * 4, (size_t)n * 4);
    return RMJ_OK;
}
// drain + format in one call: the records go to pinned staging owned by the handle and are formatted from there by a pool of host
// threads (one log per slot, events separated by '\n').  ms (optional, [3]): device gather, copy to the host, formatting.
// A size call (buf = NULL) leaves its gathered records staged; the call that follows with the same cursors, seat and flags formats that
// staging instead of draining again (the drain is then "as of the size call": what was logged since stays for the next drain).
int rmj_drain_format(rmj_handle h, uint32_t* cursor, int seat, char* buf, uint64_t cap, uint64_t* text_offsets, uint64_t* needed, uint32_t* n_events,
                     double* ms, uint32_t flags) {
    if (!h || !cursor || !text_offsets || !needed || !n_events) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    const size_t o_ev = (((size_t)n * 3 + 1) * 4 + 31) & ~(size_t)31;   // pinned: [offsets n + 1 | new cursors n | first n | pad | records]
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    const bool reuse = buf && h->stage_valid && h->stage_seat == seat && h->stage_cursor.size() == n &&
                       memcmp(h->stage_cursor.data(), cursor, (size_t)n * 4) == 0;
    if (!reuse) {
        h->stage_valid = false;
        DrainPlan P;
        int rc = drain_device(h, cursor, 0, &P, n_events);   // size pass with no record buffer ...
        if (rc) return rc;
        rc = drain_device(h, cursor, *n_events, &P, n_events);   // ... then the gather into a buffer of exactly that size (nothing ran in between)
        if (rc) return rc;
        drain_gather(h, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        auto t1 = now();
        rc = pin_for(h, o_ev + (size_t)*n_events * sizeof(RmjEvent));
        if (rc) return rc;
        uint8_t* pin = (uint8_t*)h->pin.p;
        HIPCHK(hipMemcpyAsync(pin, P.d_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pin + ((size_t)n + 1) * 4, P.d_new, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pin + ((size_t)n * 2 + 1) * 4, P.d_first, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        if (*n_events) HIPCHK(hipMemcpyAsync(pin + o_ev, P.d_ev, (size_t)*n_events * sizeof(RmjEvent), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        auto t2 = now();
        h->stage_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        h->stage_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
        h->stage_cursor.assign(cursor, cursor + n);
        h->stage_seat = seat;
        h->stage_events = *n_events;
        h->stage_valid = true;
    }
    uint8_t* pin = (uint8_t*)h->pin.p;
    *n_events = h->stage_events;
    auto t2 = now();
    *needed = rmjh::format_events((const RmjEvent*)(pin + o_ev), (const uint32_t*)pin, n, seat, buf, cap, text_offsets, 0);
    auto t3 = now();
    if (ms) {
        ms[0] = h->stage_ms[0];
        ms[1] = h->stage_ms[1];
        ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
    }
    if (!buf || *needed > cap)   // nothing was handed over: cursors and loss counters stand, the staging waits for the call with a buffer
        return fail(RMJ_ERR_RANGE, "rmj_drain_format: text buffer too small (needed holds the size; cursors unchanged)");
    h->stage_valid = false;
    if (!(flags & RMJ_DRAIN_PEEK)) {
        // book what the windows skipped (first - cursor) and move the cursors behind the windows
        const uint32_t* firsts = (const uint32_t*)(pin + ((size_t)n * 2 + 1) * 4);
        bool any = false;
        for (uint32_t g = 0; g < n && !any; g++) any = firsts[g] != cursor[g];
        if (any) {
            void* sp;
            int rc = scratch_for(h, (size_t)n * 8, &sp);
            if (rc) return rc;
            uint32_t* d = (uint32_t*)sp;
            HIPCHK(hipMemcpyAsync(d, cursor, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(d + n, firsts, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_ev_book, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, (const uint32_t*)d, (const uint32_t*)(d + n), n, h->d_ev_lost);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(h->stream));
        }
        memcpy(cursor, pin + ((size_t)n + 1) * 4, (size_t)n * 4);
    }
    return RMJ_OK;
}
// ---- MJAI text on the device (rmj_drain_text / rmj_format_events_device; k_text_*: rmj_events.hip.h) ------
// size, scan and write the text of n games (n > 0) into the handle's device buffers; *bytes = the text's size
static int text_format_device(rmj_env* h, const TextSrc& s, uint32_t n, int seat, uint32_t* d_newcur, uint64_t* bytes) {
    const uint32_t blocks = (n + 255u) / 256u;
    // the work area: record and byte counts of every game, then (at a multiple of 16 bytes) the scan's prefixes and its [blocks] + the total + a spare
    uint32_t *d_nrec, *d_bytes;
    uint64_t *d_pre, *d_blk;
    rmjh::DevLayout L(8);
    L.add(&d_nrec, (size_t)n * 4, 4); L.add(&d_bytes, (size_t)n * 4, 16); L.add(&d_pre, (size_t)n * 8); L.add(&d_blk, ((size_t)blocks + 2) * 8);
    HIPCHK(h->txt_work.need(L.bytes(), h->stream));
    HIPCHK(h->txt_offs.need(((size_t)n + 1) * 8, h->stream));
    L.bind(h->txt_work.p);
    uint64_t* d_txt_offs = (uint64_t*)h->txt_offs.p;
    hipLaunchKernelGGL(k_text_size, dim3((n + 3u) / 4u), dim3(256), 0, h->stream, s, n, seat, d_nrec, d_bytes, d_newcur);
    hipLaunchKernelGGL(k_text_scan1, dim3(blocks), dim3(256), 0, h->stream, (const uint32_t*)d_bytes, n, d_pre, d_blk);
    hipLaunchKernelGGL(k_text_scan2, dim3(1), dim3(1024), 0, h->stream, d_blk, blocks, d_txt_offs, n, d_blk + blocks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bytes, d_blk + blocks, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->txt.need(*bytes, h->stream));
    hipLaunchKernelGGL(k_text_write, dim3(n), dim3(64), 0, h->stream, s, n, seat, (const uint32_t*)d_nrec, (const uint32_t*)d_bytes, (const uint64_t*)d_pre,
                       (const uint64_t*)d_blk, d_txt_offs, (char*)h->txt.p);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// device view, or the one copy to pinned memory owned by the handle; returns with the stream synchronised
static int text_deliver(rmj_env* h, uint32_t n, uint64_t bytes, uint32_t flags, const uint32_t* d_newcur, uint32_t* cursor, RmjTextView* out,
                        std::chrono::steady_clock::time_point t0) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    HIPCHK(hipStreamSynchronize(h->stream));
    auto t1 = now();
    const size_t offs_b = ((size_t)n + 1) * 8, cur_b = cursor ? (size_t)n * 4 : 0;
    HIPCHK(h->h_txt_offs.need(offs_b + cur_b));
    const bool host = !(flags & RMJ_TEXT_ON_DEVICE);
    if (host) HIPCHK(h->h_txt.need(bytes));
    uint8_t* pin = (uint8_t*)h->h_txt_offs.p;
    if (host) {
        if (bytes) HIPCHK(hipMemcpyAsync(h->h_txt.p, h->txt.p, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pin, h->txt_offs.p, offs_b, hipMemcpyDeviceToHost, h->stream));
    }
    if (cur_b) HIPCHK(hipMemcpyAsync(pin + offs_b, d_newcur, cur_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    auto t2 = now();
    if (cur_b) memcpy(cursor, pin + offs_b, cur_b);
    out->text = host ? (const char*)h->h_txt.p : (const char*)h->txt.p;
    out->text_offsets = host ? (const uint64_t*)pin : (const uint64_t*)h->txt_offs.p;
    out->bytes = bytes;
    out->n_games = n;
    out->ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    out->ms[1] = host ? std::chrono::duration<double, std::milli>(t2 - t1).count() : 0.0;
    out->ms[2] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return RMJ_OK;
}
int rmj_drain_text(rmj_handle h, uint32_t* cursor, int seat, uint32_t flags, RmjTextView* out) {
    if (!h || !cursor || !out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = h->cfg.n_games;
    h->stage_valid = false;
    DrainPlan P;
    uint32_t n_ev = 0;
    int rc = drain_device(h, cursor, 0, &P, &n_ev);   // the windows: first[g] (no record buffer)
    if (rc) return rc;
    const TextSrc s{(const RmjEvent*)h->d.events, h->ring, (uint32_t)sizeof(RmjEvent), P.d_first, (const GState*)h->d.core};
    uint64_t bytes = 0;
    rc = text_format_device(h, s, n, seat, P.d_new, &bytes);
    if (rc) return rc;
    const bool peek = (flags & RMJ_DRAIN_PEEK) != 0;
    if (!peek) drain_book(h, P);
    HIPCHK(hipGetLastError());
    rc = text_deliver(h, n, bytes, flags, P.d_new, peek ? nullptr : cursor, out, t0);
    if (rc) return rc;
    out->n_events = n_ev;
    return RMJ_OK;
}
int rmj_format_events_device(rmj_handle h, const RmjEvent* d_ev, const uint32_t* d_offsets, uint32_t n_games, int seat, uint32_t flags, RmjTextView* out) {
    if (!h || !d_offsets || !out || (!d_ev && n_games)) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    auto t0 = std::chrono::steady_clock::now();
    h->stage_valid = false;
    uint64_t bytes = 0;
    if (n_games) {
        const TextSrc s{d_ev, 0u, (uint32_t)sizeof(RmjEvent), d_offsets, nullptr};
        int rc = text_format_device(h, s, n_games, seat, nullptr, &bytes);
        if (rc) return rc;
    } else {
        HIPCHK(h->txt_offs.need(8, h->stream));   // (no games: one offset and no work area)
        HIPCHK(hipMemsetAsync(h->txt_offs.p, 0, 8, h->stream));
    }
    uint32_t ends[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&ends[0], d_offsets, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&ends[1], d_offsets + n_games, 4, hipMemcpyDeviceToHost, h->stream));
    int rc = text_deliver(h, n_games, bytes, flags, nullptr, nullptr, out, t0);
    if (rc) return rc;
    out->n_events = ends[1] - ends[0];
    return RMJ_OK;
}
// ---- per-round rewards for a trainer on the same GPU (k_round_track: rmj_events.hip.h) --------------------
static int round_track_impl(rmj_env* h, int baseline, uint8_t* d_ended, int32_t* d_delta, int32_t* d_meta, uint8_t* d_kyoku_idx) {
    const uint32_t n = h->cfg.n_games;
    if (!h->d_track) {
        HIPCHK(hipMalloc(&h->d_track, (size_t)n * (4 + 16 + 16 + 4)));
        HIPCHK(hipMemsetAsync(h->d_track, 0, (size_t)n * (4 + 16 + 16 + 4), h->stream));
        baseline = 1;
    }
    RoundTrack T;
    uint8_t* b = (uint8_t*)h->d_track;
    T.hand_index = (uint32_t*)b; T.start_scores = (int32_t*)(b + (size_t)n * 4); T.start_meta = (int32_t*)(b + (size_t)n * 20); T.was_done = b + (size_t)n * 36; T.mark = b + (size_t)n * 37;
    hipLaunchKernelGGL(k_round_track, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, (const GState*)h->d.core, n, T, baseline, d_ended, d_delta, d_meta, d_kyoku_idx);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_round_track_device(rmj_handle h, uint8_t* d_ended, int32_t* d_delta, int32_t* d_meta, uint8_t* d_kyoku_idx) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    return round_track_impl(h, 0, d_ended, d_delta, d_meta, d_kyoku_idx);
}
int rmj_round_track_reset(rmj_handle h) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    return round_track_impl(h, 1, nullptr, nullptr, nullptr, nullptr);
}
int rmj_get_events_lost(rmj_handle h, uint32_t* lost) {
    if (!h || !lost) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->d_ev_lost) { memset(lost, 0, (size_t)h->cfg.n_games * 4); return RMJ_OK; }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(lost, h->d_ev_lost, (size_t)h->cfg.n_games * 4, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_event_views(rmj_handle h, RmjEventViews* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->d_ev_lost) {
        HIPCHK(hipMalloc(&h->d_ev_lost, (size_t)h->cfg.n_games * 4));
        HIPCHK(hipMemsetAsync(h->d_ev_lost, 0, (size_t)h->cfg.n_games * 4, h->stream));
    }
    out->n_games = h->cfg.n_games;
    out->ring = h->ring;
    out->events = h->d.events;
    out->ev_count = &h->d.core[0].ev_count;
    out->ev_count_stride = (uint32_t)sizeof(GState);
    out->lost = h->d_ev_lost;
    out->ev_base = &h->d.core[0].ev_base;
    return RMJ_OK;
}

// ---- batched hand math ---------------------------------------------------------------------
int rmj_eval_hands(int device, const RmjHandCase* cases, uint32_t n, RmjHandResult* out) {
    DevTmp tmp;
    if (!cases || !out) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    RmjHandCase* d_in;
    RmjHandResult* d_out;
    HIPCHK(tmp.alloc(&d_in, (size_t)n * sizeof(RmjHandCase)));
    HIPCHK(tmp.alloc(&d_out, (size_t)n * sizeof(RmjHandResult)));
    HIPCHK(hipMemcpy(d_in, cases, (size_t)n * sizeof(RmjHandCase), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_eval_hands, dim3((n + 15u) / 16u), dim3(256), 0, 0, d_in, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(RmjHandResult), hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_agari_counts(int device, const uint8_t* counts, uint32_t n, uint8_t* is_agari_out, uint8_t* is_tenpai, uint64_t* waits) {
    DevTmp tmp;
    if (!counts || !is_agari_out || !is_tenpai || !waits) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    uint8_t *d_c, *d_a, *d_t;
    uint64_t* d_w;
    HIPCHK(tmp.alloc(&d_c, (size_t)n * 34));
    HIPCHK(tmp.alloc(&d_a, n));
    HIPCHK(tmp.alloc(&d_t, n));
    HIPCHK(tmp.alloc(&d_w, (size_t)n * 8));
    HIPCHK(hipMemcpy(d_c, counts, (size_t)n * 34, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_agari_counts, dim3((n + 15) / 16), dim3(256), 0, 0, d_c, n, d_a, d_t, d_w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(is_agari_out, d_a, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(is_tenpai, d_t, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(waits, d_w, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_calculate_score(int device, const uint8_t* han, const uint8_t* fu, const uint8_t* is_oya, const uint8_t* is_tsumo,
                        const uint32_t* honba, const uint8_t* num_players, uint32_t n, uint32_t* out) {
    DevTmp tmp;
    if (!han || !fu || !is_oya || !is_tsumo || !honba || !num_players || !out) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    uint8_t *d_h, *d_f, *d_o, *d_t, *d_n;
    uint32_t *d_hb, *d_out;
    if ((rc = tmp.upload(han, n, &d_h)) || (rc = tmp.upload(fu, n, &d_f)) || (rc = tmp.upload(is_oya, n, &d_o)) || (rc = tmp.upload(is_tsumo, n, &d_t)) ||
        (rc = tmp.upload(num_players, n, &d_n)) || (rc = tmp.upload(honba, n, &d_hb)))
        return rc;
    HIPCHK(tmp.alloc(&d_out, (size_t)n * 16));
    hipLaunchKernelGGL(k_score, dim3((n + 255) / 256), dim3(256), 0, 0, d_h, d_f, d_o, d_t, d_hb, d_n, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    return RMJ_OK;
}

// ---- feature encoder (row A14) --------------------------------------------------------------------
// Observation.encode() of the games [g0, g1) on stream `st`.  The whole 74-channel tensor of a seat is staged at once: windows
// of 37 / 16 channels (more resident waves, the seat's work repeated per window) measured 0.195 / 0.35 ms against 0.19 ms
// for 65 536 4P games - the kernel is bound by its own instruction stream and the store epilogue, not by occupancy.
static void launch_encode_base_range(rmj_env* h, hipStream_t st, int only_active, float* d_out, uint32_t g0, uint32_t g1) {
    const dim3 grid(g1 - g0), block(64);
#define RMJ_LAUNCH_BASE(SM) \
    hipLaunchKernelGGL((k_encode_base<SM, false>), grid, block, 0, st, h->d, only_active, d_out, g0, (const uint32_t*)nullptr, (int32_t*)nullptr, 0u, (const uint32_t*)nullptr, (uint32_t*)nullptr)
    if (h->cfg.game_mode >= 3) RMJ_LAUNCH_BASE(true);
    else RMJ_LAUNCH_BASE(false);
#undef RMJ_LAUNCH_BASE
}
static int launch_encode(rmj_handle h, int only_active, float* d_out, bool ext) {
    if (!h || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const dim3 grid(h->cfg.n_games * 4), block(64);
    const float* decay = h->d_decay;
    const bool sanma = h->cfg.game_mode >= 3;
    if (sanma && ext) hipLaunchKernelGGL((k_encode_ext<true>), grid, block, 0, h->stream, h->d, only_active, decay, d_out);
    else if (ext) hipLaunchKernelGGL((k_encode_ext<false>), grid, block, 0, h->stream, h->d, only_active, decay, d_out);
    else launch_encode_base_range(h, h->stream, only_active, d_out, 0u, h->cfg.n_games);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_encode_device(rmj_handle h, int only_active, float* d_out) { return launch_encode(h, only_active, d_out, false); }
static void launch_encode_compact(rmj_env* h, float* d_out, int32_t* d_index, uint32_t capacity, uint32_t* d_count) {
    const uint32_t n = h->cfg.n_games, nb = (n + OBS_SCAN_BLOCK - 1) / OBS_SCAN_BLOCK;
    uint32_t* totals = h->d_obs_offs + n;
    hipLaunchKernelGGL(k_obs_offsets, dim3(nb), dim3(OBS_SCAN_BLOCK), 0, h->stream, (const uint32_t*)h->d.status, n, h->d_obs_offs, totals);
#define RMJ_LAUNCH_COMPACT(SM) \
    hipLaunchKernelGGL((k_encode_base<SM, true>), dim3(n), dim3(64), 0, h->stream, h->d, 2, d_out, 0u, (const uint32_t*)h->d_obs_offs, d_index, capacity, (const uint32_t*)totals, d_count)
    if (h->cfg.game_mode >= 3) RMJ_LAUNCH_COMPACT(true);
    else RMJ_LAUNCH_COMPACT(false);
#undef RMJ_LAUNCH_COMPACT
}
int rmj_encode_compact_device(rmj_handle h, float* d_out, int32_t* d_index, uint32_t capacity, uint32_t* d_count) {
    if (!h || !d_out || !d_index || !d_count) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    launch_encode_compact(h, d_out, d_index, capacity, d_count);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_step_random_encode_compact(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, float* d_out, int32_t* d_index,
                                   uint32_t capacity, uint32_t* d_count) {
    if (!h || !d_out || !d_index || !d_count) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t flags = STEP_F_RANDOM | (auto_reset ? STEP_F_AUTORESET : 0u);
    for (uint32_t s = 0; s < n_steps; s++) {
        launch_step_range(h, h->stream, nullptr, policy_seed, flags, 0u, h->cfg.n_games);
        launch_encode_compact(h, d_out, d_index, capacity, d_count);
    }
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_bench_encode_compact(rmj_handle h, float* d_out, int32_t* d_index, uint32_t capacity, uint32_t* d_count, uint32_t reps, double* avg_ms) {
    if (!h || !d_out || !d_index || !d_count || !avg_ms || reps == 0) return fail(RMJ_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    return time_launches(h->stream, reps, false, avg_ms, [&] { launch_encode_compact(h, d_out, d_index, capacity, d_count); return RMJ_OK; });
}
int rmj_encode(rmj_handle h, int only_active, float* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    const size_t bytes = (size_t)h->cfg.n_games * 4 * (size_t)h->d.enc_stride * sizeof(float);
    return fill_and_fetch(h, out, bytes, [&](void* d) { return rmj_encode_device(h, only_active, (float*)d); });
}

static size_t aux_floats(const rmj_env* h, int which) {
    const size_t np = h->cfg.game_mode >= 3 ? 3 : 4, w = h->cfg.game_mode >= 3 ? ENC_W3 : ENC_W4;
    return which == 0 ? np * 7 * w : (which == 1 ? np * 21 * 2 : np * 21);
}
int rmj_encode_aux_device(rmj_handle h, int which, float* d_out) {
    if (!h || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    if (which < 0 || which > 2) return fail(RMJ_ERR_ARG, "unknown auxiliary encoder");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->cfg.game_mode >= 3) hipLaunchKernelGGL((k_encode_aux<true>), dim3(h->cfg.n_games), dim3(64), 0, h->stream, h->d, which, d_out);
    else hipLaunchKernelGGL((k_encode_aux<false>), dim3(h->cfg.n_games), dim3(64), 0, h->stream, h->d, which, d_out);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_encode_aux(rmj_handle h, int which, float* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (which < 0 || which > 2) return fail(RMJ_ERR_ARG, "unknown auxiliary encoder");
    const size_t bytes = (size_t)h->cfg.n_games * aux_floats(h, which) * sizeof(float);
    return fill_and_fetch(h, out, bytes, [&](void* d) { return rmj_encode_aux_device(h, which, (float*)d); });
}

// sequence features (row N3, 4P only like the reference): see rmj_seq.hip.h
int rmj_encode_seq_device(rmj_handle h, int game_style, const RmjSeqBuffers* d) {
    if (!h || !d || !d->sparse || !d->n_sparse || !d->numeric || !d->progression || !d->n_progression || !d->candidates || !d->n_candidates)
        return fail(RMJ_ERR_ARG, "null argument");
    if (h->cfg.game_mode >= 3) return fail(RMJ_ERR_ARG, "sequence features exist for 4-player games only (observation/sequence_features.rs)");
    if (h->cfg.skip_mjai_logging) return fail(RMJ_ERR_ARG, "sequence features read the event log: create the handle with logging on");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_encode_seq, dim3(h->cfg.n_games), dim3(64), 0, h->stream, h->d, game_style, *d);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_encode_seq(rmj_handle h, int game_style, const RmjSeqBuffers* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    const size_t n = h->cfg.n_games;
    const size_t sz[7] = {n * 4 * RMJ_SEQ_SPARSE * 2, n * 4, n * 4 * 12 * 4, n * RMJ_SEQ_PROG * 5 * 2, n * 2, n * 4 * RMJ_SEQ_CAND * 4 * 2, n * 4};
    return encode_seq_host(h, game_style, out, sz, rmj_encode_seq_device);
}

int rmj_encode_seq_delta_device(rmj_handle h, int game_style, const RmjSeqDeltaBuffers* d) {
    if (!h || !d || !d->sparse || !d->n_sparse || !d->numeric || !d->progression || !d->n_progression || !d->candidates || !d->n_candidates)
        return fail(RMJ_ERR_ARG, "null argument");
    if (h->cfg.game_mode >= 3) return fail(RMJ_ERR_ARG, "sequence features exist for 4-player games only (observation/sequence_features.rs)");
    if (h->cfg.skip_mjai_logging) return fail(RMJ_ERR_ARG, "sequence features read the event log: create the handle with logging on");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_encode_seq_delta, dim3(h->cfg.n_games), dim3(64), 0, h->stream, h->d, game_style, *d);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_encode_seq_delta(rmj_handle h, int game_style, const RmjSeqDeltaBuffers* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    const size_t n = h->cfg.n_games;
    const size_t sz[7] = {n * 4 * RMJ_SEQ_SPARSE * 2, n * 4, n * 4 * 12 * 4, n * 4 * RMJ_SEQ_DELTA_PROG * 5 * 2, n * 4 * 2,
                          n * 4 * RMJ_SEQ_CAND * 4 * 2, n * 4};
    return encode_seq_host(h, game_style, out, sz, rmj_encode_seq_delta_device);
}

int rmj_encode_extended_device(rmj_handle h, int only_active, float* d_out) { return launch_encode(h, only_active, d_out, true); }
int rmj_encode_extended(rmj_handle h, int only_active, float* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    const size_t bytes = (size_t)h->cfg.n_games * 4 * ENC_EXT_CH * (h->cfg.game_mode >= 3 ? ENC_W3 : ENC_W4) * sizeof(float);
    return fill_and_fetch(h, out, bytes, [&](void* d) { return rmj_encode_extended_device(h, only_active, (float*)d); });
}

// ---- observation batches (k_encode_batch) ------------------------------------------------------------------
// channels x width of a feature set on this handle and the row stride in floats; an error message for what is refused
static int batch_shape(const rmj_env* h, const RmjObsBatch* b, uint32_t* ch, uint32_t* w, uint32_t* rs) {
    if (!b) return fail(RMJ_ERR_ARG, "null argument");
    const bool sanma = h->cfg.game_mode >= 3;
    *w = sanma ? ENC_W3 : ENC_W4;
    switch (b->features) {
        case RMJ_FEATURES_BASE: *ch = ENC_CH; break;
        case RMJ_FEATURES_EXTENDED: *ch = ENC_EXT_CH; break;
        case RMJ_FEATURES_DISCARD_SHANTEN:
            if (sanma) return fail(RMJ_ERR_ARG, "RMJ_FEATURES_DISCARD_SHANTEN is 4-player only (feat_v2 cannot reshape the 3P observation's 3 decay rows and (3, 4) efficiency block)");
            *ch = RMJ_FEATURES_DISCARD_SHANTEN_CHANNELS;
            break;
        default: return fail(RMJ_ERR_ARG, "unknown feature set (RMJ_FEATURES_BASE, _DISCARD_SHANTEN or _EXTENDED)");
    }
    if (b->compact != 0 && b->compact != 1) return fail(RMJ_ERR_ARG, "compact must be 0 (dense) or 1");
    const uint32_t dense = *ch * *w;
    *rs = b->row_stride ? b->row_stride : dense;
    if (b->row_stride && (b->row_stride < dense || (b->row_stride & 1u)))
        return fail(RMJ_ERR_ARG, "row stride must be 0 or an even number of floats >= C x W (" + std::to_string(dense) + ")");
    if (!b->d_out || (b->compact && (!b->d_index || !b->d_count))) return fail(RMJ_ERR_ARG, "null argument");
    return RMJ_OK;
}
// (arguments checked by batch_shape)
static void launch_encode_batch(rmj_env* h, const RmjObsBatch* b, uint32_t rs) {
    const uint32_t n = h->cfg.n_games;
    const dim3 grid(n * 4), block(64);
    const bool sanma = h->cfg.game_mode >= 3;
    const float* decay = h->d_decay;
    uint32_t* totals = h->d_obs_offs + n;
    if (b->compact)
        hipLaunchKernelGGL(k_obs_offsets, dim3((n + OBS_SCAN_BLOCK - 1) / OBS_SCAN_BLOCK), dim3(OBS_SCAN_BLOCK), 0, h->stream, (const uint32_t*)h->d.status, n,
                           h->d_obs_offs, totals);
#define RMJ_LAUNCH_BATCH(SM, F)                                                                                                          \
    do {                                                                                                                                  \
        if (b->compact)                                                                                                                   \
            hipLaunchKernelGGL((k_encode_batch<SM, F, true>), grid, block, 0, h->stream, h->d, decay, b->d_out, rs, (const uint32_t*)h->d_obs_offs, \
                               (const uint32_t*)totals, b->d_index, b->capacity, b->d_count);                                            \
        else                                                                                                                              \
            hipLaunchKernelGGL((k_encode_batch<SM, F, false>), grid, block, 0, h->stream, h->d, decay, b->d_out, rs, (const uint32_t*)nullptr, \
                               (const uint32_t*)nullptr, (int32_t*)nullptr, 0u, (uint32_t*)nullptr);                                     \
    } while (0)
    if (sanma && b->features == RMJ_FEATURES_EXTENDED) RMJ_LAUNCH_BATCH(true, RMJ_FEATURES_EXTENDED);
    else if (sanma) RMJ_LAUNCH_BATCH(true, RMJ_FEATURES_BASE);
    else if (b->features == RMJ_FEATURES_EXTENDED) RMJ_LAUNCH_BATCH(false, RMJ_FEATURES_EXTENDED);
    else if (b->features == RMJ_FEATURES_DISCARD_SHANTEN) RMJ_LAUNCH_BATCH(false, RMJ_FEATURES_DISCARD_SHANTEN);
    else RMJ_LAUNCH_BATCH(false, RMJ_FEATURES_BASE);
#undef RMJ_LAUNCH_BATCH
}
int rmj_encode_batch_device(rmj_handle h, const RmjObsBatch* b) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    uint32_t ch, w, rs;
    int rc = batch_shape(h, b, &ch, &w, &rs);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    launch_encode_batch(h, b, rs);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_encode_batch(rmj_handle h, const RmjObsBatch* b) {
    if (!h) return fail(RMJ_ERR_ARG, "null handle");
    uint32_t ch, w, rs;
    int rc = batch_shape(h, b, &ch, &w, &rs);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t rows = b->compact ? (size_t)b->capacity : (size_t)h->cfg.n_games * 4;
    const size_t out_bytes = rows * rs * sizeof(float);
    RmjObsBatch d = *b;
    rmjh::DevLayout L;
    L.add(&d.d_out, out_bytes); L.add(&d.d_index, b->compact ? (size_t)b->capacity * sizeof(int32_t) : 0); L.add(&d.d_count, sizeof(uint32_t), 1);
    if ((rc = scratch_for(h, L))) return rc;
    if (!b->compact) { d.d_index = nullptr; d.d_count = nullptr; }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!b->compact && out_bytes) HIPCHK(hipMemcpy(d.d_out, b->d_out, out_bytes, hipMemcpyHostToDevice));   // the rows that stay untouched
    launch_encode_batch(h, &d, rs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (b->compact) {
        uint32_t k = 0;
        HIPCHK(hipMemcpy(&k, d.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
        const size_t m = k < b->capacity ? k : b->capacity;
        if (m) {
            HIPCHK(hipMemcpy(b->d_out, d.d_out, m * rs * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->d_index, d.d_index, m * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        *b->d_count = k;
    } else if (out_bytes) {
        HIPCHK(hipMemcpy(b->d_out, d.d_out, out_bytes, hipMemcpyDeviceToHost));
    }
    return RMJ_OK;
}
int rmj_step_ids_encode_batch_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset, const RmjObsBatch* b) {
    if (!h || !d_action_ids) return fail(RMJ_ERR_ARG, "null argument");
    uint32_t ch, w, rs;
    int rc = batch_shape(h, b, &ch, &w, &rs);   // refused before anything is stepped
    if (rc) return rc;
    if ((rc = rmj_step_ids_device(h, d_action_ids, auto_reset))) return rc;
    launch_encode_batch(h, b, rs);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_step_sample_encode_batch_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int auto_reset,
                                        int32_t* d_ids, const RmjObsBatch* b) {
    if (!h || !d_ids) return fail(RMJ_ERR_ARG, "null argument");
    uint32_t ch, w, rs;
    int rc = batch_shape(h, b, &ch, &w, &rs);
    if (rc) return rc;
    if ((rc = rmj_sample_ids_device(h, d_logits, stride, seed, d_ids))) return rc;
    if ((rc = rmj_step_ids_device(h, d_ids, auto_reset))) return rc;
    launch_encode_batch(h, b, rs);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}

// ---- hidden-hand targets (rmj_hidden.hip.h) ----------------------------------------------------------------------
int rmj_hidden_targets_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjHiddenOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (!rows) return RMJ_OK;
    if (!d_index || !out->d_opp_hand || !out->d_opp_shanten || !out->d_opp_waits || !out->d_opp_flags) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_hidden_targets, dim3((rows + 3u) / 4u), dim3(256), 0, h->stream, h->d, d_index, rows, d_count, *out);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_hidden_targets(rmj_handle h, const int32_t* index, uint32_t rows, const RmjHiddenOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (!rows) return RMJ_OK;
    if (!index || !out->d_opp_hand || !out->d_opp_shanten || !out->d_opp_waits || !out->d_opp_flags) return fail(RMJ_ERR_ARG, "null argument");
    RmjHiddenOut d{};
    return row_call_host(h, index, rows,
                         {{&d.d_opp_waits, out->d_opp_waits, 24}, {&d.d_opp_hand, out->d_opp_hand, 102}, {&d.d_opp_flags, out->d_opp_flags, 3}, {&d.d_opp_shanten, out->d_opp_shanten, 3}},
                         [&](const int32_t* d_index) { return rmj_hidden_targets_device(h, d_index, rows, nullptr, &d); });
}
// ---- deal-in danger targets (rmj_danger.hip.h) -------------------------------------------------------------------
int rmj_danger_targets_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, uint32_t flags, const RmjDangerOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (flags & ~(uint32_t)RMJ_DANGER_URA) return fail(RMJ_ERR_ARG, "rmj_danger_targets_device: unknown flag");
    if (!rows) return RMJ_OK;
    if (!d_index || !out->d_danger) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_danger_targets, dim3((rows + 3u) / 4u), dim3(256), 0, h->stream, h->d, d_index, rows, d_count, flags, out->d_danger);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_danger_targets(rmj_handle h, const int32_t* index, uint32_t rows, uint32_t flags, const RmjDangerOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (flags & ~(uint32_t)RMJ_DANGER_URA) return fail(RMJ_ERR_ARG, "rmj_danger_targets: unknown flag");
    if (!rows) return RMJ_OK;
    if (!index || !out->d_danger) return fail(RMJ_ERR_ARG, "null argument");
    RmjDangerOut d{};
    return row_call_host(h, index, rows, {{&d.d_danger, out->d_danger, 3 * RMJ_DANGER_KINDS * 4}},
                         [&](const int32_t* d_index) { return rmj_danger_targets_device(h, d_index, rows, nullptr, flags, &d); });
}
// ---- discard efficiency table (rmj_dtable.hip.h) -----------------------------------------------------------------
int rmj_discard_table_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, uint32_t flags, const RmjDiscardTableOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (flags) return fail(RMJ_ERR_ARG, "rmj_discard_table_device: unknown flag");
    if (!rows) return RMJ_OK;
    if (!d_index || !out->d_shanten || !out->d_accept || !out->d_ukeire) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    dt_launch_rows(h->stream, h->d, d_index, rows, d_count, *out);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_discard_table(rmj_handle h, const int32_t* index, uint32_t rows, uint32_t flags, const RmjDiscardTableOut* out) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (flags) return fail(RMJ_ERR_ARG, "rmj_discard_table: unknown flag");
    if (!rows) return RMJ_OK;
    if (!index || !out->d_shanten || !out->d_accept || !out->d_ukeire) return fail(RMJ_ERR_ARG, "null argument");
    RmjDiscardTableOut d{};
    return row_call_host(h, index, rows,
                         {{&d.d_shanten, out->d_shanten, RMJ_DTAB_COLS}, {&d.d_accept, out->d_accept, RMJ_DTAB_COLS}, {&d.d_ukeire, out->d_ukeire, RMJ_DTAB_COLS},
                          {&d.d_mask, out->d_mask, RMJ_DTAB_COLS * 8}},
                         [&](const int32_t* d_index) { return rmj_discard_table_device(h, d_index, rows, nullptr, flags, &d); });
}
// ---- determinize (rmj_determinize.hip.h) ------------------------------------------------------------------------
int rmj_determinize_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDeterminize* p) {
    return rmj_determinize_ex_device(h, d_index, rows, d_count, p, 0u);
}
int rmj_determinize_ex_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDeterminize* p, uint32_t flags) {
    if (flags & ~RMJ_DETF_RIICHI_TENPAI) return fail(RMJ_ERR_ARG, "rmj_determinize: unknown flag");
    if (!h || !p) return fail(RMJ_ERR_ARG, "null argument");
    if (!rows) return RMJ_OK;
    if (!d_index) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t claim_bytes = (size_t)h->cfg.n_games * 8;
    if (!h->det_claim.p || h->det_epoch == 0xFFFFFFFFu) {   // first call (or the epochs are used up): words of epoch 0
        HIPCHK(h->det_claim.need(claim_bytes, h->stream));
        HIPCHK(hipMemsetAsync(h->det_claim.p, 0, claim_bytes, h->stream));
        h->det_epoch = 0;
    }
    DetArgs A{d_index, d_count, p->d_hold, p->d_status, (unsigned long long*)h->det_claim.p, p->seed, rows, ++h->det_epoch};
    hipLaunchKernelGGL(k_determinize_claim, dim3((rows + 255u) / 256u), dim3(256), 0, h->stream, h->d, A);
    const dim3 grid((rows + WPB - 1u) / WPB), block(64 * WPB);
    if (flags & RMJ_DETF_RIICHI_TENPAI) {
        if (h->cfg.game_mode >= 3) hipLaunchKernelGGL((k_determinize<DetV3, true>), grid, block, 0, h->stream, (const Env*)h->d_env, A);
        else hipLaunchKernelGGL((k_determinize<DetV4, true>), grid, block, 0, h->stream, (const Env*)h->d_env, A);
    } else if (h->cfg.game_mode >= 3) hipLaunchKernelGGL(k_determinize<DetV3>, grid, block, 0, h->stream, (const Env*)h->d_env, A);
    else hipLaunchKernelGGL(k_determinize<DetV4>, grid, block, 0, h->stream, (const Env*)h->d_env, A);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_determinize(rmj_handle h, const int32_t* index, uint32_t rows, const RmjDeterminize* p) { return rmj_determinize_ex(h, index, rows, p, 0u); }
int rmj_determinize_ex(rmj_handle h, const int32_t* index, uint32_t rows, const RmjDeterminize* p, uint32_t flags) {
    if (flags & ~RMJ_DETF_RIICHI_TENPAI) return fail(RMJ_ERR_ARG, "rmj_determinize: unknown flag");
    if (!h || !p) return fail(RMJ_ERR_ARG, "null argument");
    if (!rows) return RMJ_OK;
    if (!index) return fail(RMJ_ERR_ARG, "null argument");
    {   // two rows for one game: refused here (the device form carries out the lower row)
        std::vector<uint32_t> games;
        for (uint32_t i = 0; i < rows; i++)
            if ((uint32_t)index[i] < h->cfg.n_games * 4u) games.push_back((uint32_t)index[i] >> 2);
        std::sort(games.begin(), games.end());
        if (std::adjacent_find(games.begin(), games.end()) != games.end()) return fail(RMJ_ERR_ARG, "rmj_determinize: two rows name the same game");
    }
    RmjDeterminize d{p->seed, nullptr, nullptr};
    return row_call_host(h, index, rows, {{&d.d_hold, (void*)p->d_hold, 1, RowArray::UP}, {&d.d_status, p->d_status, 1}},
                         [&](const int32_t* d_index) { return rmj_determinize_ex_device(h, d_index, rows, nullptr, &d, flags); });
}
int rmj_determinize_order(uint64_t seed, uint64_t global_game, uint32_t seat, uint32_t m, uint32_t* perm) {
    if (m > 256u || (m && !perm)) return fail(RMJ_ERR_ARG, "rmj_determinize_order: m <= 256 and a perm array");
    const uint64_t base = det_base(seed, global_game);
    std::vector<uint64_t> keys(m);
    for (uint32_t i = 0; i < m; i++) keys[i] = det_key(base, seat, i);
    for (uint32_t i = 0; i < m; i++) perm[det_rank(keys.data(), m, keys[i], i)] = i;
    return RMJ_OK;
}
int rmj_determinize_swap_key(uint64_t seed, uint64_t global_game, uint32_t seat, uint32_t r, uint32_t k, uint32_t i, uint32_t j, uint64_t* key) {
    if (!key || seat >= 4u || r >= 3u || k >= 16u || i >= 16u || j >= 256u) return fail(RMJ_ERR_ARG, "rmj_determinize_swap_key: seat < 4, r < 3, k < 16, i < 16, j < 256 and a key");
    *key = det_swap_key(det_base(seed, global_game), seat, r, k, i, j);
    return RMJ_OK;
}
// ---- PPO transition collector (rmj_ppo.hip.h) ------------------------------------------------------------------
static int ppo_clear_impl(rmj_ppo* p) {
    rmj_env* h = p->env;
    const uint32_t n = h->cfg.n_games;
    HIPCHK(hipMemsetAsync(p->P.ctr, 0, PPO_C_WORDS * 4, h->stream));
    HIPCHK(hipMemsetAsync(p->P.tail, 0xFF, (size_t)n * 4, h->stream));
    HIPCHK(hipMemsetAsync(p->P.open_len, 0, (size_t)n * 4, h->stream));
    HIPCHK(hipMemsetAsync(p->P.g_serial, 0, (size_t)n * 4, h->stream));
    HIPCHK(hipMemsetAsync(p->P.broken, 0, (size_t)n, h->stream));
    return RMJ_OK;
}
int rmj_ppo_create(rmj_handle h, const RmjPpoConfig* cfg, rmj_ppo_handle* out) {
    if (!h || !cfg || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = nullptr;
    if (!cfg->capacity) return fail(RMJ_ERR_ARG, "rmj_ppo_create: the pool needs a capacity (transitions)");
    uint32_t ch, w, rs;
    float dummy;
    RmjObsBatch b{};
    b.features = cfg->features;
    b.d_out = &dummy;   // (shape check only)
    int rc = batch_shape(h, &b, &ch, &w, &rs);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    rmj_ppo* p = new rmj_ppo();
    p->env = h;
    p->cfg = *cfg;
    p->gamma_lambda = cfg->gamma * cfg->gae_lambda;
    const uint32_t n = h->cfg.n_games, cap = cfg->capacity, A = h->cfg.game_mode >= 3 ? RMJ_ACTION_SPACE_3P : RMJ_ACTION_SPACE_4P;
    PpoPool& P = p->P;
    P.capacity = cap; P.feat_floats = ch * w; P.row_floats = (ch * w + 3u) & ~3u; P.A = A;
    const size_t big = n > cap ? n : cap;
    // one allocation: the feature rows first (16-byte rows), then the 4-byte arrays, then the bytes
    const size_t c4 = (size_t)cap * 4, n4 = (size_t)n * 4;
    rmjh::DevLayout L;
    L.add(&P.feat, (size_t)cap * P.row_floats * 4);
    const size_t o_action = L.add(&P.action, c4);
    L.add(&P.value, c4); L.add(&P.logp, c4); L.add(&P.adv, c4); L.add(&P.ret, c4); L.add(&P.game, c4); L.add(&P.serial, c4); L.add(&P.t, c4); L.add(&P.prev, c4);
    L.add(&P.seg_len, c4); L.add(&P.seg_reward, c4); L.add(&P.tail, n4); L.add(&P.open_len, n4); L.add(&P.g_serial, n4); L.add(&P.rowof, n4);
    L.add(&P.offs, big * 4); L.add(&P.totals, ((big + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK) * 4); L.add(&P.ctr, PPO_C_WORDS * 4);
    L.add(&P.mask, (size_t)cap * A); L.add(&P.valid, cap); L.add(&P.broken, n);
    const size_t off = L.bytes();
    if (hipMalloc(&p->mem, off) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return fail(RMJ_ERR_HIP, "rmj_ppo_create: no device memory for a pool of " + std::to_string(off >> 20) + " MiB (capacity x row bytes: choose a smaller capacity)");
    }
    uint8_t* m = (uint8_t*)p->mem;
    L.bind(m);
    h->ppo.push_back(p);
    // everything behind the feature rows starts as zeros (the views show defined values in slots that were never filled)
    if (hipMemsetAsync(m + o_action, 0, off - o_action, h->stream) != hipSuccess || (rc = ppo_clear_impl(p))) {
        rmj_ppo_destroy(p);
        return rc ? rc : fail(RMJ_ERR_HIP, "rmj_ppo_create: hipMemsetAsync failed");
    }
    *out = p;
    return RMJ_OK;
}
int rmj_ppo_destroy(rmj_ppo_handle p) {
    if (!p) return RMJ_OK;
    rmj_env* h = p->env;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (size_t i = 0; i < h->ppo.size(); i++)
        if (h->ppo[i] == p) { h->ppo.erase(h->ppo.begin() + i); break; }
    hipFree(p->mem);
    delete p;
    return RMJ_OK;
}
int rmj_ppo_clear(rmj_ppo_handle p) {
    if (!p) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(p->env->cfg.device));
    return ppo_clear_impl(p);
}
// waves of a grid-stride launch with one wave per item: enough to fill the chip a few times over, never more than the items
static inline dim3 ppo_wave_grid(uint32_t items) { const uint32_t b = (items + 3u) / 4u; return dim3(b < 1u ? 1u : (b > 4096u ? 4096u : b)); }
int rmj_ppo_record_device(rmj_ppo_handle p, const RmjObsBatch* b, const uint8_t* d_hero, const int32_t* d_ids, const float* d_logits, uint32_t logits_stride,
                          const float* d_values) {
    if (!p || !b || !d_hero || !d_ids || !d_logits || !d_values) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = p->env;
    uint32_t ch, w, rs;
    int rc = batch_shape(h, b, &ch, &w, &rs);
    if (rc) return rc;
    if (b->features != p->cfg.features) return fail(RMJ_ERR_ARG, "rmj_ppo_record_device: the observation batch is not of the collector's feature set");
    if (logits_stride < p->P.A) return fail(RMJ_ERR_ARG, "logits row shorter than the action space");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games, nb = (n + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK;
    hipLaunchKernelGGL(k_ppo_scan, dim3(nb), dim3(PPO_SCAN_BLOCK), 0, h->stream, p->P, n, d_hero, d_ids, b->compact ? (const int32_t*)b->d_index : (const int32_t*)nullptr,
                       b->capacity, (const uint32_t*)b->d_count);
    hipLaunchKernelGGL(k_ppo_record, ppo_wave_grid(n), dim3(256), 0, h->stream, p->P, n, (const uint8_t*)h->d.mask, d_hero, d_ids, (const float*)b->d_out, rs, d_logits,
                       logits_stride, d_values);
    hipLaunchKernelGGL(k_ppo_advance, dim3(1), dim3(64), 0, h->stream, p->P, nb);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_ppo_close_device(rmj_ppo_handle p, const uint8_t* d_ended, const float* d_reward) {
    if (!p || !d_ended || !d_reward) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = p->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_ppo_close, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, p->P, n, d_ended, d_reward, p->cfg.gamma, p->gamma_lambda);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_ppo_emit_device(rmj_ppo_handle p, const RmjPpoBatch* out) {
    if (!p || !out || !out->d_count) return fail(RMJ_ERR_ARG, "null argument");
    if (out->rows && (!out->d_features || !out->d_mask || !out->d_action || !out->d_log_prob || !out->d_advantage || !out->d_return))
        return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = p->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t cap = p->P.capacity;
    PpoOut O{out->d_features, out->d_mask, out->d_action, out->d_log_prob, out->d_advantage, out->d_return, out->d_count, out->rows};
    hipLaunchKernelGGL(k_ppo_emit_scan, dim3((cap + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK), dim3(PPO_SCAN_BLOCK), 0, h->stream, p->P);
    hipLaunchKernelGGL(k_ppo_emit, ppo_wave_grid(cap), dim3(256), 0, h->stream, p->P, O);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_ppo_views(rmj_ppo_handle p, RmjPpoViews* out) {
    if (!p || !out) return fail(RMJ_ERR_ARG, "null argument");
    const PpoPool& P = p->P;
    *out = RmjPpoViews{P.capacity, P.row_floats, P.A, 0u, P.feat, P.mask, P.action, P.value, P.logp, P.adv, P.ret, P.valid, P.game, P.t, P.prev, P.seg_len, P.serial,
                       P.seg_reward, P.ctr, P.open_len};
    return RMJ_OK;
}
int rmj_ppo_counts(rmj_ppo_handle p, RmjPpoCounts* out) {
    if (!p || !out) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = p->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    uint32_t c[PPO_C_WORDS];
    HIPCHK(hipMemcpyAsync(c, p->P.ctr, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = RmjPpoCounts{c[PPO_C_FILL], c[PPO_C_VALID], c[PPO_C_DROPPED], c[PPO_C_OVERFLOWED], c[PPO_C_SEGMENTS], c[PPO_C_FILL] - c[PPO_C_VALID] - c[PPO_C_DROPPED]};
    return RMJ_OK;
}

// ---- log sample builder (rmj_logreplay.hip.h) ------------------------------------------------------------------
int rmj_logset_create(int device, const RmjEvent* events, const uint32_t* offsets, uint32_t n_logs, rmj_logset_handle* out) {
    if (!out || !offsets || (!events && offsets[n_logs])) return fail(RMJ_ERR_ARG, "null argument");
    *out = nullptr;
    if (offsets[0] != 0u) return fail(RMJ_ERR_ARG, "rmj_logset_create: offsets[0] must be 0");
    for (uint32_t l = 0; l < n_logs; l++)
        if (offsets[l + 1] < offsets[l]) return fail(RMJ_ERR_ARG, "rmj_logset_create: offsets must not decrease");
    int rc = ensure_device(device);
    if (rc) return rc;
    rmj_logset* s = new rmj_logset();
    s->device = device;
    s->M = n_logs;
    s->total = offsets[n_logs];
    s->off.assign(offsets, offsets + n_logs + 1);
    s->koff.assign(n_logs + 1, 0u);
    for (uint32_t l = 0; l < n_logs; l++) {
        uint32_t k = 0;
        for (uint32_t i = offsets[l]; i < offsets[l + 1]; i++) k += events[(size_t)i * 3].type == RMJ_EV_START_KYOKU ? 1u : 0u;
        s->koff[l + 1] = s->koff[l] + k;
        if (offsets[l + 1] - offsets[l] > s->max_len) s->max_len = offsets[l + 1] - offsets[l];
    }
    s->K = s->koff[n_logs];
    const size_t eb = (size_t)(s->total ? s->total : 1u) * 3 * sizeof(RmjEvent), ob = (size_t)(n_logs + 1) * 4;
    if (hipMalloc(&s->d_ev, eb) != hipSuccess || hipMalloc(&s->d_off, ob) != hipSuccess || hipMalloc(&s->d_koff, ob) != hipSuccess ||
        (s->total && hipMemcpy(s->d_ev, events, (size_t)s->total * 3 * sizeof(RmjEvent), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(s->d_off, s->off.data(), ob, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(s->d_koff, s->koff.data(), ob, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        rmj_logset_destroy(s);
        return fail(RMJ_ERR_HIP, "rmj_logset_create: no device memory for the event stream, or the upload failed");
    }
    *out = s;
    return RMJ_OK;
}
int rmj_logset_destroy(rmj_logset_handle s) {
    if (!s) return RMJ_OK;
    hipSetDevice(s->device);
    hipFree(s->d_ev); hipFree(s->d_off); hipFree(s->d_koff);
    hipFree(s->d_start); hipFree(s->d_end); hipFree(s->d_own); hipFree(s->d_status); hipFree(s->d_errline); hipFree(s->d_dec);
    delete s;
    return RMJ_OK;
}
int rmj_logset_info(rmj_logset_handle s, RmjLogsetInfo* out, uint32_t* kyoku_offsets) {
    if (!s || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = RmjLogsetInfo{s->M, s->total, s->K, s->max_len};
    if (kyoku_offsets) memcpy(kyoku_offsets, s->koff.data(), (size_t)(s->M + 1) * 4);
    return RMJ_OK;
}
// body of rmj_logset_create_from_text: the buffers in `tmp` are freed by the caller, whatever happens; the set's own by rmj_logset_destroy
static int logset_from_text_impl(rmj_logset* s, const uint8_t* text, const uint64_t* ranges, uint32_t num_players, uint32_t flags, DevTmp& tmp) {
    using namespace rmjlt;
    const uint32_t M = s->M;
    const bool on_device = (flags & RMJ_LOGTEXT_ON_DEVICE) != 0u;
    auto dalloc = [&](void* pp, size_t bytes, bool keep) -> int {   // pp: the address of a device pointer of any type; keep: the buffer belongs to the set
        uint8_t* q;
        const hipError_t e = tmp.alloc(&q, bytes ? bytes : 16u);
        *(void**)pp = q;
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(RMJ_ERR_HIP, "rmj_logset_create_from_text: no device memory"); }
        if (keep) tmp.release(q);
        return RMJ_OK;
    };
    int rc;
    // the ranges on the host: O(n_logs) words, checked before a kernel trusts them
    std::vector<uint64_t> hr((size_t)2 * M);
    if (M) {
        if (on_device) HIPCHK(hipMemcpy(hr.data(), ranges, hr.size() * 8, hipMemcpyDeviceToHost));
        else memcpy(hr.data(), ranges, hr.size() * 8);
    }
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t l = 0; l < M; l++) {
        const uint64_t b = hr[2 * (size_t)l], e = hr[2 * (size_t)l + 1];
        if (e < b) return fail(RMJ_ERR_ARG, "rmj_logset_create_from_text: a range ends before it begins");
        if (e - b > 0xFFFFFFFFull) return fail(RMJ_ERR_RANGE, "rmj_logset_create_from_text: a log of 4 GiB or more");
        if (e > b) { lo = b < lo ? b : lo; hi = e > hi ? e : hi; }
    }
    if (lo > hi) lo = hi = 0;
    if (hi > lo && !text) return fail(RMJ_ERR_ARG, "null argument");
    const uint8_t* d_text = text;
    const uint64_t* d_ranges = ranges;
    if (!on_device) {   // one upload of the bytes the ranges span, the ranges rebased on it
        uint8_t* t = nullptr;
        uint64_t* r = nullptr;
        if ((rc = dalloc(&t, (size_t)(hi - lo), false))) return rc;
        if ((rc = dalloc(&r, hr.size() * 8, false))) return rc;
        if (hi > lo) HIPCHK(hipMemcpy(t, text + lo, (size_t)(hi - lo), hipMemcpyHostToDevice));
        for (uint32_t l = 0; l < M; l++) {
            if (hr[2 * (size_t)l + 1] == hr[2 * (size_t)l]) hr[2 * (size_t)l] = hr[2 * (size_t)l + 1] = lo;   // an empty range may lie anywhere
            hr[2 * (size_t)l] -= lo;
            hr[2 * (size_t)l + 1] -= lo;
        }
        if (M) HIPCHK(hipMemcpy(r, hr.data(), hr.size() * 8, hipMemcpyHostToDevice));
        d_text = t;
        d_ranges = r;
    }
    uint32_t *d_cnt = nullptr, *d_choff = nullptr, *d_max = nullptr, *d_kcnt = nullptr;
    unsigned long long *d_tot = nullptr, *d_ferr = nullptr;
    const size_t ob = (size_t)(M + 1) * 4;
    if ((rc = dalloc(&d_cnt, (size_t)M * 4, false))) return rc;
    if ((rc = dalloc(&d_choff, ob, false))) return rc;
    if ((rc = dalloc(&d_max, 4, false))) return rc;
    if ((rc = dalloc(&d_kcnt, (size_t)M * 4, false))) return rc;
    if ((rc = dalloc(&d_tot, 3 * 8, false))) return rc;
    if ((rc = dalloc(&d_ferr, (size_t)M * 8, false))) return rc;
    if ((rc = dalloc(&s->d_off, ob, true))) return rc;
    if ((rc = dalloc(&s->d_koff, ob, true))) return rc;
    if ((rc = dalloc(&s->d_status, M, true))) return rc;
    if ((rc = dalloc(&s->d_errline, (size_t)M * 4, true))) return rc;
    if ((rc = dalloc(&s->d_dec, (size_t)M * 4, true))) return rc;
    HIPCHK(hipMemset(d_max, 0, 4));
    HIPCHK(hipMemset(d_kcnt, 0, (size_t)M * 4 + (M ? 0 : 16)));
    HIPCHK(hipMemset(s->d_dec, 0, (size_t)M * 4 + (M ? 0 : 16)));
    HIPCHK(hipMemset(d_ferr, 0xFF, (size_t)M * 8 + (M ? 0 : 16)));
    const dim3 per_log((M + 3u) / 4u ? (M + 3u) / 4u : 1u), b256(256);
    // line census, event offsets, chunk offsets of the parse grid
    if (M) hipLaunchKernelGGL(k_lt_lines<false>, per_log, b256, 0, 0, d_text, d_ranges, M, d_cnt, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_lt_scan, dim3(1), dim3(1024), 0, 0, d_cnt, M, 1u, s->d_off, d_tot, d_max);
    hipLaunchKernelGGL(k_lt_scan, dim3(1), dim3(1024), 0, 0, d_cnt, M, 64u, d_choff, d_tot + 1, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long tot[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(tot, d_tot, 16, hipMemcpyDeviceToHost));
    if (tot[0] > 0xFFFFFFFFull) return fail(RMJ_ERR_RANGE, "rmj_logset_create_from_text: the logs hold more than UINT32_MAX events");
    const uint32_t total = (uint32_t)tot[0], chunks = (uint32_t)tot[1];
    s->total = total;
    uint32_t *d_es = nullptr, *d_ee = nullptr, *d_el = nullptr;
    rmjp::Side* d_side = nullptr;
    if ((rc = dalloc(&d_es, (size_t)total * 4, false))) return rc;
    if ((rc = dalloc(&d_ee, (size_t)total * 4, false))) return rc;
    if ((rc = dalloc(&d_el, (size_t)total * 4, false))) return rc;
    if ((rc = dalloc(&d_side, (size_t)total * sizeof(rmjp::Side), false))) return rc;
    if ((rc = dalloc(&s->d_ev, (size_t)total * 3 * sizeof(RmjEvent), true))) return rc;
    if (total) {
        // line index, then the records
        hipLaunchKernelGGL(k_lt_lines<true>, per_log, b256, 0, 0, d_text, d_ranges, M, (uint32_t*)nullptr, (const uint32_t*)s->d_off, d_es, d_ee, d_el);
        hipLaunchKernelGGL(k_lt_parse, dim3(chunks), dim3(64), 0, 0, d_text, d_ranges, M, (const uint32_t*)s->d_off, (const uint32_t*)d_choff, (const uint32_t*)d_es,
                           (const uint32_t*)d_ee, (const uint32_t*)d_el, num_players, (flags & RMJ_LOGTEXT_MASKED_OK) ? 1u : 0u, s->d_ev, d_side, d_kcnt, s->d_dec, d_ferr);
    }
    hipLaunchKernelGGL(k_lt_scan, dim3(1), dim3(1024), 0, 0, d_kcnt, M, 1u, s->d_koff, d_tot + 2, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    // the O(n_logs) host mirrors
    s->off.assign((size_t)M + 1, 0u);
    s->koff.assign((size_t)M + 1, 0u);
    HIPCHK(hipMemcpy(s->off.data(), s->d_off, ob, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(s->koff.data(), s->d_koff, ob, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&s->max_len, d_max, 4, hipMemcpyDeviceToHost));
    s->K = s->koff[M];
    if ((rc = dalloc(&s->d_start, (size_t)s->K * 16, true))) return rc;
    if ((rc = dalloc(&s->d_end, (size_t)s->K * 16, true))) return rc;
    if ((rc = dalloc(&s->d_own, (size_t)s->K * 32, true))) return rc;
    if (M) hipLaunchKernelGGL(k_lt_tables, per_log, b256, 0, 0, (const rmjp::Side*)d_side, (const uint32_t*)s->d_off, (const uint32_t*)s->d_koff, M,
                              (const unsigned long long*)d_ferr, s->d_start, s->d_end, s->d_own, s->d_status, s->d_errline);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return RMJ_OK;
}
int rmj_logset_create_from_text(int device, const uint8_t* text, const uint64_t* ranges, uint32_t n_logs, uint32_t num_players, uint32_t flags, rmj_logset_handle* out) {
    if (!out || (!ranges && n_logs)) return fail(RMJ_ERR_ARG, "null argument");
    *out = nullptr;
    if (num_players != 3u && num_players != 4u) return fail(RMJ_ERR_ARG, "rmj_logset_create_from_text: num_players is 3 or 4");
    if (flags & ~(uint32_t)(RMJ_LOGTEXT_ON_DEVICE | RMJ_LOGTEXT_MASKED_OK)) return fail(RMJ_ERR_ARG, "rmj_logset_create_from_text: unknown flag");
    int rc = ensure_device(device);
    if (rc) return rc;
    rmj_logset* s = new rmj_logset();
    s->device = device;
    s->M = n_logs;
    {
        DevTmp tmp;
        rc = logset_from_text_impl(s, text, ranges, num_players, flags, tmp);
        if (rc) (void)hipDeviceSynchronize();
    }
    if (rc) {
        (void)hipGetLastError();
        rmj_logset_destroy(s);
        return rc;
    }
    *out = s;
    return RMJ_OK;
}
int rmj_logset_views(rmj_logset_handle s, RmjLogsetViews* out) {
    if (!s || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = RmjLogsetViews{s->d_ev, s->d_off, s->d_koff, s->d_start, s->d_end, s->d_status, s->d_errline, s->d_dec};
    return RMJ_OK;
}
int rmj_logset_status(rmj_logset_handle s, uint8_t* status, uint32_t* error_line, uint32_t* decisions, uint32_t* offsets) {
    if (!s) return fail(RMJ_ERR_ARG, "null argument");
    if ((status || error_line || decisions) && !s->d_status) return fail(RMJ_ERR_ARG, "rmj_logset_status: the set was not parsed from text, it has no status");
    HIPCHK(hipSetDevice(s->device));
    if (status && s->M) HIPCHK(hipMemcpy(status, s->d_status, s->M, hipMemcpyDeviceToHost));
    if (error_line && s->M) HIPCHK(hipMemcpy(error_line, s->d_errline, (size_t)s->M * 4, hipMemcpyDeviceToHost));
    if (decisions && s->M) HIPCHK(hipMemcpy(decisions, s->d_dec, (size_t)s->M * 4, hipMemcpyDeviceToHost));
    if (offsets) memcpy(offsets, s->off.data(), (size_t)(s->M + 1) * 4);
    return RMJ_OK;
}
// ---- GRP rank-model rows (rmj_grp.hip.h): asynchronous on the caller's stream, nothing allocated, nothing waited for
static bool grp_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0u; }
int rmj_grp_rows_device(int device, const int32_t* d_init, const int32_t* d_delta, const int32_t* d_meta, uint32_t rows, uint32_t num_players, float* d_x,
                        void* hip_stream) {
    using namespace rmjgrp;
    if (num_players != 3u && num_players != 4u) return fail(RMJ_ERR_ARG, "rmj_grp_rows_device: num_players is 3 or 4");
    if (!rows) return RMJ_OK;
    if (!d_init || !d_delta || !d_meta || !d_x) return fail(RMJ_ERR_ARG, "null argument");
    if (!grp_aligned(d_init) || !grp_aligned(d_delta) || !grp_aligned(d_meta) || !grp_aligned(d_x))
        return fail(RMJ_ERR_ARG, "rmj_grp_rows_device: the tables must be 16-byte aligned");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(k_grp_rows<false>, grp_rows_grid(rows, num_players), dim3(GRP_BLOCK), 0, (hipStream_t)hip_stream, d_init, d_delta, d_meta, rows, num_players, d_x);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_logset_grp_device(rmj_logset_handle s, uint32_t num_players, const int32_t* d_start_scores, const int32_t* d_end_scores, const RmjGrpOut* out, void* hip_stream) {
    using namespace rmjgrp;
    if (!s || !out) return fail(RMJ_ERR_ARG, "null argument");
    if (num_players != 3u && num_players != 4u) return fail(RMJ_ERR_ARG, "rmj_logset_grp_device: num_players is 3 or 4");
    const int32_t* st = d_start_scores ? d_start_scores : s->d_start;
    const int32_t* en = d_end_scores ? d_end_scores : s->d_end;
    if (!st || !en) return fail(RMJ_ERR_ARG, "rmj_logset_grp_device: a set made by rmj_logset_create holds no score tables: pass start_scores and end_scores");
    if (!s->K) return RMJ_OK;
    if (out->x && !out->meta) return fail(RMJ_ERR_ARG, "rmj_logset_grp_device: x is computed from meta: give both");
    if (!grp_aligned(st) || !grp_aligned(en) || !grp_aligned(out->meta) || !grp_aligned(out->x))
        return fail(RMJ_ERR_ARG, "rmj_logset_grp_device: the tables must be 16-byte aligned");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_grp_logs, dim3((s->M + GRP_BLOCK / 64u - 1u) / (GRP_BLOCK / 64u)), dim3(GRP_BLOCK), 0, stream, (const RmjEvent*)s->d_ev, (const uint32_t*)s->d_off,
                       (const uint32_t*)s->d_koff, s->M, (const uint8_t*)s->d_status, en, num_players, out->meta, out->rank, out->log_of);
    if (out->x)
        hipLaunchKernelGGL(k_grp_rows<true>, grp_rows_grid(s->K, num_players), dim3(GRP_BLOCK), 0, stream, st, en, (const int32_t*)out->meta, s->K, num_players, out->x);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// ---- play statistics (rmj_playstats.hip.h): one launch on the caller's stream
int rmj_logset_playstats_device(rmj_logset_handle s, uint32_t num_players, int32_t* d_rows, void* hip_stream) {
    using namespace rmjstat;
    if (!s) return fail(RMJ_ERR_ARG, "null argument");
    if (num_players != 3u && num_players != 4u) return fail(RMJ_ERR_ARG, "rmj_logset_playstats_device: num_players is 3 or 4");
    if (!s->K) return RMJ_OK;
    if (!d_rows) return fail(RMJ_ERR_ARG, "null argument");
    if (!grp_aligned(d_rows)) return fail(RMJ_ERR_ARG, "rmj_logset_playstats_device: the rows must be 16-byte aligned");
    HIPCHK(hipSetDevice(s->device));
    hipLaunchKernelGGL(k_playstats, dim3((s->M + PS_BLOCK / 64u - 1u) / (PS_BLOCK / 64u)), dim3(PS_BLOCK), 0, (hipStream_t)hip_stream, (const RmjEvent*)s->d_ev,
                       (const uint32_t*)s->d_off, (const uint32_t*)s->d_koff, s->M, (const uint8_t*)s->d_status, num_players, d_rows);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_logreplay_assign(const uint32_t* offsets, uint32_t n_logs, uint32_t n_slots, uint32_t* slot_of_log, uint32_t* slot_logs, uint32_t* slot_first, uint32_t* steps) {
    if (!offsets) return fail(RMJ_ERR_ARG, "null argument");
    if (n_slots > n_logs || (!n_slots && n_logs)) return fail(RMJ_ERR_ARG, "rmj_logreplay_assign: 1 <= n_slots <= n_logs (a slot without a log replays nothing)");
    const uint32_t st = n_slots ? rmjh::lr_assign(offsets, n_logs, n_slots, slot_of_log, slot_logs, slot_first) : 0u;
    if (!n_slots && slot_first) slot_first[0] = 0u;
    if (steps) *steps = st;
    return RMJ_OK;
}
static int logreplay_clear_impl(rmj_logreplay* r) {
    rmj_env* h = r->env;
    LogRun& R = r->R;
    const uint32_t n = R.n;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(upload_start_cursors(r->chain, r->set, n, R.pos, R.cur));
    HIPCHK(hipMemsetAsync(R.kcount, 0, (size_t)n * 4, h->stream));
    HIPCHK(hipMemsetAsync(R.tcount, 0, (size_t)n * 16, h->stream));
    HIPCHK(hipMemsetAsync(R.apply_at, 0xFF, (size_t)n * 4, h->stream));
    HIPCHK(hipMemsetAsync(R.dec_n, 0, n, h->stream));
    HIPCHK(hipMemsetAsync(R.log_status, 0, R.M ? R.M : 1u, h->stream));
    HIPCHK(hipMemsetAsync(R.traj_len, 0, (size_t)(R.K ? R.K : 1u) * 16, h->stream));
    HIPCHK(hipMemsetAsync(R.traj_broken, 0, (size_t)(R.K ? R.K : 1u) * 4, h->stream));
    HIPCHK(hipMemsetAsync(R.ctr, 0, LR_C_WORDS * 4, h->stream));
    r->chain.step = 0;
    return RMJ_OK;
}
int rmj_logreplay_create(rmj_handle h, rmj_logset_handle set, const RmjLogReplayConfig* cfg, rmj_logreplay_handle* out) {
    if (!h || !set || !cfg || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = nullptr;
    if (!cfg->capacity) return fail(RMJ_ERR_ARG, "rmj_logreplay_create: the pool needs a capacity (samples)");
    if (set->device != h->cfg.device) return fail(RMJ_ERR_ARG, "rmj_logreplay_create: the log set lives on another device");
    const uint32_t n = h->cfg.n_games;
    if (n > set->M) return fail(RMJ_ERR_ARG, "rmj_logreplay_create: more slots (the handle's games) than logs: n_slots <= M");
    uint32_t known = RMJ_LOGREPLAY_INCLUDE_PASS | RMJ_LOGREPLAY_SKIP_SINGLE_ACTION;
    for (const LogExtra& x : kLogExtras) known |= x.flag;
    if (cfg->flags & ~known) return fail(RMJ_ERR_ARG, "rmj_logreplay_create: unknown flag");
    uint32_t ch, w, rs;
    float dummy;
    RmjObsBatch b{};
    b.features = cfg->features;
    b.d_out = &dummy;   // (shape check only)
    int rc = batch_shape(h, &b, &ch, &w, &rs);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    rmj_logreplay* r = new rmj_logreplay();
    r->env = h;
    r->set = set;
    r->cfg = *cfg;
    r->cfg.gamma_powers = nullptr;
    const bool sanma = h->cfg.game_mode >= 3;
    const uint32_t cap = cfg->capacity, M = set->M, K = set->K ? set->K : 1u, A = sanma ? RMJ_ACTION_SPACE_3P : RMJ_ACTION_SPACE_4P;
    r->chain.assign(set->off.data(), M, n);
    // P[k] = gamma ** k, k < the longest log + 1 (a trajectory has fewer decisions than its log has events)
    r->n_powers = cfg->gamma_powers ? cfg->n_powers : set->max_len + 1u;
    if (!r->n_powers || (cfg->gamma_powers && cfg->n_powers < set->max_len + 1u)) {
        delete r;
        return fail(RMJ_ERR_ARG, "rmj_logreplay_create: the table of powers needs an entry per event of the longest log, plus one");
    }
    std::vector<double> pw(r->n_powers);
    for (uint32_t k = 0; k < r->n_powers; k++) pw[k] = cfg->gamma_powers ? cfg->gamma_powers[k] : std::pow(cfg->gamma, (double)k);
    LogRun& R = r->R;
    R.n = n; R.M = M; R.K = set->K; R.capacity = cap; R.feat_floats = ch * w; R.row_floats = (ch * w + 3u) & ~3u; R.A = A; R.NP = sanma ? 3u : 4u;
    R.include_pass = (cfg->flags & RMJ_LOGREPLAY_INCLUDE_PASS) ? 1u : 0u;
    R.skip_single = (cfg->flags & RMJ_LOGREPLAY_SKIP_SINGLE_ACTION) ? 1u : 0u;
    R.sanma = sanma ? 1u : 0u;
    R.ev = set->d_ev; R.off = set->d_off; R.koff = set->d_koff;
    const size_t big = n > cap ? n : cap;
    const size_t c4 = (size_t)cap * 4, n4 = (size_t)n * 4;
    rmjh::DevLayout L;
    L.add(&R.feat, (size_t)cap * R.row_floats * 4);
    const size_t o_packed = L.add(&R.packed, c4 * 2);
    L.add(&R.ret64, c4 * 2); L.add(&R.dec_action, n4 * 8); L.add(&r->d_powers, (size_t)r->n_powers * 8);
    L.add(&R.action, c4); L.add(&R.log, c4); L.add(&R.kyoku, c4); L.add(&R.seat, c4); L.add(&R.t, c4); L.add(&R.krow, c4); L.add(&R.ret, c4); L.add(&R.rank, c4);
    L.add(&R.slot_first, (size_t)(n + 1) * 4); L.add(&R.slot_logs, (size_t)(M ? M : 1u) * 4); L.add(&R.pos, n4); L.add(&R.cur, n4); L.add(&R.kcount, n4);
    L.add(&R.tcount, n4 * 4); L.add(&R.apply_at, n4); L.add(&R.dec_t, n4 * 4); L.add(&R.dec_log, n4); L.add(&R.dec_krow, n4); L.add(&R.traj_len, (size_t)K * 16);
    L.add(&R.offs, big * 4); L.add(&R.totals, ((big + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK) * 4); L.add(&R.ctr, LR_C_WORDS * 4);
    L.add(&R.mask, (size_t)cap * A); L.add(&R.dec_n, n); L.add(&R.dec_seat, n4); L.add(&R.log_status, M ? M : 1u); L.add(&R.traj_broken, (size_t)K * 4);
    const size_t off = L.bytes();
    if (hipMalloc(&r->mem, off) != hipSuccess) {
        (void)hipGetLastError();
        delete r;
        return fail(RMJ_ERR_HIP, "rmj_logreplay_create: no device memory for a pool of " + std::to_string(off >> 20) + " MiB (capacity x row bytes: choose a smaller capacity)");
    }
    for (int i = 0; i < LX_COUNT; i++) {
        const LogExtra& x = kLogExtras[i];
        if (!(cfg->flags & x.flag) || hipMalloc(&r->d_extra[i], (size_t)cap * x.slot_bytes) == hipSuccess) continue;
        (void)hipGetLastError();
        hipFree(r->mem);
        for (uint8_t* q : r->d_extra) if (q) hipFree(q);
        delete r;
        return fail(RMJ_ERR_HIP, std::string("rmj_logreplay_create: no device memory for the ") + x.noun + " records (capacity x " + std::to_string(x.slot_bytes) +
                                     " bytes: choose a smaller capacity)");
    }
    uint8_t* m = (uint8_t*)r->mem;
    L.bind(m);
    h->logreplay.push_back(r);
    // everything behind the feature rows starts as zeros (the views show defined values in slots that were never filled)
    hipError_t zeroed = hipMemsetAsync(m + o_packed, 0, off - o_packed, h->stream);
    for (int i = 0; i < LX_COUNT; i++)
        if (zeroed == hipSuccess && r->d_extra[i]) zeroed = hipMemsetAsync(r->d_extra[i], 0, (size_t)cap * kLogExtras[i].slot_bytes, h->stream);
    if (zeroed != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        upload_chain(r->chain, M, R.slot_first, R.slot_logs) != hipSuccess ||
        hipMemcpy(r->d_powers, pw.data(), (size_t)r->n_powers * 8, hipMemcpyHostToDevice) != hipSuccess || (rc = logreplay_clear_impl(r))) {
        rmj_logreplay_destroy(r);
        return rc ? rc : fail(RMJ_ERR_HIP, "rmj_logreplay_create: initialising the pool failed");
    }
    *out = r;
    return RMJ_OK;
}
int rmj_logreplay_destroy(rmj_logreplay_handle r) {
    if (!r) return RMJ_OK;
    rmj_env* h = r->env;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (size_t i = 0; i < h->logreplay.size(); i++)
        if (h->logreplay[i] == r) { h->logreplay.erase(h->logreplay.begin() + i); break; }
    hipFree(r->mem);
    for (uint8_t* q : r->d_extra) if (q) hipFree(q);
    delete r;
    return RMJ_OK;
}
int rmj_logreplay_clear(rmj_logreplay_handle r) {
    if (!r) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(r->env->cfg.device));
    return logreplay_clear_impl(r);
}
// the tail of an event step of both replays: every slot's variant applies the event the step chose for it (apply_at; LR_NO_EVENT: none)
static void launch_log_apply(rmj_env* h, uint32_t n, const RmjEvent* ev, const uint32_t* apply_at) {
    RMJ_LAUNCH_MODE(h, k_log_apply, game_grid(n), dim3(256), ev, apply_at);
}
int rmj_logreplay_run_device(rmj_logreplay_handle r, uint32_t n_steps, uint32_t* steps_left) {
    if (!r) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = r->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    const LogRun& R = r->R;
    const uint32_t n = R.n, nb = (n + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK, left = r->chain.steps - r->chain.step;
    const uint32_t todo = n_steps && n_steps < left ? n_steps : left;
    const bool sanma = h->cfg.game_mode >= 3;
    const int feat = r->cfg.features;
    const float* decay = h->d_decay;
    for (uint32_t i = 0; i < todo; i++) {
        hipLaunchKernelGGL(k_log_decide, game_grid(n), dim3(256), 0, h->stream, h->d, R, 0);
        hipLaunchKernelGGL(k_log_scan, dim3(nb), dim3(PPO_SCAN_BLOCK), 0, h->stream, R);
#define RMJ_LAUNCH_RECORD(SM, F) hipLaunchKernelGGL((k_log_record<SM, F>), dim3(n * 4), dim3(64), 0, h->stream, h->d, R, decay)
        if (sanma && feat == RMJ_FEATURES_EXTENDED) RMJ_LAUNCH_RECORD(true, RMJ_FEATURES_EXTENDED);
        else if (sanma) RMJ_LAUNCH_RECORD(true, RMJ_FEATURES_BASE);
        else if (feat == RMJ_FEATURES_EXTENDED) RMJ_LAUNCH_RECORD(false, RMJ_FEATURES_EXTENDED);
        else if (feat == RMJ_FEATURES_DISCARD_SHANTEN) RMJ_LAUNCH_RECORD(false, RMJ_FEATURES_DISCARD_SHANTEN);
        else RMJ_LAUNCH_RECORD(false, RMJ_FEATURES_BASE);
#undef RMJ_LAUNCH_RECORD
        for (int x = 0; x < LX_COUNT; x++)   // the state is still the one the rows were encoded from
            if (r->d_extra[x]) kLogExtras[x].launch(h->stream, h->d, R, r->d_extra[x]);
        launch_log_apply(h, n, R.ev, R.apply_at);
    }
    r->chain.step += todo;
    // the bookkeeping of the last step: its samples join the fill, the logs that just ended become complete
    if (n) hipLaunchKernelGGL(k_log_decide, game_grid(n), dim3(256), 0, h->stream, h->d, R, 1);
    HIPCHK(hipGetLastError());
    if (steps_left) *steps_left = r->chain.steps - r->chain.step;
    return RMJ_OK;
}
int rmj_logreplay_finalize_device(rmj_logreplay_handle r, const double* d_reward, const int32_t* d_end_scores) {
    if (!r || !d_reward || !d_end_scores) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = r->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_log_finalize, dim3((r->R.capacity + 255u) / 256u), dim3(256), 0, h->stream, r->R, d_reward, d_end_scores, (const double*)r->d_powers, r->n_powers);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_logreplay_emit_device(rmj_logreplay_handle r, const RmjLogBatch* out) {
    if (!r || !out || !out->d_count) return fail(RMJ_ERR_ARG, "null argument");
    if (out->rows && (!out->d_features || !out->d_mask || !out->d_action || !out->d_packed || !out->d_return || !out->d_return64 || !out->d_rank || !out->d_log ||
                      !out->d_kyoku || !out->d_seat || !out->d_t))
        return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = r->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t cap = r->R.capacity;
    LogOut O{out->d_features, out->d_mask, out->d_action, out->d_packed, out->d_return, out->d_return64, out->d_rank, out->d_log, out->d_kyoku, out->d_seat, out->d_t,
             out->d_count, out->rows};
    hipLaunchKernelGGL(k_log_emit_scan, dim3((cap + PPO_SCAN_BLOCK - 1) / PPO_SCAN_BLOCK), dim3(PPO_SCAN_BLOCK), 0, h->stream, r->R);
    hipLaunchKernelGGL(k_log_emit, ppo_wave_grid(cap), dim3(256), 0, h->stream, r->R, O);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
int rmj_logreplay_emit_hidden_device(rmj_logreplay_handle r, const RmjLogHiddenBatch* out) {
    const bool no_array = r && out && out->rows && (!out->d_opp_hand || !out->d_opp_shanten || !out->d_opp_waits || !out->d_opp_flags || !out->d_event);
    return logreplay_emit_extra(r, LX_HIDDEN, __func__, out, no_array, [&](hipStream_t st, const uint8_t* hid) {
        LogHiddenOut O{RmjHiddenOut{out->d_opp_hand, out->d_opp_shanten, out->d_opp_waits, out->d_opp_flags}, out->d_event, out->rows};
        hipLaunchKernelGGL(k_log_emit_hidden, ppo_wave_grid(r->R.capacity), dim3(256), 0, st, r->R, hid, O);
    });
}
int rmj_logreplay_emit_danger_device(rmj_logreplay_handle r, const RmjLogDangerBatch* out) {
    return logreplay_emit_extra(r, LX_DANGER, __func__, out, r && out && out->rows && !out->d_danger, [&](hipStream_t st, const uint8_t* dng) {
        hipLaunchKernelGGL(k_log_emit_danger, ppo_wave_grid(r->R.capacity), dim3(256), 0, st, r->R, dng, out->d_danger, out->rows);
    });
}
int rmj_logreplay_emit_dtable_device(rmj_logreplay_handle r, const RmjLogDtableBatch* out) {
    const bool no_array = r && out && out->rows && (!out->d_shanten || !out->d_accept || !out->d_ukeire);
    return logreplay_emit_extra(r, LX_DTABLE, __func__, out, no_array, [&](hipStream_t st, const uint8_t* dtb) {
        dt_launch_log_emit(st, r->R, dtb, LogDtableOut{out->d_shanten, out->d_accept, out->d_ukeire, out->rows});
    });
}
int rmj_logreplay_hidden_views(rmj_logreplay_handle r, RmjLogHiddenViews* out) {
    if (!r || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = RmjLogHiddenViews{r->R.capacity, (uint32_t)kLogExtras[LX_HIDDEN].slot_bytes, r->d_extra[LX_HIDDEN]};
    return RMJ_OK;
}
int rmj_logreplay_views(rmj_logreplay_handle r, RmjLogReplayViews* out) {
    if (!r || !out) return fail(RMJ_ERR_ARG, "null argument");
    const LogRun& R = r->R;
    *out = RmjLogReplayViews{R.capacity, R.row_floats, R.A, r->chain.steps, R.feat, R.mask, R.action, R.packed, R.ret, R.ret64, R.rank, R.log, R.kyoku, R.seat, R.t,
                             R.log_status, R.traj_len, R.traj_broken, R.ctr};
    return RMJ_OK;
}
int rmj_logreplay_counts(rmj_logreplay_handle r, RmjLogReplayCounts* out) {
    if (!r || !out) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = r->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    uint32_t c[LR_C_WORDS];
    HIPCHK(hipMemcpyAsync(c, r->R.ctr, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = RmjLogReplayCounts{c[LR_C_FILL], c[LR_C_OVERFLOWED], c[LR_C_FAILED], c[LR_C_COMPLETE], c[LR_C_DECISIONS], c[LR_C_EVENTS], r->chain.step, r->chain.steps - r->chain.step};
    return RMJ_OK;
}

// ---- log validation (rmj_logcheck.hip.h) ------------------------------------------------------------------------
const char* rmj_logcheck_name(uint32_t code) {
    static const char* const names[RMJ_LOGCHECK_CODES] = {"OK", "PARSE", "NO_START_KYOKU", "AFTER_END", "UNFINISHED", "ACTOR", "DRAW_OUT_OF_TURN", "NOT_OFFERED",
                                                          "TILE_NOT_HELD", "TILE_COUNT", "NO_LEGAL_MATCH", "SCORE_CONTINUITY", "SCORE_CONSERVATION"};
    return code < RMJ_LOGCHECK_CODES ? names[code] : nullptr;
}
int rmj_logcheck_create(rmj_handle h, rmj_logset_handle set, uint32_t n_slots, uint32_t flags, struct rmj_logcheck** out) {
    if (!h || !set || !out) return fail(RMJ_ERR_ARG, "null argument");
    *out = nullptr;
    if (set->device != h->cfg.device) return fail(RMJ_ERR_ARG, "rmj_logcheck_create: the log set lives on another device");
    if (flags & ~(uint32_t)RMJ_LOGCHECK_GUARDS) return fail(RMJ_ERR_ARG, "rmj_logcheck_create: unknown flag");
    const uint32_t games = h->cfg.n_games, n = n_slots ? n_slots : games, M = set->M;
    if (!M) return fail(RMJ_ERR_ARG, "rmj_logcheck_create: the set holds no log");
    if (n > games || n > M) return fail(RMJ_ERR_ARG, "rmj_logcheck_create: 1 <= n_slots <= the handle's games, and at most one slot per log");
    HIPCHK(hipSetDevice(h->cfg.device));
    rmj_logcheck* c = new rmj_logcheck();
    c->env = h;
    c->set = set;
    c->chain.assign(set->off.data(), M, n);
    const bool sanma = h->cfg.game_mode >= 3;
    LogCheck& R = c->R;
    R.n = n; R.M = M; R.NP = sanma ? 3u : 4u; R.sanma = sanma ? 1u : 0u;
    R.ev = set->d_ev; R.off = set->d_off; R.koff = set->d_koff; R.status = set->d_status; R.errline = set->d_errline;
    R.start = set->d_start; R.end = set->d_own;
    const size_t guard = (flags & RMJ_LOGCHECK_GUARDS) ? (size_t)RMJ_LOGCHECK_GUARD_WORDS * 4 : 0;
    const size_t M4 = (size_t)M * 4, n4 = (size_t)n * 4;
    rmjh::DevLayout L;   // the verdict arrays, a guard in front of each (which ends where the array begins) and one behind the last, then the bookkeeping
    L.add_guarded(&R.code, M, guard); L.add_guarded(&R.seat, M, guard); L.add_guarded(&R.kyoku, M4, guard); L.add_guarded(&R.event, M4, guard);
    L.add_guarded(&R.detail, M4, guard); L.add_guarded(&R.counts, RMJ_LOGCHECK_COUNTERS * 4, guard); L.guard(guard);
    L.add(&R.slot_first, (size_t)(n + 1) * 4); L.add(&R.slot_logs, M4); L.add(&R.pos, n4); L.add(&R.cur, n4); L.add(&R.kcount, n4); L.add(&R.word, n4);
    L.add(&R.seen, (size_t)n * LC_SEEN); L.add(&R.apply_at, (size_t)games * 4);
    const size_t off = L.bytes();
    if (hipMalloc(&c->mem, off) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        return fail(RMJ_ERR_HIP, "rmj_logcheck_create: no device memory for the verdicts");
    }
    uint8_t* m = (uint8_t*)c->mem;
    L.bind(m);
    // zeros everywhere, then the guards (which end where an array begins, and begin where the array's 256-byte step ends), the "nobody is
    // due" words, "no event" for every game of the handle, the assignment and the cursors; the verdicts start as OK / PARSE
    std::vector<uint32_t> gw(RMJ_LOGCHECK_GUARD_WORDS, RMJ_LOGCHECK_GUARD_WORD), word(n, (uint32_t)LC_NONE | (LC_NO_SEAT << 8));
    bool ok = hipMemsetAsync(m, 0, off, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess;
    if (guard)
        for (size_t o : L.guards()) ok = ok && hipMemcpy(m + o, gw.data(), guard, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(R.apply_at, 0xFF, (size_t)games * 4) == hipSuccess && hipMemcpy(R.word, word.data(), (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess &&
         upload_chain(c->chain, M, R.slot_first, R.slot_logs) == hipSuccess && upload_start_cursors(c->chain, set, n, R.pos, R.cur) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_logcheck_init, dim3((M + 255u) / 256u), dim3(256), 0, h->stream, R);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        hipFree(c->mem);
        delete c;
        return fail(RMJ_ERR_HIP, "rmj_logcheck_create: initialising the verdicts failed");
    }
    *out = c;
    return RMJ_OK;
}
int rmj_logcheck_destroy(struct rmj_logcheck* c) {
    if (!c) return RMJ_OK;
    rmj_env* h = c->env;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    hipFree(c->mem);
    delete c;
    return RMJ_OK;
}
int rmj_logcheck_set_scores(struct rmj_logcheck* c, const int32_t* d_start_scores, const int32_t* d_end_scores) {
    if (!c) return fail(RMJ_ERR_ARG, "null argument");
    if (!d_start_scores != !d_end_scores) return fail(RMJ_ERR_ARG, "rmj_logcheck_set_scores: give both tables or neither");
    c->R.start = d_start_scores ? d_start_scores : c->set->d_start;
    c->R.end = d_end_scores ? d_end_scores : c->set->d_own;
    return RMJ_OK;
}
int rmj_logcheck_run_device(struct rmj_logcheck* c, uint32_t n_steps, uint32_t* steps_left) {
    if (!c) return fail(RMJ_ERR_ARG, "null argument");
    rmj_env* h = c->env;
    HIPCHK(hipSetDevice(h->cfg.device));
    const LogCheck& R = c->R;
    const uint32_t left = c->chain.steps - c->chain.step, todo = n_steps && n_steps < left ? n_steps : left;
    for (uint32_t i = 0; i < todo; i++) {
        hipLaunchKernelGGL(k_log_check, game_grid(R.n), dim3(256), 0, h->stream, h->d, R, 0);
        launch_log_apply(h, R.n, R.ev, R.apply_at);
    }
    c->chain.step += todo;
    // the verdicts of the logs that just ended
    hipLaunchKernelGGL(k_log_check, game_grid(R.n), dim3(256), 0, h->stream, h->d, R, 1);
    HIPCHK(hipGetLastError());
    if (steps_left) *steps_left = c->chain.steps - c->chain.step;
    return RMJ_OK;
}
int rmj_logcheck_views(struct rmj_logcheck* c, RmjLogCheckViews* out) {
    if (!c || !out) return fail(RMJ_ERR_ARG, "null argument");
    const LogCheck& R = c->R;
    *out = RmjLogCheckViews{R.M, c->chain.steps, R.code, R.seat, R.kyoku, R.event, R.detail, R.counts};
    return RMJ_OK;
}

// ---- shanten (row A7) -------------------------------------------------------------------------------
int rmj_shanten(int device, const uint8_t* counts, uint32_t n, int sanma, int8_t* out) {
    DevTmp tmp;
    if (!counts || !out) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    ShantenTables T;
    if ((rc = shanten_tables_for(device, &T))) return rc;
    uint8_t* d_c;
    int8_t* d_o;
    HIPCHK(tmp.alloc(&d_c, (size_t)n * 34));
    HIPCHK(tmp.alloc(&d_o, n));
    HIPCHK(hipMemcpy(d_c, counts, (size_t)n * 34, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_shanten, dim3((n + 255) / 256), dim3(256), 0, 0, T, d_c, n, sanma, d_o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_o, n, hipMemcpyDeviceToHost));
    return RMJ_OK;
}

static int run_ukeire(int device, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, int mode, uint32_t* out) {
    DevTmp tmp;
    if (!counts || !out || (mode == 1 && !visible)) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    ShantenTables T;
    if ((rc = shanten_tables_for(device, &T))) return rc;
    uint8_t *d_c = nullptr, *d_v = nullptr;
    uint32_t* d_o = nullptr;
    HIPCHK(tmp.alloc(&d_c, (size_t)n * 34));
    HIPCHK(tmp.alloc(&d_o, (size_t)n * 4));
    HIPCHK(hipMemcpy(d_c, counts, (size_t)n * 34, hipMemcpyHostToDevice));
    if (mode == 1) {
        HIPCHK(tmp.alloc(&d_v, (size_t)n * 34));
        HIPCHK(hipMemcpy(d_v, visible, (size_t)n * 34, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_ukeire, dim3((n + 3) / 4), dim3(256), 0, 0, T, (const uint8_t*)d_c, (const uint8_t*)d_v, n, sanma, mode, d_o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_o, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RMJ_OK;
}
int rmj_effective_tiles(int device, const uint8_t* counts, uint32_t n, int sanma, uint32_t* out) {
    return run_ukeire(device, counts, nullptr, n, sanma, 0, out);
}
int rmj_best_ukeire(int device, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, uint32_t* out) {
    return run_ukeire(device, counts, visible, n, sanma, 1, out);
}
int rmj_discard_table_hands(int device, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, const RmjDiscardTableOut* out) {
    DevTmp tmp;
    if (!counts || !out || !out->d_shanten || !out->d_accept || !out->d_ukeire) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    if (n == 0) return RMJ_OK;
    ShantenTables T;
    if ((rc = shanten_tables_for(device, &T))) return rc;
    const size_t cells = (size_t)n * RMJ_DTAB_COLS;
    uint8_t *d_c = nullptr, *d_v = nullptr;
    RmjDiscardTableOut d{};
    HIPCHK(tmp.alloc(&d_c, (size_t)n * 34));
    HIPCHK(tmp.alloc(&d.d_shanten, cells));
    HIPCHK(tmp.alloc(&d.d_accept, cells));
    HIPCHK(tmp.alloc(&d.d_ukeire, cells));
    if (out->d_mask) HIPCHK(tmp.alloc(&d.d_mask, cells * 8));
    HIPCHK(hipMemcpy(d_c, counts, (size_t)n * 34, hipMemcpyHostToDevice));
    if (visible) {
        HIPCHK(tmp.alloc(&d_v, (size_t)n * 34));
        HIPCHK(hipMemcpy(d_v, visible, (size_t)n * 34, hipMemcpyHostToDevice));
    }
    dt_launch_hands(T, d_c, d_v, n, sanma, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out->d_shanten, d.d_shanten, cells, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->d_accept, d.d_accept, cells, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->d_ukeire, d.d_ukeire, cells, hipMemcpyDeviceToHost));
    if (out->d_mask) HIPCHK(hipMemcpy(out->d_mask, d.d_mask, cells * 8, hipMemcpyDeviceToHost));
    return RMJ_OK;
}

// ---- MJAI event ingestion (row N1) --------------------------------------------------------------
int rmj_apply_events(rmj_handle h, const RmjEvent* events) {
    if (!h || !events) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)h->cfg.n_games * 3 * sizeof(RmjEvent);
    void* sp;
    int rcs = scratch_for(h, bytes, &sp);
    if (rcs) return rcs;
    RmjEvent* d_ev = (RmjEvent*)sp;
    HIPCHK(hipMemcpyAsync(d_ev, events, bytes, hipMemcpyHostToDevice, h->stream));
    RMJ_LAUNCH_MODE(h, k_apply_event, game_grid(h->cfg.n_games), dim3(256), (const RmjEvent*)d_ev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RMJ_OK;
}

// ---- measurement -----------------------------------------------------------------------------
static int bench_rollout_impl(rmj_handle h, uint64_t policy_seed, uint32_t warmup, uint32_t steps, RmjBenchResult* out, bool count, int pol = 0, uint32_t rate = 0u) {
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = warmup ? step_policy_impl(h, policy_seed, warmup, 1, pol, rate) : RMJ_OK;
    if (rc) return rc;
    uint64_t before = 0, after = 0, full0 = 0, full1 = 0;
    if (count && ((rc = rmj_total_steps(h, &before)) || (rc = rmj_total_full_path(h, &full0)))) return rc;
    for (int i = 0; i < 2; i++)
        if (!h->ev_time[i]) HIPCHK(hipEventCreate(&h->ev_time[i]));
    hipEvent_t e0 = h->ev_time[0], e1 = h->ev_time[1];
    HIPCHK(hipEventRecord(e0, h->stream));
    rmjh::RolloutPlan ran;
    if ((rc = step_policy_impl(h, policy_seed, steps, 1, pol, rate, &ran))) return rc;
    HIPCHK(hipEventRecord(e1, h->stream));
    // (polling, not hipEventSynchronize: a blocked host thread is woken 10-20 us after the event completes - 2 % of the driver's 20-step window, which ends with this wait)
    for (;;) {
        const hipError_t qe = hipEventQuery(e1);
        if (qe == hipSuccess) break;
        if (qe != hipErrorNotReady) return fail(RMJ_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(qe));
    }
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (count && ((rc = rmj_total_steps(h, &after)) || (rc = rmj_total_full_path(h, &full1)))) return rc;
    out->total_ms = ms;
    out->launches = ran.launches;
    out->step_kernel_ms = steps ? ms / steps : 0.0;  // each stream runs `steps` launches back to back during `ms`
    out->env_steps = after - before;
    out->launches_in_flight = ran.launches_in_flight;
    out->full_path_steps = full1 - full0;
    out->queued = ran.queued;
    out->reserved = 0u;
    return RMJ_OK;
}
int rmj_bench_rollout(rmj_handle h, uint64_t policy_seed, uint32_t warmup, uint32_t steps, RmjBenchResult* out) {
    return bench_rollout_impl(h, policy_seed, warmup, steps, out, true);
}
// The timed region alone: HIP events on the handle's stream around rmj_step_random(h, policy_seed, steps, auto_reset = 1), nothing
// else issued or synchronised (the step / full-path counters of rmj_bench_rollout cost four small launches and four host round
// trips - a fifth of a 20-step rollout).  env_steps / full_path_steps are left 0: read rmj_total_steps / rmj_total_full_path
// outside the region.
int rmj_time_rollout(rmj_handle h, uint64_t policy_seed, uint32_t steps, RmjBenchResult* out) {
    return bench_rollout_impl(h, policy_seed, 0u, steps, out, false);
}
// the same around rmj_step_random_encode(h, policy_seed, steps, 1, 2, d_out) (BASELINE configs[4]); queued: the one-launch rollout ran as tickets
int rmj_time_rollout_encode(rmj_handle h, uint64_t policy_seed, uint32_t steps, float* d_out, RmjBenchResult* out) {
    DevTmp tmp;
    if (!h || !out || !d_out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipEvent_t e0, e1;
    HIPCHK(tmp.event(&e0));
    HIPCHK(tmp.event(&e1));
    HIPCHK(hipEventRecord(e0, h->stream));
    rmjh::RolloutPlan ran;
    int rc = step_encode_impl(h, policy_seed, steps, 1, 2, d_out, &ran);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    memset(out, 0, sizeof(*out));
    out->total_ms = ms;
    out->step_kernel_ms = steps ? ms / steps : 0.0;
    out->launches = ran.launches;
    out->launches_in_flight = ran.launches_in_flight;
    out->queued = ran.queued;
    return RMJ_OK;
}
// the same around rmj_step_greedy(h, policy_seed, steps, 1, call_rate_256)
int rmj_time_rollout_greedy(rmj_handle h, uint64_t policy_seed, uint32_t steps, uint32_t call_rate_256, RmjBenchResult* out) {
    return bench_rollout_impl(h, policy_seed, 0u, steps, out, false, 1, call_rate_256);
}
int rmj_set_rollout_streams(rmj_handle h, int k) {
    if (!h || k < 1 || k > RMJ_MAX_ROLLOUT_STREAMS) return fail(RMJ_ERR_ARG, "rollout streams must be 1..8");
    h->tune.want_streams = k;
    return RMJ_OK;
}
// device memory / synchronisation for a harness that has no other way to HIP (bench.py runs one GPU without torch)
int rmj_bench_device_alloc(int device, uint64_t bytes, void** out) {
    if (!out) return fail(RMJ_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    HIPCHK(hipMalloc(out, (size_t)bytes));
    HIPCHK(hipMemset(*out, 0, (size_t)bytes));
    return RMJ_OK;
}
int rmj_bench_device_free(int device, void* p) {
    int rc = ensure_device(device);
    if (rc) return rc;
    HIPCHK(hipFree(p));
    return RMJ_OK;
}
int rmj_bench_device_sync(int device) {
    int rc = ensure_device(device);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    return RMJ_OK;
}
int rmj_total_full_path(rmj_handle h, uint64_t* total) {
    if (!h || !total) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipMemsetAsync(h->d_counter, 0, 8, h->stream));
    hipLaunchKernelGGL(k_sum_full, dim3(256), dim3(256), 0, h->stream, h->d.core, h->cfg.n_games, h->d_counter);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long v = 0;
    HIPCHK(hipMemcpy(&v, h->d_counter, 8, hipMemcpyDeviceToHost));
    *total = v;
    return RMJ_OK;
}
int rmj_random_actions_device(rmj_handle h, uint64_t policy_seed, rmj_action_t* d_actions) {
    if (!h || !d_actions) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    hipLaunchKernelGGL(k_random_actions, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, policy_seed, (uint64_t*)d_actions);
    HIPCHK(hipGetLastError());
    return RMJ_OK;
}
// The unfused counterpart of rmj_bench_rollout: every step is one policy launch (k_random_actions writes packed actions
// to a device buffer) followed by one step launch that VALIDATES those actions against the stored legal lists like
// GameState::step does for an external agent (state/mod.rs:339-402); finished games restart.  One stream, whole batch.
int rmj_bench_rollout_validated(rmj_handle h, uint64_t policy_seed, uint32_t warmup, uint32_t steps, RmjBenchResult* out) {
    DevTmp tmp;
    if (!h || !out) return fail(RMJ_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint32_t n = h->cfg.n_games;
    uint64_t before = 0, after = 0, full0 = 0, full1 = 0;
    hipEvent_t e0, e1;
    HIPCHK(tmp.event(&e0));
    HIPCHK(tmp.event(&e1));
    int rc;
    for (uint32_t s = 0; s < warmup + steps; s++) {
        if (s == warmup) {
            if ((rc = rmj_total_steps(h, &before)) || (rc = rmj_total_full_path(h, &full0))) return rc;
            HIPCHK(hipEventRecord(e0, h->stream));
        }
        hipLaunchKernelGGL(k_random_actions, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, policy_seed, h->d_actions);
        launch_step_range(h, h->stream, h->d_actions, 0ull, STEP_F_AUTORESET, 0u, n);
    }
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if ((rc = rmj_total_steps(h, &after)) || (rc = rmj_total_full_path(h, &full1))) return rc;
    out->total_ms = ms;
    out->launches = steps;
    out->step_kernel_ms = steps ? ms / steps : 0.0;  // policy launch + step launch
    out->env_steps = after - before;
    out->launches_in_flight = 1;
    out->full_path_steps = full1 - full0;
    out->queued = 0u;
    out->reserved = 0u;
    return RMJ_OK;
}
// Average duration of one encoder launch over `reps` back-to-back launches (HIP events on the handle's stream): the
// roofline figure of BASELINE's feature-output configuration.  d_out like rmj_encode_device / rmj_encode_extended_device.
int rmj_bench_encode(rmj_handle h, int extended, int only_active, float* d_out, uint32_t reps, double* avg_ms) {
    if (!h || !d_out || !avg_ms || reps == 0) return fail(RMJ_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    return time_launches(h->stream, reps, false, avg_ms, [&] { return launch_encode(h, only_active, d_out, extended != 0); });
}
// Kernel-gate benchmark (the groups of riichienv-core/benches/agari_bench.rs:142-376): average duration of
// ONE launch of a hand-math kernel over `n` device-resident inputs, HIP events around `reps` back-to-back launches after a warm-up
// launch; nothing is copied back.  which: 0 = k_eval_hands (a = RmjHandCase[n]), 1 = k_agari_counts (a = counts[n][34]),
// 2 = k_shanten, 3 = k_ukeire effective tiles, 4 = k_ukeire best ukeire (b = visible[n][34]), 5 = k_score (a = han, fu, oya, tsumo,
// num_players as five byte arrays of n one after the other; b = honba u32[n]).
int rmj_bench_hand_kernel(int device, int which, const void* a, const void* b, uint32_t n, int sanma, uint32_t reps, double* avg_ms) {
    DevTmp tmp;
    if (!a || !avg_ms || n == 0 || reps == 0 || which < 0 || which > 5 || ((which == 4 || which == 5) && !b)) return fail(RMJ_ERR_ARG, "bad argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    ShantenTables T;
    if ((rc = shanten_tables_for(device, &T))) return rc;
    const size_t in_a = which == 0 ? (size_t)n * sizeof(RmjHandCase) : (which == 5 ? (size_t)n * 5 : (size_t)n * 34);
    const size_t in_b = which == 4 ? (size_t)n * 34 : (which == 5 ? (size_t)n * 4 : 0);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_o = nullptr;
    HIPCHK(tmp.alloc(&d_a, in_a));
    HIPCHK(hipMemcpy(d_a, a, in_a, hipMemcpyHostToDevice));
    if (in_b) {
        HIPCHK(tmp.alloc(&d_b, in_b));
        HIPCHK(hipMemcpy(d_b, b, in_b, hipMemcpyHostToDevice));
    }
    HIPCHK(tmp.alloc(&d_o, (size_t)n * (which == 0 ? sizeof(RmjHandResult) : 16)));
    return time_launches(0, reps, true, avg_ms, [&] {
        switch (which) {
            case 0: hipLaunchKernelGGL(k_eval_hands, dim3((n + 15u) / 16u), dim3(256), 0, 0, (const RmjHandCase*)d_a, n, (RmjHandResult*)d_o); break;
            case 1: hipLaunchKernelGGL(k_agari_counts, dim3((n + 15) / 16), dim3(256), 0, 0, (const uint8_t*)d_a, n, d_o, d_o + n, (uint64_t*)(d_o + 8 * (size_t)n)); break;
            case 2: hipLaunchKernelGGL(k_shanten, dim3((n + 255) / 256), dim3(256), 0, 0, T, (const uint8_t*)d_a, n, sanma, (int8_t*)d_o); break;
            case 3: hipLaunchKernelGGL(k_ukeire, dim3((n + 3) / 4), dim3(256), 0, 0, T, (const uint8_t*)d_a, (const uint8_t*)nullptr, n, sanma, 0, (uint32_t*)d_o); break;
            case 4: hipLaunchKernelGGL(k_ukeire, dim3((n + 3) / 4), dim3(256), 0, 0, T, (const uint8_t*)d_a, (const uint8_t*)d_b, n, sanma, 1, (uint32_t*)d_o); break;
            default: hipLaunchKernelGGL(k_score, dim3((n + 255) / 256), dim3(256), 0, 0, (const uint8_t*)d_a, (const uint8_t*)d_a + n, (const uint8_t*)d_a + 2 * (size_t)n,
                                        (const uint8_t*)d_a + 3 * (size_t)n, (const uint32_t*)d_b, (const uint8_t*)d_a + 4 * (size_t)n, n, (uint32_t*)d_o); break;
        }
        return RMJ_OK;
    });
}
// Observation outputs of ONE game (sampled parity checks at batch sizes where fetching every game's lists is wasteful)
int rmj_peek_outputs(rmj_handle h, uint32_t game, rmj_action_t* legal /*[4][64]*/, uint8_t* counts /*[4]*/, uint8_t* mask /*[4][82]*/,
                     uint64_t* waits /*[4]*/, uint32_t* status) {
    if (!h || !legal || !counts || !mask || !waits || !status) return fail(RMJ_ERR_ARG, "null argument");
    if (game >= h->cfg.n_games) return fail(RMJ_ERR_RANGE, "game index out of range");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(legal, h->d.legal + (size_t)game * 4 * RMJ_MAX_LEGAL, 4 * RMJ_MAX_LEGAL * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts, h->d.nlegal + (size_t)game * 4, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mask, h->d.mask + (size_t)game * 4 * 82, 4 * 82, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(waits, h->d.waits + (size_t)game * 4, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, h->d.status + game, 4, hipMemcpyDeviceToHost));
    return RMJ_OK;
}

#ifdef RMJ_CUTS
// instruction accounting build only (scripts/valu_sections.py): waves end at PROF mark `cut` (-1: run to the end)
extern "C" int rmj_prof_set_cut(int cut, int cut2, int cut3) {
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_cut3), &cut3, sizeof(cut3)));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_cut), &cut, sizeof(cut)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_cut2), &cut2, sizeof(cut2)));
    return RMJ_OK;
}
#endif

#if defined(RMJ_CUTS) || defined(RMJ_CENSUS)
extern "C" int rmj_prof_bail_census(uint32_t* out32, int reset) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out32, HIP_SYMBOL(rmj::g_bail_reason), 32 * sizeof(uint32_t)));
    if (reset) {
        uint32_t z[32] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_bail_reason), z, sizeof(z)));
    }
    return RMJ_OK;
}
#endif


#ifdef RMJ_RE_PROF
extern "C" int rmj_debug_re_prof(unsigned long long* out8, int reset) {
    unsigned long long z[24] = {0};
    if (out8) HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(rmj::g_re_prof), sizeof(z)));
    if (reset) HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_re_prof), z, sizeof(z)));
    return RMJ_OK;
}
#endif

#ifdef RMJ_TL4
// timeline build only (scripts/timeline4.py): rows of the waves of the last launch of k_step4<false> (allocates on first call)
int rmj_tl4_fetch(uint64_t* out, uint32_t n_waves) {
    static unsigned long long* buf = nullptr;
    static uint32_t cap = 0;
    HIPCHK(hipDeviceSynchronize());
    if (!buf) {
        cap = n_waves;
        HIPCHK(hipMalloc(&buf, (size_t)cap * RMJ_TL4_ROW * 8));
        HIPCHK(hipMemset(buf, 0, (size_t)cap * RMJ_TL4_ROW * 8));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_tl4), &buf, sizeof(buf)));
        return RMJ_OK;
    }
    HIPCHK(hipMemcpy(out, buf, (size_t)(n_waves < cap ? n_waves : cap) * RMJ_TL4_ROW * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(buf, 0, (size_t)cap * RMJ_TL4_ROW * 8));   // blocks that leave at once (heavy-first order) write nothing
    HIPCHK(hipDeviceSynchronize());
    return RMJ_OK;
}
#endif

#ifdef RMJ_QTL
// ticket timeline build only (scripts/timeline_queue.py): rows of the waves of the last k_step4_queue launch (allocates on first call)
int rmj_qtl_fetch(uint64_t* out, uint32_t n_waves) {
    static unsigned long long* buf = nullptr;
    static uint32_t cap = 0;
    HIPCHK(hipDeviceSynchronize());
    if (!buf) {
        cap = n_waves;
        HIPCHK(hipMalloc(&buf, (size_t)cap * RMJ_QTL_ROW * 8));
        HIPCHK(hipMemset(buf, 0, (size_t)cap * RMJ_QTL_ROW * 8));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_qtl), &buf, sizeof(buf)));
        return RMJ_OK;
    }
    HIPCHK(hipMemcpy(out, buf, (size_t)(n_waves < cap ? n_waves : cap) * RMJ_QTL_ROW * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(buf, 0, (size_t)cap * RMJ_QTL_ROW * 8));
    HIPCHK(hipDeviceSynchronize());
    return RMJ_OK;
}
#endif

#ifdef RMJ_PROFILE
// profiling build only (scripts/prof_sections.py): per-section wave cycles / visit counts of k_step, summed over games
int rmj_prof_fetch(uint32_t n_games, uint64_t* cyc, uint64_t* cnt, int reset) {
    static uint32_t* buf = nullptr;
    HIPCHK(hipDeviceSynchronize());
    if (!buf) {
        HIPCHK(hipMalloc(&buf, (size_t)n_games * 64 * 4));
        HIPCHK(hipMemset(buf, 0, (size_t)n_games * 64 * 4));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(rmj::g_prof_buf), &buf, sizeof(buf)));
    }
    std::vector<uint32_t> h((size_t)n_games * 64);
    HIPCHK(hipMemcpy(h.data(), buf, h.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < 32; i++) { cyc[i] = 0; cnt[i] = 0; }
    for (size_t g = 0; g < n_games; g++)
        for (int i = 0; i < 32; i++) { cyc[i] += h[g * 64 + i]; cnt[i] += h[g * 64 + 32 + i]; }
    if (reset) HIPCHK(hipMemset(buf, 0, (size_t)n_games * 64 * 4));
    return RMJ_OK;
}
#endif

}  // extern "C"

// ---- the discard table's launches: the first naming of its kernels, behind everything else in the code object (rmj_dtable.hip.h)
static void dt_launch_rows(hipStream_t st, const Env& E, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDiscardTableOut& O) {
    hipLaunchKernelGGL(k_dtable_rows<0>, dim3((rows + 3u) / 4u), dim3(256), 0, st, E, d_index, rows, d_count, O);
}
static void dt_launch_hands(const ShantenTables& T, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, const RmjDiscardTableOut& O) {
    hipLaunchKernelGGL(k_dtable_hands<0>, dim3((n + 3) / 4), dim3(256), 0, 0, T, counts, visible, n, sanma, O);
}
static void hid_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* hid) {
    hipLaunchKernelGGL(k_log_hidden, dim3(R.n * 4), dim3(64), 0, st, E, R, hid);
}
static void dng_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* dng) {
    hipLaunchKernelGGL(k_log_danger, dim3(R.n * 4), dim3(64), 0, st, E, R, dng);
}
static void dt_launch_log(hipStream_t st, const Env& E, const LogRun& R, uint8_t* dtb) {
    hipLaunchKernelGGL(k_log_dtable<0>, dim3(R.n * 4), dim3(64), 0, st, E, R, dtb);
}
static void dt_launch_log_emit(hipStream_t st, const LogRun& R, const uint8_t* dtb, const LogDtableOut& O) {
    hipLaunchKernelGGL(k_log_emit_dtable<0>, ppo_wave_grid(R.capacity), dim3(256), 0, st, R, dtb, O);
}
