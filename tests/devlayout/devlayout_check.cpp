// CPU check of the layout and slot-chain helpers of the C boundary's host code (riichienv_amd/csrc/rmj_host.h: rmjh::DevLayout,
// rmjh::SlotChain), built with g++ by tests/test_devlayout_host.py - once plain, once under AddressSanitizer + UBSan.
//
// DevLayout is held to a restatement, written out here, of the `take` lambda the pool constructors used to carry (offset = the running
// total, which advances by the size rounded up to the step), on random size lists that include 0, 1, 255, 256, 257 and sizes above 4 GiB.
// No memory of those sizes exists: bind() only forms addresses from a base, it never touches what they point at.
// SlotChain::start_cursors is held to a restatement of the loop over offset tables with logs of no events in front, behind and in runs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../riichienv_amd/csrc/rmj_host.h"

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

// ---- the restatement: the lambda of the pool constructors, with its step as a parameter
struct Take {
    size_t off = 0;
    size_t take(size_t bytes, size_t step) {
        const size_t o = off;
        off += (bytes + step - 1) & ~(step - 1);
        return o;
    }
};

static const size_t kEdge[] = {0, 1, 255, 256, 257, 4, 15, 16, 17, 31, 32, 33, 511, 512, 513, 65536, 1000003,
                               ((size_t)1 << 32) - 1, (size_t)1 << 32, ((size_t)1 << 32) + 1, ((size_t)5 << 32) + 255, ((size_t)9 << 32) + 257};
static size_t random_size(std::mt19937_64& rng) {
    const uint64_t r = rng();
    if ((r & 3) == 0) return kEdge[(r >> 8) % (sizeof(kEdge) / sizeof(kEdge[0]))];
    if ((r & 3) == 1) return (size_t)((r >> 8) % 1024);
    if ((r & 3) == 2) return (size_t)((r >> 8) % ((uint64_t)1 << 24));
    return (size_t)((r >> 8) % ((uint64_t)12 << 32));
}

// A frame of pointer slots with sentinels between, before and behind them: the registered ones are every second slot
static const uintptr_t SENTINEL = (uintptr_t)0xA5A5A5A5A5A5A5A5ull;
struct Frame {
    std::vector<char*> slot;   // [2 * n + 1]: odd = registered, even = sentinel
    explicit Frame(size_t n) : slot(2 * n + 1, (char*)SENTINEL) {}
    char** at(size_t i) { return &slot[2 * i + 1]; }
    void check_sentinels() {
        for (size_t i = 0; i < slot.size(); i += 2) CHECK(slot[i] == (char*)SENTINEL, "sentinel %zu overwritten", i);
    }
};

// one step for every array (what the pools and the 256-byte scratch layouts do): offsets and total equal the lambda's
static void uniform_case(std::mt19937_64& rng, size_t step) {
    const size_t n = 1 + (size_t)(rng() % 40);
    std::vector<size_t> sz(n), want(n), got(n);
    for (size_t& s : sz) s = random_size(rng);
    Take T;
    for (size_t i = 0; i < n; i++) want[i] = T.take(sz[i], step);
    Frame F(n);
    rmjh::DevLayout L(step);
    const bool per_call = (rng() & 1) != 0;   // the same step given with every call
    for (size_t i = 0; i < n; i++) got[i] = per_call ? L.add(F.at(i), sz[i], step) : L.add(F.at(i), sz[i]);
    for (size_t i = 0; i < n; i++) {
        CHECK(got[i] == want[i], "array %zu of %zu (step %zu): offset %zu, the lambda gives %zu", i, n, step, got[i], want[i]);
        CHECK(got[i] % step == 0, "offset %zu is no multiple of the step %zu", got[i], step);
        if (i + 1 < n) CHECK(got[i + 1] >= got[i] + sz[i] && got[i + 1] - (got[i] + sz[i]) < step, "array %zu: the next one does not follow within a step", i);
    }
    CHECK(L.bytes() == T.off, "total %zu, the lambda gives %zu", L.bytes(), T.off);
    CHECK(L.bytes() % step == 0, "total %zu is no multiple of the step", L.bytes());
    char* const base = (char*)(uintptr_t)0x7000000000ull + (size_t)(rng() % 4096) * 256;
    L.bind(base);
    for (size_t i = 0; i < n; i++) CHECK(*F.at(i) == base + want[i], "bind: pointer %zu", i);
    F.check_sentinels();
}

// a step of its own with every call (4, 16, 32, 256 and 1 for a packed tail): an array begins where the one before ends, rounded up to
// THAT array's step - the drain's 4-byte words with the records at a multiple of 32, the text work area's 16
static void mixed_case(std::mt19937_64& rng) {
    static const size_t steps[] = {4, 16, 32, 256, 1};
    const size_t n = 2 + (size_t)(rng() % 20);
    std::vector<size_t> sz(n), st(n), got(n);
    Frame F(n);
    rmjh::DevLayout L(4);
    size_t end = 0;   // restated: the running end
    for (size_t i = 0; i < n; i++) {
        sz[i] = random_size(rng);
        st[i] = steps[rng() % 5];
        got[i] = L.add(F.at(i), sz[i], st[i]);
        CHECK(got[i] == end, "array %zu begins at %zu, the one before ended at %zu", i, got[i], end);
        end = end + sz[i];
        while (end % st[i]) end++;
        CHECK(L.bytes() == end, "after array %zu: total %zu, restated %zu", i, L.bytes(), end);
        CHECK(L.bytes() % st[i] == 0 && L.bytes() - (got[i] + sz[i]) < st[i], "step %zu not honoured behind array %zu", st[i], i);
    }
    char* const base = (char*)(uintptr_t)0x7000000000ull;
    L.bind(base);
    for (size_t i = 0; i < n; i++) CHECK(*F.at(i) == base + got[i], "bind: pointer %zu", i);
    F.check_sentinels();
}

// guards: the checker's pool restated with the lambda (a guard taken in front of every verdict array, one behind the last), then guard
// sizes that are no multiple of the step: the guard still ends where its array begins
static void guard_case(std::mt19937_64& rng) {
    const size_t nv = 1 + (size_t)(rng() % 8), nb = (size_t)(rng() % 6);
    const bool whole_steps = (rng() & 1) != 0;
    const size_t guard = whole_steps ? (size_t)(rng() % 3) * 256 : (size_t)(rng() % 700);
    Take T;
    std::vector<size_t> want, want_guard, sz(nv + nb);
    for (size_t& s : sz) s = random_size(rng);
    for (size_t i = 0; i < nv; i++) {
        want_guard.push_back(T.take(guard, 256));
        want.push_back(T.take(sz[i], 256));
    }
    want_guard.push_back(T.take(guard, 256));
    for (size_t i = 0; i < nb; i++) want.push_back(T.take(sz[nv + i], 256));
    Frame F(nv + nb);
    rmjh::DevLayout L;
    std::vector<size_t> got;
    for (size_t i = 0; i < nv; i++) got.push_back(L.add_guarded(F.at(i), sz[i], guard));
    const size_t tail = L.guard(guard);
    for (size_t i = 0; i < nb; i++) got.push_back(L.add(F.at(nv + i), sz[nv + i]));
    CHECK(L.bytes() == T.off, "guarded total %zu, the lambda gives %zu", L.bytes(), T.off);
    CHECK(L.guards().size() == nv + 1, "guards listed: %zu", L.guards().size());
    for (size_t i = 0; i < nv + nb; i++) CHECK(got[i] == want[i], "guarded array %zu: %zu, the lambda gives %zu", i, got[i], want[i]);
    for (size_t i = 0; i < nv; i++) {
        CHECK(L.guards()[i] + guard == got[i], "guard %zu ends at %zu, its array begins at %zu", i, L.guards()[i] + guard, got[i]);
        const size_t before = i ? got[i - 1] + sz[i - 1] : 0;
        CHECK(L.guards()[i] >= before, "guard %zu begins inside the array before it", i);
        if (whole_steps) CHECK(L.guards()[i] == want_guard[i], "guard %zu: %zu, the lambda gives %zu", i, L.guards()[i], want_guard[i]);
    }
    CHECK(L.guards()[nv] == tail && tail == want_guard[nv], "tail guard at %zu, the lambda gives %zu", tail, want_guard[nv]);
    CHECK(tail >= got[nv - 1] + sz[nv - 1], "tail guard begins inside the last verdict array");
    char* const base = (char*)(uintptr_t)0x7000000000ull;
    L.bind(base);
    for (size_t i = 0; i < nv + nb; i++) CHECK(*F.at(i) == base + want[i], "bind: pointer %zu", i);
    F.check_sentinels();
}

// ---- slot chains: start_cursors against the loop, restated over the assignment's own tables
static void chain_case(const std::vector<uint32_t>& len, const char* what) {
    const uint32_t M = (uint32_t)len.size();
    std::vector<uint32_t> off(M + 1, 0u);
    for (uint32_t l = 0; l < M; l++) off[l + 1] = off[l] + len[l];
    for (uint32_t n = 1; n <= M; n++) {
        rmjh::SlotChain C;
        C.assign(off.data(), M, n);
        // the assignment itself, from the free function, into exactly sized arrays (the sanitizer build sees a read past them)
        std::vector<uint32_t> first(n + 1), logs(M), of_log(M);
        const uint32_t steps = rmjh::lr_assign(off.data(), M, n, of_log.data(), logs.data(), first.data());
        CHECK(C.steps == steps && C.step == 0, "%s n=%u: steps %u / %u", what, n, C.steps, steps);
        CHECK(C.slot_first == first, "%s n=%u: slot_first differs", what, n);
        for (uint32_t i = 0; i < M; i++) CHECK(C.slot_logs[i] == logs[i], "%s n=%u: slot_logs[%u]", what, n, i);
        CHECK(first[0] == 0 && first[n] == M, "%s n=%u: the chains do not cover the logs", what, n);
        uint64_t longest = 0;
        for (uint32_t s = 0; s < n; s++) {
            uint64_t sum = 0;
            for (uint32_t i = first[s]; i < first[s + 1]; i++) {
                CHECK(of_log[logs[i]] == s, "%s n=%u: log %u listed in slot %u", what, n, logs[i], s);
                sum += len[logs[i]];
            }
            if (sum > longest) longest = sum;
        }
        CHECK(steps == longest, "%s n=%u: steps %u, the longest chain has %llu events", what, n, steps, (unsigned long long)longest);
        // heap arrays of exactly n words, sentinels of their own around the call
        uint32_t* pos = new uint32_t[n];
        uint32_t* cur = new uint32_t[n];
        for (uint32_t s = 0; s < n; s++) pos[s] = cur[s] = 0xDEADBEEFu;
        C.start_cursors(off.data(), pos, cur);
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t want_pos = first[s];
            uint32_t want_cur = 0u;                          // a slot left without a log
            if (first[s] < first[s + 1]) want_cur = off[logs[first[s]]];
            CHECK(pos[s] == want_pos && cur[s] == want_cur, "%s n=%u slot %u: (pos, cur) = (%u, %u), restated (%u, %u)", what, n, s, pos[s], cur[s], want_pos, want_cur);
        }
        delete[] pos;
        delete[] cur;
    }
}

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
    std::mt19937_64 rng(20240607);
    static const size_t steps[] = {4, 16, 32, 256};
    for (uint64_t i = 0; i < rounds; i++) {
        uniform_case(rng, 256);
        uniform_case(rng, steps[i & 3]);
        mixed_case(rng);
        guard_case(rng);
    }
    // the fixed lists the issue names, in order and one by one
    {
        Take T;
        rmjh::DevLayout L;
        char* p[8];
        const size_t sz[8] = {0, 1, 255, 256, 257, ((size_t)1 << 32) + 1, 0, 7};
        for (int i = 0; i < 8; i++) {
            const size_t want = T.take(sz[i], 256), got = L.add(&p[i], sz[i]);
            CHECK(got == want, "fixed list, array %d", i);
        }
        CHECK(L.bytes() == T.off && L.bytes() > ((size_t)1 << 32), "fixed list total");
    }
    // chains: logs of no events in front, behind, in runs, alone
    chain_case({0, 5, 3}, "leading");
    chain_case({5, 3, 0}, "trailing");
    chain_case({4, 0, 0, 0, 2, 7}, "run");
    chain_case({0, 0, 3, 0, 0}, "runs at both ends");
    chain_case({0, 0, 0, 0}, "only empty logs");
    chain_case({0}, "one empty log");
    chain_case({6}, "one log");
    for (uint64_t i = 0; i < rounds / 20 + 50; i++) {
        std::vector<uint32_t> len(1 + rng() % 24);
        for (uint32_t& l : len) l = (rng() % 3 == 0) ? 0u : (uint32_t)(rng() % 40);
        chain_case(len, "random");
    }
    printf("devlayout OK %llu checks\n", (unsigned long long)g_checks);
    return 0;
}
