// The shared per-record MJAI formatter (riichienv_amd/csrc/rmj_evtext.h: evt_len / evt_write, what the device formatter runs) compiled as
// host C++ and held to the host formatter (rmj_host.h: rmjh::format_event / format_events) byte for byte.  Built and run by
// tests/test_evtext_host.py, once plain and once under -fsanitize=address,undefined.
//   1. every type byte 0..255 x seat -1..4 x every tile byte 0..255 (tile, tehai, consumed and ura tiles), n_avail 1..3;
//   2. extreme deltas, n_ura / n_consumed over their limits, every flags and pad byte;
//   3. random records in random-length games: empty games, windows that start or end inside a START_KYOKU triple, unknown types.
// For every record evt_len equals the bytes evt_write writes; per record they equal format_event's text + '\n' (0 for a TEHAI, a stop
// where format_event fails), per game the restatement (sum of evt_len up to the first stop) equals format_events' offsets and bytes.
// Prints "evtext OK ..." and exits 0, or prints the first mismatches and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../riichienv_amd/csrc/rmj_evtext.h"
#include "../../riichienv_amd/csrc/rmj_host.h"

static std::mt19937_64 rng(20261015);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }
static int failures = 0;
static uint64_t n_records = 0, n_bytes = 0;

struct StrSink {
    std::string s;
    void put(char c) { s.push_back(c); }
};

static void fill_random(RmjEvent& e) {
    uint8_t* b = reinterpret_cast<uint8_t*>(&e);
    for (size_t i = 0; i < sizeof(e); i++) b[i] = (uint8_t)rng();
}
static int32_t rnd_i32() {
    static const int32_t ext[] = {0, 1, -1, 9, 10, -10, 99, 100, 25000, -25000, 999999999, 1000000000, -1000000000, 2147483647, -2147483647 - 1};
    if (rnd(3) == 0) return ext[rnd(sizeof(ext) / sizeof(ext[0]))];
    return (int32_t)(uint32_t)rng();
}

static void fail(const char* what, const RmjEvent* w, uint32_t k, int seat, const std::string& want, const std::string& got) {
    if (failures++ < 10)
        fprintf(stderr, "MISMATCH %s: type %u seat %d record %u\n  host:   [%s]\n  evtext: [%s]\n", what, w[k].type, seat, k, want.c_str(), got.c_str());
}

// one record against format_event, n = the records available from w[k] on
static void check_record(const RmjEvent* w, uint32_t k, uint32_t n, int seat) {
    n_records++;
    const int32_t len = rmjt::evt_len_at(w, k, n, seat);
    std::string want;
    int32_t want_len;
    if (w[k].type == RMJ_EV_TEHAI) want_len = 0;
    else {
        char buf[2048];
        rmjh::Out o{buf, buf + sizeof(buf), 0};
        const int used = rmjh::format_event(o, w + k, n - k, seat);
        if (used <= 0) want_len = rmjt::RMJT_STOP;
        else {
            want.assign(buf, (size_t)o.need);
            want.push_back('\n');
            want_len = (int32_t)want.size();
        }
    }
    if (len != want_len) {
        fail("evt_len", w, k, seat, want, "len " + std::to_string(len) + " want " + std::to_string(want_len));
        return;
    }
    if (len > (int32_t)rmjt::RMJT_MAX_EVENT_BYTES) fail("RMJT_MAX_EVENT_BYTES", w, k, seat, want, std::to_string(len));
    if (len <= 0) return;
    StrSink s;
    rmjt::evt_write(s, w[k], k + 1 < n ? &w[k + 1] : nullptr, k + 2 < n ? &w[k + 2] : nullptr, seat);
    if (s.s != want) fail("evt_write", w, k, seat, want, s.s);
    n_bytes += s.s.size();
}

// 1 + 2: single records (a START_KYOKU with its two TEHAI records behind it, or fewer)
static void exhaustive() {
    RmjEvent w[3];
    for (int type = 0; type < 256; type++)
        for (int tile = 0; tile < 256; tile++)
            for (int seat = -1; seat <= 4; seat++) {
                fill_random(w[0]);
                w[0].type = (uint8_t)type;
                w[0].tile = (uint8_t)tile;
                for (int i = 0; i < 4; i++) w[0].consumed[i] = (uint8_t)(rnd(2) ? tile : rng());
                for (int i = 0; i < 5; i++) w[0].ura[i] = (uint8_t)(rnd(2) ? tile : rng());
                for (int i = 0; i < 4; i++) w[0].deltas[i] = rnd_i32();
                w[0].pad = (uint8_t)(rnd(4) ? 3 + rnd(2) : rng());
                w[0].n_ura = (uint8_t)(rnd(4) ? rnd(7) : rng());
                w[0].flags = (uint8_t)rng();
                w[0].actor = (uint8_t)(rnd(4) ? rnd(5) : rng());
                for (int t = 1; t < 3; t++) {
                    fill_random(w[t]);
                    w[t].type = rnd(16) ? (uint8_t)RMJ_EV_TEHAI : (uint8_t)rng();
                    uint8_t* pl = reinterpret_cast<uint8_t*>(&w[t]) + 4;
                    for (int i = 0; i < 26; i++) pl[i] = (uint8_t)(rnd(2) ? tile : rng());
                }
                check_record(w, 0, 3, seat);
                if (type == RMJ_EV_START_KYOKU || tile < 8) {
                    check_record(w, 0, 1 + rnd(2), seat);
                }
            }
    // extremes of the counted fields, for every flags / pad / n_ura byte
    static const int32_t ext[] = {-2147483647 - 1, 2147483647, 0, -1, 1000000000, -999999999};
    for (int type = 1; type <= RMJ_EV_TEHAI; type++)
        for (int f = 0; f < 256; f++)
            for (int seat = -1; seat <= 4; seat++) {
                fill_random(w[0]);
                w[0].type = (uint8_t)type;
                w[0].flags = (uint8_t)f;
                w[0].n_ura = (uint8_t)f;
                w[0].pad = (uint8_t)(f & 7);
                w[0].actor = (uint8_t)(255 - f);
                w[0].target = (uint8_t)f;
                for (int i = 0; i < 4; i++) w[0].deltas[i] = ext[(f + i) % 6];
                for (int t = 1; t < 3; t++) {
                    fill_random(w[t]);
                    w[t].type = RMJ_EV_TEHAI;
                }
                check_record(w, 0, 3, seat);
            }
    // the longest texts: every tile a 3-character name, every score 11 characters
    for (int seat = -1; seat <= 4; seat++) {
        memset(w, 0, sizeof(w));
        w[0].type = RMJ_EV_START_KYOKU;
        w[0].tile = 255;
        w[0].consumed[1] = w[0].consumed[2] = w[0].consumed[3] = 255;
        w[0].actor = w[0].target = 255;
        for (int i = 0; i < 4; i++) w[0].deltas[i] = -2147483647 - 1;
        for (int t = 1; t < 3; t++) {
            w[t].type = RMJ_EV_TEHAI;
            memset(reinterpret_cast<uint8_t*>(&w[t]) + 4, 16, 26);
        }
        check_record(w, 0, 3, seat);
    }
}

// 3: random games through format_events and the per-record restatement
static uint8_t random_type() {
    const uint32_t r = rnd(10000);
    if (r < 5) return (uint8_t)(19 + rnd(237));   // unknown: the game's log stops
    if (r < 7) return RMJ_EV_NONE;
    if (r < 300) return RMJ_EV_TEHAI;             // a stray continuation
    if (r < 1100) return RMJ_EV_START_KYOKU;
    return (uint8_t)(1 + rnd(17));
}
static void random_games(uint64_t want_records) {
    const uint64_t r0 = n_records;   // records checked, i.e. in front of their game's stop
    int round = 0;
    while (n_records - r0 < want_records) {
        const uint32_t n_games = 1 + rnd(300);
        std::vector<RmjEvent> ev;
        std::vector<uint32_t> offs(n_games + 1);
        for (uint32_t g = 0; g < n_games; g++) {
            offs[g] = (uint32_t)ev.size();
            const uint32_t len = rnd(8) == 0 ? 0 : rnd(rnd(4) ? 200 : 1500);
            std::vector<RmjEvent> s;
            while (s.size() < len + 4) {   // a stream, then a window cut from it (starting / ending inside triples)
                RmjEvent e;
                fill_random(e);
                e.type = random_type();
                e.pad = (uint8_t)(rnd(8) ? 3 + rnd(2) : rng());
                e.n_ura = (uint8_t)(rnd(8) ? rnd(6) : rng());
                if (rnd(4) == 0) for (int i = 0; i < 4; i++) e.deltas[i] = rnd_i32();
                if (rnd(2)) e.actor = (uint8_t)rnd(4);
                if (rnd(2)) e.flags = (uint8_t)(rnd(8) | (rnd(6) << 4));
                s.push_back(e);
                if (e.type == RMJ_EV_START_KYOKU && rnd(50)) {
                    for (int t = 0; t < 2; t++) {
                        RmjEvent c;
                        fill_random(c);
                        c.type = RMJ_EV_TEHAI;
                        s.push_back(c);
                    }
                }
            }
            const uint32_t lo = rnd(4);
            ev.insert(ev.end(), s.begin() + lo, s.begin() + lo + len);
        }
        offs[n_games] = (uint32_t)ev.size();
        const int seat = (int)rnd(6) - 1;
        std::vector<uint64_t> toffs(n_games + 1);
        const uint64_t need = rmjh::format_events(ev.data(), offs.data(), n_games, seat, nullptr, 0, toffs.data(), 1 + rnd(4));
        std::vector<char> host(need + 1);
        rmjh::format_events(ev.data(), offs.data(), n_games, seat, host.data(), need, toffs.data(), 1 + rnd(4));
        // the restatement: per record sizes, each game stops at its first RMJT_STOP
        uint64_t base = 0;
        std::string text;
        for (uint32_t g = 0; g < n_games; g++) {
            if (toffs[g] != base && failures++ < 10) fprintf(stderr, "MISMATCH offsets: round %d game %u: %llu vs %llu\n", round, g,
                                                             (unsigned long long)toffs[g], (unsigned long long)base);
            const RmjEvent* w = ev.data() + offs[g];
            const uint32_t n = offs[g + 1] - offs[g];
            uint64_t sz = 0;
            for (uint32_t k = 0; k < n; k++) {
                const int32_t l = rmjt::evt_len_at(w, k, n, seat);
                if (l < 0) break;
                check_record(w, k, n, seat);
                if (l == 0) continue;
                StrSink s;
                rmjt::evt_write(s, w[k], k + 1 < n ? &w[k + 1] : nullptr, k + 2 < n ? &w[k + 2] : nullptr, seat);
                text += s.s;
                sz += (uint64_t)l;
            }
            base += sz;
        }
        if (toffs[n_games] != base || text.size() != need || memcmp(text.data(), host.data(), need) != 0) {
            if (failures++ < 10) fprintf(stderr, "MISMATCH text: round %d: %llu bytes vs %llu\n", round, (unsigned long long)need, (unsigned long long)text.size());
        }
        round++;
    }
}

int main(int argc, char** argv) {
    const uint64_t want = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000;
    exhaustive();
    const uint64_t single = n_records;
    random_games(want);
    if (failures) {
        fprintf(stderr, "evtext FAILED: %d mismatches\n", failures);
        return 1;
    }
    printf("evtext OK: %llu single records, %llu records in random games, %llu bytes written\n", (unsigned long long)single,
           (unsigned long long)(n_records - single), (unsigned long long)n_bytes);
    return 0;
}
