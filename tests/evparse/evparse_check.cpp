// Host check of the shared line parser (riichienv_amd/csrc/rmj_evparse.h) - driven by tests/test_evparse_host.py.
//   evparse_check <corpus> <out>
// corpus: u32 n, then per line { u32 len, u8 num_players, u8 masked_ok, u8 pad[2], bytes[len] }.  Every line is copied into a heap block
// of exactly its length before it is parsed, so AddressSanitizer sees any read outside [p, p + len).
// out: per line { RmjEvent recs[3] (96 bytes), rmjp::Side (40 bytes) }.
// pad[0] = 1 marks the first line of a log: <out>.tables receives, per log, { u32 n_kyokus, u32 status, n_kyokus x { i32 start[4], i32 end[4] } } from
// rmjp::KyokuWalk over the side structs of the log's lines (the walk the device's table kernel runs).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../riichienv_amd/csrc/rmj_evparse.h"

static_assert(sizeof(RmjEvent) == 32, "RmjEvent is 32 bytes");
static_assert(sizeof(rmjp::Side) == 40, "Side is 40 bytes");

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    if (buf.size() < 4) return 2;
    uint32_t n;
    memcpy(&n, buf.data(), 4);
    size_t at = 4;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    size_t ok = 0;
    FILE* t = fopen((std::string(argv[2]) + ".tables").c_str(), "wb");
    if (!t) return 2;
    rmjp::KyokuWalk walk;
    std::vector<int32_t> rows;
    bool in_log = false;
    auto flush = [&]() {
        if (!in_log) return;
        int32_t s[4], e[4];
        if (walk.finish(s, e)) { rows.insert(rows.end(), s, s + 4); rows.insert(rows.end(), e, e + 4); }
        const uint32_t head[2] = {(uint32_t)(rows.size() / 8), walk.st};
        fwrite(head, 4, 2, t);
        fwrite(rows.data(), 4, rows.size(), t);
        rows.clear();
        walk = rmjp::KyokuWalk();
    };
    for (uint32_t i = 0; i < n; i++) {
        if (at + 8 > buf.size()) return 3;
        uint32_t len;
        memcpy(&len, buf.data() + at, 4);
        const uint32_t np = buf[at + 4];
        const bool masked = buf[at + 5] != 0;
        if (buf[at + 6]) { flush(); in_log = true; }
        at += 8;
        if (at + len > buf.size()) return 3;
        uint8_t* line = (uint8_t*)malloc(len ? len : 1);   // exact size (a zero-length line gets a block it must not read)
        if (len) memcpy(line, buf.data() + at, len);
        at += len;
        RmjEvent recs[3];
        rmjp::Side side;
        memset(recs, 0xAB, sizeof(recs));
        memset(&side, 0xAB, sizeof(side));
        const uint8_t st = len ? rmjp::parse_line(line, len, np, masked, recs, &side) : rmjp::parse_line(line + 1, 0, np, masked, recs, &side);
        free(line);
        if (st != side.status) return 4;
        ok += st == RMJ_LOGTEXT_OK;
        fwrite(recs, 1, sizeof(recs), o);
        fwrite(&side, 1, sizeof(side), o);
        if (in_log) {
            int32_t s[4], e[4];
            if (st != RMJ_LOGTEXT_OK) walk.fail(st);
            else if (walk.feed(side, s, e)) { rows.insert(rows.end(), s, s + 4); rows.insert(rows.end(), e, e + 4); }
        }
    }
    flush();
    fclose(t);
    fclose(o);
    printf("evparse OK %u lines %zu parsed\n", n, ok);
    return 0;
}
