// zignal_amd/csrc/zg_tracer_step.h on the CPU (tests/test_tracer_step_host.py builds this with g++ -fsanitize=address,undefined,
// -D__host__= -D__device__= -ffp-contract=off). argv[1]: tests/golden/tracer_step_dist.bin, records of eight little-endian words
// (px py ax ay bx by as i32, the distance's f32 bits, which return). Standard input, from tests/golden/tracer_step.json:
//   "C prev_k mask want"   tracer_choose(prev_k, mask) == want
//   "S prev_k k bits"      the bits of tracer_score(prev_k, k)
// Prints "tracer step ok <lines> <records>" when everything matched.
#include "../../zignal_amd/csrc/zg_tracer_step.h"

#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// which of distanceToSegment's returns a triple takes, decided as the header decides it
static int which_return(float px, float py, float ax, float ay, float bx, float by) {
    const float abx = bx - ax, aby = by - ay, apx = px - ax, apy = py - ay;
    const float ab_len_sq = abx * abx + aby * aby;
    if (ab_len_sq == 0.0f) return 0;
    const float t = (apx * abx + apy * aby) / ab_len_sq;
    return t <= 0.0f ? 1 : (t >= 1.0f ? 2 : 3);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> rec;
    uint32_t w[8];
    while (std::fread(w, 4, 8, f) == 8) rec.insert(rec.end(), w, w + 8);
    std::fclose(f);
    int seen[4] = {0, 0, 0, 0};
    const size_t records = rec.size() / 8;
    for (size_t i = 0; i < records; ++i) {
        int32_t v[6];
        std::memcpy(v, &rec[8 * i], sizeof v);
        const float d = zg::tracer_distance_to_segment((float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5]);
        const int which = which_return((float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5]);
        if (bits_of(d) != rec[8 * i + 6] || (uint32_t)which != rec[8 * i + 7]) {
            std::printf("distance record %zu: got %08x return %d, want %08x return %u\n", i, bits_of(d), which, rec[8 * i + 6], rec[8 * i + 7]);
            return 1;
        }
        seen[which]++;
    }
    if (!(seen[0] && seen[1] && seen[2] && seen[3])) {
        std::printf("a return of distanceToSegment was never taken: %d %d %d %d\n", seen[0], seen[1], seen[2], seen[3]);
        return 1;
    }
    size_t lines = 0;
    char kind;
    int a, b;
    unsigned c;
    while (std::scanf(" %c %d %d %x", &kind, &a, &b, &c) == 4) {
        if (kind == 'C') {
            const int got = zg::tracer_choose(a, (uint32_t)b);
            if (got != (int)c - 1) { // the wanted neighbour travels as want + 1
                std::printf("choose(%d, %02x): got %d, want %d\n", a, b, got, (int)c - 1);
                return 1;
            }
        } else if (kind == 'S') {
            const uint32_t got = bits_of(zg::tracer_score(a, b));
            if (got != c) {
                std::printf("score(%d, %d): got %08x, want %08x\n", a, b, got, c);
                return 1;
            }
        } else {
            return 2;
        }
        ++lines;
    }
    for (int k = 0; k < 8; ++k) {
        static const int want[8][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
        if (zg::tracer_drow(k) != want[k][0] || zg::tracer_dcol(k) != want[k][1]) {
            std::printf("offset %d\n", k);
            return 1;
        }
    }
    std::printf("tracer step ok %zu %zu\n", lines, records);
    return 0;
}
