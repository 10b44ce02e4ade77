// zignal::BruteForceMatcher, Match and MatchStats of the C++ host mirror against the reference's loops (src/features/matcher.zig:44-233)
// written out here: the reference's own unit tests (:273-413), then host and device forms on clustered descriptors, whole lists
// compared. Needs a GPU: built and run by tests/test_cpp_match.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static void setBit(BinaryDescriptor &d, int i) { d.bits[i / 8] |= (uint8_t)(1u << (i % 8)); }
static uint32_t hamming(const BinaryDescriptor &a, const BinaryDescriptor &b) {
    uint32_t n = 0;
    for (int i = 0; i < 32; ++i) n += (uint32_t)__builtin_popcount((unsigned)(a.bits[i] ^ b.bits[i]));
    return n;
}
static bool same(const std::vector<Match> &a, const std::vector<Match> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Match)) == 0);
}

// matcher.zig:44-106, :214-233
static std::vector<Match> refMatch(const BruteForceMatcher &m, const std::vector<BinaryDescriptor> &q, const std::vector<BinaryDescriptor> &t) {
    std::vector<Match> out;
    if (q.empty() || t.empty()) return out;
    for (size_t qi = 0; qi < q.size(); ++qi) {
        uint32_t best = 0xFFFFFFFFu, second = 0xFFFFFFFFu;
        size_t best_idx = 0;
        for (size_t ti = 0; ti < t.size(); ++ti) {
            const uint32_t d = hamming(q[qi], t[ti]);
            if (d < best) { second = best; best = d; best_idx = ti; }
            else if (d < second) second = d;
        }
        if (!(best <= m.max_distance && (second == 0xFFFFFFFFu || (float)best < m.ratio_threshold * (float)second))) continue;
        if (m.cross_check) {
            uint32_t rb = 0xFFFFFFFFu;
            size_t ri = 0;
            for (size_t k = 0; k < q.size(); ++k) {
                const uint32_t d = hamming(t[best_idx], q[k]);
                if (d < rb) { rb = d; ri = k; }
            }
            if (ri != qi) continue;
        }
        out.push_back(Match{(uint32_t)qi, (uint32_t)best_idx, (float)best});
    }
    return out;
}
// :109-162 and :165-212; std::stable_sort keeps equal distances in train order, as the reference's sort does
static std::vector<std::vector<Match>> refRows(const std::vector<BinaryDescriptor> &q, const std::vector<BinaryDescriptor> &t, size_t k, float limit, bool radius) {
    std::vector<std::vector<Match>> out;
    if (q.empty() || t.empty() || (!radius && k == 0)) return out;
    for (size_t qi = 0; qi < q.size(); ++qi) {
        std::vector<Match> row;
        for (size_t ti = 0; ti < t.size(); ++ti) {
            const float d = (float)hamming(q[qi], t[ti]);
            if (!radius || d <= limit) row.push_back(Match{(uint32_t)qi, (uint32_t)ti, d});
        }
        std::stable_sort(row.begin(), row.end(), [](const Match &a, const Match &b) { return a.distance < b.distance; });
        if (!radius) {
            row.resize(std::min(k, row.size()));
            std::vector<Match> kept;
            for (const Match &m : row) if (m.distance <= limit) kept.push_back(m);
            row = kept;
        }
        out.push_back(row);
    }
    return out;
}
static bool sameRows(const std::vector<std::vector<Match>> &a, const std::vector<std::vector<Match>> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (!same(a[i], b[i])) return false;
    return true;
}

// train: random, with copies and near copies of earlier entries; queries: train entries with 0 .. 90 bits flipped, or random
static void clustered(size_t nq, size_t nt, std::vector<BinaryDescriptor> &q, std::vector<BinaryDescriptor> &t) {
    static const int flips[8] = {0, 3, 10, 30, 60, 64, 65, 90};
    t.assign(nt, BinaryDescriptor{});
    q.assign(nq, BinaryDescriptor{});
    for (size_t i = 0; i < nt; ++i) {
        for (int b = 0; b < 32; ++b) t[i].bits[b] = (uint8_t)(rnd() >> 24);
        if (i > 0 && rnd() % 10 == 0) {
            t[i] = t[rnd() % i];
            if (rnd() % 2) for (int f = (int)(rnd() % 39) + 1; f > 0; --f) t[i].bits[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
    }
    for (size_t i = 0; i < nq; ++i) {
        for (int b = 0; b < 32; ++b) q[i].bits[b] = (uint8_t)(rnd() >> 24);
        if (rnd() % 5 != 0) {
            q[i] = t[rnd() % nt];
            for (int f = flips[rnd() % 8]; f > 0; --f) q[i].bits[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
        if (i > 0 && rnd() % 10 == 0) q[i] = q[rnd() % i];
    }
}

int main() {
    if (zg_init(0) != ZG_OK) { std::printf("no gfx950 device: %s\n", zg_last_error()); return 77; }

    { // matcher.zig:273-313 "BruteForceMatcher basic matching"
        std::vector<BinaryDescriptor> a(2), b(2);
        setBit(a[0], 0); setBit(a[0], 10); setBit(a[1], 5); setBit(a[1], 15);
        setBit(b[0], 0); setBit(b[0], 11); setBit(b[1], 100); setBit(b[1], 200);
        BruteForceMatcher m;
        m.max_distance = 100;
        const auto got = m.match(a, b);
        EXPECT(!got.empty() && got[0].query_idx == 0 && got[0].train_idx == 0);
        EXPECT(same(got, refMatch(m, a, b)));
    }
    { // :315-358 "BruteForceMatcher cross-check"
        std::vector<BinaryDescriptor> a(2), b(2);
        setBit(a[0], 0); setBit(b[0], 0);
        for (int i = 0; i < 100; ++i) setBit(a[1], i);
        for (int i = 100; i < 200; ++i) setBit(b[1], i);
        BruteForceMatcher plain, cross;
        plain.max_distance = cross.max_distance = 256;
        cross.cross_check = true;
        EXPECT(cross.match(a, b).size() <= plain.match(a, b).size());
        EXPECT(same(cross.match(a, b), refMatch(cross, a, b)) && same(plain.match(a, b), refMatch(plain, a, b)));
    }
    { // :360-398 "BruteForceMatcher kNN matching"
        std::vector<BinaryDescriptor> q(1), t(3);
        setBit(q[0], 0);
        setBit(t[0], 1); setBit(t[1], 1); setBit(t[1], 2); setBit(t[2], 1); setBit(t[2], 2); setBit(t[2], 3);
        const auto rows = BruteForceMatcher().knnMatch(q, t, 2);
        EXPECT(rows.size() == 1 && rows[0].size() == 2 && rows[0][0].distance == 2.0f && rows[0][1].distance == 3.0f && rows[0][0].train_idx == 0);
    }
    { // :400-413 "MatchStats computation", and the empty list
        const std::vector<Match> ms = {{0, 0, 10.0f}, {1, 1, 20.0f}, {2, 2, 30.0f}};
        const MatchStats s = MatchStats::compute(ms);
        EXPECT(s.total_matches == 3 && s.mean_distance == 20.0f && s.min_distance == 10.0f && s.max_distance == 30.0f);
        const MatchStats e = MatchStats::compute({});
        EXPECT(e.total_matches == 0 && e.mean_distance == 0.0f && e.min_distance == 0.0f && e.max_distance == 0.0f);
    }

    const size_t shapes[][2] = {{1, 1}, {65, 129}, {200, 513}, {300, 257}};
    for (const auto &shape : shapes) {
        std::vector<BinaryDescriptor> q, t;
        clustered(shape[0], shape[1], q, t);
        for (int cross = 0; cross < 2; ++cross) {
            for (float ratio : {0.8f, 2.0f}) {
                BruteForceMatcher m;
                m.cross_check = cross != 0;
                m.ratio_threshold = ratio;
                const auto want = refMatch(m, q, t);
                EXPECT(same(m.match(q, t), want));
                // the device form on a query buffer with room to spare and a device count word
                const uint32_t nq = (uint32_t)q.size(), nt = (uint32_t)t.size(), cq = nq + 7;
                void *mem = nullptr;
                const size_t qb = (size_t)cq * 32, tb = (size_t)nt * 32, mb = (size_t)cq * sizeof(Match);
                check(zg_malloc(&mem, qb + tb + mb + 8));
                char *base = (char *)mem;
                std::vector<BinaryDescriptor> padded(cq, q[0]); // the tail would match if it were read
                std::copy(q.begin(), q.end(), padded.begin());
                check(zg_memcpy_h2d(base, padded.data(), qb, nullptr));
                check(zg_memcpy_h2d(base + qb, t.data(), tb, nullptr));
                check(zg_memcpy_h2d(base + qb + tb + mb, &nq, 4, nullptr));
                uint32_t *dcount = (uint32_t *)(base + qb + tb + mb + 4);
                m.matchInto({(const BinaryDescriptor *)base, cq, (const uint32_t *)(base + qb + tb + mb)}, {(const BinaryDescriptor *)(base + qb), nt},
                            (Match *)(base + qb + tb), cq, dcount);
                uint32_t n = 0;
                check(zg_memcpy_d2h(&n, dcount, 4, nullptr));
                std::vector<Match> got(std::min(n, cq));
                if (!got.empty()) check(zg_memcpy_d2h(got.data(), base + qb + tb, got.size() * sizeof(Match), nullptr));
                EXPECT(n == want.size() && same(got, want));
                check(zg_free(mem));
            }
        }
        BruteForceMatcher m;
        for (size_t k : {(size_t)1, (size_t)3, t.size() + 2}) EXPECT(sameRows(m.knnMatch(q, t, k), refRows(q, t, k, (float)m.max_distance, false)));
        for (float r : {0.0f, 40.0f, 64.5f}) EXPECT(sameRows(m.radiusMatch(q, t, r), refRows(q, t, 0, r, true)));
        const auto ms = m.match(q, t);
        const MatchStats s = MatchStats::compute(ms);
        float sum = 0.0f;
        for (const Match &x : ms) sum += x.distance;
        EXPECT(s.total_matches == ms.size() && (ms.empty() || s.mean_distance == sum / (float)ms.size()));
    }
    EXPECT(BruteForceMatcher().match({}, {}).empty() && BruteForceMatcher().knnMatch({}, {}, 2).empty() && BruteForceMatcher().radiusMatch({}, {}, 1.0f).empty());

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("cpp match ok\n");
    return 0;
}
