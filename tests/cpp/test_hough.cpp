// zignal::HoughTransform of the C++ host mirror against the reference's loops (src/image/hough.zig:75-257) written out here: the
// reference's own unit test (:259-285), then random edges in a box past the image's edge and the pure tie-order accumulator, whole
// accumulators and line lists compared byte for byte. @sin / @cos of an f32 are the one thing this file cannot restate, so the
// reference lines take their end points from the library and compare angle, radius and score; the end points are compared against
// tests/hough_ref.py by the Python tests. Needs a GPU: built and run by tests/test_cpp_hough.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

// hough.zig:75-139 with the tables the library made (tests/test_hough_oracle.py compares those with the restated init)
static void refCompute(uint32_t size, const std::vector<int32_t> &cos_t, const std::vector<int32_t> &sin_t, const Image<uint8_t> &edges,
                       const Rectangle<uint32_t> &box, std::vector<uint32_t> &acc) {
    const uint32_t even = size % 2 == 0 ? size : size - 1;
    const uint32_t ar = std::min(box.r, edges.cols), ab = std::min(box.b, edges.rows);
    if (box.l >= ar || box.t >= ab) return;
    const int32_t size_minus_one = (int32_t)size - 1, offset = (int32_t)std::lround(65536.0 * (double)even / 4.0);
    for (uint32_t r = box.t; r < ab; ++r) {
        const int32_t y_val = 2 * ((int32_t)r - (int32_t)box.t) - size_minus_one;
        for (uint32_t c = box.l; c < ar; ++c) {
            if (edges.data[(size_t)r * edges.stride + c] == 0) continue;
            const int32_t x_val = 2 * ((int32_t)c - (int32_t)box.l) - size_minus_one;
            for (uint32_t t = 0; t < size; ++t) {
                const int32_t rho = x_val * cos_t[t] + y_val * sin_t[t];
                const int32_t rr = ((rho >> 1) + (offset << 1)) >> 16;
                if (rr >= 0 && rr < (int32_t)size) acc[(size_t)rr * size + t] += 1;
            }
        }
    }
}

struct RefLine { float angle, radius; uint32_t score; };
// hough.zig:142-212 up to the kept candidates
static std::vector<RefLine> refFind(uint32_t size, const std::vector<uint32_t> &acc, uint32_t threshold, float a_thr, float r_thr, size_t *candidates) {
    std::vector<RefLine> lines, kept;
    *candidates = 0;
    if (size < 3) return kept;
    const uint32_t even = size % 2 == 0 ? size : size - 1;
    const float center = (float)(size - 1) / 2.0f;
    for (uint32_t r = 1; r + 1 < size; ++r)
        for (uint32_t c = 1; c + 1 < size; ++c) {
            const uint32_t votes = acc[(size_t)r * size + c];
            if (votes < threshold) continue;
            bool is_max = true;
            for (uint32_t nr = r - 1; nr < r + 2 && is_max; ++nr)
                for (uint32_t nc = c - 1; nc < c + 2; ++nc)
                    if (acc[(size_t)nr * size + nc] > votes) { is_max = false; break; }
            if (!is_max) continue;
            volatile float angle = 180.0f * ((float)c - center) / (float)even; // volatile: one rounding an operation, whatever the compiler's flags
            volatile float radius = ((float)r - center) * std::sqrt(2.0f);
            lines.push_back(RefLine{angle, radius, votes});
        }
    *candidates = lines.size();
    std::stable_sort(lines.begin(), lines.end(), [](const RefLine &a, const RefLine &b) { return a.score > b.score; });
    for (const RefLine &cand : lines) {
        bool too_close = false;
        for (const RefLine &e : kept) {
            const float da = std::fabs(e.angle - cand.angle), dr = std::fabs(e.radius - cand.radius);
            if ((da < a_thr && dr < r_thr) || ((180.0f - da) < a_thr && std::fabs(e.radius + cand.radius) < r_thr)) { too_close = true; break; }
        }
        if (!too_close) kept.push_back(cand);
    }
    return kept;
}

static bool sameLines(const std::vector<HoughTransform::Line> &got, const std::vector<RefLine> &want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); ++i)
        if (std::memcmp(&got[i].angle, &want[i].angle, 4) || std::memcmp(&got[i].radius, &want[i].radius, 4) || got[i].score != want[i].score) return false;
    return true;
}

static void expectThrowsInvalid(uint32_t size) {
    bool thrown = false;
    try { HoughTransform h(size); } catch (const InvalidArgument &) { thrown = true; }
    EXPECT(thrown);
}

int main() {
    check(zg_init(0));
    // "HoughTransform: invalid size" (:281-285)
    expectThrowsInvalid(0);
    expectThrowsInvalid(1);

    // "HoughTransform: detect horizontal line" (:259-279)
    {
        const uint32_t size = 64;
        Image<uint8_t> edges = Image<uint8_t>::init(size, size);
        std::memset(edges.data, 0, (size_t)size * size);
        for (uint32_t c = 0; c < size; ++c) edges.data[32 * size + c] = 255;
        HoughTransform hough(size);
        Image<uint32_t> acc = Image<uint32_t>::init(size, size);
        std::memset(acc.data, 0, (size_t)size * size * 4);
        hough.compute(edges, Rectangle<uint32_t>{0, 0, size, size}, acc);
        uint64_t sum = 0;
        for (size_t i = 0; i < (size_t)size * size; ++i) sum += acc.data[i];
        EXPECT(sum == 4096);
        const std::vector<HoughTransform::Line> lines = hough.findLines(acc, 30, 10.0f, 5.0f);
        EXPECT(lines.size() >= 1 && std::fabs(lines[0].angle) <= 2.0f);
        EXPECT(lines.size() == 1 && lines[0].angle == 1.40625f && lines[0].radius == 0.70710677f && lines[0].score == 64);
        EXPECT(lines[0].p1[0] == 0.0f && lines[0].p2[0] == 64.0f);
        bool thrown = false;
        try { hough.compute(edges, Rectangle<uint32_t>{0, 0, size, size + 1}, acc); } catch (const DimensionMismatch &) { thrown = true; }
        EXPECT(thrown);
    }

    // random edges, the box past the right and bottom edge, a non-zero start; host form and device form
    for (uint32_t size : {5u, 33u, 64u, 97u}) {
        const uint32_t rows = size + 7, cols = size + 3;
        Image<uint8_t> edges = Image<uint8_t>::init(rows, cols);
        for (size_t i = 0; i < (size_t)rows * cols; ++i) edges.data[i] = rnd() % 16 == 0 ? (uint8_t)(1 + rnd() % 255) : 0;
        const Rectangle<uint32_t> box{5, 9, 5 + size, 9 + size};
        std::vector<int32_t> cos_t, sin_t;
        HoughTransform::tables(size, cos_t, sin_t);
        HoughTransform hough(size, cos_t, sin_t);
        std::vector<uint32_t> want((size_t)size * size);
        for (uint32_t &v : want) v = rnd() % 3;
        Image<uint32_t> acc = Image<uint32_t>::init(size, size);
        std::memcpy(acc.data, want.data(), want.size() * 4);
        refCompute(size, cos_t, sin_t, edges, box, want);
        hough.compute(edges, box, acc);
        EXPECT(std::memcmp(acc.data, want.data(), want.size() * 4) == 0);

        const uint32_t threshold = std::max(1u, *std::max_element(want.begin(), want.end()) / 2);
        size_t candidates = 0;
        const std::vector<RefLine> kept = refFind(size, want, threshold, 5.0f, 5.0f, &candidates);
        const std::vector<HoughTransform::Line> lines = hough.findLines(acc, threshold, 5.0f, 5.0f);
        EXPECT(sameLines(lines, kept));

        // the device forms on a stream of their own
        Stream stream = Stream::create();
        DeviceImage<uint8_t> dedges = DeviceImage<uint8_t>::init(rows, cols, stream.handle());
        check(zg_memcpy_h2d(dedges.data, edges.data, (size_t)rows * cols, stream.handle()));
        void *mem = nullptr;
        const size_t acc_b = (size_t)size * size * 4, lines_b = (kept.size() + 1) * sizeof(HoughTransform::Line);
        check(zg_malloc(&mem, acc_b + lines_b + 16));
        uint32_t *dacc = (uint32_t *)mem;
        HoughTransform::Line *dlines = (HoughTransform::Line *)((char *)mem + acc_b);
        uint32_t *dcounts = (uint32_t *)((char *)mem + acc_b + lines_b);
        std::vector<uint32_t> zeros((size_t)size * size, 0), got((size_t)size * size);
        check(zg_memcpy_h2d(dacc, zeros.data(), acc_b, stream.handle()));
        hough.computeInto(dedges, box, dacc, size, stream.handle());
        hough.computeInto(dedges, box, dacc, size, stream.handle()); // adds: twice the votes
        check(zg_memcpy_d2h(got.data(), dacc, acc_b, stream.handle()));
        std::vector<uint32_t> twice((size_t)size * size, 0);
        refCompute(size, cos_t, sin_t, edges, box, twice);
        refCompute(size, cos_t, sin_t, edges, box, twice);
        EXPECT(got == twice);
        check(zg_memcpy_h2d(dacc, want.data(), acc_b, stream.handle()));
        hough.findLinesInto(dacc, size, threshold, nullptr, 5.0f, 5.0f, 65536, dlines, (uint32_t)kept.size() + 1, dcounts, stream.handle());
        uint32_t counts[2] = {0, 0};
        std::vector<HoughTransform::Line> dl(kept.size());
        check(zg_memcpy_d2h(counts, dcounts, 8, stream.handle()));
        if (!dl.empty()) check(zg_memcpy_d2h(dl.data(), dlines, dl.size() * sizeof(HoughTransform::Line), stream.handle()));
        EXPECT(counts[0] == candidates && counts[1] == kept.size());
        EXPECT(dl.size() == lines.size() && (dl.empty() || std::memcmp(dl.data(), lines.data(), dl.size() * sizeof(HoughTransform::Line)) == 0));
        check(zg_free(mem));
    }

    // the pure tie-order case: 49 candidates of score 0, 14 lines
    {
        HoughTransform hough(9);
        Image<uint32_t> acc = Image<uint32_t>::init(9, 9);
        std::memset(acc.data, 0, 81 * 4);
        size_t candidates = 0;
        const std::vector<RefLine> kept = refFind(9, std::vector<uint32_t>(81, 0), 0, 10.0f, 5.0f, &candidates);
        const std::vector<HoughTransform::Line> lines = hough.findLines(acc, 0, 10.0f, 5.0f);
        EXPECT(candidates == 49 && kept.size() == 14 && sameLines(lines, kept));
        EXPECT(hough.findLines(acc, 0, NAN, 5.0f).size() == 49 && hough.findLines(acc, 0, -1.0f, -1.0f).size() == 49);
    }

    if (failures) { std::printf("cpp hough: %d failure(s)\n", failures); return 1; }
    std::printf("cpp hough ok\n");
    return 0;
}
