// zignal::Tracer of the C++ host mirror against tests/golden/tracer_cpp_paths.bin, which tests/tracer_ref.py wrote: a 48 x 64 edge map
// (rows, cols as u32, then the bytes), the restatement's [paths, points], the path offsets and the points' f32 bits. The host form and the
// device form must both return that list bit for bit; raw paths (epsilon 0) keep every pixel of a kept path; the asynchronous form
// honours its capacities. argv[1]: the fixture. Needs a GPU: built and run by tests/test_cpp_tracer.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool same(const std::vector<Tracer::Path> &got, const std::vector<uint32_t> &offsets, const std::vector<float> &points) {
    if (got.size() + 1 != offsets.size()) return false;
    for (size_t i = 0; i < got.size(); ++i) {
        if (got[i].size() != offsets[i + 1] - offsets[i]) return false;
        if (std::memcmp(got[i].data(), &points[2 * (size_t)offsets[i]], got[i].size() * 8)) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t shape[2], counts[2];
    EXPECT(std::fread(shape, 4, 2, f) == 2);
    Image<uint8_t> edges = Image<uint8_t>::init(shape[0], shape[1]);
    EXPECT(std::fread(edges.data, 1, (size_t)shape[0] * shape[1], f) == (size_t)shape[0] * shape[1]);
    EXPECT(std::fread(counts, 4, 2, f) == 2);
    std::vector<uint32_t> offsets((size_t)counts[0] + 1);
    std::vector<float> points(2 * (size_t)counts[1]);
    EXPECT(std::fread(offsets.data(), 4, offsets.size(), f) == offsets.size());
    EXPECT(std::fread(points.data(), 4, points.size(), f) == points.size());
    std::fclose(f);
    EXPECT(counts[0] >= 4 && offsets.back() == counts[1]);

    check(zg_init(0));
    const Tracer tracer;
    EXPECT(same(tracer.trace(edges), offsets, points));

    Stream stream = Stream::create();
    DeviceImage<uint8_t> dev = DeviceImage<uint8_t>::init(shape[0], shape[1], stream.handle());
    check(zg_memcpy_h2d(dev.data, edges.data, (size_t)shape[0] * shape[1], stream.handle()));
    EXPECT(same(tracer.trace(dev), offsets, points));

    // raw paths: every pixel of every kept path, each once, 8-adjacent from point to point
    Tracer raw;
    raw.simplification_epsilon = 0.0f;
    raw.min_path_length = 1;
    size_t edge_pixels = 0, raw_points = 0;
    for (size_t i = 0; i < (size_t)shape[0] * shape[1]; ++i) edge_pixels += edges.data[i] > 0;
    for (const Tracer::Path &p : raw.trace(dev)) {
        raw_points += p.size();
        for (size_t i = 0; i < p.size(); ++i) {
            EXPECT(edges.at((uint32_t)p[i].y, (uint32_t)p[i].x) > 0);
            if (i) EXPECT(std::fabs(p[i].x - p[i - 1].x) <= 1.0f && std::fabs(p[i].y - p[i - 1].y) <= 1.0f);
        }
    }
    EXPECT(raw_points == edge_pixels);

    // the asynchronous form with room for two paths: two whole paths, the full need in counts[0..1]
    void *mem = nullptr;
    check(zg_malloc(&mem, 4096));
    Point2 *dpoints = (Point2 *)mem;
    uint32_t *doffsets = (uint32_t *)((char *)mem + 2048), *dcounts = doffsets + 16, got[4], got_offsets[3];
    tracer.traceInto(dev, dpoints, 256, doffsets, 2, dcounts);
    check(zg_memcpy_d2h(got, dcounts, 16, stream.handle()));
    check(zg_memcpy_d2h(got_offsets, doffsets, 12, stream.handle()));
    EXPECT(got[0] == counts[0] && got[1] == counts[1] && got[2] == 2 && got[3] == offsets[2]);
    EXPECT(std::memcmp(got_offsets, offsets.data(), 12) == 0);
    check(zg_free(mem));

    if (failures) { std::printf("cpp tracer: %d failure(s)\n", failures); return 1; }
    std::printf("cpp tracer ok\n");
    return 0;
}
