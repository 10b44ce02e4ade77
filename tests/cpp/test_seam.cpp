// Image<T>::seamCarve and DeviceImage<T>::seamCarve of the C++ host mirror against the example's loops (examples/src/seam_carving.zig:22-102)
// written out here: computeEnergy with its clamp at `cols` and its skip at -1, computeSeam with its strict compares in the order left,
// centre, right, removeSeam. The edge map of every iteration comes from the library's own sobel (held to the oracle by the Python
// suite), so this program checks the part that is new: the staged C entry points against the loops, the host and device forms of the
// iteration against the staged calls, both axes, seams compared with the frames. Needs a GPU: built and run by tests/test_cpp_seam.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static std::vector<uint32_t> refEnergy(const Image<uint8_t> &edges) {
    const int64_t rows = edges.rows, cols = edges.cols;
    std::vector<uint32_t> energy((size_t)rows * cols);
    for (int64_t c = 0; c < cols; ++c) energy[c] = edges.at(0, c);
    for (int64_t r = 1; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) {
            uint32_t least = 0xffffffffu;
            for (int64_t i = -1; i <= 1; ++i) {
                int64_t x = c + i;
                if (x == cols) x = cols - 1;
                if (x < 0) continue; // atOrNull
                const uint32_t val = energy[(size_t)((r - 1) * cols + x)];
                if (val < least) least = val;
            }
            energy[(size_t)(r * cols + c)] = edges.at(r, c) + least;
        }
    return energy;
}

static std::vector<uint32_t> refSeam(const std::vector<uint32_t> &energy, int64_t rows, int64_t cols) {
    std::vector<uint32_t> seam((size_t)rows);
    const int64_t row = rows - 1;
    seam[row] = 0;
    for (int64_t c = 0; c < cols; ++c)
        if (energy[(size_t)(row * cols + c)] < energy[(size_t)(row * cols + seam[row])]) seam[row] = (uint32_t)c;
    for (int64_t y = rows - 2; y >= 0; --y) {
        seam[y] = seam[y + 1];
        for (int64_t i = -1; i <= 1; ++i) {
            int64_t x = (int64_t)seam[y + 1] + i;
            if (x == cols) x = cols - 1;
            if (x < 0) continue;
            if (energy[(size_t)(y * cols + x)] < energy[(size_t)(y * cols + seam[y])]) seam[y] = (uint32_t)x;
        }
    }
    return seam;
}

template <typename T> static Image<T> refRemove(const Image<T> &image, const std::vector<uint32_t> &seam) {
    Image<T> out = Image<T>::init(image.rows, image.cols - 1);
    for (uint32_t r = 0; r < image.rows; ++r)
        for (uint32_t c = 0, o = 0; c < image.cols; ++c)
            if (c != seam[r]) out.at(r, o++) = image.at(r, c);
    return out;
}

template <typename T> static bool sameBytes(const Image<T> &a, const Image<T> &b) {
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (uint32_t r = 0; r < a.rows; ++r)
        if (std::memcmp(&a.at(r, 0), &b.at(r, 0), (size_t)a.cols * sizeof(T))) return false;
    return true;
}

template <typename T> static Image<T> transposed(const Image<T> &a) {
    Image<T> t = Image<T>::init(a.cols, a.rows);
    for (uint32_t r = 0; r < a.rows; ++r)
        for (uint32_t c = 0; c < a.cols; ++c) t.at(c, r) = a.at(r, c);
    return t;
}

static void value(uint8_t &p, uint32_t v) { p = (uint8_t)v; }
static void value(Rgba<uint8_t> &p, uint32_t v) { p = {(uint8_t)v, (uint8_t)(v >> 3), (uint8_t)(255 - v), (uint8_t)(v | 1)}; }
static void value(Rgb<float> &p, uint32_t v) { p = {(float)v / 255.0f, (float)(v & 63) / 64.0f, 0.5f}; }

// blocks of a few levels with noise on top: edges of every strength, and flat stretches where the sums tie
template <typename T> static Image<T> frame(uint32_t rows, uint32_t cols) {
    Image<T> img = Image<T>::init(rows, cols);
    std::vector<uint32_t> coarse((size_t)(rows / 5 + 1) * (cols / 7 + 1));
    for (uint32_t &v : coarse) v = (rnd() >> 8) % 4 * 60;
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t c = 0; c < cols; ++c) value(img.at(r, c), coarse[(size_t)(r / 5) * (cols / 7 + 1) + c / 7] + ((rnd() >> 8) % 8 == 0 ? (rnd() >> 8) % 16 : 0));
    return img;
}

// n iterations through the loops above, the edge map from the library's host sobel
template <typename T> static Image<T> refCarve(const Image<T> &src, uint32_t n, std::vector<uint32_t> &seams) {
    Image<T> cur = src;
    seams.clear();
    for (uint32_t k = 0; k < n; ++k) {
        const Image<uint8_t> edges = cur.sobel();
        const std::vector<uint32_t> energy = refEnergy(edges);
        // the staged entry points, host forms, against the loops
        std::vector<uint32_t> got_energy(energy.size()), got_seam(cur.rows);
        const zg_image e = edges.desc();
        check(zg_seam_energy_host(&e, got_energy.data()));
        EXPECT(got_energy == energy);
        const std::vector<uint32_t> seam = refSeam(energy, cur.rows, cur.cols);
        check(zg_seam_find_host(got_energy.data(), cur.rows, cur.cols, got_seam.data()));
        EXPECT(got_seam == seam);
        Image<T> next = refRemove(cur, seam);
        Image<T> got_next = Image<T>::init(cur.rows, cur.cols - 1);
        const zg_image s = cur.desc(), d = got_next.desc();
        check(zg_seam_remove_host(&s, seam.data(), &d));
        EXPECT(sameBytes(got_next, next));
        seams.insert(seams.end(), seam.begin(), seam.end());
        cur = next;
    }
    return cur;
}

template <typename T> static void carve(uint32_t rows, uint32_t cols, uint32_t n) {
    const Image<T> src = frame<T>(rows, cols);
    const Image<T> keep = src;
    std::vector<uint32_t> want_seams;
    const Image<T> want = refCarve(src, n, want_seams);
    // host form
    std::vector<uint32_t> seams((size_t)n * rows, 77u);
    const Image<T> host = src.seamCarve(n, false, seams.data());
    EXPECT(sameBytes(host, want));
    EXPECT(seams == want_seams);
    EXPECT(sameBytes(src, keep));
    // device form on a stream of its own
    Stream stream = Stream::create();
    DeviceImage<T> dev = DeviceImage<T>::init(rows, cols, stream.handle());
    check(zg_memcpy_h2d(dev.data, src.data, (size_t)rows * cols * sizeof(T), stream.handle()));
    void *dseams = nullptr;
    check(zg_malloc(&dseams, (size_t)n * rows * 4));
    const DeviceImage<T> out = dev.seamCarve(n, false, (uint32_t *)dseams);
    Image<T> back = Image<T>::init(rows, cols - n);
    std::vector<uint32_t> back_seams((size_t)n * rows);
    check(zg_memcpy_d2h(back.data, out.data, (size_t)rows * (cols - n) * sizeof(T), stream.handle()));
    check(zg_memcpy_d2h(back_seams.data(), dseams, (size_t)n * rows * 4, stream.handle()));
    EXPECT(sameBytes(back, want));
    EXPECT(back_seams == want_seams);
    check(zg_free(dseams));
    // horizontal: the transposed frame carved, transposed back
    if (rows < 2) return;
    const uint32_t nh = n < rows ? n : rows - 1;
    const Image<T> turned = transposed(src);
    std::vector<uint32_t> turned_seams;
    const Image<T> want_h = transposed(refCarve(turned, nh, turned_seams));
    std::vector<uint32_t> hseams(turned_seams.size(), 77u);
    const Image<T> got_h = src.seamCarve(nh, true, hseams.data());
    EXPECT(sameBytes(got_h, want_h));
    EXPECT(hseams == turned_seams);
}

int main() {
    check(zg_init(0));
    const uint32_t B = zg_seam_band_rows(), S = zg_seam_strip_cols();
    EXPECT(B >= 2 && S >= 8);
    // the reserved argument, and a seam count the frame does not have
    {
        Image<uint8_t> img = frame<uint8_t>(4, 6);
        Image<uint8_t> out = Image<uint8_t>::init(4, 5);
        const zg_image s = img.desc(), d = out.desc();
        EXPECT(zg_seam_carve_host(&s, &d, 1, ZG_SEAM_VERTICAL, &s, nullptr) == ZG_ERR_UNSUPPORTED);
        bool thrown = false;
        try { (void)img.seamCarve(6); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown);
    }
    carve<uint8_t>(1, 9, 3);
    carve<uint8_t>(B + 1, S + 1, 4);
    carve<Rgba<uint8_t>>(2 * B + 1, S + 5, 5);
    carve<Rgb<float>>(B - 1, 2 * S + 3, 3);
    if (failures) { std::printf("cpp seam: %d failure(s)\n", failures); return 1; }
    std::printf("cpp seam ok\n");
    return 0;
}
