// Image<T>::floodFill and DeviceImage<T>::floodFill of the C++ host mirror against the reference's loop (src/image/flood_fill.zig:59-131)
// written out here: a stack, `visited` set before the push, fill_value written at the pop, pixelDistance in f64 with a real square
// root. The reference's own four tests (src/image/tests/flood_fill.zig), then random frames of four pixel types past a tile in both
// directions, both modes and connectivities, host form and device form, whole images compared byte for byte and the counts with them.
// Needs a GPU: built and run by tests/test_cpp_flood.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 1234;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

// pixelDistance (:28-51): volatile keeps one rounding an operation, whatever the compiler's flags
static double dist(uint8_t a, uint8_t b) { return std::fabs((double)a - (double)b); }
static double dist(float a, float b) { return std::fabs((double)a - (double)b); }
template <typename E> static double distFields(const E *a, const E *b, int n) {
    volatile double sum_sq = 0.0;
    for (int i = 0; i < n; ++i) {
        volatile double diff = (double)a[i] - (double)b[i];
        volatile double sq = diff * diff;
        sum_sq = sum_sq + sq;
    }
    return std::sqrt(sum_sq);
}
template <typename E> static double dist(const Rgb<E> &a, const Rgb<E> &b) { return distFields(&a.r, &b.r, 3); }
template <typename E> static double dist(const Rgba<E> &a, const Rgba<E> &b) { return distFields(&a.r, &b.r, 4); }

template <typename T> static uint32_t refFloodFill(const Image<T> &image, uint32_t start_row, uint32_t start_col, const T &fill_value, const FloodFillOptions &o) {
    static const int offsets[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
    const T seed_val = image.at(start_row, start_col);
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    std::vector<char> visited((size_t)image.rows * image.cols, 0);
    stack.push_back({start_row, start_col});
    visited[(size_t)start_row * image.cols + start_col] = 1;
    uint32_t filled = 0;
    while (!stack.empty()) {
        const auto curr = stack.back();
        stack.pop_back();
        const T orig_val = image.at(curr.first, curr.second);
        image.at(curr.first, curr.second) = fill_value;
        ++filled;
        const T compare = o.mode == FloodFillOptions::ThresholdMode::seed ? seed_val : orig_val;
        for (int k = 0; k < (int)o.connectivity; ++k) {
            const int64_t nr = (int64_t)curr.first + offsets[k][0], nc = (int64_t)curr.second + offsets[k][1];
            if (nr < 0 || nr >= image.rows || nc < 0 || nc >= image.cols) continue;
            const size_t idx = (size_t)nr * image.cols + (size_t)nc;
            if (!visited[idx] && dist(image.at(nr, nc), compare) <= o.threshold) {
                visited[idx] = 1;
                stack.push_back({(uint32_t)nr, (uint32_t)nc});
            }
        }
    }
    return filled;
}

template <typename T> static bool sameBytes(const Image<T> &a, const Image<T> &b) {
    for (uint32_t r = 0; r < a.rows; ++r)
        if (std::memcmp(&a.at(r, 0), &b.at(r, 0), (size_t)a.cols * sizeof(T))) return false;
    return true;
}

static void value(uint8_t &p, uint32_t v) { p = (uint8_t)(100 + v); }
static void value(float &p, uint32_t v) { p = 0.25f * (float)v; }
static void value(Rgb<uint8_t> &p, uint32_t v) { p = {(uint8_t)(100 + v), 7, (uint8_t)(50 + (v & 1))}; }
static void value(Rgba<float> &p, uint32_t v) { p = {0.5f, 0.125f * (float)v, 0.75f, 0.25f * (float)(v & 1)}; }

// patches three pixels wide of four levels: components of every size that cross the tile edges
template <typename T> static void frames(double threshold, const T &fill_value) {
    const uint32_t tile = zg_flood_fill_tile();
    const uint32_t rows = tile + 9, cols = 2 * tile + 5;
    Image<T> src = Image<T>::init(rows, cols);
    std::vector<uint32_t> coarse((size_t)(rows / 3 + 1) * (cols / 3 + 1));
    for (uint32_t &v : coarse) v = rnd() % 4;
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t c = 0; c < cols; ++c) value(src.at(r, c), rnd() % 10 == 0 ? rnd() % 4 : coarse[(size_t)(r / 3) * (cols / 3 + 1) + c / 3]);
    Stream stream = Stream::create();
    void *count_mem = nullptr;
    check(zg_malloc(&count_mem, 16));
    for (int mode = 0; mode < 2; ++mode)
        for (int conn = 4; conn <= 8; conn += 4) {
            FloodFillOptions o;
            o.threshold = threshold;
            o.connectivity = conn == 4 ? FloodFillOptions::Connectivity::four : FloodFillOptions::Connectivity::eight;
            o.mode = mode == 0 ? FloodFillOptions::ThresholdMode::seed : FloodFillOptions::ThresholdMode::neighbor;
            const uint32_t row = tile - 1, col = tile;
            Image<T> want = src, host = src;
            const uint32_t n = refFloodFill(want, row, col, fill_value, o);
            EXPECT(n > 1);
            EXPECT(host.floodFill(row, col, fill_value, o) == n);
            EXPECT(sameBytes(host, want));
            // the device form on a stream of its own, the seed in device memory
            DeviceImage<T> dev = DeviceImage<T>::init(rows, cols, stream.handle());
            check(zg_memcpy_h2d(dev.data, src.data, (size_t)rows * cols * sizeof(T), stream.handle()));
            uint32_t *dseed = (uint32_t *)count_mem + 1, *dcount = (uint32_t *)count_mem;
            const uint32_t seed[2] = {row, col};
            check(zg_memcpy_h2d(dseed, seed, 8, stream.handle()));
            dev.floodFill(0, 0, fill_value, o, dseed, dcount);
            Image<T> back = Image<T>::init(rows, cols);
            uint32_t count = 0;
            check(zg_memcpy_d2h(back.data, dev.data, (size_t)rows * cols * sizeof(T), stream.handle()));
            check(zg_memcpy_d2h(&count, dcount, 4, stream.handle()));
            EXPECT(count == n);
            EXPECT(sameBytes(back, want));
        }
    check(zg_free(count_mem));
}

int main() {
    check(zg_init(0));
    // "flood fill connectivity"
    {
        Image<uint8_t> img = Image<uint8_t>::init(5, 5);
        std::memset(img.data, 0, 25);
        const int cross[9][2] = {{0, 1}, {1, 2}, {2, 0}, {2, 1}, {2, 2}, {2, 3}, {2, 4}, {3, 2}, {4, 2}};
        for (const auto &p : cross) img.at(p[0], p[1]) = 5;
        Image<uint8_t> img4 = img, img8 = img;
        FloodFillOptions o;
        EXPECT(img4.floodFill(2, 2, 9, o) == 8);
        EXPECT(img4.at(0, 1) == 5 && img4.at(1, 2) == 9 && img4.at(2, 2) == 9);
        o.connectivity = FloodFillOptions::Connectivity::eight;
        EXPECT(img8.floodFill(2, 2, 9, o) == 9);
        EXPECT(img8.at(0, 1) == 9 && img8.at(1, 2) == 9 && img8.at(2, 2) == 9);
    }
    // "flood fill relative threshold modes"
    {
        Image<uint8_t> a = Image<uint8_t>::init(1, 5);
        for (uint8_t c = 0; c < 5; ++c) a.at(0, c) = c;
        Image<uint8_t> b = a;
        FloodFillOptions o;
        o.threshold = 1.0;
        a.floodFill(0, 0, 9, o);
        const uint8_t want_seed[5] = {9, 9, 2, 3, 4}, want_neighbor[5] = {9, 9, 9, 9, 9};
        EXPECT(std::memcmp(a.data, want_seed, 5) == 0);
        o.mode = FloodFillOptions::ThresholdMode::neighbor;
        b.floodFill(0, 0, 9, o);
        EXPECT(std::memcmp(b.data, want_neighbor, 5) == 0);
    }
    // "flood fill RGB color images"
    {
        Image<Rgb<uint8_t>> img = Image<Rgb<uint8_t>>::init(1, 3);
        img.at(0, 0) = {100, 100, 100};
        img.at(0, 1) = {100, 100, 103};
        img.at(0, 2) = {100, 100, 107};
        Image<Rgb<uint8_t>> img4 = img, img8 = img;
        const Rgb<uint8_t> red{255, 0, 0};
        FloodFillOptions o;
        o.threshold = 4.0;
        EXPECT(img4.floodFill(0, 0, red, o) == 2);
        EXPECT(img4.at(0, 1).r == 255 && img4.at(0, 2).b == 107 && img4.at(0, 2).r == 100);
        o.threshold = 8.0;
        EXPECT(img8.floodFill(0, 0, red, o) == 3);
        EXPECT(img8.at(0, 2).r == 255 && img8.at(0, 2).b == 0);
    }
    // "flood fill error bounds"
    {
        Image<uint8_t> img = Image<uint8_t>::init(3, 3);
        std::memset(img.data, 0, 9);
        FloodFillOptions o;
        o.threshold = 1.0;
        bool thrown = false;
        try { img.floodFill(3, 3, 9, o); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown && img.at(2, 2) == 0);
    }

    frames<uint8_t>(1.0, 7);
    frames<float>(0.25, -3.5f);
    frames<Rgb<uint8_t>>(std::sqrt(2.0), Rgb<uint8_t>{1, 2, 3});
    frames<Rgba<float>>(std::sqrt(0.125 * 0.125 + 0.25 * 0.25), Rgba<float>{-1.0f, -2.0f, -3.0f, -4.0f});

    if (failures) { std::printf("cpp flood: %d failure(s)\n", failures); return 1; }
    std::printf("cpp flood ok\n");
    return 0;
}
