// Image<T> and DeviceImage<T>::percentileBlur / minBlur / maxBlur / midpointBlur / alphaTrimmedMeanBlur of the C++ host mirror
// (src/image.zig:672-783) against a sort of every window written out here, bit for bit: radius 2 (the direct kernel) and radius 16 (the
// sliding-histogram kernel), u8 and Rgba(u8) frames, all four borders, host form and device form on a stream of its own, and the error
// sets. Needs a GPU: built and run by tests/test_cpp_order_stat.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 2468;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

// border.resolveIndex (src/image/border.zig:46-63): the index, or -1 for a dropped sample (value 0)
static long resolve(long idx, long length, BorderMode border) {
    if (idx >= 0 && idx < length) return idx;
    switch (border) {
    case BorderMode::zero: return -1;
    case BorderMode::replicate: return idx < 0 ? 0 : length - 1;
    case BorderMode::mirror: {
        if (length == 1) return 0;
        const long period = 2 * (length - 1);
        long m = idx % period;
        if (m < 0) m += period;
        return m >= length ? period - m : m;
    }
    default: {
        long m = idx % length;
        if (m < 0) m += length;
        return m;
    }
    }
}

static int channels(const uint8_t &) { return 1; }
static int channels(const Rgba<uint8_t> &) { return 4; }
static uint8_t &channel(uint8_t &p, int) { return p; }
static uint8_t &channel(Rgba<uint8_t> &p, int c) { return c == 0 ? p.r : c == 1 ? p.g : c == 2 ? p.b : p.a; }

enum Op { PERCENTILE, MIDPOINT, TRIMMED };

// order_statistic_blur.zig on the sorted window: percentile (histogram.zig:586-610), midpoint (:318-325), alpha-trimmed mean (:327-375)
template <typename T> static Image<T> reference(const Image<T> &src, long radius, Op op, double param, BorderMode border) {
    Image<T> out = Image<T>::init(src.rows, src.cols);
    const size_t area = (size_t)(2 * radius + 1) * (size_t)(2 * radius + 1);
    std::vector<uint8_t> win(area);
    for (long r = 0; r < (long)src.rows; ++r)
        for (long c = 0; c < (long)src.cols; ++c)
            for (int ch = 0; ch < channels(src.at(0, 0)); ++ch) {
                size_t n = 0;
                for (long dy = -radius; dy <= radius; ++dy)
                    for (long dx = -radius; dx <= radius; ++dx) {
                        const long rr = resolve(r + dy, src.rows, border), cc = resolve(c + dx, src.cols, border);
                        win[n++] = rr >= 0 && cc >= 0 ? channel(src.at((size_t)rr, (size_t)cc), ch) : 0;
                    }
                std::sort(win.begin(), win.end());
                unsigned res;
                if (op == PERCENTILE) {
                    const double rank_floor = std::floor(param * (double)(area - 1) + 1e-12);
                    res = win[std::min((size_t)rank_floor, area - 1)];
                } else if (op == MIDPOINT) {
                    res = (win.front() + win.back() + 1u) / 2u;
                } else {
                    const size_t trim = std::min((size_t)std::floor(param * (double)area), area / 2), kept = area - 2 * trim;
                    size_t sum = 0;
                    for (size_t k = trim; k < area - trim; ++k) sum += win[k];
                    res = (unsigned)std::min<size_t>((sum + kept / 2) / kept, 255);
                }
                channel(out.at((size_t)r, (size_t)c), ch) = (uint8_t)res;
            }
    return out;
}

template <typename T> static bool same(const Image<T> &a, const Image<T> &b) {
    for (uint32_t r = 0; r < a.rows; ++r)
        if (std::memcmp(&a.at(r, 0), &b.at(r, 0), a.cols * sizeof(T)) != 0) return false;
    return true;
}

template <typename T> static void frames(uint32_t radius, BorderMode border) {
    const uint32_t rows = 11, cols = 70;
    Image<T> a = Image<T>::init(rows, cols), got = Image<T>::init(rows, cols);
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t c = 0; c < cols; ++c)
            for (int ch = 0; ch < channels(a.at(0, 0)); ++ch) channel(a.at(r, c), ch) = (uint8_t)(rnd() >> 24);
    const Image<T> want_pct = reference(a, radius, PERCENTILE, 0.37, border), want_min = reference(a, radius, PERCENTILE, 0.0, border),
                   want_max = reference(a, radius, PERCENTILE, 1.0, border), want_mid = reference(a, radius, MIDPOINT, 0.0, border),
                   want_trim = reference(a, radius, TRIMMED, 0.2, border);
    // host forms
    a.percentileBlur(got, radius, 0.37, border); EXPECT(same(got, want_pct));
    a.minBlur(got, radius, border); EXPECT(same(got, want_min));
    a.maxBlur(got, radius, border); EXPECT(same(got, want_max));
    a.midpointBlur(got, radius, border); EXPECT(same(got, want_mid));
    a.alphaTrimmedMeanBlur(got, radius, 0.2, border); EXPECT(same(got, want_trim));
    // device forms on a stream of their own
    Stream stream = Stream::create();
    DeviceImage<T> da = DeviceImage<T>::fromHost(a, stream.handle()), dout = DeviceImage<T>::init(rows, cols, stream.handle());
    da.percentileBlur(dout, radius, 0.37, border); EXPECT(same(dout.toHost(), want_pct));
    da.minBlur(dout, radius, border); EXPECT(same(dout.toHost(), want_min));
    da.maxBlur(dout, radius, border); EXPECT(same(dout.toHost(), want_max));
    da.midpointBlur(dout, radius, border); EXPECT(same(dout.toHost(), want_mid));
    da.alphaTrimmedMeanBlur(dout, radius, 0.2, border); EXPECT(same(dout.toHost(), want_trim));
}

int main() {
    check(zg_init(0));
    const BorderMode borders[4] = {BorderMode::zero, BorderMode::replicate, BorderMode::mirror, BorderMode::wrap};
    for (uint32_t radius : {2u, 16u})
        for (BorderMode border : borders) {
            frames<uint8_t>(radius, border);
            frames<Rgba<uint8_t>>(radius, border);
        }
    // error.DimensionMismatch, error.InvalidPercentile, error.InvalidTrim; radius past 256 is unsupported
    {
        Image<uint8_t> a = Image<uint8_t>::init(8, 8), b = Image<uint8_t>::init(8, 9), c = Image<uint8_t>::init(8, 8);
        bool mismatch = false, percentile = false, trim = false, radius = false;
        try { a.minBlur(b, 16, BorderMode::mirror); } catch (const DimensionMismatch &) { mismatch = true; }
        try { a.percentileBlur(c, 16, 1.5, BorderMode::mirror); } catch (const InvalidArgument &) { percentile = true; }
        try { a.alphaTrimmedMeanBlur(c, 16, 0.5, BorderMode::mirror); } catch (const InvalidArgument &) { trim = true; }
        try { a.maxBlur(c, 257, BorderMode::mirror); } catch (const Error &) { radius = true; }
        EXPECT(mismatch && percentile && trim && radius);
    }
    if (failures) { std::printf("cpp order-stat: %d failure(s)\n", failures); return 1; }
    std::printf("cpp order-stat ok\n");
    return 0;
}
