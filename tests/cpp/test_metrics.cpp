// Image<T>::psnr / meanPixelError / ssim and their DeviceImage<T> forms of the C++ host mirror against the reference's loops
// (src/image/metrics.zig:10-166) written out here, bit for bit: the reference's own two tests, then random frames of four pixel types,
// host form and device form (with and without a device result), the SSIM map included. The library's own window is fetched with
// zg_ssim_window_host and handed to the loop. Needs a GPU: built and run by tests/test_cpp_metrics.py.
#include <cmath>
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

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// fields of a pixel as f64, in declaration order; volatile keeps one rounding an operation, whatever the compiler's flags
static int fields(uint8_t p, double *f) { f[0] = p; return 1; }
static int fields(float p, double *f) { f[0] = p; return 1; }
template <typename E> static int fields(const Rgb<E> &p, double *f) { f[0] = p.r; f[1] = p.g; f[2] = p.b; return 3; }
template <typename E> static int fields(const Rgba<E> &p, double *f) { f[0] = p.r; f[1] = p.g; f[2] = p.b; f[3] = p.a; return 4; }

template <typename T> struct IsByte { static constexpr bool value = false; };
template <> struct IsByte<uint8_t> { static constexpr bool value = true; };
template <> struct IsByte<Rgb<uint8_t>> { static constexpr bool value = true; };
template <> struct IsByte<Rgba<uint8_t>> { static constexpr bool value = true; };

// getPixelScalar (:188-203)
template <typename T> static double scalar(const T &p) {
    double f[4];
    const int n = fields(p, f);
    if (n == 1) return f[0];
    if (IsByte<T>::value) {
        volatile double r = f[0] / 255.0, g = f[1] / 255.0, b = f[2] / 255.0;
        volatile double x = 0.2126 * r, y = 0.7152 * g, z = 0.0722 * b;
        volatile double s = x + y;
        s = s + z;
        return s * 255.0;
    }
    volatile double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + f[i];
    return sum / (double)n;
}

// psnr's mse (:15-48) or meanPixelError's mean (:119-160)
template <typename T> static double refMean(const Image<T> &a, const Image<T> &b, bool squared) {
    volatile double total = 0.0;
    size_t count = 0;
    for (uint32_t r = 0; r < a.rows; ++r)
        for (uint32_t c = 0; c < a.cols; ++c) {
            double fa[4], fb[4];
            const int n = fields(a.at(r, c), fa);
            fields(b.at(r, c), fb);
            for (int i = 0; i < n; ++i) {
                volatile double diff = fa[i] - fb[i];
                volatile double term = squared ? diff * diff : std::fabs(diff);
                total = total + term;
                ++count;
            }
        }
    return total / (double)count;
}

template <typename T> static double refSsim(const Image<T> &a, const Image<T> &b, const double *w, std::vector<double> *map) {
    const double l = IsByte<T>::value ? 255.0 : 1.0;
    const double c1 = (0.01 * l) * (0.01 * l), c2 = (0.03 * l) * (0.03 * l);
    volatile double ssim_sum = 0.0, weight_sum = 0.0;
    for (uint32_t row = 5; row < a.rows - 5; ++row)
        for (uint32_t col = 5; col < a.cols - 5; ++col) {
            volatile double mu_x = 0, mu_y = 0, mu_x_sq = 0, mu_y_sq = 0, mu_xy = 0;
            for (uint32_t dy = 0; dy < 11; ++dy)
                for (uint32_t dx = 0; dx < 11; ++dx) {
                    const double weight = w[dy * 11 + dx];
                    const double val_x = scalar(a.at(row - 5 + dy, col - 5 + dx)), val_y = scalar(b.at(row - 5 + dy, col - 5 + dx));
                    volatile double wx = weight * val_x, wy = weight * val_y;
                    volatile double wxx = wx * val_x, wyy = wy * val_y, wxy = wx * val_y;
                    mu_x = mu_x + wx;
                    mu_y = mu_y + wy;
                    mu_x_sq = mu_x_sq + wxx;
                    mu_y_sq = mu_y_sq + wyy;
                    mu_xy = mu_xy + wxy;
                }
            volatile double xx = mu_x * mu_x, yy = mu_y * mu_y, xy = mu_x * mu_y;
            volatile double vx = mu_x_sq - xx, vy = mu_y_sq - yy;
            const double sigma_x_sq = vx > 0.0 ? vx : 0.0, sigma_y_sq = vy > 0.0 ? vy : 0.0;
            volatile double sigma_xy = mu_xy - xy;
            volatile double n1 = 2.0 * mu_x;
            n1 = n1 * mu_y;
            n1 = n1 + c1;
            volatile double n2 = 2.0 * sigma_xy;
            n2 = n2 + c2;
            volatile double d1 = xx + yy;
            d1 = d1 + c1;
            volatile double d2 = sigma_x_sq + sigma_y_sq;
            d2 = d2 + c2;
            volatile double numerator = n1 * n2, denominator = d1 * d2;
            volatile double q = numerator / denominator;
            if (map) map->push_back((double)q);
            ssim_sum = ssim_sum + q;
            weight_sum = weight_sum + 1.0;
        }
    return ssim_sum / weight_sum;
}

static void value(uint8_t &p) { p = (uint8_t)(rnd() >> 24); }
static void value(float &p) { p = (float)(rnd() >> 8) / 16777216.0f; }
static void value(Rgb<uint8_t> &p) { p = {(uint8_t)(rnd() >> 24), (uint8_t)(rnd() >> 24), (uint8_t)(rnd() >> 24)}; }
static void value(Rgba<float> &p) { p = {(float)(rnd() >> 8) / 16777216.0f, (float)(rnd() >> 8) / 16777216.0f, (float)(rnd() >> 8) / 16777216.0f, (float)(rnd() >> 8) / 16777216.0f}; }

template <typename T> static void frames(const double *window) {
    const uint32_t rows = 41, cols = 150;
    Image<T> a = Image<T>::init(rows, cols), b = Image<T>::init(rows, cols);
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t c = 0; c < cols; ++c) {
            value(a.at(r, c));
            b.at(r, c) = a.at(r, c);
            if (rnd() % 3 == 0) value(b.at(r, c));
        }
    const double max_value = IsByte<T>::value ? 255.0 : 1.0;
    const double mse = refMean(a, b, true), mpe = refMean(a, b, false) / max_value;
    std::vector<double> want_map;
    const double want_ssim = refSsim(a, b, window, &want_map);
    // host forms
    EXPECT(sameBits(a.psnr(b), zg_psnr_from_mse(mse, max_value)));
    EXPECT(sameBits(a.meanPixelError(b), mpe));
    std::vector<double> map(want_map.size(), -1.0);
    EXPECT(sameBits(a.ssim(b, nullptr, map.data()), want_ssim));
    EXPECT(std::memcmp(map.data(), want_map.data(), map.size() * 8) == 0);
    EXPECT(a.psnr(a) == INFINITY && a.meanPixelError(a) == 0.0);
    // device forms on a stream of their own
    Stream stream = Stream::create();
    DeviceImage<T> da = DeviceImage<T>::init(rows, cols, stream.handle()), db = DeviceImage<T>::init(rows, cols, stream.handle());
    check(zg_memcpy_h2d(da.data, a.data, (size_t)rows * cols * sizeof(T), stream.handle()));
    check(zg_memcpy_h2d(db.data, b.data, (size_t)rows * cols * sizeof(T), stream.handle()));
    EXPECT(sameBits(da.psnr(db), zg_psnr_from_mse(mse, max_value)));
    EXPECT(sameBits(da.meanPixelError(db), mpe));
    EXPECT(sameBits(da.ssim(db), want_ssim));
    void *mem = nullptr;
    check(zg_malloc(&mem, 3 * sizeof(zg_metric_result) + want_map.size() * 8));
    zg_metric_result *res = (zg_metric_result *)mem;
    double *dmap = (double *)(res + 3);
    EXPECT(da.psnr(db, res + 0) == 0 && da.meanPixelError(db, res + 1) == 0 && da.ssim(db, res + 2, dmap) == 0);
    zg_metric_result back[3];
    check(zg_memcpy_d2h(back, res, sizeof back, stream.handle()));
    check(zg_memcpy_d2h(map.data(), dmap, map.size() * 8, stream.handle()));
    EXPECT(sameBits(back[0].value, mse) && sameBits(back[1].value, mpe) && sameBits(back[2].value, want_ssim));
    EXPECT(back[0].count == (uint64_t)rows * cols * (sizeof(T) / (IsByte<T>::value ? 1 : 4)) && back[2].count == want_map.size());
    EXPECT(std::memcmp(map.data(), want_map.data(), map.size() * 8) == 0);
    check(zg_free(mem));
}

int main() {
    check(zg_init(0));
    double window[121];
    check(zg_ssim_window_host(window));
    // "meanPixelError RGB example" (:251-272)
    {
        Image<Rgb<uint8_t>> a = Image<Rgb<uint8_t>>::init(1, 1), b = Image<Rgb<uint8_t>>::init(1, 1);
        a.at(0, 0) = {255, 0, 0};
        b.at(0, 0) = {0, 0, 0};
        EXPECT(std::fabs(a.meanPixelError(b) - 1.0 / 3.0) <= 1e-9);
    }
    // "ssim rgb scales with luminance" (:274-293)
    {
        Image<Rgb<uint8_t>> a = Image<Rgb<uint8_t>>::init(12, 12), b = Image<Rgb<uint8_t>>::init(12, 12);
        for (uint32_t r = 0; r < 12; ++r)
            for (uint32_t c = 0; c < 12; ++c) {
                a.at(r, c) = (r + c) % 2 == 0 ? Rgb<uint8_t>{255, 0, 0} : Rgb<uint8_t>{0, 255, 0};
                b.at(r, c) = {0, 0, 0};
            }
        const double got = a.ssim(b);
        EXPECT(got < 0.99 && sameBits(got, refSsim(a, b, window, nullptr)));
        // error.ImageTooSmall and error.DimensionMismatch
        Image<Rgb<uint8_t>> small = Image<Rgb<uint8_t>>::init(10, 12), other = Image<Rgb<uint8_t>>::init(12, 13);
        bool too_small = false, mismatch = false;
        try { small.ssim(small); } catch (const InvalidArgument &) { too_small = true; }
        try { a.psnr(other); } catch (const DimensionMismatch &) { mismatch = true; }
        EXPECT(too_small && mismatch);
    }

    frames<uint8_t>(window);
    frames<float>(window);
    frames<Rgb<uint8_t>>(window);
    frames<Rgba<float>>(window);

    if (failures) { std::printf("cpp metrics: %d failure(s)\n", failures); return 1; }
    std::printf("cpp metrics ok\n");
    return 0;
}
