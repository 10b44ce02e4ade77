// zignal::FeatureDistributionMatching<T> (zignal_amd/cpp/zignal_hip.hpp) over Image and over DeviceImage: a correlated noise frame against a
// result recorded from the Python restatement of the reference (tests/golden/fdm_cpp_rgb.rgb, which tests/test_cpp_fdm.py holds to
// tests/fdm_ref.py), fdm.zig's own three patterns (:325-420 colour, :429-464 u8, :531-581 a grey target) with fdm.zig's own assertions, the
// state machine's two errors and updateFrames. fdm.zig's colour pattern gets no recording: its r and g are independent, their covariance
// is exactly 0, the reference's Welford recurrence leaves 1.6e-19 there, and the sign of that noise decides the sign of a column of U.
// Needs a GPU: built and run by tests/test_cpp_fdm.py, which passes the directory of the recording.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

typedef Rgb<uint8_t> Px;

static Image<Px> pattern(bool target) { // fdm.zig:329-353
    Image<Px> im = Image<Px>::init(50, 50);
    for (uint32_t i = 0; i < 2500; ++i) {
        const uint32_t x = i % 50, y = i / 50;
        im.at(y, x) = target ? Px{(uint8_t)(50 + x % 30), (uint8_t)(70 + y % 20), (uint8_t)(90 + (x + y) % 35)}
                             : Px{(uint8_t)(100 + x % 20), (uint8_t)(150 + y % 15), (uint8_t)(80 + (x + y) % 25)};
    }
    return im;
}
// 40 x 48 of three mixed noise bytes a pixel, as tests/test_cpp_fdm.py makes them: every covariance well away from zero
static Image<Px> noise(uint32_t s, uint32_t shift) {
    Image<Px> im = Image<Px>::init(40, 48);
    for (uint32_t i = 0; i < 40 * 48; ++i) {
        uint32_t v[3];
        for (uint32_t &b : v) {
            s = s * 1664525u + 1013904223u;
            b = s >> 24;
        }
        im.at(i / 48, i % 48) = Px{(uint8_t)(v[0] / 2 + 60 - shift), (uint8_t)(v[0] / 4 + v[1] / 2 + 30), (uint8_t)(v[1] / 4 + v[2] / 2 + v[0] / 8 + shift)};
    }
    return im;
}
static const size_t NOISE_BYTES = 40 * 48 * 3;
static bool meansAndVariancesMatch(const Image<Px> &got, const Image<Px> &tgt) { // fdm.zig:355-426
    double mean[2][3] = {}, var[2][3] = {};
    const Image<Px> *both[2] = {&got, &tgt};
    for (int k = 0; k < 2; ++k) {
        for (uint32_t i = 0; i < 2500; ++i) {
            const Px p = both[k]->at(i / 50, i % 50);
            mean[k][0] += p.r; mean[k][1] += p.g; mean[k][2] += p.b;
        }
        for (double &m : mean[k]) m /= 2500.0;
        for (uint32_t i = 0; i < 2500; ++i) {
            const Px p = both[k]->at(i / 50, i % 50);
            const double d[3] = {p.r - mean[k][0], p.g - mean[k][1], p.b - mean[k][2]};
            for (int c = 0; c < 3; ++c) var[k][c] += d[c] * d[c] / 2500.0;
        }
    }
    bool ok = true;
    for (int c = 0; c < 3; ++c) ok = ok && std::fabs(mean[0][c] - mean[1][c]) <= 2.0 && std::fabs(var[0][c] - var[1][c]) <= 1.0;
    return ok;
}
static std::vector<uint8_t> recording(const std::string &path) {
    std::vector<uint8_t> bytes;
    if (FILE *f = std::fopen(path.c_str(), "rb")) {
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
        std::fclose(f);
    }
    return bytes;
}
template <typename T> static bool sameBytes(const Image<T> &a, const void *b, size_t n) {
    return n == (size_t)a.rows * a.cols * sizeof(T) && std::memcmp(a.data, b, n) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    check(zg_init(0));
    const std::vector<uint8_t> want = recording(std::string(argv[1]) + "/fdm_cpp_rgb.rgb");
    EXPECT(want.size() == NOISE_BYTES);

    { // host images
        Image<Px> src = noise(5, 0), tgt = noise(77, 20);
        FeatureDistributionMatching<Px> fdm;
        bool threw = false;
        try { fdm.update(); } catch (const NoTargetSet &) { threw = true; }
        EXPECT(threw);
        fdm.setTarget(tgt);
        threw = false;
        try { fdm.update(); } catch (const NoSourceSet &) { threw = true; }
        EXPECT(threw);
        fdm.setSource(src);
        fdm.update();
        EXPECT(sameBytes(src, want.data(), want.size()));
        EXPECT(sameBytes(tgt, noise(77, 20).data, NOISE_BYTES));
    }
    { // device images: the same bytes, and updateFrames over three frames
        Image<Px> src = noise(5, 0), tgt = noise(77, 20);
        DeviceImage<Px> dsrc = DeviceImage<Px>::fromHost(src), dtgt = DeviceImage<Px>::fromHost(tgt);
        FeatureDistributionMatching<Px, DeviceImage> fdm;
        fdm.match(dsrc, dtgt);
        Image<Px> out = dsrc.toHost();
        EXPECT(sameBytes(out, want.data(), want.size()));
        DeviceImage<Px> a = DeviceImage<Px>::fromHost(src), b = DeviceImage<Px>::fromHost(tgt), c = DeviceImage<Px>::fromHost(src);
        fdm.updateFrames({&a, &b, &c});
        EXPECT(sameBytes(a.toHost(), want.data(), want.size()));
        EXPECT(sameBytes(c.toHost(), want.data(), want.size()));
        EXPECT(sameBytes(b.toHost(), tgt.data, NOISE_BYTES)); // the target against itself
    }
    { // fdm.zig's own colour test, host and device: means within 2.0 and variances within 1 of the target's
        Image<Px> src = pattern(false), tgt = pattern(true);
        DeviceImage<Px> dsrc = DeviceImage<Px>::fromHost(src), dtgt = DeviceImage<Px>::fromHost(tgt);
        FeatureDistributionMatching<Px> host_fdm;
        host_fdm.match(src, tgt);
        EXPECT(meansAndVariancesMatch(src, tgt));
        FeatureDistributionMatching<Px, DeviceImage> fdm;
        fdm.match(dsrc, dtgt);
        EXPECT(sameBytes(dsrc.toHost(), src.data, 7500));
    }
    { // u8: 0 .. 99 onto 100 .. 199, the mean becomes 149.5 exactly (fdm.zig:429-464)
        Image<uint8_t> src = Image<uint8_t>::init(1, 100), tgt = Image<uint8_t>::init(1, 100);
        for (uint32_t i = 0; i < 100; ++i) { src.at(0, i) = (uint8_t)i; tgt.at(0, i) = (uint8_t)(100 + i); }
        FeatureDistributionMatching<uint8_t> fdm;
        fdm.match(src, tgt);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < 100; ++i) sum += src.at(0, i);
        EXPECT(sum == 14950);
    }
    { // a grey Rgba target: r = g = b, alpha 0 (fdm.zig:196)
        Image<Rgba<uint8_t>> src = Image<Rgba<uint8_t>>::init(12, 12), tgt = Image<Rgba<uint8_t>>::init(12, 12);
        for (uint32_t i = 0; i < 144; ++i) {
            const uint32_t x = i % 12, y = i / 12;
            src.at(y, x) = Rgba<uint8_t>{(uint8_t)((x * 30 + y * 5) % 255), (uint8_t)((x * 15 + y * 40) % 255), (uint8_t)((x * 50 + y * 25) % 255), 200};
            const uint8_t v = (uint8_t)(40 + i % 160);
            tgt.at(y, x) = Rgba<uint8_t>{v, v, v, 255};
        }
        DeviceImage<Rgba<uint8_t>> dsrc = DeviceImage<Rgba<uint8_t>>::fromHost(src), dtgt = DeviceImage<Rgba<uint8_t>>::fromHost(tgt);
        FeatureDistributionMatching<Rgba<uint8_t>, DeviceImage> fdm;
        fdm.match(dsrc, dtgt);
        Image<Rgba<uint8_t>> out = dsrc.toHost();
        double mean = 0.0, target_mean = 0.0;
        bool gray = true;
        for (uint32_t i = 0; i < 144; ++i) {
            const Rgba<uint8_t> p = out.at(i / 12, i % 12);
            gray = gray && p.r == p.g && p.g == p.b && p.a == 0;
            mean += p.r;
            target_mean += tgt.at(i / 12, i % 12).r;
        }
        EXPECT(gray);
        EXPECT(std::fabs(mean / 144.0 - target_mean / 144.0) <= 2.0);
    }
    if (failures == 0) std::printf("cpp fdm ok\n");
    return failures ? 1 : 0;
}
