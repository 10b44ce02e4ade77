// The C++ mirror of geometry fitting (zignal_amd/cpp/zignal_hip_transform.hpp): zignal::fit on host points and zignal::DeviceFit on device
// points, for the three kinds in float and double, against records written by the Python restatement of the reference
// (tests/golden/transform_cpp_records.bin, which tests/test_cpp_transform.py holds to tests/transform_ref.py), then project, inv, and
// DeviceFit::warp against Fit::warp with the downloaded matrix. Needs a GPU: built and run by tests/test_cpp_transform.py, which passes the
// directory of the recording.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip_transform.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const uint32_t N = 12;
// twelve integer points and their image under an integer affine map plus 0 .. 3 of noise, as tests/test_cpp_transform.py makes them: exact in
// float and in double
template <typename T> static void points(std::vector<FitPoint<T>> &from, std::vector<FitPoint<T>> &to) {
    uint32_t s = 2024;
    auto next = [&s]() { s = s * 1664525u + 1013904223u; return s >> 16; };
    for (uint32_t i = 0; i < N; ++i) {
        const int x = (int)(next() % 320), y = (int)(next() % 240);
        const int tx = 2 * x - y + 7 + (int)(next() % 4), ty = x + 2 * y - 5 + (int)(next() % 4);
        from.push_back({(T)x, (T)y});
        to.push_back({(T)tx, (T)ty});
    }
}

// status and the nine coefficients as doubles: a float fit's are its float values widened
static bool same_as_recording(const zg_transform_fit &r, const double *want, int scalar) {
    if ((double)r.status != want[0]) return false;
    for (int i = 0; i < 9; ++i) {
        if (std::memcmp(&r.m64[i], &want[1 + i], 8) != 0) return false;
        const float f = (float)want[1 + i];
        if (scalar == ZG_SCALAR_F64 && std::memcmp(&r.m32[i], &f, 4) != 0) return false;
    }
    return true;
}

template <typename T> static void one_scalar(const double *recording) {
    const int scalar = std::is_same<T, float>::value ? ZG_SCALAR_F32 : ZG_SCALAR_F64;
    std::vector<FitPoint<T>> from, to;
    points(from, to);
    FitPoint<T> *dfrom = nullptr, *dto = nullptr, *dout = nullptr;
    check(zg_malloc((void **)&dfrom, N * sizeof(FitPoint<T>)));
    check(zg_malloc((void **)&dto, N * sizeof(FitPoint<T>)));
    check(zg_malloc((void **)&dout, N * sizeof(FitPoint<T>)));
    check(zg_memcpy_h2d(dfrom, from.data(), N * sizeof(FitPoint<T>), nullptr));
    check(zg_memcpy_h2d(dto, to.data(), N * sizeof(FitPoint<T>), nullptr));
    for (int kind = 0; kind < 3; ++kind) {
        const double *want = recording + (kind * 2 + scalar) * 10;
        Fit host;
        int host_status = ZG_FIT_OK;
        try {
            host = fit<T>((TransformKind)kind, from, to);
        } catch (const FitFailed &e) {
            host_status = e.status;
        }
        EXPECT((double)host_status == want[0]);
        DeviceFit dev;
        dev.fitPoints<T>((TransformKind)kind, dfrom, dto, N, nullptr, nullptr);
        const Fit got = dev.download(nullptr);
        EXPECT(same_as_recording(got.record, want, scalar));
        EXPECT(got.record.n_points == N && got.record.kind == kind);
        if (host_status != ZG_FIT_OK) continue;
        EXPECT(std::memcmp(&host.record, &got.record, sizeof(zg_transform_fit)) == 0);
        // project: the device's lane per point against the host's
        dev.project<T>(dfrom, dout, N, nullptr);
        std::vector<FitPoint<T>> projected(N);
        check(zg_memcpy_d2h(projected.data(), dout, N * sizeof(FitPoint<T>), nullptr));
        for (uint32_t i = 0; i < N; ++i) {
            const FitPoint<T> p = host.project<T>(from[i]);
            EXPECT(std::memcmp(&p, &projected[i], sizeof p) == 0);
        }
        if (kind == (int)TransformKind::projective) {
            DeviceFit inverse;
            dev.invertInto<T>(inverse, nullptr);
            const Fit a = inverse.download(nullptr), b = host.inv<T>();
            EXPECT(std::memcmp(&a.record, &b.record, sizeof(zg_transform_fit)) == 0);
        } else {
            bool threw = false;
            try { (void)host.inv<T>(); } catch (const FitFailed &e) { threw = e.status == ZG_FIT_BAD_INPUT; }
            EXPECT(threw);
        }
    }
    zg_free(dfrom); zg_free(dto); zg_free(dout);
}

static void warps() {
    Image<uint8_t> frame = Image<uint8_t>::init(97, 131);
    uint32_t s = 7;
    for (uint32_t i = 0; i < 97 * 131; ++i) { s = s * 1664525u + 1013904223u; frame.at(i / 131, i % 131) = (uint8_t)(s >> 24); }
    std::vector<FitPoint<double>> from = {{0, 0}, {130, 0}, {0, 96}, {130, 96}, {60, 40}}, to = {{3, 2}, {126, 6}, {5, 93}, {128, 90}, {61, 42}};
    DeviceImage<uint8_t> src = DeviceImage<uint8_t>::fromHost(frame);
    FitPoint<double> *dfrom = nullptr, *dto = nullptr;
    check(zg_malloc((void **)&dfrom, 5 * sizeof(FitPoint<double>)));
    check(zg_malloc((void **)&dto, 5 * sizeof(FitPoint<double>)));
    check(zg_memcpy_h2d(dfrom, from.data(), 5 * sizeof(FitPoint<double>), nullptr));
    check(zg_memcpy_h2d(dto, to.data(), 5 * sizeof(FitPoint<double>), nullptr));
    for (int kind = 0; kind < 3; ++kind) {
        DeviceFit dev;
        dev.fitPoints<double>((TransformKind)kind, dfrom, dto, 5, nullptr, nullptr);
        const Fit host = dev.download(nullptr);
        EXPECT(host.ok());
        DeviceImage<uint8_t> a = DeviceImage<uint8_t>::init(97, 131), b = DeviceImage<uint8_t>::init(97, 131);
        dev.warp(src, a, Interpolation::bilinear());
        host.warp(src, b, Interpolation::bilinear());
        Image<uint8_t> ha = Image<uint8_t>::init(97, 131), hb = Image<uint8_t>::init(97, 131);
        a.download(ha);
        b.download(hb);
        EXPECT(std::memcmp(ha.data, hb.data, 97 * 131) == 0);
        EXPECT(std::memcmp(ha.data, frame.data, 97 * 131) != 0);
    }
    // too few points: the record says so, and the warp leaves its destination as it is
    DeviceFit bad;
    bad.fitPoints<double>(TransformKind::projective, dfrom, dto, 3, nullptr, nullptr);
    EXPECT(bad.download(nullptr).record.status == ZG_FIT_BAD_COUNT);
    DeviceImage<uint8_t> keep = DeviceImage<uint8_t>::fromHost(frame);
    bad.warp(src, keep, Interpolation::bilinear());
    Image<uint8_t> hk = Image<uint8_t>::init(97, 131);
    keep.download(hk);
    EXPECT(std::memcmp(hk.data, frame.data, 97 * 131) == 0);
    bool threw = false;
    try { (void)fit<double>(TransformKind::similarity, {{0, 0}, {0, 0}}, {{1, 1}, {1, 1}}); } catch (const FitFailed &e) { threw = e.status == ZG_FIT_RANK_DEFICIENT; }
    EXPECT(threw);
    zg_free(dfrom); zg_free(dto);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    check(zg_init(0));
    double recording[60];
    FILE *f = std::fopen((std::string(argv[1]) + "/transform_cpp_records.bin").c_str(), "rb");
    if (!f || std::fread(recording, sizeof recording, 1, f) != 1) { std::printf("FAIL: no recording\n"); return 1; }
    std::fclose(f);
    one_scalar<float>(recording);
    one_scalar<double>(recording);
    warps();
    if (failures) return 1;
    std::printf("cpp transform ok\n");
    return 0;
}
