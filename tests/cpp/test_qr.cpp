// zignal::QrDetector of the C++ host mirror against tests/golden/qr_cpp_case.bin, which tests/qr_ref.py wrote: a binary map (rows, cols
// as u32, then the bytes), the restatement's detection record, the number of grids, the grid records and the module bytes. The host form
// and the device form must both return that bit for bit; the asynchronous form honours its capacities; a grey frame made from the map
// gives the same grids through both thresholds. argv[1]: the fixture. Needs a GPU: built and run by tests/test_cpp_qr.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool same(const std::vector<QrGrid> &got, const std::vector<zg_qr_grid> &grids, const std::vector<uint8_t> &modules, int binarize) {
    if (got.size() != grids.size()) return false;
    for (size_t i = 0; i < got.size(); ++i) {
        const zg_qr_grid &w = grids[i];
        const QrGrid &g = got[i];
        if (g.binarize != binarize || g.version != w.version || g.dim != w.dim || g.fourth_index != w.fourth_index || g.version_hint != w.version_hint) return false;
        if (std::memcmp(g.corners, w.corners, sizeof w.corners) || std::memcmp(g.transform, w.transform, sizeof w.transform)) return false;
        if (g.modules.size() != (size_t)w.dim * w.dim || std::memcmp(g.modules.data(), &modules[w.modules_offset], g.modules.size())) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t shape[2], n = 0;
    EXPECT(std::fread(shape, 4, 2, f) == 2);
    const size_t pixels = (size_t)shape[0] * shape[1];
    Image<uint8_t> binary = Image<uint8_t>::init(shape[0], shape[1]);
    EXPECT(std::fread(binary.data, 1, pixels, f) == pixels);
    zg_qr_detection want;
    EXPECT(std::fread(&want, sizeof want, 1, f) == 1);
    EXPECT(std::fread(&n, 4, 1, f) == 1);
    std::vector<zg_qr_grid> grids(n);
    EXPECT(std::fread(grids.data(), sizeof(zg_qr_grid), n, f) == n);
    std::vector<uint8_t> modules(want.modules_written);
    EXPECT(std::fread(modules.data(), 1, modules.size(), f) == modules.size());
    std::fclose(f);
    EXPECT(n >= 2 && want.grids_total == n && want.grids_written == n);

    check(zg_init(0));
    const QrDetector detector;
    std::vector<QrGrid> got;
    zg_qr_detection det = detector.detectPass(binary, ZG_QR_BINARY, got);
    EXPECT(std::memcmp(&det, &want, sizeof det) == 0);
    EXPECT(same(got, grids, modules, ZG_QR_BINARY));

    Stream stream = Stream::create();
    DeviceImage<uint8_t> dev = DeviceImage<uint8_t>::init(shape[0], shape[1], stream.handle());
    check(zg_memcpy_h2d(dev.data, binary.data, pixels, stream.handle()));
    got.clear();
    det = detector.detectPass(dev, ZG_QR_BINARY, got);
    EXPECT(std::memcmp(&det, &want, sizeof det) == 0);
    EXPECT(same(got, grids, modules, ZG_QR_BINARY));

    // the asynchronous form with room for one grid: one whole grid, the full need in grids_total
    void *mem = nullptr;
    check(zg_malloc(&mem, 65536));
    zg_qr_detection *ddet = (zg_qr_detection *)mem;
    zg_qr_grid *dgrids = (zg_qr_grid *)((char *)mem + 2048);
    uint8_t *dmodules = (uint8_t *)mem + 4096;
    detector.detectInto(dev, ZG_QR_BINARY, ddet, dgrids, 1, dmodules, 60000);
    zg_qr_grid first;
    check(zg_memcpy_d2h(&det, ddet, sizeof det, stream.handle()));
    check(zg_memcpy_d2h(&first, dgrids, sizeof first, stream.handle()));
    EXPECT(det.grids_total == n && det.grids_written == 1 && det.modules_written == grids[0].dim * grids[0].dim);
    EXPECT(std::memcmp(&first, &grids[0], sizeof first) == 0);
    check(zg_free(mem));

    // a grey frame with the map's two levels far apart: both thresholds give the map back, so detect() is the list twice
    Image<uint8_t> gray = Image<uint8_t>::init(shape[0], shape[1]);
    for (size_t i = 0; i < pixels; ++i) gray.data[i] = binary.data[i] ? 200 : 30;
    std::vector<QrGrid> passes = detector.detect(gray);
    std::vector<QrGrid> otsu;
    bool ordered = true; // the adaptive pass's grids first
    for (const QrGrid &g : passes) {
        if (g.binarize == ZG_QR_OTSU) otsu.push_back(g);
        else ordered = ordered && otsu.empty() && g.binarize == ZG_QR_ADAPTIVE;
    }
    EXPECT(ordered && same(otsu, grids, modules, ZG_QR_OTSU));

    if (failures) { std::printf("cpp qr: %d failure(s)\n", failures); return 1; }
    std::printf("cpp qr ok\n");
    return 0;
}
