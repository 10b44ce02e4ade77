// The quantisation module of the C++ host mirror (DeviceImage<T>::colorHistogram, medianCut, dither, mapToPalette, Palette) against the
// reference's loops written out here: applyErrorDiffusion as the in-place scatter of src/image/dither.zig:208-331 with its interior and
// its bounds-checked branch, applyOrdered (:113-196), ColorLookupTable.init (src/image/quantize.zig:66-159), the histogram scan of
// medianCut (:188-237) and mapImageToPalette (src/codecs/gif.zig:875-920). Frames lie past a band and a phase of the device kernel
// in both directions. Needs a GPU: built and run by tests/test_cpp_quantize.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;
typedef Rgb<uint8_t> Px;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static std::vector<uint8_t> refLut(const Px *pal, uint32_t n) {
    std::vector<uint8_t> lut(32768);
    for (int r = 0; r < 32; ++r)
        for (int g = 0; g < 32; ++g)
            for (int b = 0; b < 32; ++b) {
                const int tr = r << 3 | r >> 2, tg = g << 3 | g >> 2, tb = b << 3 | b >> 2;
                uint32_t best = 0xffffffffu;
                for (uint32_t i = 0; i < n; ++i) {
                    const int dr = pal[i].r - tr, dg = pal[i].g - tg, db = pal[i].b - tb;
                    const uint32_t score = (uint32_t)(dr * dr + dg * dg + db * db) << 8 | i;
                    if (score < best) best = score;
                }
                lut[r << 10 | g << 5 | b] = (uint8_t)(best & 0xff);
            }
    return lut;
}
static uint8_t lookup(const std::vector<uint8_t> &lut, Px p) { return lut[(p.r >> 3) << 10 | (p.g >> 3) << 5 | (p.b >> 3)]; }

static int divTruncPow2(int value, int shift) { return value >= 0 ? value >> shift : (value + (1 << shift) - 1) >> shift; }
static uint8_t clampToU8(int v) { return v < 0 ? 0 : v > 255 ? 255 : (uint8_t)v; }
static void updatePixel(Px &p, int er, int eg, int eb, int weight, int shift) {
    p.r = clampToU8(p.r + divTruncPow2(er * weight, shift));
    p.g = clampToU8(p.g + divTruncPow2(eg * weight, shift));
    p.b = clampToU8(p.b + divTruncPow2(eb * weight, shift));
}

struct Entry { int dx, dy, weight, shift; };
static const Entry FS[4] = {{1, 0, 7, 4}, {-1, 1, 3, 4}, {0, 1, 5, 4}, {1, 1, 1, 4}};
static const Entry ATK[6] = {{1, 0, 1, 3}, {2, 0, 1, 3}, {-1, 1, 1, 3}, {0, 1, 1, 3}, {1, 1, 1, 3}, {0, 2, 1, 3}};

static void refErrorDiffusion(Px *data, int rows, int cols, const Px *pal, const std::vector<uint8_t> &lut, bool atkinson) {
    const Entry *entries = atkinson ? ATK : FS;
    const int n_entries = atkinson ? 6 : 4, reach = atkinson ? 2 : 1;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const Px current = data[r * cols + c], quantized = pal[lookup(lut, current)];
            data[r * cols + c] = quantized;
            const int er = current.r - quantized.r, eg = current.g - quantized.g, eb = current.b - quantized.b;
            if (r < rows - reach && c > 0 && c < cols - reach) { // the interior branch: the same entries, unchecked
                for (int k = 0; k < n_entries; ++k) updatePixel(data[(r + entries[k].dy) * cols + c + entries[k].dx], er, eg, eb, entries[k].weight, entries[k].shift);
            } else {
                for (int k = 0; k < n_entries; ++k) {
                    const int nc = c + entries[k].dx, nr = r + entries[k].dy;
                    if (nr >= 0 && nr < rows && nc >= 0 && nc < cols) updatePixel(data[nr * cols + nc], er, eg, eb, entries[k].weight, entries[k].shift);
                }
            }
        }
}

static const int BAYER[8][8] = {{0, 32, 8, 40, 2, 34, 10, 42},  {48, 16, 56, 24, 50, 18, 58, 26}, {12, 44, 4, 36, 14, 46, 6, 38}, {60, 28, 52, 20, 62, 30, 54, 22},
                                {3, 35, 11, 43, 1, 33, 9, 41}, {51, 19, 59, 27, 49, 17, 57, 25}, {15, 47, 7, 39, 13, 45, 5, 37}, {63, 31, 55, 23, 61, 29, 53, 21}};
static void refOrdered(Px *data, int rows, int cols, const Px *pal, const std::vector<uint8_t> &lut) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const int offset = (BAYER[r & 7][c & 7] - 32) >> 1;
            Px &p = data[r * cols + c];
            const Px v{clampToU8(p.r + offset), clampToU8(p.g + offset), clampToU8(p.b + offset)};
            p = pal[lookup(lut, v)];
        }
}

template <typename T> static T *toDevice(const std::vector<T> &v) {
    void *mem = nullptr;
    check(zg_malloc(&mem, v.size() * sizeof(T)));
    check(zg_memcpy_h2d(mem, v.data(), v.size() * sizeof(T), nullptr));
    return (T *)mem;
}

int main() {
    check(zg_init(0));
    uint32_t band = 0, phase = 0, per_launch = 0;
    zg_dither_geometry(&band, &phase, &per_launch);
    EXPECT(band == 64 && phase >= 128 && per_launch >= band);

    // the fixed palettes (quantize.zig:415-473) and the host table against the loop above
    const Palette p676 = Palette::fixed(PaletteMode::fixed6x7x6()), vga = Palette::fixed(PaletteMode::fixedVga16()), web = Palette::fixed(PaletteMode::fixedWeb216());
    EXPECT(p676.size == 252 && vga.size == 16 && web.size == 216);
    EXPECT(p676.colors[251].r == 255 && p676.colors[49].g == 43 && vga.colors[7].b == 192 && web.colors[215].g == 255);
    EXPECT(vga.lookupTable() == refLut(vga.colors, vga.size));

    const uint32_t rows = band + 7, cols = phase + 11;
    std::vector<Px> frame((size_t)rows * cols);
    for (Px &p : frame) p = Px{(uint8_t)(rnd() >> 24), (uint8_t)(rnd() >> 24), (uint8_t)(rnd() >> 24)};
    Palette greys;
    greys.colors[0] = Px{64, 64, 64};
    greys.colors[1] = Px{192, 192, 192};
    greys.size = 2;

    Stream stream = Stream::create();
    const Palette *palettes[3] = {&greys, &vga, &p676};
    for (const Palette *pal : palettes) {
        const std::vector<uint8_t> lut = refLut(pal->colors, pal->size);
        Px *pal_dev = toDevice(std::vector<Px>(pal->colors, pal->colors + pal->size));
        void *lut_mem = nullptr;
        check(zg_malloc(&lut_mem, 32768));
        check(zg_palette_lut(&pal_dev->r, pal->size, (uint8_t *)lut_mem, stream.handle()));
        std::vector<uint8_t> lut_back(32768);
        check(zg_memcpy_d2h(lut_back.data(), lut_mem, 32768, stream.handle()));
        EXPECT(lut_back == lut);
        const DitherMode modes[3] = {DitherMode::floyd_steinberg, DitherMode::atkinson, DitherMode::ordered};
        for (DitherMode mode : modes) {
            std::vector<Px> want = frame;
            if (mode == DitherMode::ordered) refOrdered(want.data(), rows, cols, pal->colors, lut);
            else refErrorDiffusion(want.data(), rows, cols, pal->colors, lut, mode == DitherMode::atkinson);
            DeviceImage<Px> dev = DeviceImage<Px>::init(rows, cols, stream.handle());
            check(zg_memcpy_h2d(dev.data, frame.data(), frame.size() * sizeof(Px), stream.handle()));
            dev.dither(pal_dev, pal->size, (const uint8_t *)lut_mem, mode);
            std::vector<Px> back(frame.size());
            check(zg_memcpy_d2h(back.data(), dev.data, back.size() * sizeof(Px), stream.handle()));
            EXPECT(std::memcmp(back.data(), want.data(), back.size() * sizeof(Px)) == 0);
        }
        // mapImageToPalette with Floyd-Steinberg: the dithered frame looked up again
        {
            std::vector<Px> work = frame;
            refErrorDiffusion(work.data(), rows, cols, pal->colors, lut, false);
            DeviceImage<Px> dev = DeviceImage<Px>::init(rows, cols, stream.handle());
            check(zg_memcpy_h2d(dev.data, frame.data(), frame.size() * sizeof(Px), stream.handle()));
            DeviceImage<uint8_t> indices = DeviceImage<uint8_t>::init(rows, cols, stream.handle());
            dev.mapToPalette(indices, pal_dev, pal->size, true);
            std::vector<uint8_t> back(frame.size());
            check(zg_memcpy_d2h(back.data(), indices.data, back.size(), stream.handle()));
            bool same = true;
            for (size_t i = 0; i < back.size(); ++i) same = same && back[i] == lookup(lut, work[i]);
            EXPECT(same);
        }
        check(zg_free(lut_mem));
        check(zg_free(pal_dev));
    }

    // the histogram scan of medianCut: counts, and the order in which the cells were first met
    {
        DeviceImage<Px> dev = DeviceImage<Px>::init(rows, cols, stream.handle());
        check(zg_memcpy_h2d(dev.data, frame.data(), frame.size() * sizeof(Px), stream.handle()));
        void *mem = nullptr;
        check(zg_malloc(&mem, 2 * 32768 * sizeof(uint32_t)));
        dev.colorHistogram((uint32_t *)mem, (uint32_t *)mem + 32768);
        std::vector<uint32_t> got(2 * 32768), counts(32768, 0), first(32768, 0xFFFFFFFFu);
        check(zg_memcpy_d2h(got.data(), mem, got.size() * sizeof(uint32_t), stream.handle()));
        for (size_t i = 0; i < frame.size(); ++i) {
            const uint32_t key = (uint32_t)(frame[i].r >> 3) << 10 | (uint32_t)(frame[i].g >> 3) << 5 | (uint32_t)(frame[i].b >> 3);
            if (counts[key]++ == 0) first[key] = (uint32_t)i;
        }
        EXPECT(std::memcmp(got.data(), counts.data(), 32768 * 4) == 0 && std::memcmp(got.data() + 32768, first.data(), 32768 * 4) == 0);
        check(zg_stream_synchronize(stream.handle()));
        const Palette cut = dev.medianCut(16), built = dev.buildPalette(PaletteMode::adaptive(16));
        Palette host_cut;
        check(zg_median_cut_from_histogram_host(counts.data(), first.data(), 16, 256, &host_cut.colors[0].r, &host_cut.size));
        EXPECT(cut.size == 16 && built.size == 16 && host_cut.size == 16);
        EXPECT(std::memcmp(cut.colors, host_cut.colors, 48) == 0 && std::memcmp(built.colors, host_cut.colors, 48) == 0);
        check(zg_free(mem));
    }

    if (failures) { std::printf("cpp quantize: %d failure(s)\n", failures); return 1; }
    std::printf("cpp quantize ok\n");
    return 0;
}
