// Canvas<T> of the C++ host mirror against the reference's loops (src/canvas/Canvas.zig) written out here for the calls whose loops are
// short: fillRectangle in both modes (:608-632, with Rgba.blend(.normal), src/blending.zig:27-157), drawLine's Bresenham walk (:187-240)
// and drawBresenhamCircle (:826-860) with a translucent colour, which blends the points that two of its eight offsets name twice. Then a
// list of every kind of command through the host form and the device form (Canvas<T, DeviceImage>::flush and ::draw with a device count
// word), which must agree byte for byte. Needs a GPU: built and run by tests/test_cpp_canvas.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

typedef Rgba<uint8_t> Px;

// volatile keeps one rounding an operation, whatever the compiler's flags
static uint8_t toU8(float v) {
    volatile float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    volatile float s = 255.0f * c;
    return (uint8_t)(int)std::round(s);
}
static Px blendNormal(Px base, Px o) {
    if (o.a == 0) return base;
    if (base.a == 0 || o.a == 255) return o;
    volatile float b[4] = {base.r / 255.0f, base.g / 255.0f, base.b / 255.0f, base.a / 255.0f};
    volatile float v[4] = {o.r / 255.0f, o.g / 255.0f, o.b / 255.0f, o.a / 255.0f};
    volatile float one_minus = 1.0f - v[3];
    volatile float base_weight = b[3] * one_minus;
    volatile float result_a = v[3] + base_weight;
    volatile float inv = 1.0f / result_a;
    uint8_t out[3];
    for (int i = 0; i < 3; ++i) {
        volatile float x = v[i] * v[3];
        volatile float y = b[i] * base_weight;
        volatile float s = x + y;
        volatile float t = s * inv;
        out[i] = toU8(t);
    }
    return Px{out[0], out[1], out[2], toU8(result_a)};
}
static void setPixel(const Image<Px> &im, int64_t row, int64_t col, Px color) {
    if (row < 0 || col < 0 || row >= im.rows || col >= im.cols) return;
    im.at(row, col) = color.a != 255 ? blendNormal(im.at(row, col), color) : color;
}
static uint32_t clampCoord(float v, uint32_t size) { return (uint32_t)std::trunc(std::fmax(0.0f, std::fmin(v, (float)size))); }
static void refFillRectangle(const Image<Px> &im, Rectangle<float> r, Px color, DrawMode mode) {
    const uint32_t l = clampCoord(r.l, im.cols), t = clampCoord(r.t, im.rows), rr = clampCoord(r.r, im.cols), b = clampCoord(r.b, im.rows);
    if (l >= rr || t >= b) return;
    for (uint32_t row = t; row < b; ++row)
        for (uint32_t col = l; col < rr; ++col) {
            if (mode == DrawMode::fast) im.at(row, col) = color; else setPixel(im, row, col, color);
        }
}
static void refLineBresenham(const Image<Px> &im, Point2 p1, Point2 p2, Px color) { // the general case: neither horizontal nor vertical
    int x1 = (int)p1.x, y1 = (int)p1.y;
    const int x2 = (int)p2.x, y2 = (int)p2.y;
    const int dx = std::abs(x2 - x1), dy = std::abs(y2 - y1), sx = x1 < x2 ? 1 : -1, sy = y1 < y2 ? 1 : -1;
    int err = dx - dy;
    for (;;) {
        if (y1 >= 0 && x1 >= 0 && y1 < (int)im.rows && x1 < (int)im.cols) im.at(y1, x1) = color;
        if (x1 == x2 && y1 == y2) break;
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x1 += sx; }
        if (e2 < dx) { err += dx; y1 += sy; }
    }
}
static void refCircleBresenham(const Image<Px> &im, Point2 center, float radius, Px color) {
    const float cx = std::round(center.x), cy = std::round(center.y);
    float x = std::round(radius), y = 0, err = 0;
    while (x >= y) {
        const float o[8][2] = {{x, y}, {-x, y}, {x, -y}, {-x, -y}, {y, x}, {-y, x}, {y, -x}, {-y, -x}};
        for (const auto &p : o) setPixel(im, (int64_t)std::floor(cy + p[1]), (int64_t)std::floor(cx + p[0]), color);
        if (err <= 0) { y += 1; err += 2 * y + 1; }
        if (err > 0) { x -= 1; err -= 2 * x + 1; }
    }
}

static Image<Px> frame(uint32_t rows, uint32_t cols) {
    Image<Px> im = Image<Px>::init(rows, cols);
    uint32_t s = 99;
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t c = 0; c < cols; ++c) {
            s = s * 1664525u + 1013904223u;
            im.at(r, c) = Px{(uint8_t)(s >> 24), (uint8_t)(s >> 16), (uint8_t)(s >> 8), (uint8_t)((s & 3) == 0 ? 0 : ((s & 3) == 1 ? 140 : 255))};
        }
    return im;
}
static bool sameBytes(const Image<Px> &a, const Image<Px> &b) { return std::memcmp(a.data, b.data, (size_t)a.rows * a.cols * sizeof(Px)) == 0; }

template <class C> static void everyKind(C &cv, uint32_t width, DrawMode mode, Px color) {
    cv.fillRectangle({4.5f, 6.0f, 40.0f, 30.25f}, color, mode).drawLine({2.5f, 3.0f}, {50.0f, 41.5f}, color, width, mode);
    cv.drawLine({10.0f, 44.0f}, {55.0f, 44.0f}, color, width, mode).drawRectangle({8.0f, 9.0f, 47.0f, 38.0f}, color, width, mode);
    cv.drawCircle({30.0f, 25.0f}, 14.5f, color, width, mode).fillCircle({20.25f, 30.5f}, 9.0f, color, mode);
    cv.drawPolygon({{30, 4}, {56, 20}, {40, 46}, {6, 36}}, color, width, mode);
    cv.fillPolygon({{5, 5}, {20, 22}, {36, 6}, {54, 30}, {30, 45}, {4, 34}}, color, mode);
}

int main() {
    check(zg_init(0));
    const uint32_t rows = zg_canvas_tile() * 3 + 2, cols = zg_canvas_tile() * 3 + 11;
    const Image<Px> src = frame(rows, cols);
    const Px translucent{250, 20, 60, 128}, opaque{10, 200, 90, 255};

    { // the reference's loops
        Image<Px> want = src, got = src;
        refFillRectangle(want, {3.7f, -2.0f, 41.2f, 33.9f}, translucent, DrawMode::soft);
        refFillRectangle(want, {20.0f, 20.0f, 900.0f, 27.5f}, translucent, DrawMode::fast);
        refLineBresenham(want, {-4.0f, 2.0f}, {52.9f, 40.1f}, opaque);
        refLineBresenham(want, {30.5f, 48.0f}, {22.0f, -3.0f}, translucent);
        refCircleBresenham(want, {25.4f, 24.6f}, 17.3f, translucent);
        refCircleBresenham(want, {3.0f, 40.0f}, 0.3f, translucent);
        Canvas<Px> cv(got);
        cv.fillRectangle({3.7f, -2.0f, 41.2f, 33.9f}, translucent, DrawMode::soft).fillRectangle({20.0f, 20.0f, 900.0f, 27.5f}, translucent, DrawMode::fast);
        cv.drawLine({-4.0f, 2.0f}, {52.9f, 40.1f}, opaque).drawLine({30.5f, 48.0f}, {22.0f, -3.0f}, translucent);
        cv.drawCircle({25.4f, 24.6f}, 17.3f, translucent).drawCircle({3.0f, 40.0f}, 0.3f, translucent);
        EXPECT(cv.commands().size() == 6);
        cv.flush();
        EXPECT(cv.commands().empty());
        EXPECT(sameBytes(got, want));
        EXPECT(!sameBytes(got, src));
    }
    // every kind: host form == device form (flush), and the device-list form with a count word draws the prefix
    for (int m = 0; m < 2; ++m)
        for (uint32_t width : {1u, 2u, 5u}) {
            const DrawMode mode = m ? DrawMode::soft : DrawMode::fast;
            Image<Px> host = src;
            Canvas<Px> hc(host);
            everyKind(hc, width, mode, translucent);
            const std::vector<zg_draw_cmd> cmds = hc.commands();
            hc.flush();
            Stream stream = Stream::create();
            DeviceImage<Px> dev = DeviceImage<Px>::fromHost(src, stream.handle());
            Canvas<Px, DeviceImage> dc(dev);
            everyKind(dc, width, mode, translucent);
            dc.flush();
            Image<Px> back = Image<Px>::init(rows, cols);
            dev.download(back);
            EXPECT(sameBytes(back, host));
            EXPECT(!sameBytes(back, src));
            // the first three commands (no polygon among them) from device memory, counted by a device word
            Image<Px> prefix = src;
            Canvas<Px> pc(prefix);
            pc.fillRectangle({4.5f, 6.0f, 40.0f, 30.25f}, translucent, mode).drawLine({2.5f, 3.0f}, {50.0f, 41.5f}, translucent, width, mode);
            pc.drawLine({10.0f, 44.0f}, {55.0f, 44.0f}, translucent, width, mode);
            pc.flush();
            void *mem = nullptr;
            check(zg_malloc(&mem, cmds.size() * sizeof(zg_draw_cmd) + 16));
            const uint32_t three = 3;
            check(zg_memcpy_h2d((char *)mem + 16, cmds.data(), cmds.size() * sizeof(zg_draw_cmd), stream.handle()));
            check(zg_memcpy_h2d(mem, &three, 4, stream.handle()));
            dev.upload(src);
            dc.draw((const zg_draw_cmd *)((char *)mem + 16), (uint32_t)cmds.size(), (const uint32_t *)mem);
            dev.download(back);
            EXPECT(sameBytes(back, prefix));
            check(zg_free(mem));
        }
    { // outside the contract: refused by the host form before anything is drawn
        Image<Px> host = src;
        Canvas<Px> cv(host);
        cv.fillCircle({10, 10}, 5, opaque).drawLine({0, 0}, {NAN, 5}, opaque);
        bool thrown = false;
        try { cv.flush(); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown && sameBytes(host, src));
    }
    if (failures) { std::printf("cpp canvas: %d failure(s)\n", failures); return 1; }
    std::printf("cpp canvas ok\n");
    return 0;
}
