// The arc methods of Canvas<T> (zignal_amd/cpp/zignal_hip.hpp) against results recorded from the Python restatement of the reference
// (tests/canvas_arcs_ref.py; the recordings are tests/golden/canvas_arcs_cpp_{soft,fast}.rgba, which tests/test_cpp_canvas_arcs.py holds
// to the restatement): drawArc and fillArc through the host form (Canvas<T>::flush over an Image) and through the device form
// (Canvas<T, DeviceImage>::flush, which takes zg_canvas_draw_arcs for a list that holds an arc). Needs a GPU: built and run by
// tests/test_cpp_canvas_arcs.py, which passes the directory of the recordings.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../zignal_amd/cpp/zignal_hip.hpp"

using namespace zignal;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

typedef Rgba<uint8_t> Px;
static const uint32_t ROWS = 48, COLS = 64;

static Image<Px> frame() { // tests/test_cpp_canvas_arcs.py makes the same frame
    Image<Px> im = Image<Px>::init(ROWS, COLS);
    uint32_t s = 99;
    for (uint32_t r = 0; r < ROWS; ++r)
        for (uint32_t c = 0; c < COLS; ++c) {
            s = s * 1664525u + 1013904223u;
            im.at(r, c) = Px{(uint8_t)(s >> 24), (uint8_t)(s >> 16), (uint8_t)(s >> 8), (uint8_t)((s & 3) == 0 ? 0 : ((s & 3) == 1 ? 140 : 255))};
        }
    return im;
}
static bool sameBytes(const Image<Px> &a, const std::vector<uint8_t> &b) {
    return b.size() == (size_t)a.rows * a.cols * sizeof(Px) && std::memcmp(a.data, b.data(), b.size()) == 0;
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

// the list tests/test_cpp_canvas_arcs.py records; every angle is an f32 value
template <class C> static void arcs(C &cv, uint32_t width, DrawMode mode, Px color) {
    cv.fillArc({30.0f, 24.0f}, 20.0f, 0.5f, 4.0f, color, mode);
    cv.drawLine({2.0f, 3.0f}, {60.0f, 40.0f}, color, 2, mode);
    cv.drawArc({32.0f, 22.5f}, 18.0f, 4.0f, 1.0f, color, width, mode);
    cv.drawArc({16.0f, 16.0f}, 12.0f, -2.5f, -0.5f, color, 1, mode);
    cv.fillArc({44.25f, 30.5f}, 11.0f, 5.5f, 8.0f, color, mode);
    cv.drawArc({40.0f, 24.0f}, 9.0f, 0.25f, 7.0f, color, width, mode); // 2 pi and more: the circle
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_canvas_arcs <directory of the recordings>\n"); return 2; }
    check(zg_init(0));
    const Image<Px> src = frame();
    const Px translucent{250, 20, 60, 128}, opaque{10, 200, 90, 255};
    for (int m = 0; m < 2; ++m) {
        const DrawMode mode = m ? DrawMode::soft : DrawMode::fast;
        const uint32_t width = m ? 2u : 3u;
        const Px color = m ? translucent : opaque;
        const std::vector<uint8_t> want = recording(std::string(argv[1]) + (m ? "/canvas_arcs_cpp_soft.rgba" : "/canvas_arcs_cpp_fast.rgba"));
        EXPECT(want.size() == (size_t)ROWS * COLS * 4);
        Image<Px> host = src;
        Canvas<Px> hc(host);
        arcs(hc, width, mode, color);
        EXPECT(hc.commands().size() == 6 && hc.commands()[0].kind == ZG_DRAW_FILL_ARC && hc.commands()[2].kind == ZG_DRAW_ARC && hc.commands()[2].n_vertices == 1);
        hc.flush();
        EXPECT(sameBytes(host, want));
        Stream stream = Stream::create();
        DeviceImage<Px> dev = DeviceImage<Px>::fromHost(src, stream.handle());
        Canvas<Px, DeviceImage> dc(dev);
        arcs(dc, width, mode, color);
        dc.flush();
        Image<Px> back = Image<Px>::init(ROWS, COLS);
        dev.download(back);
        EXPECT(sameBytes(back, want));
    }
    { // outside the contract: refused by the host form before anything is drawn; an angle that is not finite is inside it and draws nothing
        Image<Px> host = src;
        Canvas<Px> cv(host);
        cv.drawArc({10.0f, 10.0f}, NAN, 0.0f, 1.0f, opaque, 2);
        bool thrown = false;
        try { cv.flush(); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown && std::memcmp(host.data, src.data, (size_t)ROWS * COLS * 4) == 0);
        cv.fillArc({10.0f, 10.0f}, 8.0f, NAN, 1.0f, opaque, DrawMode::soft);
        cv.flush();
        EXPECT(std::memcmp(host.data, src.data, (size_t)ROWS * COLS * 4) == 0);
    }
    if (failures) { std::printf("cpp canvas arcs: %d failure(s)\n", failures); return 1; }
    std::printf("cpp canvas arcs ok\n");
    return 0;
}
