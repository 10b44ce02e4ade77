// BitmapFont and Canvas<T>::drawText (zignal_amd/cpp/zignal_hip.hpp) against results recorded from the Python restatement of the reference
// (tests/canvas_text_ref.py; the recordings are tests/golden/canvas_text_cpp_{soft,fast}.rgba, which tests/test_cpp_canvas_text.py holds to
// the restatement): text between other commands through the host form (Canvas<T>::flush over an Image) and through the device form
// (Canvas<T, DeviceImage>::flush, which cuts the list into runs). The two fonts are made here and, the same way, in the Python test.
// Needs a GPU: built and run by tests/test_cpp_canvas_text.py, which passes the directory of the recordings.
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

static Image<Px> frame() { // tests/test_cpp_canvas_curves.py makes the same frame
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

// `count` bytes of the LCG above from seed `s` (its top byte), as tests/test_cpp_canvas_text.py makes them
static std::vector<uint8_t> noise(uint32_t s, size_t count) {
    std::vector<uint8_t> out(count);
    for (size_t i = 0; i < count; ++i) {
        s = s * 1664525u + 1013904223u;
        out[i] = (uint8_t)(s >> 24);
    }
    return out;
}
// an 8 x 8 fixed font for 'H' .. 'O': noise, with H two bars and a bridge, I a bar, O a box
static BitmapFont fixedFont() {
    std::vector<uint8_t> data = noise(7, 8 * 8);
    const uint8_t H[8] = {0x81, 0x81, 0x81, 0x81, 0xFF, 0x81, 0x81, 0x81}, I[8] = {0x7E, 0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x7E},
                  O[8] = {0xFF, 0x81, 0x81, 0x81, 0x81, 0x81, 0x81, 0xFF};
    std::memcpy(&data[0], H, 8);
    std::memcpy(&data[8], I, 8);
    std::memcpy(&data[56], O, 8);
    return BitmapFont::fromFixed(8, 8, 'H', data);
}
// a glyph table: 'j' reaches left of the pen, U+03A9 is taller than the line and two bytes wide, U+2192 advances by nothing
static BitmapFont tableFont() {
    std::vector<uint8_t> data = noise(11, 12 + 28 + 5);
    std::vector<zg_glyph> glyphs(3);
    glyphs[0] = zg_glyph{0x2192, 40, 7, 5, 0, 3, 0};
    glyphs[1] = zg_glyph{'j', 0, 6, 12, -2, 1, 5};
    glyphs[2] = zg_glyph{0x3A9, 12, 11, 14, -1, -2, 12};
    return BitmapFont::fromGlyphs(10, glyphs, data, 9);
}

// the list tests/test_cpp_canvas_text.py records
template <class C> static void scene(C &cv, const BitmapFont &fixed, const BitmapFont &table, float scale, DrawMode mode, Px color) {
    cv.fillRectangle({4.0f, 3.0f, 56.0f, 40.0f}, Px{20, 30, 200, 160}, DrawMode::soft);
    cv.drawText("HI\nOK", {6.5f, 5.25f}, color, fixed, scale, mode);
    cv.drawLine({2.0f, 8.0f}, {60.0f, 30.0f}, Px{250, 250, 10, 128}, 3, DrawMode::soft);
    cv.drawText("NO", {-3.0f, 20.5f}, color, fixed, 1.0f, mode);
    cv.drawText("j\xCE\xA9\xE2\x86\x92j", {30.0f, 28.0f}, color, table, scale, mode); // j, U+03A9, U+2192, j
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_canvas_text <directory of the recordings>\n"); return 2; }
    check(zg_init(0));
    const Image<Px> src = frame();
    const BitmapFont fixed = fixedFont(), table = tableFont();
    const Px translucent{250, 20, 60, 128}, opaque{10, 200, 90, 255};
    {
        const Rectangle<float> b = fixed.textBounds("HI\nOK", 2.5f), t = table.textBounds("j\xCE\xA9\xE2\x86\x92j", 1.0f);
        EXPECT(b.l == 0 && b.t == 0 && b.r == 40.0f && b.b == 40.0f);
        EXPECT(t.r == 22.0f && t.b == 10.0f);
        const std::vector<uint32_t> cps = decodeUtf8("j\xCE\xA9\xE2\x86\x92\xF0\x9F\x98\x80");
        EXPECT(cps.size() == 4 && cps[0] == 'j' && cps[1] == 0x3A9 && cps[2] == 0x2192 && cps[3] == 0x1F600);
    }
    for (int m = 0; m < 2; ++m) {
        const DrawMode mode = m ? DrawMode::soft : DrawMode::fast;
        const float scale = m ? 2.5f : 1.5f;
        const Px color = m ? translucent : opaque;
        const std::vector<uint8_t> want = recording(std::string(argv[1]) + (m ? "/canvas_text_cpp_soft.rgba" : "/canvas_text_cpp_fast.rgba"));
        EXPECT(want.size() == (size_t)ROWS * COLS * 4);
        Image<Px> host = src;
        Canvas<Px> hc(host);
        scene(hc, fixed, table, scale, mode, color);
        EXPECT(hc.commands().size() == 2);
        hc.flush();
        EXPECT(sameBytes(host, want));
        Stream stream = Stream::create();
        DeviceImage<Px> dev = DeviceImage<Px>::fromHost(src, stream.handle());
        Canvas<Px, DeviceImage> dc(dev);
        scene(dc, fixed, table, scale, mode, color);
        dc.flush();
        Image<Px> back = Image<Px>::init(ROWS, COLS);
        dev.download(back);
        EXPECT(sameBytes(back, want));
    }
    { // outside the contract: refused by the host form before anything is drawn; scale <= 0 is inside it and draws nothing
        Image<Px> host = src;
        Canvas<Px> cv(host);
        cv.drawText("HI", {10.0f, 10.0f}, opaque, fixed, NAN);
        bool thrown = false;
        try { cv.flush(); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown && std::memcmp(host.data, src.data, (size_t)ROWS * COLS * 4) == 0);
        cv.drawText("HI", {10.0f, 10.0f}, opaque, fixed, -1.0f, DrawMode::soft);
        cv.flush();
        EXPECT(std::memcmp(host.data, src.data, (size_t)ROWS * COLS * 4) == 0);
        thrown = false;
        try { std::vector<zg_glyph> twice(2, zg_glyph{'a', 0, 1, 1, 0, 0, 1}); (void)BitmapFont::fromGlyphs(8, twice, std::vector<uint8_t>(4), 8); } catch (const InvalidArgument &) { thrown = true; }
        EXPECT(thrown);
    }
    if (failures) { std::printf("cpp canvas text: %d failure(s)\n", failures); return 1; }
    std::printf("cpp canvas text ok\n");
    return 0;
}
