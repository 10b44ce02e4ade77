// canvas_text.hip — Canvas(T).drawText (reference src/canvas/Canvas.zig:1476-1658) with the parts of BitmapFont it calls
// (src/font/BitmapFont.zig:61-170, :226-248) as a device operation of its own over a list of text commands and a caller-supplied font:
//   renderGlyphUnscaled    :1548-1582  scale == 1 in either mode: one write per lit bit at floor(pen) + offsets
//   renderGlyphFastScaled  :1586-1605  a block of pixels per lit bit, clipped to the text rectangle; neighbouring blocks overlap at a
//                                      fractional scale, so one glyph can write a pixel two or four times
//   renderGlyphSoftScaled  :1609-1658  per destination pixel the box-filtered coverage of the source bits as alpha
// composited exactly as the canvas composites (zg_blend.h), through the gather and the pixel writer k_canvas uses (zg_canvas_tile.h): every
// write is applied in the reference's order and as often as the reference makes it.
//   k_text_prep   one lane per command: checks the command, runs getTextBounds and then the pen — two sequential f32 recurrences that must
//                 not re-associate — and writes one entry per codepoint (pen position, resolved glyph, pixel box) and the command's clip
//                 rectangle. A command's entries begin at the sum of the codepoints of the commands before it, so the entries are in
//                 (command, codepoint) order by construction and their number is bounded by what the host knows (n_codepoints).
//   k_text        per tile: tile_gather over the entries, with an entry's box as the test and its glyph, by one of the three paths, as what
//                 a hit does.
#include "zg_canvas_tile.h"
#include "zg_scan.h"

#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace zg {

// One codepoint of one command as k_text_prep resolved it. 32 bytes.
struct TxEntry {
    float x, y;             // the pen before the glyph
    uint32_t bitmap_offset; // into font.data
    uint32_t cmd;
    uint8_t width, height, bytes_per_row, pad;
    int16_t x_offset, y_offset;
    ushort4 box; // l t r b in pixels, r and b exclusive, inside the image; all 0: nothing to draw
};
static_assert(sizeof(TxEntry) == 32, "TxEntry is 32 bytes");

struct TxGlyph { // getGlyphInfo + getCharData
    uint32_t bitmap_offset;
    int width, height, x_offset, y_offset, bytes_per_row;
};

// The glyph table's entry for a codepoint, or n_glyphs: the table is sorted and every codepoint is unique
__host__ __device__ inline uint32_t tx_find(const zg_font &f, uint32_t cp) {
    uint32_t lo = 0, hi = f.n_glyphs;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (f.glyphs[mid].codepoint < cp) lo = mid + 1; else hi = mid;
    }
    return lo < f.n_glyphs && f.glyphs[lo].codepoint == cp ? lo : f.n_glyphs;
}
// getCharAdvanceWidth (:118-139)
__host__ __device__ inline float tx_advance(const zg_font &f, uint32_t cp) {
    if (f.glyphs == nullptr) return (float)f.char_width;
    const uint32_t i = tx_find(f, cp);
    if (i == f.n_glyphs) return (float)f.char_width;
    return f.glyphs[i].device_width > 0 ? (float)f.glyphs[i].device_width : 0.0f;
}
// getGlyphInfo and getCharData both non-null (:65-92, :226-248), and the bitmap inside data_len
__host__ __device__ inline bool tx_glyph(const zg_font &f, uint32_t cp, TxGlyph &g) {
    uint64_t size;
    if (f.glyphs == nullptr) {
        if (cp > 255u || cp < f.first_char || cp > f.last_char) return false;
        g.width = f.char_width; g.height = f.char_height; g.x_offset = 0; g.y_offset = 0;
        g.bytes_per_row = ((int)f.char_width + 7) / 8;
        size = (uint64_t)g.height * (uint64_t)g.bytes_per_row;
        const uint64_t offset = (uint64_t)(cp - f.first_char) * size;
        if (offset + size > f.data_len) return false;
        g.bitmap_offset = (uint32_t)offset;
        return true;
    }
    const uint32_t i = tx_find(f, cp);
    if (i == f.n_glyphs) return false;
    const zg_glyph q = f.glyphs[i];
    g.width = q.width; g.height = q.height; g.x_offset = q.x_offset; g.y_offset = q.y_offset;
    g.bytes_per_row = ((int)q.width + 7) / 8;
    size = (uint64_t)g.height * (uint64_t)g.bytes_per_row;
    if ((uint64_t)q.bitmap_offset + size > f.data_len) return false;
    g.bitmap_offset = q.bitmap_offset;
    return true;
}

// getTextBounds (:144-170): r = width, b = height; l = t = 0
__host__ __device__ inline void tx_bounds(const zg_font &f, const uint32_t *cps, uint32_t n, float scale, float &out_width, float &out_height) {
    float width = 0, current_line_width = 0, lines = 1;
    const float char_height_scaled = (float)f.char_height * scale;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t cp = cps[k];
        if (cp == 10u) {
            width = fmaxf(width, current_line_width);
            current_line_width = 0;
            lines += 1;
        } else {
            current_line_width += tx_advance(f, cp) * scale;
        }
    }
    out_width = fmaxf(width, current_line_width);
    out_height = lines * char_height_scaled;
}

// The codepoints a command takes of the call's entry budget: its own count when its range lies in the array and is not longer than the bound
__host__ __device__ inline uint32_t tx_budget(const zg_text_cmd &c, uint32_t n_codepoints) {
    if (c.n_codepoints > ZG_TEXT_MAX_CODEPOINTS || c.first_codepoint > n_codepoints || c.n_codepoints > n_codepoints - c.first_codepoint) return 0;
    return c.n_codepoints;
}
// 0: inside the contract. 1: refused as an invalid argument, 2: as unsupported (too many codepoints in one command)
__host__ __device__ inline int tx_check(const zg_text_cmd &c, const uint32_t *codepoints, uint32_t n_codepoints) {
    if (c.mode != ZG_DRAW_FAST && c.mode != ZG_DRAW_SOFT) return 1;
    if (!(fabsf(c.x) <= ZG_CANVAS_MAX_COORD) || !(fabsf(c.y) <= ZG_CANVAS_MAX_COORD)) return 1; // NaN fails both
    if (!(fabsf(c.scale) < INFINITY) || c.scale > ZG_TEXT_MAX_SCALE) return 1;
    if (c.first_codepoint > n_codepoints || c.n_codepoints > n_codepoints - c.first_codepoint) return 1;
    if (c.n_codepoints > ZG_TEXT_MAX_CODEPOINTS) return 2;
    for (uint32_t k = 0; k < c.n_codepoints; ++k)
        if (codepoints[c.first_codepoint + k] > 0x10FFFFu) return 1;
    return 0;
}

__global__ __launch_bounds__(256) void k_text_prep(zg_font font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *count_device, const uint32_t *codepoints,
                                                   uint32_t n_codepoints, int rows, int cols, TxEntry *entries, float4 *clips, uint32_t *total_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t count = count_device ? min(*count_device, n) : n;
    // where this command's entries begin: the budgets of the commands before it, first of the blocks before this one, then inside it
    uint64_t mine = 0;
    for (uint32_t j = threadIdx.x; j < blockIdx.x * 256u; j += 256u)
        if (j < count) mine += tx_budget(cmds[j], n_codepoints);
    uint64_t before_block, block_total;
    block_exclusive_sum64<uint64_t>(mine, &before_block);
    const uint32_t budget = i < count ? tx_budget(cmds[i], n_codepoints) : 0u;
    const uint64_t offset = before_block + block_exclusive_sum64<uint64_t>((uint64_t)budget, &block_total);
    if (i >= n) return;
    const bool fits = offset + budget <= n_codepoints;
    // exactly one lane writes the number of entries: the first command that does not fit (everything from it on is skipped), or the last
    if (!fits && offset <= n_codepoints) *total_out = (uint32_t)offset;
    else if (fits && i == n - 1) *total_out = (uint32_t)(offset + budget);
    if (i >= count || !fits || budget == 0) return;

    const zg_text_cmd c = cmds[i];
    const uint32_t *cps = codepoints + c.first_codepoint;
    TxEntry *out = entries + offset;
    TxEntry e;
    e.x = 0; e.y = 0; e.bitmap_offset = 0; e.cmd = i; e.width = 0; e.height = 0; e.bytes_per_row = 0; e.pad = 0; e.x_offset = 0; e.y_offset = 0;
    e.box = make_ushort4(0, 0, 0, 0);
    bool draws = tx_check(c, codepoints, n_codepoints) == 0 && c.scale > 0;
    float4 clip = make_float4(0, 0, 0, 0);
    if (draws) { // drawText's text_rect, image_rect and Rectangle.intersect (:1501-1514)
        float width, height;
        tx_bounds(font, cps, c.n_codepoints, c.scale, width, height);
        clip.x = fmaxf(c.x + 0.0f, 0.0f); clip.y = fmaxf(c.y + 0.0f, 0.0f);
        clip.z = fminf(c.x + width, (float)cols); clip.w = fminf(c.y + height, (float)rows);
        draws = !(clip.x >= clip.z || clip.y >= clip.w);
    }
    clips[i] = clip;
    if (!draws) {
        for (uint32_t k = 0; k < c.n_codepoints; ++k) out[k] = e;
        return;
    }
    float x = c.x, y = c.y;
    const float start_x = x, line_height = (float)font.char_height * c.scale;
    const float fc = (float)cols, fr = (float)rows;
    for (uint32_t k = 0; k < c.n_codepoints; ++k) {
        const uint32_t cp = cps[k];
        TxEntry g = e;
        if (cp == 10u) {
            x = start_x;
            y += line_height;
            out[k] = g;
            continue;
        }
        TxGlyph q;
        if (tx_glyph(font, cp, q) && q.width > 0 && q.height > 0) {
            g.x = x; g.y = y; g.bitmap_offset = q.bitmap_offset;
            g.width = (uint8_t)q.width; g.height = (uint8_t)q.height; g.bytes_per_row = (uint8_t)q.bytes_per_row;
            g.x_offset = (int16_t)q.x_offset; g.y_offset = (int16_t)q.y_offset;
            // everything any of the three paths can write, three pixels to spare for the rounding of these sums (magnitudes below 2^23)
            const float ox = (float)q.x_offset * c.scale, oy = (float)q.y_offset * c.scale;
            const float l = floorf(x + ox) - 3.0f, t = floorf(y + oy) - 3.0f;
            const float r = ceilf(x + ox + (float)q.width * c.scale) + 4.0f, b = ceilf(y + oy + (float)q.height * c.scale) + 4.0f;
            const int bl = (int)fminf(fmaxf(l, 0.0f), fc), bt = (int)fminf(fmaxf(t, 0.0f), fr);
            const int br = (int)fminf(fmaxf(r, 0.0f), fc), bb = (int)fminf(fmaxf(b, 0.0f), fr);
            if (bl < br && bt < bb) g.box = make_ushort4((unsigned short)bl, (unsigned short)bt, (unsigned short)br, (unsigned short)bb);
        }
        out[k] = g;
        x += tx_advance(font, cp) * c.scale;
    }
}

// getGlyphBit (:1476-1482): bits LSB first; an index past the glyph's slice reads 0
__device__ inline bool tx_bit(const uint8_t *char_data, int len, int row, int col, int bytes_per_row) {
    const int at = row * bytes_per_row + (col >> 3);
    if (at >= len) return false;
    return (char_data[at] >> (col & 7)) & 1;
}

template <int PIX> struct Tx : TilePixel<PIX> {
    using TilePixel<PIX>::col;
    using TilePixel<PIX>::row;
    using TilePixel<PIX>::pixel;

    __device__ __forceinline__ void unscaled(const TxEntry &e, const uint8_t *data, Rgba8 color) {
        const int c = col - ((int)floorf(e.x) + (int)e.x_offset), r = row - ((int)floorf(e.y) + (int)e.y_offset);
        if (c < 0 || c >= (int)e.width || r < 0 || r >= (int)e.height) return;
        if (tx_bit(data + e.bitmap_offset, (int)e.height * (int)e.bytes_per_row, r, c, e.bytes_per_row)) pixel(color);
    }

    // The bits whose block [max(floor(b), clip.lo), min(ceil(b + scale), clip.hi)) can hold pixel p on one axis: b < p + 1 and b + scale > p,
    // so (p - pen) / scale - 1 < index + offset < (p + 1 - pen) / scale. At scale >= 1 that is a window of five around the quotient (the
    // f32 quotient is off by less than 1/2 at these magnitudes); below 1 every bit of the glyph is a candidate. Membership itself is
    // decided with the reference's expressions.
    __device__ __forceinline__ void candidates(float p, float pen, float scale, int offset, int size, int &lo, int &hi) const {
        lo = 0; hi = size - 1;
        if (scale >= 1.0f) {
            const float q = floorf((p - pen) / scale - (float)offset);
            lo = (int)fmaxf(q - 2.0f, 0.0f);
            hi = (int)fminf(q + 2.0f, (float)(size - 1));
        }
    }
    __device__ __forceinline__ bool in_block(float pen, int index, int offset, float scale, float clip_lo, float clip_hi, int p) const {
        const float base = pen + ((float)index + (float)offset) * scale;
        const float start = fmaxf(floorf(base), clip_lo), end = fminf(ceilf(base + scale), clip_hi);
        if (end < 0.0f) return false; // the cast the reference leaves undefined: the bit writes nothing
        return p >= (int)start && p < (int)end;
    }
    __device__ __forceinline__ void fast_scaled(const TxEntry &e, const uint8_t *data, Rgba8 color, float scale, float4 clip) {
        int r0, r1, c0, c1;
        candidates((float)row, e.y, scale, e.y_offset, e.height, r0, r1);
        candidates((float)col, e.x, scale, e.x_offset, e.width, c0, c1);
        const uint8_t *char_data = data + e.bitmap_offset;
        const int len = (int)e.height * (int)e.bytes_per_row;
        int writes = 0;
        for (int r = r0; r <= r1; ++r) {
            if (!in_block(e.y, r, e.y_offset, scale, clip.y, clip.w, row)) continue;
            for (int c = c0; c <= c1; ++c)
                if (tx_bit(char_data, len, r, c, e.bytes_per_row) && in_block(e.x, c, e.x_offset, scale, clip.x, clip.z, col)) ++writes;
        }
        for (int k = 0; k < writes; ++k) pixel(color); // the same colour every time: only the number of writes matters
    }

    __device__ __forceinline__ float coverage(const TxEntry &e, const uint8_t *char_data, int len, float dx, float dy, float scale) const {
        const float glyph_width_f = (float)e.width, glyph_height_f = (float)e.height;
        const float sample_radius = 0.5f / scale;
        const float src_x = dx / scale, src_y = dy / scale;
        const float x0 = src_x - sample_radius, x1 = src_x + sample_radius, y0 = src_y - sample_radius, y1 = src_y + sample_radius;
        const float row_start_f = fmaxf(0.0f, floorf(y0)), row_end_f = fminf(glyph_height_f - 1.0f, ceilf(y1));
        const float col_start_f = fmaxf(0.0f, floorf(x0)), col_end_f = fminf(glyph_width_f - 1.0f, ceilf(x1));
        float total_coverage = 0;
        for (float row_f = row_start_f; row_f <= row_end_f; row_f += 1.0f) {
            for (float col_f = col_start_f; col_f <= col_end_f; col_f += 1.0f) {
                if (!tx_bit(char_data, len, (int)row_f, (int)col_f, e.bytes_per_row)) continue;
                const float overlap_x = clampf(fminf(x1, col_f + 1.0f) - fmaxf(x0, col_f), 0.0f, 1.0f);
                const float overlap_y = clampf(fminf(y1, row_f + 1.0f) - fmaxf(y0, row_f), 0.0f, 1.0f);
                total_coverage += overlap_x * overlap_y;
            }
        }
        const float box_area = (x1 - x0) * (y1 - y0);
        return total_coverage / box_area;
    }
    // dest = pen + d + offset * scale for d = 0, 1, ... below ceil(size * scale); the pixel is floor(dest) (setPoint; atOrNull's trunc gate
    // lets through nothing that floor does not: a coordinate in (-1, 0) passes the gate and is dropped by setPoint). The d that land on this
    // lane's pixel lie within two of p - floor(pen + offset * scale); each is tested with the reference's expression.
    __device__ __forceinline__ void soft_scaled(const TxEntry &e, const uint8_t *data, Rgba8 color, float scale) {
        const float dest_width = ceilf((float)e.width * scale), dest_height = ceilf((float)e.height * scale);
        const float ox = (float)e.x_offset * scale, oy = (float)e.y_offset * scale;
        const float dx_mid = (float)col - floorf(e.x + ox), dy_mid = (float)row - floorf(e.y + oy);
        const uint8_t *char_data = data + e.bitmap_offset;
        const int len = (int)e.height * (int)e.bytes_per_row;
        for (float dy = fmaxf(dy_mid - 2.0f, 0.0f); dy <= dy_mid + 2.0f && dy < dest_height; dy += 1.0f) {
            if (floorf(e.y + dy + oy) != (float)row) continue;
            for (float dx = fmaxf(dx_mid - 2.0f, 0.0f); dx <= dx_mid + 2.0f && dx < dest_width; dx += 1.0f) {
                if (floorf(e.x + dx + ox) != (float)col) continue;
                const float normalized_coverage = coverage(e, char_data, len, dx, dy, scale);
                if (normalized_coverage > 0) pixel(fade(color, normalized_coverage));
            }
        }
    }
};

template <int PIX>
__global__ __launch_bounds__(256) void k_text(DImg img, zg_font font, const zg_text_cmd *cmds, const TxEntry *entries, const float4 *clips, const uint32_t *total) {
    const int tx0 = (int)blockIdx.x * CV_TILE, ty0 = (int)blockIdx.y * CV_TILE;
    Tx<PIX> tx;
    tx.place(img);
    tile_gather<PIX>(
        img, tx, *total, [&](uint32_t i) { return tile_meets_box(entries[i].box, tx0, ty0); },
        [&](uint32_t i) {
            const TxEntry e = entries[i];
            const zg_text_cmd c = cmds[e.cmd];
            if (!tx.inside) return;
            const ushort4 b = e.box;
            if (tx.col < (int)b.x || tx.col >= (int)b.z || tx.row < (int)b.y || tx.row >= (int)b.w) return;
            const Rgba8 color = rgba_of(c.color);
            if (c.scale == 1.0f) tx.unscaled(e, font.data, color);
            else if (c.mode == ZG_DRAW_FAST) tx.fast_scaled(e, font.data, color, c.scale, clips[e.cmd]);
            else tx.soft_scaled(e, font.data, color, c.scale);
        });
}

static int check_text_args(const zg_font *font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *codepoints, uint32_t n_codepoints) {
    ZG_REQUIRE(font != nullptr, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: null font");
    ZG_REQUIRE(font->data_len == 0 || font->data != nullptr, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: null font data");
    ZG_REQUIRE(font->reserved == 0, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: the font's reserved word is %u", font->reserved);
    ZG_REQUIRE(n == 0 || cmds != nullptr, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: null cmds");
    ZG_REQUIRE(n_codepoints == 0 || codepoints != nullptr, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: null codepoints");
    ZG_REQUIRE(n <= ZG_TEXT_MAX_COMMANDS, ZG_ERR_UNSUPPORTED, "canvas_draw_text: %u commands (at most %u a call)", n, ZG_TEXT_MAX_COMMANDS);
    ZG_REQUIRE(n_codepoints <= ZG_TEXT_MAX_TOTAL, ZG_ERR_UNSUPPORTED, "canvas_draw_text: %u codepoints (at most %u a call)", n_codepoints, ZG_TEXT_MAX_TOTAL);
    return ZG_OK;
}

static int text_draw(const zg_image *img, const zg_font &font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *count_device, const uint32_t *codepoints,
                     uint32_t n_codepoints, hipStream_t s) {
    if (n == 0 || n_codepoints == 0 || img->rows == 0 || img->cols == 0) return ZG_OK;
    ScratchBlock sc(s);
    TxEntry *entries;
    float4 *clips;
    uint32_t *total;
    sc.take(entries, n_codepoints);
    sc.take(clips, n);
    sc.take(total, 1);
    int rc;
    if ((rc = sc.alloc())) return rc;
    k_text_prep<<<ceil_div(n, 256), 256, 0, s>>>(font, cmds, n, count_device, codepoints, n_codepoints, (int)img->rows, (int)img->cols, entries, clips, total);
    if ((rc = launch_ok("k_text_prep"))) return rc;
    const dim3 grid = tile_grid(img);
    const DImg d = dimg(img);
    dispatch_u8_pixel(img->pixel, [&](auto pix) { k_text<decltype(pix)::value><<<grid, 256, 0, s>>>(d, font, cmds, entries, clips, total); });
    return launch_ok("k_text");
}

} // namespace zg

using namespace zg;

extern "C" {

size_t zg_sizeof_font(void) { return sizeof(zg_font); }
size_t zg_sizeof_glyph(void) { return sizeof(zg_glyph); }
size_t zg_sizeof_text_cmd(void) { return sizeof(zg_text_cmd); }

int zg_font_check(const zg_font *f) {
    ZG_REQUIRE(f != nullptr, ZG_ERR_INVALID_ARGUMENT, "font_check: null font");
    ZG_REQUIRE(f->data_len == 0 || f->data != nullptr, ZG_ERR_INVALID_ARGUMENT, "font_check: null data");
    ZG_REQUIRE(f->reserved == 0, ZG_ERR_INVALID_ARGUMENT, "font_check: the reserved word is %u", f->reserved);
    if (f->glyphs == nullptr) {
        ZG_REQUIRE(f->n_glyphs == 0, ZG_ERR_INVALID_ARGUMENT, "font_check: %u glyphs and no table", f->n_glyphs);
        ZG_REQUIRE(f->last_char >= f->first_char, ZG_ERR_INVALID_ARGUMENT, "font_check: last_char %u below first_char %u", f->last_char, f->first_char);
        const uint64_t need = (uint64_t)(f->last_char - f->first_char + 1) * f->char_height * (((uint64_t)f->char_width + 7) / 8);
        ZG_REQUIRE(need <= f->data_len, ZG_ERR_INVALID_ARGUMENT, "font_check: %u bytes of data, characters %u .. %u of %u x %u need %llu", f->data_len,
                   f->first_char, f->last_char, f->char_width, f->char_height, (unsigned long long)need);
        return ZG_OK;
    }
    for (uint32_t i = 0; i < f->n_glyphs; ++i) {
        const zg_glyph &g = f->glyphs[i];
        ZG_REQUIRE(g.codepoint <= 0x10FFFFu, ZG_ERR_INVALID_ARGUMENT, "font_check: glyph %u has codepoint 0x%X", i, g.codepoint);
        ZG_REQUIRE(i == 0 || f->glyphs[i - 1].codepoint < g.codepoint, ZG_ERR_INVALID_ARGUMENT,
                   "font_check: glyph %u (codepoint 0x%X) does not come after glyph %u (0x%X): the table is sorted and every codepoint is unique", i, g.codepoint,
                   i - 1, i ? f->glyphs[i - 1].codepoint : 0u);
        const uint64_t size = (uint64_t)g.height * (((uint64_t)g.width + 7) / 8);
        ZG_REQUIRE((uint64_t)g.bitmap_offset + size <= f->data_len, ZG_ERR_INVALID_ARGUMENT, "font_check: glyph %u's bitmap [%u, +%llu) leaves the %u bytes of data", i,
                   g.bitmap_offset, (unsigned long long)size, f->data_len);
    }
    return ZG_OK;
}

int zg_font_upload(const zg_font *host_font, zg_font *device_font) {
    ZG_REQUIRE(device_font != nullptr, ZG_ERR_INVALID_ARGUMENT, "font_upload: null device_font");
    if (const int rc = zg_font_check(host_font)) return rc;
    const size_t table_at = align256((size_t)host_font->data_len + 1); // the bitmaps first, so that the block is the font's data pointer
    char *block = nullptr;
    ZG_HIP(hipMalloc((void **)&block, table_at + (size_t)host_font->n_glyphs * sizeof(zg_glyph) + 1));
    int rc = ZG_OK;
    if (host_font->data_len) rc = upload_pageable(block, host_font->data, host_font->data_len, nullptr);
    if (!rc && host_font->n_glyphs) rc = upload_pageable(block + table_at, host_font->glyphs, (size_t)host_font->n_glyphs * sizeof(zg_glyph), nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = ZG_ERR_HIP;
    if (rc) {
        (void)hipFree(block);
        return rc;
    }
    *device_font = *host_font;
    device_font->data = (const uint8_t *)block;
    device_font->glyphs = host_font->glyphs ? (const zg_glyph *)(block + table_at) : nullptr;
    return ZG_OK;
}

int zg_font_free(zg_font *device_font) {
    if (device_font == nullptr || device_font->data == nullptr) return ZG_OK;
    void *block = (void *)device_font->data;
    std::memset(device_font, 0, sizeof(*device_font));
    ZG_HIP(hipFree(block));
    return ZG_OK;
}

int zg_text_bounds_host(const zg_font *host_font, const uint32_t *codepoints, uint32_t n, float scale, float out_ltrb[4]) {
    ZG_REQUIRE(out_ltrb != nullptr, ZG_ERR_INVALID_ARGUMENT, "text_bounds: null out_ltrb");
    ZG_REQUIRE(n == 0 || codepoints != nullptr, ZG_ERR_INVALID_ARGUMENT, "text_bounds: null codepoints");
    if (const int rc = zg_font_check(host_font)) return rc;
    out_ltrb[0] = 0; out_ltrb[1] = 0;
    tx_bounds(*host_font, codepoints, n, scale, out_ltrb[2], out_ltrb[3]);
    return ZG_OK;
}

int zg_canvas_draw_text(const zg_image *img, const zg_font *font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *count_device, const uint32_t *codepoints,
                        uint32_t n_codepoints, zg_stream stream) {
    if (const int rc = check_draw_image(img, true, "canvas_draw_text")) return rc;
    if (const int rc = check_text_args(font, cmds, n, codepoints, n_codepoints)) return rc;
    ZG_REQUIRE(font->glyphs != nullptr || font->n_glyphs == 0, ZG_ERR_INVALID_ARGUMENT, "canvas_draw_text: %u glyphs and no table", font->n_glyphs);
    return text_draw(img, *font, cmds, n, count_device, codepoints, n_codepoints, as_stream(stream));
}

int zg_canvas_draw_text_host(const zg_image *img, const zg_font *host_font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *codepoints, uint32_t n_codepoints) {
    if (const int rc = check_draw_image(img, false, "canvas_draw_text")) return rc;
    if (const int rc = check_text_args(host_font, cmds, n, codepoints, n_codepoints)) return rc;
    if (const int rc = zg_font_check(host_font)) return rc;
    uint64_t running = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int bad = tx_check(cmds[i], codepoints, n_codepoints);
        ZG_REQUIRE(bad != 2, ZG_ERR_UNSUPPORTED, "canvas_draw_text: command %u has %u codepoints (at most %u)", i, cmds[i].n_codepoints, ZG_TEXT_MAX_CODEPOINTS);
        ZG_REQUIRE(bad == 0, ZG_ERR_INVALID_ARGUMENT,
                   "canvas_draw_text: command %u is outside the contract (mode, finite position of magnitude <= %g, finite scale <= %g, codepoint range, codepoints <= 0x10FFFF)",
                   i, (double)ZG_CANVAS_MAX_COORD, (double)ZG_TEXT_MAX_SCALE);
        running += cmds[i].n_codepoints;
        ZG_REQUIRE(running <= n_codepoints, ZG_ERR_UNSUPPORTED, "canvas_draw_text: the commands up to %u name %llu codepoints, the array holds %u", i,
                   (unsigned long long)running, n_codepoints);
    }
    if (n == 0 || n_codepoints == 0) return ZG_OK;
    zg_font dfont;
    int rc;
    if ((rc = zg_font_upload(host_font, &dfont))) return rc;
    ScratchBlock sc;
    zg_text_cmd *dcmds;
    uint32_t *dcps;
    sc.take(dcmds, n);
    sc.take(dcps, n_codepoints);
    if (!(rc = sc.alloc()) && !(rc = upload_pageable(dcmds, cmds, (size_t)n * sizeof(zg_text_cmd), nullptr)) &&
        !(rc = upload_pageable(dcps, codepoints, (size_t)n_codepoints * sizeof(uint32_t), nullptr)))
        rc = host_in_place(img, true, [&](const zg_image *d) { return text_draw(d, dfont, dcmds, n, nullptr, dcps, n_codepoints, nullptr); });
    const int rc_free = zg_font_free(&dfont);
    return rc ? rc : rc_free;
}

} // extern "C"
