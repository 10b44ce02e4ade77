/* zignal_hip_text.h — the text module of libzignal_hip.so: Canvas(T).drawText (reference src/canvas/Canvas.zig:1476-1658) with the parts
 * of BitmapFont it calls (src/font/BitmapFont.zig:61-170, :226-248, GlyphData.zig), as a device operation of its own over a list of text
 * commands. The font is the caller's: the library ships no glyph data. Included by zignal_hip.h (include that one); zg_image, zg_stream and
 * the status codes come from there, ZG_DRAW_FAST / ZG_DRAW_SOFT and ZG_CANVAS_MAX_* from zignal_hip_canvas.h. */
#ifndef ZIGNAL_HIP_TEXT_H
#define ZIGNAL_HIP_TEXT_H

#include "zignal_hip.h"
#include "zignal_hip_canvas.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZG_TEXT_MAX_SCALE 64.0f         /* scale of one command; at 64 a 255-pixel glyph is 16320 pixels, half of ZG_CANVAS_MAX_SIZE */
#define ZG_TEXT_MAX_CODEPOINTS 65536u   /* codepoints of one command: its pen is walked by one lane */
#define ZG_TEXT_MAX_COMMANDS 65536u     /* n of one call */
#define ZG_TEXT_MAX_TOTAL 16777216u     /* n_codepoints of one call */

/* GlyphData of a variable-width font plus the codepoint it belongs to (the reference keeps that in a hash map). 16 bytes, no padding. */
typedef struct zg_glyph {
    uint32_t codepoint;
    uint32_t bitmap_offset; /* into the font's data; rows of (width + 7) / 8 bytes, bits LSB first */
    uint8_t width, height;
    int16_t x_offset, y_offset; /* added to the pen, in glyph pixels (scaled with the text) */
    int16_t device_width;       /* the advance; <= 0 advances by 0 */
} zg_glyph;

/* BitmapFont by value; data and glyphs are device pointers for zg_canvas_draw_text and host pointers for the *_host and *_check calls.
 * glyphs == NULL: the fixed layout — the bitmap of codepoint c (first_char <= c <= last_char) is char_height rows of
 * (char_width + 7) / 8 bytes at (c - first_char) * char_height * that; every glyph is char_width x char_height, offsets 0, advance
 * char_width. glyphs != NULL: the glyph table — n_glyphs entries sorted by codepoint, every codepoint once (found by binary search);
 * first_char and last_char are unused. In both forms a codepoint the font lacks draws nothing and advances by char_width, and a line
 * is char_height pixels high. 32 bytes. */
typedef struct zg_font {
    const uint8_t *data;
    const zg_glyph *glyphs;
    uint32_t data_len, n_glyphs;
    uint8_t char_width, char_height, first_char, last_char;
    uint32_t reserved; /* 0 */
} zg_font;

/* drawText(text, (x, y), color, font, scale, mode): the text is codepoints[first_codepoint .. first_codepoint + n_codepoints) of the
 * call's codepoint array ('\n' = 10 starts a new line). 28 bytes, no padding. */
typedef struct zg_text_cmd {
    float x, y, scale;
    int32_t mode;     /* ZG_DRAW_FAST | ZG_DRAW_SOFT */
    uint8_t color[4]; /* r g b a */
    uint32_t first_codepoint, n_codepoints;
} zg_text_cmd;

/* sizeof of the three structs as the library was built (the zg_sizeof_step rule). */
ZG_API size_t zg_sizeof_font(void);
ZG_API size_t zg_sizeof_glyph(void);
ZG_API size_t zg_sizeof_text_cmd(void);

/* A font with host pointers: ZG_ERR_INVALID_ARGUMENT for a null font, null data with data_len > 0, a glyph table that is not strictly
 * ascending by codepoint (unsorted or a codepoint twice) or holds a codepoint above 0x10FFFF, a glyph whose bitmap
 * [bitmap_offset, + height * ((width + 7) / 8)) leaves data_len, a fixed font with last_char < first_char or whose data_len does not
 * cover first_char .. last_char, a reserved word that is not 0. No device call. */
ZG_API int zg_font_check(const zg_font *host_font);
/* zg_font_check, then the two tables in one device allocation, synchronously: *device_font is the font with device pointers, to be
 * passed by address to zg_canvas_draw_text and released with zg_font_free (which zeroes it; a zeroed font is ignored). */
ZG_API int zg_font_upload(const zg_font *host_font, zg_font *device_font);
ZG_API int zg_font_free(zg_font *device_font);

/* BitmapFont.getTextBounds(text, scale): out_ltrb = l t r b (l = t = 0), in the reference's sequential f32 arithmetic. Host only. */
ZG_API int zg_text_bounds_host(const zg_font *host_font, const uint32_t *codepoints, uint32_t n, float scale, float out_ltrb[4]);

/* Executes cmds[0 .. count) in list order into img (u8, Rgb(u8) or Rgba(u8); limits as zg_canvas_draw), in place, byte for byte as the
 * reference making the same drawText calls with an Rgba(u8) colour one after another: a pixel's lane keeps the pixel in a register,
 * applies every write that reaches it in the reference's order and as often as the reference makes it (the blocks of neighbouring bits
 * of a .fast text at a fractional scale overlap; it matters on Rgba(u8) with a != 255), and stores once. Pixels that nothing writes are
 * not stored; bytes between cols and stride are never touched. The three paths: scale == 1 (either mode) lights the glyph's bits at
 * the floor of the pen; .fast scaled writes a block per lit bit, clipped to the intersection of the advance-width text rectangle with
 * the image (this path only); .soft scaled writes box-filtered coverage through setPixel. Only an Rgba(u8) image is composited into.
 * scale <= 0, an empty text and a text whose rectangle misses the image draw nothing.
 * font: by address on the host, its pointers on the device (zg_font_upload). A glyph whose bitmap leaves data_len is skipped.
 * cmds: n commands on the device. count_device: NULL or a device word, as in zg_canvas_draw. codepoints: n_codepoints words on the device
 * (NULL when 0), shared by the commands; ranges may overlap or repeat.
 * A command outside the contract is skipped on the device: a mode that is neither fast nor soft; x, y or scale not finite; |x| or |y|
 * above ZG_CANVAS_MAX_COORD; scale above ZG_TEXT_MAX_SCALE; a codepoint range outside the array; more than ZG_TEXT_MAX_CODEPOINTS
 * codepoints; a codepoint above 0x10FFFF; and, because the scratch is sized from n_codepoints, every command from the one on at which
 * the running total of the (in-range) commands' codepoints passes n_codepoints — a list whose ranges tile the array never gets there.
 * In the one case where the reference has no defined result — a .fast scaled bit whose block lies wholly left of or above the frame,
 * where it casts a negative float to u32 — the bit writes nothing.
 * n above ZG_TEXT_MAX_COMMANDS or n_codepoints above ZG_TEXT_MAX_TOTAL: ZG_ERR_UNSUPPORTED.
 * Asynchronous on `stream`, two launches, 32 bytes of scratch per codepoint and 16 per command, no host synchronisation, copy or upload,
 * recordable into a graph from a process's first call. In a process without a device the call answers its argument errors, then ZG_ERR_HIP. */
ZG_API int zg_canvas_draw_text(const zg_image *img, const zg_font *font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *count_device,
                               const uint32_t *codepoints, uint32_t n_codepoints, zg_stream stream);

/* Host pointers (img->data, the font's tables, cmds, codepoints), synchronous. The font goes through zg_font_check, and a command
 * outside the contract is refused before anything is drawn: ZG_ERR_UNSUPPORTED for more than ZG_TEXT_MAX_CODEPOINTS codepoints in a
 * command or a total above n_codepoints, ZG_ERR_INVALID_ARGUMENT for everything else. */
ZG_API int zg_canvas_draw_text_host(const zg_image *img, const zg_font *host_font, const zg_text_cmd *cmds, uint32_t n,
                                    const uint32_t *codepoints, uint32_t n_codepoints);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_TEXT_H */
