/* The reference's applyErrorDiffusion (src/image/dither.zig:208-331) restated in C: the in-place scatter in raster order, one thread.
 * tools/bench_quantize.py builds it with -O2 and times it beside the device kernel; it is the CPU yardstick of DESIGN.md §8, not a test. */
#include <stdint.h>

static inline int div_trunc_pow2(int value, int shift) { return value >= 0 ? value >> shift : (value + (1 << shift) - 1) >> shift; }
static inline uint8_t clamp_u8(int v) { return v < 0 ? 0 : v > 255 ? 255 : (uint8_t)v; }
static inline void update(uint8_t *p, const int *err, int weight, int shift) {
    p[0] = clamp_u8(p[0] + div_trunc_pow2(err[0] * weight, shift));
    p[1] = clamp_u8(p[1] + div_trunc_pow2(err[1] * weight, shift));
    p[2] = clamp_u8(p[2] + div_trunc_pow2(err[2] * weight, shift));
}

static const int FS[4][4] = {{1, 0, 7, 4}, {-1, 1, 3, 4}, {0, 1, 5, 4}, {1, 1, 1, 4}}; /* dx, dy, weight, shift */
static const int ATK[6][4] = {{1, 0, 1, 3}, {2, 0, 1, 3}, {-1, 1, 1, 3}, {0, 1, 1, 3}, {1, 1, 1, 3}, {0, 2, 1, 3}};

void dither_literal(uint8_t *data, int rows, int cols, const uint8_t *palette, const uint8_t *lut, int atkinson) {
    const int(*entries)[4] = atkinson ? ATK : FS;
    const int n = atkinson ? 6 : 4, reach = atkinson ? 2 : 1;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            uint8_t *p = data + ((long)r * cols + c) * 3;
            const uint8_t *q = palette + 3 * lut[(p[0] >> 3) << 10 | (p[1] >> 3) << 5 | (p[2] >> 3)];
            const int err[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
            p[0] = q[0], p[1] = q[1], p[2] = q[2];
            if (r < rows - reach && c > 0 && c < cols - reach) {
                for (int k = 0; k < n; ++k) update(p + ((long)entries[k][1] * cols + entries[k][0]) * 3, err, entries[k][2], entries[k][3]);
            } else {
                for (int k = 0; k < n; ++k) {
                    const int nc = c + entries[k][0], nr = r + entries[k][1];
                    if (nr >= 0 && nr < rows && nc >= 0 && nc < cols) update(data + ((long)nr * cols + nc) * 3, err, entries[k][2], entries[k][3]);
                }
            }
        }
}
