/* zignal_hip_qr.h — the QR detector of libzignal_hip.so: reference src/qrcode/detector.zig:57-641 as a device operation from a frame to
 * the sampled module grids and their corners, which are what detectAndDecode hands to decoder.decodeModules. Decoding the grids
 * (decoder.zig, reed_solomon.zig, segment.zig, matrix.zig) is host work on a few kilobytes and is not part of this library. Included by
 * zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there, zg_draw_cmd from zignal_hip_canvas.h. */
#ifndef ZIGNAL_HIP_QR_H
#define ZIGNAL_HIP_QR_H

#include "zignal_hip.h"
#include "zignal_hip_canvas.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZG_QR_MAX_FINDERS 64   /* detector.zig:87 */
#define ZG_QR_MAX_VERSIONS 8   /* :112 */
#define ZG_QR_MAX_FOURTHS 5    /* :122 */
#define ZG_QR_MAX_MODULES 31329 /* 177 x 177, version 40 */

#define ZG_QR_ADAPTIVE 0 /* thresholdAdaptiveMean, radius max(min(rows, cols) / 16, 8), c = 4 (:73-74) */
#define ZG_QR_OTSU 1     /* thresholdOtsu (:79) */
#define ZG_QR_BINARY 2   /* src is already binary and is used where it is: a pixel is dark iff its byte is 0 (:166-168) */

/* FinderPattern (:170-175): centre (x = column, y = row), module size, merged hits. */
typedef struct zg_qr_finder {
    float x, y, module_size, hits;
} zg_qr_finder;

/* Fourth (:410-413). */
typedef struct zg_qr_fourth {
    float x, y;
    uint32_t is_alignment;
} zg_qr_fourth;

/* Every intermediate result of detectAndDecode (:86-156) on one binary map. What a stage did not reach is zero. */
typedef struct zg_qr_detection {
    zg_qr_finder finders[ZG_QR_MAX_FINDERS]; /* the merged list as pickFinderTriple gets it (:97-109) */
    uint32_t finder_count;                   /* its length: after the hits >= 2 filter when that leaves three or more */
    uint32_t merged_count;                   /* the length before the filter */
    uint32_t triple_found;
    zg_qr_finder triple[3];                  /* top left, top right, bottom left */
    uint32_t version_estimate;
    uint32_t version_count;                  /* the final candidate list (:112-117 and the hints of :141-145) */
    uint8_t versions[ZG_QR_MAX_VERSIONS];
    uint32_t fourth_count;
    zg_qr_fourth fourths[ZG_QR_MAX_FOURTHS];
    uint32_t grids_total;                    /* the grids the reference would hand to the decoder; does not depend on the capacities */
    uint32_t grids_written;
    uint32_t modules_written;                /* bytes */
} zg_qr_detection;

/* One trial of the loops at :126-153 that passed sampleTimingLines, timingOk and sampleGrid. */
typedef struct zg_qr_grid {
    uint32_t version, dim;
    uint32_t fourth_index;   /* into zg_qr_detection.fourths */
    uint32_t modules_offset; /* the grid's dim * dim bytes (0 or 1, row-major) start here in `modules` */
    int32_t version_hint;    /* decoder.readVersion of this grid for version >= 7, else -1 */
    float corners[8];        /* symbolCorners (:611-619): top left, top right, bottom left, bottom right, (x, y) each */
    uint32_t reserved;
    double transform[9];     /* module space to image space, row-major */
} zg_qr_grid;

ZG_API size_t zg_qr_sizeof_detection(void);
ZG_API size_t zg_qr_sizeof_grid(void);

/* The bytes of scratch one zg_qr_detect call on a rows x cols frame takes from the library's cache (about 8 per pixel, 9 when src is
 * not Image(u8)). */
ZG_API size_t zg_qr_scratch_bytes(uint32_t rows, uint32_t cols);

/* detectAndDecode up to the decoder, on one binarisation of src.
 *   src        an image on the device (a view is taken as a view). Image(u8) is used as it is; another pixel type goes through
 *              zg_convert to u8 into scratch first (:50-55). rows < 21 or cols < 21: an empty result, not an error (:58).
 *   binarize   ZG_QR_ADAPTIVE, ZG_QR_OTSU or ZG_QR_BINARY (Image(u8) only). The reference runs ADAPTIVE and goes on to OTSU only when
 *              nothing decoded; that is the caller's knowledge, so the caller makes the second call.
 *   detection  one record
 *   grids      grid_capacity records, in the reference's order of trial. The reference stops at its first successful decode; every
 *              trial is emitted here, and the list up to any trial is what the reference has computed by then.
 *   modules    module_capacity bytes: the grids' modules back to back
 * Only whole grids are written, and writing stops at the first grid that does not fit either capacity: grids_written and
 * modules_written say how far it went; grids_total does not depend on the capacities. grids and modules may be NULL with capacity 0.
 * rows * cols >= 2^31: ZG_ERR_UNSUPPORTED. Status codes are decided before anything is enqueued. Asynchronous on `stream`, a fixed number
 * of launches for a given frame size and pixel type, zg_qr_scratch_bytes of scratch, no host synchronisation, copy or upload, recordable
 * into a graph from a process's first call. In a process without a device the call answers its argument errors, then ZG_ERR_HIP. */
ZG_API int zg_qr_detect(const zg_image *src, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                        uint32_t module_capacity, zg_stream stream);

/* Host pointers (src->data, detection, grids, modules), synchronous. grids and modules may be NULL with capacity 0 to ask for the
 * counts alone. */
ZG_API int zg_qr_detect_host(const zg_image *src, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                             uint32_t module_capacity);

/* The device-side builder from zg_qr_detect's outputs to a Canvas command list: four ZG_DRAW_LINE commands per written grid, outlining
 * `corners` top left -> top right -> bottom right -> bottom left -> top left, one lane per edge. capacity is the length of cmds_out:
 * the first min(4 * grids_written, capacity) commands are written and *count_out (a device word, the count_device of zg_canvas_draw)
 * receives that number. color: four host bytes, r g b a. Asynchronous on `stream`, one launch, no synchronisation, recordable. */
ZG_API int zg_canvas_cmds_from_qr(const zg_qr_grid *grids, const zg_qr_detection *detection, uint32_t capacity, const uint8_t *color, uint32_t width,
                                  int mode, zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_QR_H */
