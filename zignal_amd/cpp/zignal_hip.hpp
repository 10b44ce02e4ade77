// zignal_hip.hpp — C++ host-side mirror of zignal's `Image(T)` over the C ABI of libzignal_hip.so.
//
// The reference is compiled code (Zig) and no Zig toolchain exists in this build image, so this header is the
// compiled-language face of the drop-in: same method names, argument meaning and error behaviour as reference
// src/image.zig (line numbers per method). Zig error unions become exceptions:
//   error.DimensionMismatch -> zignal::DimensionMismatch, error.InvalidSigma / InvalidScaleFactor /
//   InvalidDimensions -> zignal::InvalidArgument, error.OutOfMemory -> std::bad_alloc.
// Header only; link with -lzignal_hip.
//
// Two image classes share one set of methods (detail::Ops, written once):
//   Image<T>        pixels in host memory (std::vector-backed or borrowed). Every call is synchronous and crosses
//                   PCIe twice (zg_<op>_host), exactly like calling the reference's CPU method — the drop-in for code
//                   that touches pixels between calls.
//   DeviceImage<T>  pixels in HBM (zg_malloc), a stream to order work on. Calls go to the stream-taking entry points
//                   (zg_<op>) and return as soon as the work is enqueued; a chain such as the CLI's
//                   `pipeline [blur, resize]` (reference src/cli/pipeline.zig:153-179) keeps its intermediate images
//                   on the GPU and crosses PCIe once on the way in (upload / fromHost) and once on the way out
//                   (download / toHost). This is the one that runs at the measured kernel rates.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/zignal_hip.h"

namespace zignal {

struct Error : std::runtime_error { int status; Error(int s, const std::string &m) : std::runtime_error(m), status(s) {} };
struct DimensionMismatch : Error { using Error::Error; };
struct InvalidArgument : Error { using Error::Error; };
// an error of a codec's error set (src/codecs/png.zig); name() is the Zig error name, e.g. "InvalidCrc"
struct CodecError : Error {
    using Error::Error;
    std::string name() const { const std::string m = what(); return m.substr(0, m.find(' ')); }
};

inline void check(int status) {
    if (status == ZG_OK) return;
    const std::string msg = zg_last_error();
    if (status == ZG_ERR_DIMENSION_MISMATCH) throw DimensionMismatch(status, msg);
    if (status == ZG_ERR_INVALID_ARGUMENT) throw InvalidArgument(status, msg);
    if (status == ZG_ERR_OUT_OF_MEMORY) throw std::bad_alloc();
    if (status == ZG_ERR_CODEC) throw CodecError(status, msg);
    throw Error(status, msg);
}

// pixel structs with the reference's memory layout (src/color.zig:286-290, :400)
template <typename T> struct Rgb { T r, g, b; };
template <typename T> struct Rgba { T r, g, b, a; };
template <typename T> struct Oklab { T l, a, b; };

template <typename T> struct PixelTraits;
template <> struct PixelTraits<uint8_t> { static constexpr int pixel = ZG_PIXEL_U8, space = ZG_CS_GRAY; };
template <> struct PixelTraits<float> { static constexpr int pixel = ZG_PIXEL_F32, space = ZG_CS_GRAY; };
template <> struct PixelTraits<Rgb<uint8_t>> { static constexpr int pixel = ZG_PIXEL_RGB_U8, space = ZG_CS_RGB; };
template <> struct PixelTraits<Rgba<uint8_t>> { static constexpr int pixel = ZG_PIXEL_RGBA_U8, space = ZG_CS_RGBA; };
template <> struct PixelTraits<Rgb<float>> { static constexpr int pixel = ZG_PIXEL_RGB_F32, space = ZG_CS_RGB; };
template <> struct PixelTraits<Rgba<float>> { static constexpr int pixel = ZG_PIXEL_RGBA_F32, space = ZG_CS_RGBA; };
template <> struct PixelTraits<Oklab<float>> { static constexpr int pixel = ZG_PIXEL_RGB_F32, space = ZG_CS_OKLAB; };

enum class BorderMode : int { zero = 0, replicate = 1, mirror = 2, wrap = 3 };          // border.zig:10-18
struct Interpolation {                                                                   // interpolation.zig:53-68
    int kind; float b = 0, c = 0;
    static Interpolation nearest() { return {ZG_INTERP_NEAREST}; }
    static Interpolation bilinear() { return {ZG_INTERP_BILINEAR}; }
    static Interpolation bicubic() { return {ZG_INTERP_BICUBIC}; }
    static Interpolation catmull_rom() { return {ZG_INTERP_CATMULL_ROM}; }
    static Interpolation mitchell(float b, float c) { return {ZG_INTERP_MITCHELL, b, c}; }
    static Interpolation lanczos() { return {ZG_INTERP_LANCZOS}; }
    zg_method c_method() const { return zg_method{kind, b, c, nullptr}; }
};
struct FloodFillOptions {                                                                // flood_fill.zig:5-26
    enum class Connectivity { four = 4, eight = 8 };
    enum class ThresholdMode { seed = ZG_FLOOD_MODE_SEED, neighbor = ZG_FLOOD_MODE_NEIGHBOR };
    double threshold = 0;
    Connectivity connectivity = Connectivity::four;
    ThresholdMode mode = ThresholdMode::seed;
    zg_flood_fill_options c_options() const { return zg_flood_fill_options{threshold, (int)connectivity, (int)mode}; }
};
// dither.Mode (dither.zig:18-30) and PaletteMode (quantize.zig:476-498) with the reference's ordinals, and a palette of up to 256 colours
enum class DitherMode : int { none = ZG_DITHER_NONE, floyd_steinberg = ZG_DITHER_FLOYD_STEINBERG, atkinson = ZG_DITHER_ATKINSON, ordered = ZG_DITHER_ORDERED,
                              automatic = ZG_DITHER_AUTO };
struct PaletteMode {
    int kind;
    uint32_t max_colors = 256;
    static PaletteMode fixed6x7x6() { return {ZG_PALETTE_FIXED_6X7X6}; }
    static PaletteMode fixedVga16() { return {ZG_PALETTE_FIXED_VGA16}; }
    static PaletteMode fixedWeb216() { return {ZG_PALETTE_FIXED_WEB216}; }
    static PaletteMode adaptive(uint32_t max_colors = 256) { return {ZG_PALETTE_ADAPTIVE, max_colors}; }
};
struct Palette {
    Rgb<uint8_t> colors[256];
    uint32_t size = 0;
    // the fixed palettes of buildPalette (quantize.zig:502-521): host tables, no GPU needed
    static Palette fixed(PaletteMode mode) {
        Palette p;
        check(zg_build_palette(nullptr, mode.kind, mode.max_colors, &p.colors[0].r, &p.size));
        return p;
    }
    // ColorLookupTable.init (quantize.zig:66-159) on the host: 32768 bytes indexed by r5 << 10 | g5 << 5 | b5
    std::vector<uint8_t> lookupTable() const {
        std::vector<uint8_t> lut(ZG_HISTOGRAM_CELLS);
        check(zg_palette_lut_host(&colors[0].r, size, lut.data()));
        return lut;
    }
};
template <typename T> struct Rectangle { T l, t, r, b; T width() const { return l >= r ? T(0) : r - l; } T height() const { return t >= b ? T(0) : b - t; } };
struct ProjectiveTransform { float m[9]; };                                              // geometry/transforms.zig:197

// A HIP stream owned by the caller; DeviceImage work is ordered on one. The default-constructed handle is the default stream.
class Stream {
  public:
    Stream() = default;
    static Stream create() { Stream s; check(zg_stream_create(&s.s_)); s.owned_ = true; return s; }
    Stream(Stream &&o) noexcept : s_(o.s_), owned_(o.owned_) { o.s_ = nullptr; o.owned_ = false; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s_ = o.s_; owned_ = o.owned_; o.s_ = nullptr; o.owned_ = false; } return *this; }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { release(); }
    zg_stream handle() const { return s_; }
    void synchronize() const { check(zg_stream_synchronize(s_)); }
  private:
    void release() { if (owned_ && s_) (void)zg_stream_destroy(s_); s_ = nullptr; owned_ = false; }
    zg_stream s_ = nullptr;
    bool owned_ = false;
};

template <typename T> class Image;
template <typename T> class DeviceImage;

namespace detail {

// Every hot-path method of Image(T), written once. `run(dev_fn, host_fn, args...)` calls zg_<op>(args..., stream) for a
// DeviceImage and zg_<op>_host(args...) for an Image; `Of<U>` is the same kind of image with pixel type U.
template <template <typename> class Img, typename T> class Ops {
    using Derived = Img<T>;
    template <typename U> using Of = Img<U>;
    const Derived &self() const { return static_cast<const Derived &>(*this); }
    template <class DevFn, class HostFn, class... A> void run(DevFn dev, HostFn host, A... a) const {
        if constexpr (Derived::on_device) check(dev(a..., self().stream()));
        else check(host(a...));
    }
    // op: 0 percentile, 1 midpoint, 2 alpha-trimmed mean (zg_order_statistic_blur)
    void orderStatistic(const Derived &out, uint32_t radius, int op, double param, BorderMode border, const char *what) const {
        if (!hasSameShape(out)) throw DimensionMismatch(1, what);
        const zg_image s = desc(), d = out.desc();
        run(zg_order_statistic_blur, zg_order_statistic_blur_host, &s, &d, radius, op, param, (int)border);
    }
    // psnr, meanPixelError and ssim: see the public methods
    template <class DevFn, class HostFn>
    double metric(DevFn dev, HostFn host, const Derived &other, const zg_metric_options &opt, zg_metric_result *result_device, bool is_psnr) const {
        const zg_image a = desc(), b = other.desc();
        double value = 0;
        if constexpr (Derived::on_device) {
            if (result_device) {
                check(dev(&a, &b, &opt, result_device, self().stream()));
                return 0;
            }
            void *mem = nullptr;
            check(zg_malloc(&mem, sizeof(zg_metric_result)));
            zg_metric_result r{};
            int rc = dev(&a, &b, &opt, (zg_metric_result *)mem, self().stream());
            if (rc == ZG_OK) rc = zg_memcpy_d2h(&r, mem, sizeof r, self().stream()); // waits for the stream
            zg_free(mem);
            check(rc);
            value = is_psnr ? zg_psnr_from_mse(r.value, PixelTraits<T>::pixel == ZG_PIXEL_U8 || PixelTraits<T>::pixel == ZG_PIXEL_RGB_U8 ||
                                                                PixelTraits<T>::pixel == ZG_PIXEL_RGBA_U8 ? 255.0 : 1.0)
                            : r.value;
        } else {
            check(host(&a, &b, &opt, &value, (zg_metric_result *)nullptr));
        }
        return value;
    }

  public:
    uint32_t rows = 0, cols = 0;
    size_t stride = 0;
    T *data = nullptr; // host pointer (Image) or device pointer (DeviceImage): never dereference the latter on the host

    template <class O> bool hasSameShape(const O &o) const { return rows == o.rows && cols == o.cols; }
    bool isContiguous() const { return cols == stride; }
    zg_image desc() const { return zg_image{(void *)data, stride, rows, cols, PixelTraits<T>::pixel}; }

    // ---- filters ----
    void convolveSeparable(const Derived &out, const std::vector<float> &kx, const std::vector<float> &ky, BorderMode border) const { // image.zig:935
        if (!hasSameShape(out)) throw DimensionMismatch(1, "convolveSeparable");
        const zg_image s = desc(), d = out.desc();
        run(zg_conv_separable, zg_conv_separable_host, &s, &d, kx.data(), (uint32_t)kx.size(), ky.data(), (uint32_t)ky.size(), (int)border);
    }
    void gaussianBlur(const Derived &out, float sigma) const {                           // image.zig:954
        if (!hasSameShape(out)) throw DimensionMismatch(1, "gaussianBlur");
        const zg_image s = desc(), d = out.desc();
        run(zg_gaussian_blur, zg_gaussian_blur_host, &s, &d, sigma);
    }
    template <size_t KH, size_t KW> void convolve(const Derived &out, const float (&kernel)[KH][KW], BorderMode border) const { // image.zig:917
        if (!hasSameShape(out)) throw DimensionMismatch(1, "convolve");
        const zg_image s = desc(), d = out.desc();
        run(zg_convolve, zg_convolve_host, &s, &d, &kernel[0][0], (uint32_t)KH, (uint32_t)KW, (int)border);
    }
    void boxBlur(const Derived &out, uint32_t radius) const {                            // image.zig:635
        if (!hasSameShape(out)) throw DimensionMismatch(1, "boxBlur");
        const zg_image s = desc(), d = out.desc();
        run(zg_box_blur, zg_box_blur_host, &s, &d, radius);
    }
    void medianBlur(const Derived &out, uint32_t radius) const {                          // image.zig:653
        if (!hasSameShape(out)) throw DimensionMismatch(1, "medianBlur");
        const zg_image s = desc(), d = out.desc();
        run(zg_order_statistic_blur, zg_order_statistic_blur_host, &s, &d, radius, 0, 0.5, (int)ZG_BORDER_MIRROR);
    }
    // the other order-statistic blurs (image.zig:672-783): radius up to 256, u8 and all-u8 struct pixels
    void percentileBlur(const Derived &out, uint32_t radius, double percentile, BorderMode border) const {     // image.zig:672
        orderStatistic(out, radius, 0, percentile, border, "percentileBlur");
    }
    void minBlur(const Derived &out, uint32_t radius, BorderMode border) const {                               // image.zig:696
        orderStatistic(out, radius, 0, 0.0, border, "minBlur");
    }
    void maxBlur(const Derived &out, uint32_t radius, BorderMode border) const {                               // image.zig:719
        orderStatistic(out, radius, 0, 1.0, border, "maxBlur");
    }
    void midpointBlur(const Derived &out, uint32_t radius, BorderMode border) const {                          // image.zig:742
        orderStatistic(out, radius, 1, 0.0, border, "midpointBlur");
    }
    void alphaTrimmedMeanBlur(const Derived &out, uint32_t radius, double trim_fraction, BorderMode border) const { // image.zig:767
        orderStatistic(out, radius, 2, trim_fraction, border, "alphaTrimmedMeanBlur");
    }
    void equalize() const { const zg_image s = desc(); run(zg_equalize, zg_equalize_host, &s); } // image.zig:824 (in place)
    void sharpen(const Derived &out, uint32_t radius) const {                             // image.zig:785
        if (!hasSameShape(out)) throw DimensionMismatch(1, "sharpen");
        const zg_image s = desc(), d = out.desc();
        run(zg_sharpen, zg_sharpen_host, &s, &d, radius);
    }
    void invert() const { const zg_image s = desc(); run(zg_invert, zg_invert_host, &s); }  // image.zig:494 (in place)
    Of<uint8_t> sobel() const {                                                          // image.zig:1001 (out allocated here)
        auto out = Of<uint8_t>::like(self(), rows, cols);
        const zg_image s = desc(), d = out.desc();
        run(zg_sobel, zg_sobel_host, &s, &d);
        return out;
    }
    void canny(const Of<uint8_t> &out, float sigma, float low_threshold, float high_threshold) const {      // image.zig:1047
        if (rows != out.rows || cols != out.cols) throw DimensionMismatch(1, "canny");
        const zg_image s = desc(), d = out.desc();
        run(zg_canny, zg_canny_host, &s, &d, sigma, low_threshold, high_threshold);
    }
    struct ShenCastan { float smooth = 0.9f; uint32_t window_size = 7; float high_ratio = 0.99f, low_rel = 0.5f; bool hysteresis = true, use_nms = false; }; // ShenCastan.zig:9-32
    void shenCastan(const Of<uint8_t> &out, const ShenCastan &o = {}) const {            // image.zig:1015
        if (rows != out.rows || cols != out.cols) throw DimensionMismatch(1, "shenCastan");
        const zg_image s = desc(), d = out.desc();
        run(zg_shen_castan, zg_shen_castan_host, &s, &d, o.smooth, o.window_size, o.high_ratio, o.low_rel, o.hysteresis ? 1 : 0, o.use_nms ? 1 : 0);
    }
    void motionBlurLinear(const Derived &out, float angle, uint32_t distance) const {    // image.zig:1077 (.linear)
        if (!hasSameShape(out)) throw DimensionMismatch(1, "motionBlur");
        const zg_image s = desc(), d = out.desc();
        run(zg_motion_blur_linear, zg_motion_blur_linear_host, &s, &d, angle, std::cos(angle), std::sin(angle), distance);
    }
    void motionBlurRadial(const Derived &out, float center_x, float center_y, float strength, bool spin) const {  // (.radial_zoom / .radial_spin)
        if (!hasSameShape(out)) throw DimensionMismatch(1, "motionBlur");
        const zg_image s = desc(), d = out.desc();
        run(zg_motion_blur_radial, zg_motion_blur_radial_host, &s, &d, center_x, center_y, strength, spin ? 1 : 0);
    }
    // ---- resampling ----
    void resize(const Derived &out, Interpolation method) const {                        // image.zig:523
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        run(zg_resize, zg_resize_host, &s, &d, &m);
    }
    Derived scale(float factor, Interpolation method) const {                            // image.zig:530
        if (factor <= 0) throw InvalidArgument(2, "InvalidScaleFactor");
        const uint32_t nr = (uint32_t)std::round((float)rows * factor), nc = (uint32_t)std::round((float)cols * factor);
        if (nr == 0 || nc == 0) throw InvalidArgument(2, "InvalidDimensions");
        Derived out = Derived::like(self(), nr, nc);
        resize(out, method);
        return out;
    }
    Rectangle<uint32_t> letterbox(const Derived &out, Interpolation method) const {      // image.zig:546
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        uint32_t r[4];
        run(zg_letterbox, zg_letterbox_host, &s, &d, &m, r);
        return {r[0], r[1], r[2], r[3]};
    }
    void warp(const Derived &out, const ProjectiveTransform &t, Interpolation method) const { // image.zig:621
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        run(zg_warp, zg_warp_host, &s, &d, (int)ZG_TRANSFORM_PROJECTIVE, t.m, &m);
    }
    void rotateInto(const Derived &out, float angle, Interpolation method, BorderMode border) const { // image.zig:566
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        run(zg_rotate_into, zg_rotate_into_host, &s, &d, angle, std::cos(angle), std::sin(angle), &m, (int)border);
    }
    Derived rotate(float angle, Interpolation method, BorderMode border) const {         // image.zig:558
        uint32_t r, c;
        check(zg_rotate_bounds(rows, cols, angle, std::cos(angle), std::sin(angle), &r, &c));
        Derived out = Derived::like(self(), r, c);
        rotateInto(out, angle, method, border);
        return out;
    }
    void extract(const Derived &out, Rectangle<float> rect, float angle, Interpolation method, BorderMode border) const { // image.zig:593
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        const float r[4] = {rect.l, rect.t, rect.r, rect.b};
        run(zg_extract, zg_extract_host, &s, &d, r, angle, std::cos(angle), std::sin(angle), &m, (int)border);
    }
    Derived crop(Rectangle<float> rect) const {                                          // image.zig:582
        const float r[4] = {rect.l, rect.t, rect.r, rect.b};
        uint32_t nr, nc;
        check(zg_crop_dims(r, &nr, &nc));
        Derived out = Derived::like(self(), nr, nc);
        const zg_image s = desc(), d = out.desc();
        run(zg_crop, zg_crop_host, &s, &d, r);
        return out;
    }
    void fill(const T &value) const { const zg_image s = desc(); run(zg_fill, zg_fill_host, &s, (const void *)&value); } // image.zig:187
    void setBorder(Rectangle<uint32_t> rect, const T &value) const {                      // image.zig:200
        const zg_image s = desc();
        const uint32_t r[4] = {rect.l, rect.t, rect.r, rect.b};
        run(zg_set_border, zg_set_border_host, &s, r, (const void *)&value);
    }
    // image.zig:831 -> flood_fill.zig:59, in place. An Image is filled synchronously and the number of filled pixels returned. A DeviceImage's
    // fill is enqueued on stream() and 0 returned: seed_device, when not null, is two device words (row, col) read in place of row and col,
    // filled_count_device a device word that receives the count. A seed outside the image throws InvalidArgument (error.OutOfBounds).
    uint32_t floodFill(uint32_t row, uint32_t col, const T &fill_value, const FloodFillOptions &options = {}, const uint32_t *seed_device = nullptr,
                       uint32_t *filled_count_device = nullptr) const {
        const zg_image s = desc();
        const zg_flood_fill_options o = options.c_options();
        uint32_t filled = 0;
        if constexpr (Derived::on_device) check(zg_flood_fill(&s, row, col, seed_device, (const void *)&fill_value, &o, filled_count_device, self().stream()));
        else check(zg_flood_fill_host(&s, row, col, (const void *)&fill_value, &o, &filled));
        return filled;
    }
    // examples/src/seam_carving.zig:104-144, n times: sobel, computeEnergy, computeSeam, removeSeam. The result is a new rows x (cols - n)
    // image (horizontal: (rows - n) x cols, the library's own definition through the transposed frame); this image is left unchanged.
    // seams, when not null, receives n * rows words (n * cols for horizontal): host memory for an Image, device memory for a DeviceImage,
    // whose carve is enqueued on stream().
    Derived seamCarve(uint32_t n, bool horizontal = false, uint32_t *seams = nullptr) const {
        Derived out = horizontal ? Derived::like(self(), rows > n ? rows - n : 0, cols) : Derived::like(self(), rows, cols > n ? cols - n : 0);
        const zg_image s = desc(), d = out.desc();
        run(zg_seam_carve, zg_seam_carve_host, &s, &d, n, horizontal ? ZG_SEAM_HORIZONTAL : ZG_SEAM_VERTICAL, (const zg_image *)nullptr, seams);
        return out;
    }
    // ---- quantisation and dithering (quantize.zig, dither.zig, gif.zig:875-920): DeviceImage only, enqueued on stream() ----
    // counts_device and first_device are 32768 device words each (quantize.zig:188-237; first: the raster index of a cell's first pixel)
    void colorHistogram(uint32_t *counts_device, uint32_t *first_device) const {
        static_assert(Derived::on_device, "colorHistogram is a device operation");
        const zg_image s = desc();
        check(zg_color_histogram(&s, counts_device, first_device, self().stream()));
    }
    // medianCut (quantize.zig:175-412) into a host palette; synchronises the default stream once
    Palette medianCut(uint32_t max_colors = 256) const {
        static_assert(Derived::on_device, "medianCut is a device operation");
        Palette p;
        const zg_image s = desc();
        check(zg_median_cut(&s, max_colors, 256, &p.colors[0].r, &p.size));
        return p;
    }
    Palette buildPalette(PaletteMode mode) const {                                       // quantize.zig:502-527
        static_assert(Derived::on_device, "buildPalette is a device operation");
        Palette p;
        const zg_image s = desc();
        check(zg_build_palette(&s, mode.kind, mode.max_colors, &p.colors[0].r, &p.size));
        return p;
    }
    // dither.apply (dither.zig:34-41), in place on an Rgb(u8) image; the palette and its table (zg_palette_lut) are device memory
    void dither(const Rgb<uint8_t> *palette_device, uint32_t n, const uint8_t *lut_device, DitherMode mode) const {
        static_assert(Derived::on_device, "dither is a device operation");
        const zg_image s = desc();
        check(zg_dither(&s, &palette_device->r, n, lut_device, (int)mode, self().stream()));
    }
    // mapImageToPalette (gif.zig:875-920) into a u8 index plane of the same shape; transparent_index < 0: none
    void mapToPalette(const Of<uint8_t> &indices, const Rgb<uint8_t> *palette_device, uint32_t n, bool use_dither, int transparent_index = -1) const {
        static_assert(Derived::on_device, "mapToPalette is a device operation");
        const zg_image s = desc(), d = indices.desc();
        check(zg_palette_map(&s, &d, &palette_device->r, n, use_dither ? 1 : 0, transparent_index, self().stream()));
    }
    // ---- metrics (metrics.zig:10-54 psnr, :56-112 ssim, :114-166 meanPixelError) ----
    // An Image is measured synchronously and the method's f64 returned. A DeviceImage's metric is enqueued on stream(): with
    // result_device (a device zg_metric_result: value is the mse for psnr, the method's value otherwise) nothing waits and 0 is returned;
    // without it the call waits for the stream and returns the value. ssim_map, when not null, is (rows - 10) x (cols - 10) f64 on the
    // image's side; window, when not null, 121 host weights in place of the library's. A shape mismatch throws DimensionMismatch, an
    // image below 11 x 11 InvalidArgument (error.ImageTooSmall).
    double psnr(const Derived &other, zg_metric_result *result_device = nullptr) const {
        return metric(zg_psnr, zg_psnr_host, other, zg_metric_options{nullptr, nullptr}, result_device, true);
    }
    double meanPixelError(const Derived &other, zg_metric_result *result_device = nullptr) const {
        return metric(zg_mean_pixel_error, zg_mean_pixel_error_host, other, zg_metric_options{nullptr, nullptr}, result_device, false);
    }
    double ssim(const Derived &other, zg_metric_result *result_device = nullptr, double *ssim_map = nullptr, const double *window = nullptr) const {
        return metric(zg_ssim, zg_ssim_host, other, zg_metric_options{window, ssim_map}, result_device, false);
    }
    void flipLeftRight() const { const zg_image s = desc(); run(zg_flip_left_right, zg_flip_left_right_host, &s); }   // transforms.zig:28
    void flipTopBottom() const { const zg_image s = desc(); run(zg_flip_top_bottom, zg_flip_top_bottom_host, &s); }   // transforms.zig:36
    // ---- colour ----
    template <typename Target> void convertInto(const Of<Target> &out) const {          // image.zig:396
        const zg_image s = desc(), d = out.desc();
        run(zg_convert, zg_convert_host, &s, (int)PixelTraits<T>::space, &d, (int)PixelTraits<Target>::space, (const float *)nullptr);
    }
    template <typename Target> Of<Target> convert() const {                              // image.zig:418
        Of<Target> out = Of<Target>::like(self(), rows, cols);
        convertInto<Target>(out);
        return out;
    }
    // resize then convert in one call (zg_resize_convert): the pipeline steps [resize, convert] without the intermediate image
    template <typename Target> void resizeConvertInto(const Of<Target> &out, Interpolation method) const {
        const zg_image s = desc(), d = out.desc(); const zg_method m = method.c_method();
        run(zg_resize_convert, zg_resize_convert_host, &s, (int)PixelTraits<T>::space, &d, (int)PixelTraits<Target>::space, &m, (const float *)nullptr);
    }
    // ---- file output (src/codecs/jpeg.zig:307, src/codecs/png.zig:1400); the file lands in host memory either way ----
    std::vector<uint8_t> encodeJpeg(const zg_jpeg_encode_options *options = nullptr) const {
        uint8_t *mem = nullptr;
        size_t n = 0;
        const zg_image s = desc();
        run(zg_jpeg_encode, zg_jpeg_encode_host, &s, (int)PixelTraits<T>::space, options, &mem, &n);
        std::vector<uint8_t> out(mem, mem + n);
        zg_jpeg_free(mem);
        return out;
    }
    std::vector<uint8_t> encodePng(const zg_png_encode_options *options = nullptr) const {
        uint8_t *mem = nullptr;
        size_t n = 0;
        const zg_image s = desc();
        run(zg_png_encode, zg_png_encode_host, &s, (int)PixelTraits<T>::space, options, &mem, &n);
        std::vector<uint8_t> out(mem, mem + n);
        zg_png_free(mem);
        return out;
    }
};

} // namespace detail

// Image(T): rows, cols, stride (pixels), data — owning (init) or borrowed (initFromSlice / view), in host memory.
template <typename T> class Image : public detail::Ops<Image, T> {
    using Base = detail::Ops<Image, T>;

  public:
    static constexpr bool on_device = false;
    using Base::rows; using Base::cols; using Base::stride; using Base::data;

    Image() = default;
    Image(Image &&o) noexcept { *this = std::move(o); }
    Image &operator=(Image &&o) noexcept {
        rows = o.rows; cols = o.cols; stride = o.stride; data = o.data; owned_ = std::move(o.owned_); // a moved vector keeps its buffer
        o.rows = o.cols = 0; o.stride = 0; o.data = nullptr;
        return *this;
    }
    Image(const Image &o) { *this = o; }
    Image &operator=(const Image &o) { // an owning image is copied with its pixels, a borrowed one stays a borrow
        if (this == &o) return *this;
        rows = o.rows; cols = o.cols; stride = o.stride; owned_ = o.owned_;
        data = o.owned_.empty() ? o.data : owned_.data() + (o.data - o.owned_.data());
        return *this;
    }
    static Image init(uint32_t rows, uint32_t cols) {                                    // image.zig:124-134
        Image im;
        im.owned_.resize((size_t)rows * cols);
        im.rows = rows; im.cols = cols; im.stride = cols; im.data = im.owned_.data();
        return im;
    }
    template <class Proto> static Image like(const Proto &, uint32_t rows, uint32_t cols) { return init(rows, cols); }
    static Image initFromSlice(uint32_t rows, uint32_t cols, T *data) {                  // image.zig:161-170
        Image im; im.rows = rows; im.cols = cols; im.stride = cols; im.data = data; return im;
    }
    Image view(Rectangle<uint32_t> rect) const {                                         // image.zig:332-352
        const uint32_t l = rect.l, t = rect.t, r = std::min(rect.r, cols), b = std::min(rect.b, rows);
        Image v;
        if (l >= r || t >= b) return v;
        v.rows = b - t; v.cols = r - l; v.stride = stride; v.data = data + (size_t)t * stride + l;
        return v;
    }
    T &at(size_t r, size_t c) const { return data[r * stride + c]; }                     // image.zig:426-430
    zg_stream stream() const { return nullptr; }

    // ---- file input (image.zig:239-287: the format comes from the signature; src/codecs/png.zig, src/codecs/jpeg.zig) ----
    static Image loadFromBytes(const uint8_t *bytes, size_t len) {                                          // image.zig:265
        if (len >= 2 && bytes[0] == 0xFF && bytes[1] == 0xD8) {                                             // jpeg.zig:2825
            zg_jpeg_header h;
            check(zg_jpeg_probe(bytes, len, nullptr, &h, nullptr));
            Image out = init(h.height, h.width);
            const zg_image d = out.desc();
            check(zg_jpeg_decode_host(bytes, len, nullptr, &d, PixelTraits<T>::space, nullptr));
            return out;
        }
        zg_png_header h;                                                                                    // png.zig:1151
        check(zg_png_probe(bytes, len, nullptr, &h, nullptr, nullptr));
        Image out = init(h.height, h.width);
        const zg_image d = out.desc();
        check(zg_png_decode_host(bytes, len, nullptr, &d, PixelTraits<T>::space, nullptr));
        return out;
    }

  private:
    std::vector<T> owned_;
};

// Image(T) whose pixels live in HBM. Owning (init / fromHost / results of scale, crop, convert ...) or a non-owning view.
// Move-only. All methods of detail::Ops enqueue on stream() and return; call synchronize() (or download, which does)
// before looking at results from the host.
template <typename T> class DeviceImage : public detail::Ops<DeviceImage, T> {
    using Base = detail::Ops<DeviceImage, T>;

  public:
    static constexpr bool on_device = true;
    using Base::rows; using Base::cols; using Base::stride; using Base::data;

    DeviceImage() = default;
    DeviceImage(DeviceImage &&o) noexcept { *this = std::move(o); }
    DeviceImage &operator=(DeviceImage &&o) noexcept {
        if (this == &o) return *this;
        deinit();
        rows = o.rows; cols = o.cols; stride = o.stride; data = o.data; stream_ = o.stream_; owned_ = o.owned_;
        o.rows = o.cols = 0; o.stride = 0; o.data = nullptr; o.owned_ = nullptr;
        return *this;
    }
    DeviceImage(const DeviceImage &) = delete;
    DeviceImage &operator=(const DeviceImage &) = delete;
    ~DeviceImage() { deinit(); }

    static DeviceImage init(uint32_t rows, uint32_t cols, zg_stream stream = nullptr) {  // image.zig:124-134, in HBM
        DeviceImage im;
        check(zg_malloc(&im.owned_, (size_t)rows * cols * sizeof(T)));
        im.rows = rows; im.cols = cols; im.stride = cols; im.data = (T *)im.owned_; im.stream_ = stream;
        return im;
    }
    template <class Proto> static DeviceImage like(const Proto &proto, uint32_t rows, uint32_t cols) { return init(rows, cols, proto.stream()); }
    void deinit() {                                                                       // image.zig:173
        if (owned_) (void)zg_free(owned_); // hipFree waits for work that still uses the block
        owned_ = nullptr; data = nullptr; rows = cols = 0; stride = 0;
    }
    static DeviceImage fromHost(const Image<T> &host, zg_stream stream = nullptr) {
        DeviceImage im = init(host.rows, host.cols, stream);
        im.upload(host);
        return im;
    }
    void upload(const Image<T> &host) const {   // one trip across PCIe, strides honoured; complete on return
        const zg_image d = this->desc(), s = host.desc();
        check(zg_image_upload(&d, &s, stream_));
    }
    void download(const Image<T> &host) const { // waits for the stream's work on this image, then one trip back
        const zg_image d = host.desc(), s = this->desc();
        check(zg_image_download(&d, &s, stream_));
    }
    // convolveSeparable / gaussianBlur over several planes of one shape in one launch (zg_conv_separable_planes / zg_gaussian_blur_planes):
    // the reference's f32 route is per plane (Image(Rgba(f32)).convolveSeparable is a compile error, convolution.zig:431-435), so RGBA f32
    // data held as four Image(f32) planes goes through here. Asynchronous on planes[0]'s stream.
    static void convolveSeparablePlanes(const std::vector<const DeviceImage *> &planes, const std::vector<const DeviceImage *> &outs,
                                        const std::vector<float> &kx, const std::vector<float> &ky, BorderMode border) {
        if (planes.size() != outs.size()) throw DimensionMismatch(1, "convolveSeparablePlanes");
        if (planes.empty()) return;
        std::vector<zg_image> s, d;
        for (size_t i = 0; i < planes.size(); ++i) { s.push_back(planes[i]->desc()); d.push_back(outs[i]->desc()); }
        check(zg_conv_separable_planes(s.data(), d.data(), (uint32_t)s.size(), kx.data(), (uint32_t)kx.size(), ky.data(), (uint32_t)ky.size(), (int)border,
                                       planes[0]->stream()));
    }
    static void gaussianBlurPlanes(const std::vector<const DeviceImage *> &planes, const std::vector<const DeviceImage *> &outs, float sigma) {
        if (planes.size() != outs.size()) throw DimensionMismatch(1, "gaussianBlurPlanes");
        if (planes.empty()) return;
        std::vector<zg_image> s, d;
        for (size_t i = 0; i < planes.size(); ++i) { s.push_back(planes[i]->desc()); d.push_back(outs[i]->desc()); }
        check(zg_gaussian_blur_planes(s.data(), d.data(), (uint32_t)s.size(), sigma, planes[0]->stream()));
    }
    Image<T> toHost() const {
        Image<T> out = Image<T>::init(rows, cols);
        download(out);
        return out;
    }
    DeviceImage view(Rectangle<uint32_t> rect) const {                                   // image.zig:332-352 (non-owning)
        const uint32_t l = rect.l, t = rect.t, r = std::min(rect.r, cols), b = std::min(rect.b, rows);
        DeviceImage v;
        v.stream_ = stream_;
        if (l >= r || t >= b) return v;
        v.rows = b - t; v.cols = r - l; v.stride = stride; v.data = data + (size_t)t * stride + l;
        return v;
    }
    zg_stream stream() const { return stream_; }
    void setStream(zg_stream s) { stream_ = s; }
    void synchronize() const { check(zg_stream_synchronize(stream_)); }

    // decode a PNG / JPEG file straight into HBM (host: entropy layers; device: everything per pixel)
    static DeviceImage loadFromBytes(const uint8_t *bytes, size_t len, zg_stream stream = nullptr) {        // image.zig:265
        if (len >= 2 && bytes[0] == 0xFF && bytes[1] == 0xD8) {
            zg_jpeg_header h;
            check(zg_jpeg_probe(bytes, len, nullptr, &h, nullptr));
            DeviceImage out = init(h.height, h.width, stream);
            const zg_image d = out.desc();
            check(zg_jpeg_decode(bytes, len, nullptr, &d, PixelTraits<T>::space, nullptr, stream));
            return out;
        }
        zg_png_header h;
        check(zg_png_probe(bytes, len, nullptr, &h, nullptr, nullptr));
        DeviceImage out = init(h.height, h.width, stream);
        const zg_image d = out.desc();
        check(zg_png_decode(bytes, len, nullptr, &d, PixelTraits<T>::space, nullptr, stream));
        return out;
    }

  private:
    void *owned_ = nullptr;
    zg_stream stream_ = nullptr;
};

// ImagePyramid(T) (src/image/pyramid.zig:11-170) resident on the device: level 0 is the source itself (not copied, pyramid.zig:54), level i
// the source blurred with sigma_i = blur_sigma * sqrt(scale_i^2 - 1) (only if > 0.5) and resized bilinearly to trunc(dim / scale_i),
// scale_i = pow(scale_factor, i); a level below 8 x 8 truncates the pyramid. `build` is ONE call of the C ABI: every level is enqueued
// without a host round trip (they fork over internal streams and join back into the source's stream).
template <typename T> struct ImagePyramid {
    std::vector<DeviceImage<T>> levels; // levels[0] is a view of the source
    float scale_factor = 0, blur_sigma = 0;
    static ImagePyramid build(const DeviceImage<T> &source, uint8_t n_levels, float scale_factor, float blur_sigma) {       // pyramid.zig:31-102
        ImagePyramid p;
        p.scale_factor = scale_factor;
        p.blur_sigma = blur_sigma;
        p.levels.push_back(source.view(Rectangle<uint32_t>{0, 0, source.cols, source.rows}));
        std::vector<zg_image> descs;
        std::vector<float> sigmas;
        for (uint32_t i = 1; i < n_levels; ++i) {
            uint32_t r = 0, c = 0;
            float sigma = 0;
            check(zg_pyramid_level(source.rows, source.cols, zg_pyramid_scale(scale_factor, i), blur_sigma, &r, &c, &sigma));
            if (r < 8 || c < 8) break;                                                                                       // pyramid.zig:63-73
            p.levels.push_back(DeviceImage<T>::init(r, c, source.stream()));
            descs.push_back(p.levels.back().desc());
            sigmas.push_back(sigma);
        }
        const zg_image s = source.desc();
        check(zg_pyramid_build(&s, descs.data(), sigmas.data(), (uint32_t)descs.size(), source.stream()));
        return p;
    }
    static ImagePyramid buildDefault(const DeviceImage<T> &source) { return build(source, 8, 1.2f, 1.6f); }                 // pyramid.zig:105-107
    size_t nLevels() const { return levels.size(); }
    float getScale(size_t level) const { return zg_pyramid_scale(scale_factor, (uint32_t)level); }                          // pyramid.zig:122-125
};

// The `pipeline` command (src/cli/pipeline.zig:153-179) over a batch of equally shaped frames resident on the device: a recipe is a
// list of steps, `run` sends every frame through them in order with one zg_batch_pipeline call (a launch per step over the whole
// batch where the library has a batched kernel, fused neighbours where it has a fused one; equal to the per-frame methods bit for bit).
struct Pipeline {
    std::vector<zg_step> steps;
    // zg_step carries no size field: a library built from another header must not be handed arrays of this header's struct (zignal_hip.h: zg_sizeof_step)
    Pipeline() {
        if (zg_sizeof_step() != sizeof(zg_step))
            throw Error(ZG_ERR_INVALID_ARGUMENT, "libzignal_hip: sizeof(zg_step) is " + std::to_string(zg_sizeof_step()) + " in the library, " + std::to_string(sizeof(zg_step)) +
                                                     " in this header: rebuild one of them");
    }
    Pipeline &gaussianBlur(float sigma) { zg_step s{}; s.kind = ZG_STEP_GAUSSIAN_BLUR; s.sigma = sigma; steps.push_back(s); return *this; }              // cli/blur.zig:113-120
    Pipeline &boxBlur(uint32_t radius) { zg_step s{}; s.kind = ZG_STEP_BOX_BLUR; s.radius = radius; steps.push_back(s); return *this; }                  // cli/blur.zig:109-112
    Pipeline &medianBlur(uint32_t radius = 1) { zg_step s{}; s.kind = ZG_STEP_MEDIAN_BLUR; s.radius = radius; steps.push_back(s); return *this; }          // cli/blur.zig:116-123
    // cli/blur.zig:124-146; the angle is in radians, cos_a / sin_a are the caller's own cosine and sine of it (as in Image::motionBlurLinear)
    Pipeline &motionBlurLinear(float angle, float cos_a, float sin_a, uint32_t distance) {
        zg_step s{}; s.kind = ZG_STEP_MOTION_BLUR; s.motion = ZG_MOTION_LINEAR; s.angle = angle; s.cos_a = cos_a; s.sin_a = sin_a; s.distance = distance; steps.push_back(s); return *this;
    }
    Pipeline &motionBlurRadial(float center_x = 0.5f, float center_y = 0.5f, float strength = 0.5f, bool spin = false) {                             // cli/blur.zig:147-170
        zg_step s{}; s.kind = ZG_STEP_MOTION_BLUR; s.motion = spin ? ZG_MOTION_RADIAL_SPIN : ZG_MOTION_RADIAL_ZOOM;
        s.center_x = center_x; s.center_y = center_y; s.strength = strength; steps.push_back(s); return *this;
    }
    // edges.apply (cli/edges.zig:126-135): convert(u8) -> detector -> convert back; the frames keep their type
    Pipeline &edgesSobel() { zg_step s{}; s.kind = ZG_STEP_EDGES; s.edges = ZG_EDGES_SOBEL; steps.push_back(s); return *this; }
    Pipeline &edgesCanny(float sigma = 1.0f, float low = 50.0f, float high = 100.0f) {                                                                // cli/edges.zig:98-104
        zg_step s{}; s.kind = ZG_STEP_EDGES; s.edges = ZG_EDGES_CANNY; s.sigma = sigma; s.low = low; s.high = high; steps.push_back(s); return *this;
    }
    Pipeline &edgesShenCastan(float smooth = 0.9f, uint32_t window_size = 7, float high_ratio = 0.99f, float low_rel = 0.5f, bool use_nms = false) { // cli/edges.zig:105-118
        zg_step s{}; s.kind = ZG_STEP_EDGES; s.edges = ZG_EDGES_SHEN_CASTAN; s.sigma = smooth; s.window = window_size; s.high = high_ratio; s.low = low_rel; s.use_nms = use_nms;
        steps.push_back(s); return *this;
    }
    Pipeline &resize(uint32_t rows, uint32_t cols, Interpolation method = Interpolation::bilinear()) {                                                // cli/resize.zig:77-99
        zg_step s{}; s.kind = ZG_STEP_RESIZE; s.out_rows = rows; s.out_cols = cols; s.method = method.c_method(); steps.push_back(s); return *this;
    }
    template <typename Target> Pipeline &convert() {                                                                                                  // image.zig:418
        zg_step s{}; s.kind = ZG_STEP_CONVERT; s.dst_pixel = PixelTraits<Target>::pixel; s.dst_space = PixelTraits<Target>::space; steps.push_back(s); return *this;
    }
    Pipeline &warp(int transform, const float *m, int n_coefficients, uint32_t rows, uint32_t cols, Interpolation method = Interpolation::bilinear()) {  // image.zig:621
        zg_step s{}; s.kind = ZG_STEP_WARP; s.transform = transform; s.out_rows = rows; s.out_cols = cols; s.method = method.c_method();
        for (int i = 0; i < n_coefficients && i < 9; ++i) s.m[i] = m[i];
        steps.push_back(s); return *this;
    }
    // shape and type of the frames after the steps
    void outShape(uint32_t rows, uint32_t cols, int pixel, int space, uint32_t &out_rows, uint32_t &out_cols, int &out_pixel) const {
        check(zg_batch_pipeline_shape(rows, cols, pixel, space, steps.data(), (uint32_t)steps.size(), &out_rows, &out_cols, &out_pixel, nullptr));
    }
    // n frames of Src, rows x cols each, back to back at `src` (device memory) -> frames of Dst at `dst` (device memory, n * outShape)
    template <typename Src> void run(const Src *src, uint32_t n_frames, uint32_t rows, uint32_t cols, void *dst, zg_stream stream = nullptr) const {
        check(zg_batch_pipeline(src, n_frames, rows, cols, PixelTraits<Src>::pixel, PixelTraits<Src>::space, steps.data(), (uint32_t)steps.size(), dst, stream));
    }
    // the same over every device of a zg_multi context: src / dst live on the context's root device, the call returns when the results are complete
    template <typename Src> void runMulti(zg_multi ctx, const Src *src_root, uint32_t n_frames, uint32_t rows, uint32_t cols, void *dst_root, float times_ms[3] = nullptr) const {
        check(zg_multi_batch_pipeline(ctx, src_root, n_frames, rows, cols, PixelTraits<Src>::pixel, PixelTraits<Src>::space, steps.data(), (uint32_t)steps.size(), dst_root,
                                      times_ms));
    }
};

// ---- features: FAST (src/features/Fast.zig, KeyPoint.zig) ----
using KeyPoint = zg_keypoint; // KeyPoint.zig:9-28, field for field
static_assert(sizeof(KeyPoint) == 28, "zg_keypoint is KeyPoint's 28 bytes");

// Fast (src/features/Fast.zig:16-24): the reference's fields and defaults; detect returns its list (:38-72), order included, bit for bit.
struct Fast {
    uint8_t threshold = 20;
    bool nonmax_suppression = true;
    uint8_t min_contiguous = 9;

    // host image: the count first, then the list (two synchronous calls)
    std::vector<KeyPoint> detect(const Image<uint8_t> &image) const {
        const zg_image s = image.desc();
        uint32_t n = 0;
        check(zg_fast_detect_host(&s, threshold, min_contiguous, nonmax_suppression, nullptr, 0, &n));
        std::vector<KeyPoint> out(n);
        if (n) check(zg_fast_detect_host(&s, threshold, min_contiguous, nonmax_suppression, out.data(), n, &n));
        return out;
    }
    // device image, list back on the host: device scratch for `capacity` keypoints, run once more with the exact length when the list is
    // longer (the result is deterministic). Synchronises the image's stream.
    std::vector<KeyPoint> detect(const DeviceImage<uint8_t> &image, uint32_t capacity = 1u << 16) const {
        for (;;) {
            void *mem = nullptr;
            check(zg_malloc(&mem, (size_t)capacity * sizeof(KeyPoint) + sizeof(uint32_t)));
            KeyPoint *kps = (KeyPoint *)mem;
            uint32_t *dcount = (uint32_t *)(kps + capacity);
            uint32_t n = 0;
            const zg_image s = image.desc();
            int rc = zg_fast_detect(&s, threshold, min_contiguous, nonmax_suppression, kps, capacity, dcount, image.stream());
            if (rc == ZG_OK) rc = zg_memcpy_d2h(&n, dcount, sizeof(n), image.stream());
            std::vector<KeyPoint> out;
            if (rc == ZG_OK && n <= capacity) {
                out.resize(n);
                if (n) rc = zg_memcpy_d2h(out.data(), kps, (size_t)n * sizeof(KeyPoint), image.stream());
            }
            (void)zg_free(mem);
            check(rc);
            if (n <= capacity) return out;
            capacity = n;
        }
    }
    // asynchronous device form (zg_fast_detect): keypoints / count are device memory; *count receives the full length
    void detectInto(const DeviceImage<uint8_t> &image, KeyPoint *keypoints, uint32_t capacity, uint32_t *count) const {
        const zg_image s = image.desc();
        check(zg_fast_detect(&s, threshold, min_contiguous, nonmax_suppression, keypoints, capacity, count, image.stream()));
    }
};

// ---- features: ORB (src/features/orb.zig, BinaryDescriptor.zig) ----
using BinaryDescriptor = zg_binary_descriptor; // BinaryDescriptor.zig:10
static_assert(sizeof(BinaryDescriptor) == 32, "zg_binary_descriptor is BinaryDescriptor's 32 bytes");

// Orb (src/features/orb.zig:87-109): the reference's fields and defaults; keypoints and descriptors in its order, bit for bit.
struct Orb {
    enum ScoreType { harris_score = ZG_ORB_HARRIS_SCORE, fast_score = ZG_ORB_FAST_SCORE };
    size_t n_features = 500;
    float scale_factor = 1.2f;
    uint8_t n_levels = 8;
    uint8_t edge_threshold = 15;
    uint8_t first_level = 0;
    uint8_t wta_k = 2;
    uint8_t fast_threshold = 20;
    ScoreType score_type = fast_score;
    const float *orientation_weights = nullptr; // null, or the caller's 31 x 31 table (orb.zig:340-357)

    struct Features {
        std::vector<KeyPoint> keypoints;
        std::vector<BinaryDescriptor> descriptors;
    };

    zg_orb_params params() const {
        return zg_orb_params{(uint32_t)(n_features > 0xFFFFFFFFu ? 0xFFFFFFFFu : n_features), scale_factor, n_levels, edge_threshold, first_level, wta_k,
                             fast_threshold, (int32_t)score_type, orientation_weights};
    }
    std::vector<uint32_t> featuresPerLevel() const { // orb.zig:279-334
        const zg_orb_params p = params();
        std::vector<uint32_t> out(n_levels);
        check(zg_orb_features_per_level(&p, out.data()));
        return out;
    }
    uint8_t adaptiveThreshold(uint32_t level) const { // orb.zig:511-517
        const zg_orb_params p = params();
        const int rc = zg_orb_adaptive_threshold(&p, level);
        if (rc < 0) check(-rc);
        return (uint8_t)rc;
    }
    // host image (orb.zig:250-276; with_descriptors = false is Orb.detect): the count first, then the arrays
    Features detectAndCompute(const Image<uint8_t> &image, bool with_descriptors = true) const {
        const zg_image s = image.desc();
        const zg_orb_params p = params();
        uint32_t n = 0;
        check(zg_orb_detect_and_compute_host(&s, &p, nullptr, nullptr, 0, &n));
        Features f;
        f.keypoints.resize(n);
        if (with_descriptors) f.descriptors.resize(n);
        if (n) check(zg_orb_detect_and_compute_host(&s, &p, f.keypoints.data(), with_descriptors ? f.descriptors.data() : nullptr, n, &n));
        return f;
    }
    std::vector<KeyPoint> detect(const Image<uint8_t> &image) const { return detectAndCompute(image, false).keypoints; }
    std::vector<BinaryDescriptor> compute(const Image<uint8_t> &image, const std::vector<KeyPoint> &keypoints) const { // orb.zig:133-144
        const zg_image s = image.desc();
        const zg_orb_params p = params();
        std::vector<BinaryDescriptor> out(keypoints.size());
        if (!keypoints.empty()) check(zg_orb_compute_host(&s, &p, keypoints.data(), (uint32_t)keypoints.size(), out.data()));
        return out;
    }
    // asynchronous device forms: keypoints / descriptors / count are device memory; *count receives the full length
    void detectAndComputeInto(const DeviceImage<uint8_t> &image, KeyPoint *keypoints, BinaryDescriptor *descriptors, uint32_t capacity, uint32_t *count) const {
        const zg_image s = image.desc();
        const zg_orb_params p = params();
        check(zg_orb_detect_and_compute(&s, &p, keypoints, descriptors, capacity, count, image.stream()));
    }
    void computeInto(const DeviceImage<uint8_t> &image, const KeyPoint *keypoints, uint32_t n, BinaryDescriptor *descriptors) const {
        const zg_image s = image.desc();
        const zg_orb_params p = params();
        check(zg_orb_compute(&s, &p, keypoints, n, descriptors, image.stream()));
    }
};

// ---- features: BruteForceMatcher (src/features/matcher.zig) ----
using Match = zg_match; // matcher.zig:10-19 with 32-bit indices
static_assert(sizeof(Match) == 12, "zg_match is 12 bytes");

// MatchStats (matcher.zig:237-270)
struct MatchStats {
    size_t total_matches = 0;
    float mean_distance = 0, min_distance = 0, max_distance = 0;
    static MatchStats compute(const std::vector<Match> &matches) {
        zg_match_statistics s{};
        check(zg_match_stats(matches.empty() ? nullptr : matches.data(), matches.size(), &s));
        MatchStats out;
        out.total_matches = s.total_matches;
        out.mean_distance = s.mean_distance;
        out.min_distance = s.min_distance;
        out.max_distance = s.max_distance;
        return out;
    }
};

// BruteForceMatcher (matcher.zig:33-41): the reference's fields and defaults; match / knnMatch / radiusMatch return its lists, order
// included, bit for bit.
struct BruteForceMatcher {
    bool cross_check = false;
    uint32_t max_distance = 64;
    float ratio_threshold = 0.8f;

    // a descriptor array in device memory and, optionally, the device word that says how many count (what Orb::detectAndComputeInto wrote)
    struct DeviceDescriptors {
        const BinaryDescriptor *data;
        uint32_t capacity;
        const uint32_t *count = nullptr;
        zg_descriptor_set set() const { return zg_descriptor_set{data, capacity, count}; }
    };

    zg_matcher_params params() const { return zg_matcher_params{cross_check ? 1 : 0, max_distance, ratio_threshold}; }
    static zg_descriptor_set hostSet(const std::vector<BinaryDescriptor> &d) {
        return zg_descriptor_set{d.empty() ? nullptr : d.data(), (uint32_t)d.size(), nullptr};
    }

    std::vector<Match> match(const std::vector<BinaryDescriptor> &query, const std::vector<BinaryDescriptor> &train) const { // :44-106
        const zg_descriptor_set q = hostSet(query), t = hostSet(train);
        const zg_matcher_params p = params();
        std::vector<Match> out(query.size());
        uint32_t n = 0;
        check(zg_match_descriptors_host(&q, &t, &p, out.empty() ? nullptr : out.data(), q.capacity, &n));
        out.resize(n);
        return out;
    }
    std::vector<std::vector<Match>> knnMatch(const std::vector<BinaryDescriptor> &query, const std::vector<BinaryDescriptor> &train, size_t k) const { // :109-162
        if (query.empty() || train.empty() || k == 0) return {};
        const zg_descriptor_set q = hostSet(query), t = hostSet(train);
        const zg_matcher_params p = params();
        const uint32_t kk = (uint32_t)(k < train.size() ? k : train.size()); // a row is never longer
        std::vector<Match> flat(query.size() * kk);
        std::vector<uint32_t> rows(query.size());
        check(zg_match_knn_host(&q, &t, &p, kk, flat.data(), rows.data()));
        std::vector<std::vector<Match>> out(query.size());
        for (size_t i = 0; i < out.size(); ++i) out[i].assign(flat.begin() + i * kk, flat.begin() + i * kk + rows[i]);
        return out;
    }
    std::vector<std::vector<Match>> radiusMatch(const std::vector<BinaryDescriptor> &query, const std::vector<BinaryDescriptor> &train, float max_dist) const { // :165-212
        if (query.empty() || train.empty()) return {};
        const zg_descriptor_set q = hostSet(query), t = hostSet(train);
        std::vector<uint32_t> rows(query.size());
        uint32_t n = 0;
        check(zg_match_radius_host(&q, &t, max_dist, nullptr, 0, rows.data(), &n)); // the row lengths first
        std::vector<Match> flat(n);
        if (n) check(zg_match_radius_host(&q, &t, max_dist, flat.data(), n, rows.data(), &n));
        std::vector<std::vector<Match>> out(query.size());
        size_t at = 0;
        for (size_t i = 0; i < out.size(); at += rows[i++]) out[i].assign(flat.begin() + at, flat.begin() + at + rows[i]);
        return out;
    }
    // asynchronous device forms: every pointer is device memory; nothing is synchronised, all three can be recorded into a graph
    void matchInto(const DeviceDescriptors &query, const DeviceDescriptors &train, Match *matches, uint32_t capacity, uint32_t *count, zg_stream stream = nullptr) const {
        const zg_descriptor_set q = query.set(), t = train.set();
        const zg_matcher_params p = params();
        check(zg_match_descriptors(&q, &t, &p, matches, capacity, count, stream));
    }
    void knnMatchInto(const DeviceDescriptors &query, const DeviceDescriptors &train, uint32_t k, Match *matches, uint32_t *row_counts, zg_stream stream = nullptr) const {
        const zg_descriptor_set q = query.set(), t = train.set();
        const zg_matcher_params p = params();
        check(zg_match_knn(&q, &t, &p, k, matches, row_counts, stream));
    }
    void radiusMatchInto(const DeviceDescriptors &query, const DeviceDescriptors &train, float max_dist, Match *matches, uint32_t capacity, uint32_t *row_counts,
                         uint32_t *count, zg_stream stream = nullptr) const {
        const zg_descriptor_set q = query.set(), t = train.set();
        check(zg_match_radius(&q, &t, max_dist, matches, capacity, row_counts, count, stream));
    }
};

// ---- image: HoughTransform (src/image/hough.zig) ----
// HoughTransform (hough.zig:11-230): compute adds the votes of a size x size box of an edge map to a size x size accumulator, findLines
// returns the reference's list of lines, order included, bit for bit.
class HoughTransform {
  public:
    using Line = zg_hough_line; // hough.zig:13-25, field for field
    static_assert(sizeof(Line) == 28, "zg_hough_line is 28 bytes");

    explicit HoughTransform(uint32_t size) : size_(size) { check(zg_hough_create(size, &h_)); }          // init (:38-66)
    HoughTransform(uint32_t size, const std::vector<int32_t> &cos_table, const std::vector<int32_t> &sin_table) : size_(size) {
        if (cos_table.size() != size || sin_table.size() != size) throw InvalidArgument(ZG_ERR_INVALID_ARGUMENT, "HoughTransform: size entries a table");
        check(zg_hough_create_with_tables(size, cos_table.data(), sin_table.data(), &h_));
    }
    HoughTransform(HoughTransform &&o) noexcept : h_(o.h_), size_(o.size_) { o.h_ = nullptr; }
    HoughTransform &operator=(HoughTransform &&o) noexcept { if (this != &o) { release(); h_ = o.h_; size_ = o.size_; o.h_ = nullptr; } return *this; }
    HoughTransform(const HoughTransform &) = delete;
    HoughTransform &operator=(const HoughTransform &) = delete;
    ~HoughTransform() { release(); }

    uint32_t size() const { return size_; }
    uint32_t evenSize() const { return size_ % 2 == 0 ? size_ : size_ - 1; }
    zg_hough_t handle() const { return h_; }
    static void tables(uint32_t size, std::vector<int32_t> &cos_table, std::vector<int32_t> &sin_table) {
        cos_table.assign(size, 0);
        sin_table.assign(size, 0);
        check(zg_hough_tables_host(size, cos_table.data(), sin_table.data()));
    }

    // compute (:75-139): host images; the votes are added to `accumulator`, which the caller clears
    void compute(const Image<uint8_t> &edges, const Rectangle<uint32_t> &box, const Image<uint32_t> &accumulator) const;
    // findLines (:142-204) of a host accumulator. Repeated with more room when the candidates or lines outnumber the first guess.
    std::vector<Line> findLines(const Image<uint32_t> &accumulator, uint32_t threshold, float angle_nms_thresh, float radius_nms_thresh) const;
    // asynchronous device forms: every pointer is device memory; nothing is synchronised, both can be recorded into a graph
    void computeInto(const DeviceImage<uint8_t> &edges, const Rectangle<uint32_t> &box, uint32_t *accumulator, size_t acc_stride, zg_stream stream = nullptr) const;
    void findLinesInto(const uint32_t *accumulator, size_t acc_stride, uint32_t threshold, const uint32_t *threshold_device, float angle_nms_thresh,
                       float radius_nms_thresh, uint32_t max_candidates, Line *lines, uint32_t capacity, uint32_t *counts, zg_stream stream = nullptr) const {
        check(zg_hough_find_lines(h_, accumulator, acc_stride, threshold, threshold_device, angle_nms_thresh, radius_nms_thresh, max_candidates, lines,
                                  capacity, counts, stream));
    }

  private:
    void release() { if (h_) (void)zg_hough_destroy(h_); h_ = nullptr; }
    zg_hough_t h_ = nullptr;
    uint32_t size_ = 0;
};

// (Image<uint32_t> is a shape and a buffer here: u32 is no pixel type of the image ops, and none of them is instantiated for it)
inline void HoughTransform::compute(const Image<uint8_t> &edges, const Rectangle<uint32_t> &box, const Image<uint32_t> &accumulator) const {
    if (accumulator.rows != size_ || accumulator.cols != size_) throw DimensionMismatch(ZG_ERR_DIMENSION_MISMATCH, "HoughTransform::compute: accumulator"); // :77
    const zg_image e = edges.desc();
    check(zg_hough_compute_host(h_, &e, box.l, box.t, box.r, box.b, accumulator.data, accumulator.stride));
}
inline std::vector<HoughTransform::Line> HoughTransform::findLines(const Image<uint32_t> &accumulator, uint32_t threshold, float angle_nms_thresh,
                                                                   float radius_nms_thresh) const {
    if (accumulator.rows != size_ || accumulator.cols != size_) throw DimensionMismatch(ZG_ERR_DIMENSION_MISMATCH, "HoughTransform::findLines: accumulator");
    uint32_t max_candidates = 4096, capacity = 256;
    for (;;) {
        std::vector<Line> out(capacity);
        uint32_t counts[2] = {0, 0};
        check(zg_hough_find_lines_host(h_, accumulator.data, accumulator.stride, threshold, angle_nms_thresh, radius_nms_thresh, max_candidates, out.data(),
                                       capacity, counts));
        if (counts[0] > ZG_HOUGH_MAX_CANDIDATES) throw Error(ZG_ERR_UNSUPPORTED, "HoughTransform::findLines: more than ZG_HOUGH_MAX_CANDIDATES candidates");
        if (counts[0] > max_candidates) { max_candidates = counts[0]; continue; }
        if (counts[1] > capacity) { capacity = counts[1]; continue; }
        out.resize(counts[1]);
        return out;
    }
}
inline void HoughTransform::computeInto(const DeviceImage<uint8_t> &edges, const Rectangle<uint32_t> &box, uint32_t *accumulator, size_t acc_stride,
                                        zg_stream stream) const {
    const zg_image e = edges.desc();
    check(zg_hough_compute(h_, &e, box.l, box.t, box.r, box.b, accumulator, acc_stride, stream));
}

// ---- canvas: Canvas(T) (src/canvas/Canvas.zig) ----
enum class DrawMode { fast = ZG_DRAW_FAST, soft = ZG_DRAW_SOFT };                         // Canvas.zig:19-24
struct Point2 { float x, y; };
// BitmapFont (src/font/BitmapFont.zig) with the caller's glyph data, in the reference's two forms; checked when made (zg_font_check) and
// uploaded to the current device on first use there. The library ships no glyphs.
inline std::vector<uint32_t> decodeUtf8(const std::string &s) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < s.size();) {
        const uint8_t b = (uint8_t)s[i];
        const int extra = b < 0x80 ? 0 : (b >> 5) == 6 ? 1 : (b >> 4) == 14 ? 2 : (b >> 3) == 30 ? 3 : -1;
        if (extra < 0 || i + (size_t)extra >= s.size() + (extra ? 0 : 1)) throw Error(ZG_ERR_INVALID_ARGUMENT, "decodeUtf8: invalid UTF-8");
        uint32_t cp = extra == 0 ? b : (uint32_t)(b & (0x3F >> extra));
        for (int k = 1; k <= extra; ++k) {
            const uint8_t c = (uint8_t)s[i + (size_t)k];
            if ((c >> 6) != 2) throw Error(ZG_ERR_INVALID_ARGUMENT, "decodeUtf8: invalid UTF-8");
            cp = (cp << 6) | (c & 0x3Fu);
        }
        out.push_back(cp);
        i += (size_t)extra + 1;
    }
    return out;
}
class BitmapFont {
  public:
    // glyph c is char_height rows of (char_width + 7) / 8 bytes at (c - first_char) times that, bits LSB first; the font ends with the last whole glyph of data
    static BitmapFont fromFixed(uint8_t char_width, uint8_t char_height, uint8_t first_char, std::vector<uint8_t> data) {
        const size_t per_char = (size_t)char_height * (((size_t)char_width + 7) / 8), count = per_char ? data.size() / per_char : 0;
        if (count < 1) throw Error(ZG_ERR_INVALID_ARGUMENT, "BitmapFont::fromFixed: no whole glyph in data");
        BitmapFont f;
        f.meta_.char_width = char_width; f.meta_.char_height = char_height; f.meta_.first_char = first_char;
        f.meta_.last_char = (uint8_t)std::min<size_t>(255, (size_t)first_char + count - 1);
        f.data_ = std::move(data);
        f.checked();
        return f;
    }
    // the glyph table (sorted by codepoint here); a line is char_height high, a codepoint the table lacks advances by char_width
    static BitmapFont fromGlyphs(uint8_t char_height, std::vector<zg_glyph> glyphs, std::vector<uint8_t> data, uint8_t char_width) {
        BitmapFont f;
        f.meta_.char_width = char_width; f.meta_.char_height = char_height;
        std::stable_sort(glyphs.begin(), glyphs.end(), [](const zg_glyph &a, const zg_glyph &b) { return a.codepoint < b.codepoint; });
        f.glyphs_ = std::move(glyphs);
        f.table_ = true;
        f.data_ = std::move(data);
        f.checked();
        return f;
    }
    BitmapFont(BitmapFont &&o) noexcept : meta_(o.meta_), data_(std::move(o.data_)), glyphs_(std::move(o.glyphs_)), table_(o.table_), device_(o.device_) { o.device_ = zg_font{}; }
    BitmapFont(const BitmapFont &) = delete;
    BitmapFont &operator=(const BitmapFont &) = delete;
    ~BitmapFont() { (void)zg_font_free(&device_); }
    zg_font host() const {
        zg_font f = meta_;
        f.data = data_.data(); f.data_len = (uint32_t)data_.size();
        f.glyphs = table_ ? (glyphs_.empty() ? &no_glyph_ : glyphs_.data()) : nullptr; f.n_glyphs = (uint32_t)glyphs_.size();
        return f;
    }
    const zg_font &device() const { // uploaded on first use
        if (device_.data == nullptr) {
            const zg_font h = host();
            check(zg_font_upload(&h, &device_));
        }
        return device_;
    }
    // getTextBounds: l = t = 0, r and b exclusive
    Rectangle<float> textBounds(const std::string &utf8, float scale = 1.0f) const {
        const std::vector<uint32_t> cps = decodeUtf8(utf8);
        const zg_font h = host();
        float ltrb[4];
        check(zg_text_bounds_host(&h, cps.data(), (uint32_t)cps.size(), scale, ltrb));
        return Rectangle<float>{ltrb[0], ltrb[1], ltrb[2], ltrb[3]};
    }

  private:
    BitmapFont() = default;
    void checked() const {
        if (zg_sizeof_font() != sizeof(zg_font) || zg_sizeof_glyph() != sizeof(zg_glyph) || zg_sizeof_text_cmd() != sizeof(zg_text_cmd)) // the zg_sizeof_step rule
            throw Error(ZG_ERR_INVALID_ARGUMENT, "libzignal_hip: zg_font, zg_glyph or zg_text_cmd has another size in the library than in this header");
        const zg_font h = host();
        check(zg_font_check(&h));
    }
    zg_font meta_{};
    std::vector<uint8_t> data_;
    std::vector<zg_glyph> glyphs_;
    bool table_ = false;
    zg_glyph no_glyph_{};
    mutable zg_font device_{};
};

// Canvas(T) over an Image<T> or DeviceImage<T> of u8, Rgb<uint8_t> or Rgba<uint8_t>: the draw methods (lines, rectangles, circles, arcs,
// polygons, Bézier curves, spline polygons) append to a command list, flush()
// executes it into the image in list order (zg_canvas_draw_host for host pixels; for device pixels the two lists are uploaded and
// zg_canvas_draw — zg_canvas_draw_arcs when the list holds an arc — runs on the image's stream) and empties it. The result equals the reference making the same calls, byte for byte.
template <typename T, template <class> class Img = Image> class Canvas {
  public:
    static_assert(PixelTraits<T>::pixel == ZG_PIXEL_U8 || PixelTraits<T>::pixel == ZG_PIXEL_RGB_U8 || PixelTraits<T>::pixel == ZG_PIXEL_RGBA_U8,
                  "Canvas draws on u8, Rgb<uint8_t> and Rgba<uint8_t> images");
    explicit Canvas(const Img<T> &image) : image_(&image) {
        if (zg_sizeof_draw_cmd() != sizeof(zg_draw_cmd)) // the zg_sizeof_step rule
            throw Error(ZG_ERR_INVALID_ARGUMENT, "libzignal_hip: sizeof(zg_draw_cmd) is " + std::to_string(zg_sizeof_draw_cmd()) + " in the library, " +
                                                     std::to_string(sizeof(zg_draw_cmd)) + " in this header");
    }
    Canvas &drawLine(Point2 p1, Point2 p2, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return add(ZG_DRAW_LINE, mode, width, color, p1.x, p1.y, p2.x, p2.y);
    }
    Canvas &drawRectangle(Rectangle<float> r, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return add(ZG_DRAW_RECT, mode, width, color, r.l, r.t, r.r, r.b);
    }
    Canvas &fillRectangle(Rectangle<float> r, Rgba<uint8_t> color, DrawMode mode = DrawMode::fast) { return add(ZG_DRAW_FILL_RECT, mode, 1, color, r.l, r.t, r.r, r.b); }
    Canvas &drawCircle(Point2 center, float radius, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return add(ZG_DRAW_CIRCLE, mode, width, color, center.x, center.y, radius, 0.0f);
    }
    Canvas &fillCircle(Point2 center, float radius, Rgba<uint8_t> color, DrawMode mode = DrawMode::fast) {
        return add(ZG_DRAW_FILL_CIRCLE, mode, 1, color, center.x, center.y, radius, 0.0f);
    }
    // angles in radians from the positive x axis towards positive y, any finite value; |end - start| >= 2 pi is the circle
    Canvas &drawArc(Point2 center, float radius, float start_angle, float end_angle, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return addArc(ZG_DRAW_ARC, center, radius, start_angle, end_angle, mode, width, color);
    }
    Canvas &fillArc(Point2 center, float radius, float start_angle, float end_angle, Rgba<uint8_t> color, DrawMode mode = DrawMode::fast) {
        return addArc(ZG_DRAW_FILL_ARC, center, radius, start_angle, end_angle, mode, 1, color);
    }
    Canvas &drawPolygon(const std::vector<Point2> &polygon, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_POLYGON, polygon, mode, width, color);
    }
    Canvas &fillPolygon(const std::vector<Point2> &polygon, Rgba<uint8_t> color, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_FILL_POLYGON, polygon, mode, 1, color);
    }
    Canvas &drawQuadraticBezier(Point2 p0, Point2 p1, Point2 p2, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_QUAD_BEZIER, {p0, p1, p2}, mode, width, color);
    }
    Canvas &drawCubicBezier(Point2 p0, Point2 p1, Point2 p2, Point2 p3, Rgba<uint8_t> color, uint32_t width = 1, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_CUBIC_BEZIER, {p0, p1, p2, p3}, mode, width, color);
    }
    // tension: 0 (sharp corners) to 1 (smoothest), clamped as in the reference
    Canvas &drawSplinePolygon(const std::vector<Point2> &polygon, Rgba<uint8_t> color, uint32_t width, float tension, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_SPLINE_POLYGON, polygon, mode, width, color, tension);
    }
    // at most ZG_CANVAS_MAX_CURVE_POINTS points once tessellated
    Canvas &fillSplinePolygon(const std::vector<Point2> &polygon, Rgba<uint8_t> color, float tension, DrawMode mode = DrawMode::fast) {
        return addPolygon(ZG_DRAW_FILL_SPLINE_POLYGON, polygon, mode, 1, color, tension);
    }
    // drawText: UTF-8 text ('\n' starts a new line) with its top left corner at `position`. scale == 1 lights the glyphs' bits in either mode;
    // otherwise .fast writes a block per bit and .soft box-filtered coverage. The font must outlive flush().
    Canvas &drawText(const std::string &utf8, Point2 position, Rgba<uint8_t> color, const BitmapFont &font, float scale = 1.0f, DrawMode mode = DrawMode::fast) {
        TextItem t{};
        t.cmd.x = position.x; t.cmd.y = position.y; t.cmd.scale = scale; t.cmd.mode = (int32_t)mode;
        t.cmd.color[0] = color.r; t.cmd.color[1] = color.g; t.cmd.color[2] = color.b; t.cmd.color[3] = color.a;
        t.codepoints = decodeUtf8(utf8);
        t.font = &font;
        t.after = cmds_.size();
        texts_.push_back(std::move(t));
        return *this;
    }
    const std::vector<zg_draw_cmd> &commands() const { return cmds_; }
    // A list with text in it is cut into maximal runs of text and of everything else, issued in list order: the others through
    // zg_canvas_draw (or _arcs, or _host), a run of text through zg_canvas_draw_text (or _host), one call per font.
    void flush() {
        std::vector<zg_draw_cmd> cmds;
        std::vector<float> vertices;
        std::vector<TextItem> texts;
        cmds.swap(cmds_);
        vertices.swap(vertices_);
        texts.swap(texts_);
        size_t done = 0;
        for (size_t i = 0; i < texts.size();) {
            if (texts[i].after > done) flushShapes(cmds.data() + done, texts[i].after - done, vertices);
            done = texts[i].after;
            size_t j = i + 1;
            while (j < texts.size() && texts[j].after == done && texts[j].font == texts[i].font) ++j;
            flushText(texts.data() + i, j - i);
            i = j;
        }
        if (cmds.size() > done) flushShapes(cmds.data() + done, cmds.size() - done, vertices);
    }
    // the device-list form of drawText: every pointer is device memory (the font's through font.device()); asynchronous, recordable into a graph
    void drawTexts(const BitmapFont &font, const zg_text_cmd *cmds, uint32_t n, const uint32_t *codepoints, uint32_t n_codepoints, const uint32_t *count_device = nullptr) const {
        const zg_image d = image_->desc();
        check(zg_canvas_draw_text(&d, &font.device(), cmds, n, count_device, codepoints, n_codepoints, image_->stream()));
    }

  private:
    struct TextItem {
        zg_text_cmd cmd;
        std::vector<uint32_t> codepoints;
        const BitmapFont *font;
        size_t after; // the number of other commands issued before it
    };
    void flushText(const TextItem *items, size_t count) {
        std::vector<zg_text_cmd> cmds;
        std::vector<uint32_t> cps;
        for (size_t k = 0; k < count; ++k) {
            zg_text_cmd c = items[k].cmd;
            c.first_codepoint = (uint32_t)cps.size(); c.n_codepoints = (uint32_t)items[k].codepoints.size();
            cps.insert(cps.end(), items[k].codepoints.begin(), items[k].codepoints.end());
            cmds.push_back(c);
        }
        const zg_image d = image_->desc();
        const uint32_t n = (uint32_t)cmds.size(), ncp = (uint32_t)cps.size();
        if constexpr (!Img<T>::on_device) {
            const zg_font h = items[0].font->host();
            check(zg_canvas_draw_text_host(&d, &h, cmds.data(), n, ncp ? cps.data() : nullptr, ncp));
        } else {
            if (ncp == 0) return;
            const zg_font &f = items[0].font->device();
            void *mem = nullptr;
            const size_t cmd_bytes = (cmds.size() * sizeof(zg_text_cmd) + 255) / 256 * 256;
            check(zg_malloc(&mem, cmd_bytes + cps.size() * sizeof(uint32_t) + 256));
            int rc = zg_memcpy_h2d(mem, cmds.data(), cmds.size() * sizeof(zg_text_cmd), image_->stream());
            if (!rc) rc = zg_memcpy_h2d((char *)mem + cmd_bytes, cps.data(), cps.size() * sizeof(uint32_t), image_->stream());
            if (!rc) rc = zg_canvas_draw_text(&d, &f, (const zg_text_cmd *)mem, n, nullptr, (const uint32_t *)((char *)mem + cmd_bytes), ncp, image_->stream());
            (void)zg_free(mem); // waits for the draw that reads the lists
            check(rc);
        }
    }
    // `count` commands of the list; their vertex ranges index the whole vertex array
    void flushShapes(const zg_draw_cmd *cmds_at, size_t count, const std::vector<float> &vertices) {
        const std::vector<zg_draw_cmd> cmds(cmds_at, cmds_at + count);
        if (cmds.empty()) return;
        const zg_image d = image_->desc();
        const uint32_t n = (uint32_t)cmds.size(), nv = (uint32_t)(vertices.size() / 2);
        if constexpr (!Img<T>::on_device) {
            check(zg_canvas_draw_host(&d, cmds.data(), n, nv ? vertices.data() : nullptr, nv));
        } else {
            void *mem = nullptr;
            const size_t cmd_bytes = (cmds.size() * sizeof(zg_draw_cmd) + 255) / 256 * 256;
            check(zg_malloc(&mem, cmd_bytes + vertices.size() * sizeof(float) + 256));
            int rc = zg_memcpy_h2d(mem, cmds.data(), cmds.size() * sizeof(zg_draw_cmd), image_->stream());
            if (!rc && nv) rc = zg_memcpy_h2d((char *)mem + cmd_bytes, vertices.data(), vertices.size() * sizeof(float), image_->stream());
            bool arcs = false; // the entry point whose kernel knows arcs only for a list that holds one
            for (const zg_draw_cmd &c : cmds) arcs = arcs || c.kind == ZG_DRAW_ARC || c.kind == ZG_DRAW_FILL_ARC;
            if (!rc) rc = (arcs ? zg_canvas_draw_arcs : zg_canvas_draw)(&d, (const zg_draw_cmd *)mem, n, nullptr, nv ? (const float *)((char *)mem + cmd_bytes) : nullptr, nv, image_->stream());
            (void)zg_free(mem); // waits for the draw that reads the lists
            check(rc);
        }
    }

  public:
    // the device-list form: every pointer is device memory; asynchronous, nothing is synchronised, recordable into a graph
    // arcs: zg_canvas_draw_arcs, for a list that may hold ZG_DRAW_ARC or ZG_DRAW_FILL_ARC (zg_canvas_draw skips them)
    void draw(const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device = nullptr, const float *vertices = nullptr, uint32_t n_vertices = 0,
              bool arcs = false) const {
        const zg_image d = image_->desc();
        check((arcs ? zg_canvas_draw_arcs : zg_canvas_draw)(&d, cmds, n, count_device, vertices, n_vertices, image_->stream()));
    }

  private:
    Canvas &add(int kind, DrawMode mode, uint32_t width, Rgba<uint8_t> color, float a, float b, float c, float e) {
        zg_draw_cmd cmd{};
        cmd.kind = kind; cmd.mode = (int32_t)mode; cmd.width = width;
        cmd.color[0] = color.r; cmd.color[1] = color.g; cmd.color[2] = color.b; cmd.color[3] = color.a;
        cmd.p[0] = a; cmd.p[1] = b; cmd.p[2] = c; cmd.p[3] = e;
        cmds_.push_back(cmd);
        return *this;
    }
    Canvas &addPolygon(int kind, const std::vector<Point2> &polygon, DrawMode mode, uint32_t width, Rgba<uint8_t> color, float p0 = 0.0f) {
        add(kind, mode, width, color, p0, 0, 0, 0);
        cmds_.back().first_vertex = (uint32_t)(vertices_.size() / 2);
        cmds_.back().n_vertices = (uint32_t)polygon.size();
        for (const Point2 &p : polygon) { vertices_.push_back(p.x); vertices_.push_back(p.y); }
        return *this;
    }
    Canvas &addArc(int kind, Point2 center, float radius, float start_angle, float end_angle, DrawMode mode, uint32_t width, Rgba<uint8_t> color) {
        add(kind, mode, width, color, center.x, center.y, radius, 0.0f);
        cmds_.back().first_vertex = (uint32_t)(vertices_.size() / 2); // the angle pair is one entry of the vertex array
        cmds_.back().n_vertices = 1;
        vertices_.push_back(start_angle); vertices_.push_back(end_angle);
        return *this;
    }
    const Img<T> *image_;
    std::vector<zg_draw_cmd> cmds_;
    std::vector<float> vertices_;
    std::vector<TextItem> texts_;
};

// FeatureDistributionMatching(T) (src/fdm.zig:19-274) for T = uint8_t, Rgb<uint8_t>, Rgba<uint8_t>: setTarget once, then setSource and
// update for every frame; the source is matched in place. Over Image (the default) every update stages source and target and is
// synchronous (zg_fdm_match_host); over DeviceImage setTarget leaves the target's statistics in device memory and update enqueues moments,
// transform and apply on the source's stream with nothing copied or synchronised (zg_fdm_match_frames). The images are borrowed: they
// outlive the calls that use them. The statistics come from exact integer moments, not from the reference's Welford recurrence
// (include/zignal_hip_fdm.h says what that can change: a byte whose value before rounding is a tie); on an Rgba frame against a grey target
// alpha becomes 0, as in the reference.
struct NoTargetSet : std::logic_error { NoTargetSet() : std::logic_error("NoTargetSet") {} };   // fdm.zig:142
struct NoSourceSet : std::logic_error { NoSourceSet() : std::logic_error("NoSourceSet") {} };   // fdm.zig:143
template <typename T, template <typename> class Img = Image> class FeatureDistributionMatching {
    static_assert(PixelTraits<T>::pixel == ZG_PIXEL_U8 || PixelTraits<T>::pixel == ZG_PIXEL_RGB_U8 || PixelTraits<T>::pixel == ZG_PIXEL_RGBA_U8,
                  "FeatureDistributionMatching takes u8, Rgb(u8) and Rgba(u8) (fdm.zig:20)");
    static constexpr bool on_device = std::is_same<Img<T>, DeviceImage<T>>::value;

  public:
    FeatureDistributionMatching() = default;
    FeatureDistributionMatching(const FeatureDistributionMatching &) = delete;
    FeatureDistributionMatching &operator=(const FeatureDistributionMatching &) = delete;
    ~FeatureDistributionMatching() { if (records_) zg_free(records_); }

    void setTarget(const Img<T> &target) {                                                // fdm.zig:68-124
        target_ = target.desc();
        if constexpr (on_device) {
            if (!records_) check(zg_malloc(&records_, 512));
            zg_fdm_moments *m = (zg_fdm_moments *)records_;
            check(zg_fdm_compute_moments(&target_, m, target.stream()));
            check(zg_fdm_target_from_moments(m, prepared(), target.stream()));
        }
        has_target_ = true;
    }
    void setSource(const Img<T> &source) { source_ = &source; }                            // fdm.zig:127-130
    void update() {                                                                        // fdm.zig:141-273
        if (!has_target_) throw NoTargetSet();
        if (!source_) throw NoSourceSet();
        const zg_image s = source_->desc();
        if constexpr (on_device) check(zg_fdm_match_frames(&s, 1, nullptr, prepared(), source_->stream()));
        else check(zg_fdm_match_host(&s, &target_));
    }
    void match(const Img<T> &source, const Img<T> &target) {                               // fdm.zig:133-137
        setTarget(target);
        setSource(source);
        update();
    }
    // every frame against the target set before, in one chain (on the first frame's stream)
    void updateFrames(const std::vector<const Img<T> *> &frames) {
        if (!has_target_) throw NoTargetSet();
        if (frames.empty()) return;
        std::vector<zg_image> d;
        for (const Img<T> *f : frames) d.push_back(f->desc());
        if constexpr (on_device) check(zg_fdm_match_frames(d.data(), (uint32_t)d.size(), nullptr, prepared(), frames[0]->stream()));
        else check(zg_fdm_match_frames_host(d.data(), (uint32_t)d.size(), &target_));
    }

  private:
    zg_fdm_target *prepared() const { return (zg_fdm_target *)((char *)records_ + 256); }
    zg_image target_{};
    const Img<T> *source_ = nullptr;
    void *records_ = nullptr; // device: the target's moments, and at 256 bytes its zg_fdm_target
    bool has_target_ = false;
};

// ---- features: Tracer (src/features/Tracer.zig) ----
// The reference's two fields and defaults; trace returns its list of paths, each a list of (x = col, y = row) points, bit for bit.
struct Tracer {
    uint32_t min_path_length = 5;
    float simplification_epsilon = 1.0f;
    using Path = std::vector<Point2>;

    zg_tracer_options c_options() const { return zg_tracer_options{min_path_length, simplification_epsilon}; }

    // host image: the counts first, then the lists (two synchronous calls)
    std::vector<Path> trace(const Image<uint8_t> &edges) const {
        const zg_image s = edges.desc();
        const zg_tracer_options o = c_options();
        uint32_t counts[4] = {0, 0, 0, 0};
        check(zg_trace_paths_host(&s, &o, nullptr, 0, nullptr, 0, counts));
        std::vector<Point2> points(counts[1]);
        std::vector<uint32_t> offsets((size_t)counts[0] + 1);
        check(zg_trace_paths_host(&s, &o, points.empty() ? nullptr : &points[0].x, counts[1], offsets.data(), counts[0], counts));
        return split(points, offsets);
    }
    // device image, lists back on the host: the counts first, then device scratch of exactly that size. Synchronises the image's stream.
    std::vector<Path> trace(const DeviceImage<uint8_t> &edges) const {
        void *mem = nullptr;
        check(zg_malloc(&mem, 32));
        uint32_t counts[4] = {0, 0, 0, 0};
        int rc = traceIntoStatus(edges, nullptr, 0, (uint32_t *)mem + 4, 0, (uint32_t *)mem);
        if (rc == ZG_OK) rc = zg_memcpy_d2h(counts, mem, sizeof counts, edges.stream());
        (void)zg_free(mem);
        check(rc);
        const size_t point_bytes = ((size_t)counts[1] * sizeof(Point2) + 255) / 256 * 256, offset_bytes = ((size_t)counts[0] + 1) * 4;
        check(zg_malloc(&mem, point_bytes + offset_bytes + 16));
        uint32_t *doffsets = (uint32_t *)((char *)mem + point_bytes), *dcounts = doffsets + counts[0] + 1;
        std::vector<Point2> points(counts[1]);
        std::vector<uint32_t> offsets((size_t)counts[0] + 1);
        rc = traceIntoStatus(edges, counts[1] ? (Point2 *)mem : nullptr, counts[1], doffsets, counts[0], dcounts);
        if (rc == ZG_OK) rc = zg_memcpy_d2h(offsets.data(), doffsets, offset_bytes, edges.stream());
        if (rc == ZG_OK && counts[1]) rc = zg_memcpy_d2h(points.data(), mem, (size_t)counts[1] * sizeof(Point2), edges.stream());
        (void)zg_free(mem);
        check(rc);
        return split(points, offsets);
    }
    // asynchronous device form (zg_trace_paths): points, path_offsets (path_capacity + 1 words) and counts (four words) are device memory
    void traceInto(const DeviceImage<uint8_t> &edges, Point2 *points, uint32_t point_capacity, uint32_t *path_offsets, uint32_t path_capacity,
                   uint32_t *counts) const {
        check(traceIntoStatus(edges, points, point_capacity, path_offsets, path_capacity, counts));
    }

  private:
    int traceIntoStatus(const DeviceImage<uint8_t> &edges, Point2 *points, uint32_t point_capacity, uint32_t *path_offsets, uint32_t path_capacity,
                        uint32_t *counts) const {
        const zg_image s = edges.desc();
        const zg_tracer_options o = c_options();
        return zg_trace_paths(&s, &o, points ? &points->x : nullptr, point_capacity, path_offsets, path_capacity, counts, edges.stream());
    }
    static std::vector<Path> split(const std::vector<Point2> &points, const std::vector<uint32_t> &offsets) {
        std::vector<Path> paths(offsets.size() - 1);
        for (size_t i = 0; i + 1 < offsets.size(); ++i) paths[i].assign(points.begin() + offsets[i], points.begin() + offsets[i + 1]);
        return paths;
    }
};
static_assert(sizeof(Point2) == 8, "a traced point is two f32");

// ---- qrcode: the detector (src/qrcode/detector.zig:57-641) ----
// A frame to the sampled module grids and their corners, which are what the reference hands to decoder.decodeModules, in the reference's
// order of trial, bit for bit. Decoding the grids is host work outside this library.
struct QrGrid {
    int binarize = 0;          // the pass that produced it: ZG_QR_ADAPTIVE, ZG_QR_OTSU or ZG_QR_BINARY
    uint32_t version = 0, dim = 0, fourth_index = 0;
    int32_t version_hint = -1; // decoder.readVersion of this grid for version >= 7
    float corners[8] = {};     // top left, top right, bottom left, bottom right, (x, y) each
    double transform[9] = {};  // module space to image space, row-major
    std::vector<uint8_t> modules; // dim * dim, 0 or 1
};

struct QrDetector {
    // host image, one binarisation: the counts first, then the lists (two synchronous calls). The record of every stage comes back.
    template <typename T> zg_qr_detection detectPass(const Image<T> &image, int binarize, std::vector<QrGrid> &out) const {
        const zg_image s = image.desc();
        zg_qr_detection det;
        check(zg_qr_detect_host(&s, binarize, &det, nullptr, 0, nullptr, 0));
        const uint32_t n = det.grids_total;
        std::vector<zg_qr_grid> grids(n);
        std::vector<uint8_t> modules((size_t)n * ZG_QR_MAX_MODULES);
        check(zg_qr_detect_host(&s, binarize, &det, n ? grids.data() : nullptr, n, n ? modules.data() : nullptr, n * ZG_QR_MAX_MODULES));
        append(out, grids, modules, det.grids_written, binarize);
        return det;
    }
    // device image, lists back on the host: the counts first, then device scratch of exactly that size. Synchronises the image's stream.
    template <typename T> zg_qr_detection detectPass(const DeviceImage<T> &image, int binarize, std::vector<QrGrid> &out) const {
        void *mem = nullptr;
        check(zg_malloc(&mem, sizeof(zg_qr_detection)));
        zg_qr_detection det;
        int rc = detectIntoStatus(image, binarize, (zg_qr_detection *)mem, nullptr, 0, nullptr, 0);
        if (rc == ZG_OK) rc = zg_memcpy_d2h(&det, mem, sizeof det, image.stream());
        (void)zg_free(mem);
        check(rc);
        const uint32_t n = det.grids_total;
        const size_t grid_bytes = ((size_t)n * sizeof(zg_qr_grid) + 255) / 256 * 256, module_bytes = ((size_t)n * ZG_QR_MAX_MODULES + 255) / 256 * 256;
        check(zg_malloc(&mem, grid_bytes + module_bytes + sizeof(zg_qr_detection)));
        zg_qr_grid *dgrids = (zg_qr_grid *)mem;
        uint8_t *dmodules = (uint8_t *)mem + grid_bytes;
        zg_qr_detection *ddet = (zg_qr_detection *)((char *)mem + grid_bytes + module_bytes);
        std::vector<zg_qr_grid> grids(n);
        std::vector<uint8_t> modules((size_t)n * ZG_QR_MAX_MODULES);
        rc = detectIntoStatus(image, binarize, ddet, n ? dgrids : nullptr, n, n ? dmodules : nullptr, n * ZG_QR_MAX_MODULES);
        if (rc == ZG_OK) rc = zg_memcpy_d2h(&det, ddet, sizeof det, image.stream());
        if (rc == ZG_OK && det.grids_written) rc = zg_memcpy_d2h(grids.data(), dgrids, (size_t)det.grids_written * sizeof(zg_qr_grid), image.stream());
        if (rc == ZG_OK && det.modules_written) rc = zg_memcpy_d2h(modules.data(), dmodules, det.modules_written, image.stream());
        (void)zg_free(mem);
        check(rc);
        append(out, grids, modules, det.grids_written, binarize);
        return det;
    }
    // The adaptive pass's grids followed by the Otsu pass's (detector.zig:71-82), each tagged with its pass: the reference runs the second
    // pass only when nothing of the first decoded, so a decoder walking this list in order reproduces it.
    template <typename Img> std::vector<QrGrid> detect(const Img &image) const {
        std::vector<QrGrid> out;
        detectPass(image, ZG_QR_ADAPTIVE, out);
        detectPass(image, ZG_QR_OTSU, out);
        return out;
    }
    // asynchronous device form (zg_qr_detect): detection, grids and modules are device memory
    template <typename T>
    void detectInto(const DeviceImage<T> &image, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                    uint32_t module_capacity) const {
        check(detectIntoStatus(image, binarize, detection, grids, grid_capacity, modules, module_capacity));
    }

  private:
    template <typename T>
    int detectIntoStatus(const DeviceImage<T> &image, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                         uint32_t module_capacity) const {
        const zg_image s = image.desc();
        return zg_qr_detect(&s, binarize, detection, grids, grid_capacity, modules, module_capacity, image.stream());
    }
    static void append(std::vector<QrGrid> &out, const std::vector<zg_qr_grid> &grids, const std::vector<uint8_t> &modules, uint32_t written, int binarize) {
        for (uint32_t i = 0; i < written; ++i) {
            const zg_qr_grid &g = grids[i];
            QrGrid q;
            q.binarize = binarize;
            q.version = g.version;
            q.dim = g.dim;
            q.fourth_index = g.fourth_index;
            q.version_hint = g.version_hint;
            std::memcpy(q.corners, g.corners, sizeof q.corners);
            std::memcpy(q.transform, g.transform, sizeof q.transform);
            q.modules.assign(modules.begin() + g.modules_offset, modules.begin() + g.modules_offset + (size_t)g.dim * g.dim);
            out.push_back(q);
        }
    }
};
static_assert(sizeof(zg_qr_detection) == 1176 && sizeof(zg_qr_grid) == 128, "the detector's two records");

} // namespace zignal
