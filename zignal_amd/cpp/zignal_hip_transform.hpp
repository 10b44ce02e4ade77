// zignal_hip_transform.hpp — the C++ mirror of the geometry-fitting module (include/zignal_hip_transform.h): SimilarityTransform.find,
// AffineTransform.find and ProjectiveTransform.find of the reference (src/geometry/transforms.zig:47-112, :155-191, :242-290).
//   fit<T>(kind, from, to)        find on host points (FitPoint<T> is two T): host arithmetic, the reference's bit for bit except affine on 86 or
//                                 more points (the header says why). Returns a Fit; FitFailed where the reference returns an error.
//   DeviceFit                     a zg_transform_fit in device memory: fitPoints / fitMatches enqueue a fit on a stream, warp resamples a
//                                 DeviceImage with the matrix read from the record (nothing copied or synchronised), project and invert work on
//                                 the record too, download reads it back.
// Include after, or instead of, zignal_hip.hpp.
#pragma once
#include "zignal_hip.hpp"

namespace zignal {

enum class TransformKind : int { similarity = ZG_TRANSFORM_SIMILARITY, affine = ZG_TRANSFORM_AFFINE, projective = ZG_TRANSFORM_PROJECTIVE };
template <typename T> struct FitPoint { T x, y; };

struct FitFailed : std::runtime_error { // error.NotConverged, error.RankDeficient, or a count or an index out of bounds
    int status;
    explicit FitFailed(int s)
        : std::runtime_error(s == ZG_FIT_NOT_CONVERGED ? "NotConverged" : s == ZG_FIT_RANK_DEFICIENT ? "RankDeficient" : s == ZG_FIT_BAD_COUNT ? "BadCount" : "BadInput"),
          status(s) {}
};

namespace detail {
template <typename T> constexpr int scalar_of() {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "a fit runs in float or double");
    return std::is_same<T, float>::value ? ZG_SCALAR_F32 : ZG_SCALAR_F64;
}
} // namespace detail

// The outcome of find: the record, and the reference's fields read out of it.
struct Fit {
    zg_transform_fit record{};
    TransformKind kind() const { return (TransformKind)record.kind; }
    bool ok() const { return record.status == ZG_FIT_OK; }
    // matrix (row, col) and bias (row) of a similarity or affine transform, or matrix (row, col) of a projective one, in T
    template <typename T> T matrix(int r, int c) const {
        const int i = record.kind == ZG_TRANSFORM_PROJECTIVE ? r * 3 + c : r * 2 + c;
        return std::is_same<T, float>::value ? (T)record.m32[i] : (T)record.m64[i];
    }
    template <typename T> T bias(int r) const { return std::is_same<T, float>::value ? (T)record.m32[4 + r] : (T)record.m64[4 + r]; }
    template <typename T> FitPoint<T> project(FitPoint<T> p) const {                           // transforms.zig:39-42, :147-150, :224-231
        FitPoint<T> o;
        check(zg_transform_project_points_host(&record, detail::scalar_of<T>(), &p, &o, 1));
        return o;
    }
    template <typename T> Fit inv() const {                                              // ProjectiveTransform.inv; FitFailed for the reference's null
        Fit o;
        check(zg_transform_invert_host(&record, detail::scalar_of<T>(), &o.record));
        if (!o.ok()) throw FitFailed(o.record.status);
        return o;
    }
    // Image.warp with this transform, on host or device images (the f32 coefficients, as zg_warp takes them)
    template <class Img> void warp(const Img &src, const Img &out, Interpolation method) const {
        const zg_image s = src.desc(), d = out.desc();
        const zg_method m = method.c_method();
        if constexpr (Img::on_device) check(zg_warp(&s, &d, record.kind, record.m32, &m, src.stream()));
        else check(zg_warp_host(&s, &d, record.kind, record.m32, &m));
    }
};

// SimilarityTransform(T).init / AffineTransform(T).init / ProjectiveTransform(T).init
template <typename T> Fit fit(TransformKind kind, const std::vector<FitPoint<T>> &from, const std::vector<FitPoint<T>> &to) {
    if (from.size() != to.size()) throw std::invalid_argument("from and to have one length");
    Fit f;
    check(zg_transform_fit_points_host((int)kind, detail::scalar_of<T>(), from.data(), to.data(), (uint32_t)from.size(), nullptr, &f.record));
    if (!f.ok()) throw FitFailed(f.record.status);
    return f;
}

// A record in device memory. Move-only; every method but download enqueues on the given stream and returns.
class DeviceFit {
  public:
    DeviceFit() { check(zg_malloc((void **)&rec_, sizeof(zg_transform_fit))); }
    DeviceFit(DeviceFit &&o) noexcept : rec_(o.rec_) { o.rec_ = nullptr; }
    DeviceFit &operator=(DeviceFit &&o) noexcept { if (this != &o) { release(); rec_ = o.rec_; o.rec_ = nullptr; } return *this; }
    DeviceFit(const DeviceFit &) = delete;
    DeviceFit &operator=(const DeviceFit &) = delete;
    ~DeviceFit() { release(); }
    zg_transform_fit *device() const { return rec_; }

    // from, to: capacity points of T in device memory; count: null or a device word
    template <typename T> void fitPoints(TransformKind kind, const FitPoint<T> *from, const FitPoint<T> *to, uint32_t capacity, const uint32_t *count, zg_stream stream) const {
        check(zg_transform_fit_points((int)kind, detail::scalar_of<T>(), from, to, capacity, count, rec_, stream));
    }
    // the lists of Orb.detectAndCompute and BruteForceMatcher.match, all in device memory; train_to_query: the map warp needs to bring the
    // query frame onto the train frame's grid
    template <typename T> void fitMatches(TransformKind kind, const zg_keypoint *query, uint32_t n_query, const zg_keypoint *train, uint32_t n_train, const zg_match *matches,
                                          uint32_t capacity, const uint32_t *count, bool train_to_query, zg_stream stream) const {
        check(zg_transform_fit_matches((int)kind, detail::scalar_of<T>(), query, n_query, train, n_train, matches, capacity, count, train_to_query ? 1 : 0, rec_, stream));
    }
    template <typename T> void project(const FitPoint<T> *in, FitPoint<T> *out, uint32_t n, zg_stream stream) const {
        check(zg_transform_project_points(rec_, detail::scalar_of<T>(), in, out, n, stream));
    }
    template <typename T> void invertInto(const DeviceFit &out, zg_stream stream) const { check(zg_transform_invert(rec_, detail::scalar_of<T>(), out.rec_, stream)); }
    // Image.warp with the record's matrix; a record that is not ZG_FIT_OK leaves `out` untouched
    template <typename P> void warp(const DeviceImage<P> &src, const DeviceImage<P> &out, Interpolation method) const {
        const zg_image s = src.desc(), d = out.desc();
        const zg_method m = method.c_method();
        check(zg_warp_fitted(&s, &d, rec_, &m, src.stream()));
    }
    Fit download(zg_stream stream) const { // waits for the stream
        Fit f;
        check(zg_memcpy_d2h(&f.record, rec_, sizeof(zg_transform_fit), stream));
        return f;
    }

  private:
    void release() { if (rec_) (void)zg_free(rec_); rec_ = nullptr; }
    zg_transform_fit *rec_ = nullptr;
};

} // namespace zignal
