// transform_fit.hip — SimilarityTransform.find, AffineTransform.find and ProjectiveTransform.find (reference src/geometry/transforms.zig) on
// the device (include/zignal_hip_transform.h). A fit is one workgroup: a latency problem, not a bandwidth one. The arithmetic is
// zg_transform_fit.h's, the header the host forms compile too, walked by all 256 lanes with the same values; the workgroup's executor
// (Coop, below) is where the lanes divide the work:
//   gather   a lane per match reads the match and its two keypoints and writes from / to in the fit's scalar type
//   rows     operations independent from one row to the next (the SVD's column updates and Givens updates, pinv's rows): dealt to lanes
//   chains   the ordered sums (means, sigma and covariance, the 45 distinct entries of accum, the SVD's dot products over rows, q.dot(pinv)):
//            all lanes compute CHUNK points' terms into LDS, then one lane per sum adds them in index order
//   solo     what is one dependent chain anyway (the 2 x 2 SVD, the 8 x 8 solve, every scalar store): lane 0 between two barriers. The 9 x 9 SVD
//            goes through the executor like the N x 3 one: measured faster than on one lane (profiles/transform_bench.txt)
// Every work array lives in LDS; affine's N x 3 U too (96 KB for f64 at N = 4096).
#include "zg_common.h"
#include "zg_transform_fit.h"

#include "../../include/zignal_hip_transform.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 128;        // points a stage of an ordered sum takes (zg_transform_chunk)
constexpr int STRIDE = CHUNK + 1; // of one sum's terms in the stage: the adding lanes read different banks

static_assert(sizeof(zg_transform_fit) == 128 && sizeof(zg_tf::Record) == 128, "the record of zignal_hip_transform.h");
static_assert(offsetof(zg_transform_fit, m64) == offsetof(zg_tf::Record, m64) && offsetof(zg_transform_fit, m32) == offsetof(zg_tf::Record, m32) &&
                  offsetof(zg_transform_fit, status) == offsetof(zg_tf::Record, status) && offsetof(zg_transform_fit, svd_converged) == offsetof(zg_tf::Record, svd_converged),
              "zg_tf::Record is zg_transform_fit field for field");
static_assert(ZG_FIT_OK == zg_tf::FIT_OK && ZG_FIT_NOT_CONVERGED == zg_tf::FIT_NOT_CONVERGED && ZG_FIT_RANK_DEFICIENT == zg_tf::FIT_RANK_DEFICIENT &&
                  ZG_FIT_BAD_COUNT == zg_tf::FIT_BAD_COUNT && ZG_FIT_BAD_INPUT == zg_tf::FIT_BAD_INPUT, "the status values");
static_assert(ZG_TRANSFORM_SIMILARITY == zg_tf::KIND_SIMILARITY && ZG_TRANSFORM_AFFINE == zg_tf::KIND_AFFINE && ZG_TRANSFORM_PROJECTIVE == zg_tf::KIND_PROJECTIVE, "the kinds");
static_assert(ZG_FIT_MAX_POINTS == zg_tf::MAX_POINTS && ZG_FIT_MAX_POINTS_AFFINE == zg_tf::MAX_POINTS_AFFINE, "the bounds");

// sums a kind runs at once: similarity 5, affine 6, projective 45
constexpr int max_chains(int kind) { return kind == ZG_TRANSFORM_PROJECTIVE ? (int)zg_tf::MAX_CHAINS : 6; }

// zg_transform_fit.h's executor for one workgroup of THREADS lanes. Every method is called by all lanes, with the same arguments; every
// method ends in a barrier, and begins with one where it writes what lanes may still be reading.
template <typename T> struct Coop {
    T *stage;  // max_chains * STRIDE
    int *word; // first()'s
    bool unstaged; // tuning hook: a single sum is multiplied and added by lane 0 alone, no stage

    template <typename F> __device__ inline void rows(int r0, int r1, F f) {
        __syncthreads();
        for (int k = r0 + (int)threadIdx.x; k < r1; k += THREADS) f(k);
        __syncthreads();
    }
    template <int K, typename U, typename F> __device__ inline void chains(int r0, int r1, F term, U *out) {
        const int tid = (int)threadIdx.x;
        U s = (U)0;
        __syncthreads();
        if (K == 1 && unstaged) {
            if (tid == 0) {
                for (int k = r0; k < r1; ++k) s += term(k, 0);
                out[0] = s;
            }
            __syncthreads();
            return;
        }
        for (int base = r0; base < r1; base += CHUNK) {
            const int cnt = min(CHUNK, r1 - base);
            if (base != r0) __syncthreads(); // the adding lanes are done with the stage
            for (int idx = tid; idx < K * cnt; idx += THREADS) {
                const int c = idx / cnt, j = idx - c * cnt;
                stage[c * STRIDE + j] = term(base + j, c);
            }
            __syncthreads();
            if (tid < K) {
                const T *mine = stage + tid * STRIDE;
                for (int j = 0; j < cnt; ++j) s += mine[j];
            }
        }
        if (tid < K) out[tid] = s;
        __syncthreads();
    }
    template <typename P> __device__ inline int first(int r0, int r1, P pred) {
        __syncthreads();
        if (threadIdx.x == 0) *word = r1;
        __syncthreads();
        for (int k = r0 + (int)threadIdx.x; k < r1; k += THREADS) {
            if (pred(k)) {
                atomicMin(word, k);
                break;
            }
        }
        __syncthreads();
        return *word;
    }
    template <typename F> __device__ inline void solo(F f) {
        __syncthreads();
        if (threadIdx.x == 0) f();
        __syncthreads();
    }
};

struct FitArgs {
    const void *from, *to; // points of the fit's scalar type, or null with matches
    const zg_keypoint *query_kps, *train_kps;
    const zg_match *matches;
    uint32_t n_query, n_train, capacity;
    int32_t train_to_query;
    const uint32_t *count;
    void *gathered; // with matches: room for min(capacity, the kind's bound) from points, then as many to points
    uint32_t gathered_points;
    int32_t variant; // ZIGNAL_HIP_FIT_VARIANT: bit 0 the 9 x 9 SVD on one lane, bit 1 single sums unstaged
    zg_transform_fit *out;
};

template <typename T, int KIND> __global__ __launch_bounds__(THREADS) void k_fit(FitArgs a) {
    __shared__ zg_tf::Work<T> work;
    __shared__ T stage[max_chains(KIND) * STRIDE];
    __shared__ T big[KIND == ZG_TRANSFORM_AFFINE ? 3 * (int)zg_tf::MAX_POINTS_AFFINE : 1];
    __shared__ int word;
    const int tid = (int)threadIdx.x;
    zg_tf::Record *out = (zg_tf::Record *)a.out;
    const uint32_t n = a.count ? min(*a.count, a.capacity) : a.capacity;
    if (n < (uint32_t)zg_tf::min_points(KIND) || n > (uint32_t)zg_tf::max_points(KIND)) { // uniform
        if (tid == 0) zg_tf::failed_record(KIND, zg_tf::FIT_BAD_COUNT, n, out);
        return;
    }
    const T *from = (const T *)a.from, *to = (const T *)a.to;
    if (a.matches) { // n <= gathered_points: the host sized the room to min(capacity, the bound)
        T *gf = (T *)a.gathered, *gt = gf + 2 * (size_t)a.gathered_points;
        if (tid == 0) word = 0;
        __syncthreads();
        for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) {
            const zg_match m = a.matches[i];
            if (m.query_idx >= a.n_query || m.train_idx >= a.n_train) {
                word = 1; // every lane that writes, writes 1
                continue;
            }
            const zg_keypoint *kq = a.query_kps + m.query_idx, *kt = a.train_kps + m.train_idx;
            const zg_keypoint *kf = a.train_to_query ? kt : kq, *ko = a.train_to_query ? kq : kt;
            gf[2 * i] = (T)kf->x;
            gf[2 * i + 1] = (T)kf->y;
            gt[2 * i] = (T)ko->x;
            gt[2 * i + 1] = (T)ko->y;
        }
        __syncthreads();
        if (word != 0) { // uniform
            if (tid == 0) zg_tf::failed_record(KIND, zg_tf::FIT_BAD_INPUT, n, out);
            return;
        }
        from = gf;
        to = gt;
    }
    Coop<T> x{stage, &word, (a.variant & 2) != 0};
    if constexpr (KIND == ZG_TRANSFORM_SIMILARITY) zg_tf::find_similarity<T>(x, from, to, (int)n, &work);
    else if constexpr (KIND == ZG_TRANSFORM_AFFINE) zg_tf::find_affine<T>(x, from, to, (int)n, big, &work);
    else zg_tf::find_projective<T>(x, from, to, (int)n, &work, (a.variant & 1) == 0);
    if (tid == 0) zg_tf::to_record(KIND, work.status, n, work.converged, work.m, out); // work.m is the identity unless the status is OK
}

template <typename T> __global__ __launch_bounds__(THREADS) void k_project(const zg_transform_fit *fit, const T *in, T *out, uint32_t n) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    T ox, oy;
    zg_tf::project_record<T>((const zg_tf::Record *)fit, in[2 * (size_t)i], in[2 * (size_t)i + 1], ox, oy);
    out[2 * (size_t)i] = ox;
    out[2 * (size_t)i + 1] = oy;
}

template <typename T> __global__ __launch_bounds__(64) void k_invert(const zg_transform_fit *fit, zg_transform_fit *out) {
    if (threadIdx.x != 0) return;
    zg_tf::Record r; // in == out is fine: read first
    zg_tf::invert_record<T>((const zg_tf::Record *)fit, &r);
    *(zg_tf::Record *)out = r;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------

int check_kind_scalar(int kind, int scalar, const char *who) {
    ZG_REQUIRE(kind >= ZG_TRANSFORM_SIMILARITY && kind <= ZG_TRANSFORM_PROJECTIVE, ZG_ERR_INVALID_ARGUMENT, "%s: invalid transform kind %d", who, kind);
    ZG_REQUIRE(scalar == ZG_SCALAR_F32 || scalar == ZG_SCALAR_F64, ZG_ERR_INVALID_ARGUMENT, "%s: invalid scalar type %d", who, scalar);
    return ZG_OK;
}
int check_points(const void *from, const void *to, uint32_t capacity, const void *out, const char *who) {
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null record", who);
    ZG_REQUIRE(capacity == 0 || (from != nullptr && to != nullptr), ZG_ERR_INVALID_ARGUMENT, "%s: null points", who);
    return ZG_OK;
}
int check_matches(const zg_keypoint *q, uint32_t nq, const zg_keypoint *t, uint32_t nt, const zg_match *m, uint32_t capacity, const void *out, const char *who) {
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null record", who);
    ZG_REQUIRE(capacity == 0 || m != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null matches", who);
    ZG_REQUIRE((nq == 0 || q != nullptr) && (nt == 0 || t != nullptr), ZG_ERR_INVALID_ARGUMENT, "%s: null keypoints", who);
    return ZG_OK;
}

template <typename T> int launch_fit_t(int kind, const FitArgs &a, hipStream_t s) {
    switch (kind) {
    case ZG_TRANSFORM_SIMILARITY: hipLaunchKernelGGL((k_fit<T, ZG_TRANSFORM_SIMILARITY>), dim3(1), dim3(THREADS), 0, s, a); break;
    case ZG_TRANSFORM_AFFINE: hipLaunchKernelGGL((k_fit<T, ZG_TRANSFORM_AFFINE>), dim3(1), dim3(THREADS), 0, s, a); break;
    default: hipLaunchKernelGGL((k_fit<T, ZG_TRANSFORM_PROJECTIVE>), dim3(1), dim3(THREADS), 0, s, a); break;
    }
    return launch_ok("k_fit");
}

// Tuning hook, read once per process: ZIGNAL_HIP_FIT_VARIANT=1 runs projective's 9 x 9 SVD on one lane instead of through the
// workgroup's executor (3-10 % slower: 128.8 against 116.4 us at 500 points in f32), =2 lets lane 0 multiply and add the SVD's dot products itself instead of
// staging the products (affine 15-20 % slower), =3 both. The results are the same bits; profiles/transform_bench.txt has the times.
int fit_variant() {
    static const int v = [] {
        const char *e = std::getenv("ZIGNAL_HIP_FIT_VARIANT");
        return e ? std::atoi(e) & 3 : 0;
    }();
    return v;
}

int launch_fit(int kind, int scalar, FitArgs a, hipStream_t s) {
    a.variant = fit_variant();
    ScratchBlock sc(s);
    if (a.matches) {
        a.gathered_points = std::min(a.capacity, (uint32_t)zg_tf::max_points(kind));
        if (const int rc = sc.alloc(align256((size_t)a.gathered_points * 4 * (scalar == ZG_SCALAR_F32 ? 4 : 8)))) return rc;
        a.gathered = sc.p;
    }
    return scalar == ZG_SCALAR_F32 ? launch_fit_t<float>(kind, a, s) : launch_fit_t<double>(kind, a, s);
}

// the header with the Serial executor on n points that are in bounds
template <typename T> void fit_serial(int kind, const T *from, const T *to, uint32_t n, zg_tf::Record *out) {
    std::vector<T> big(kind == ZG_TRANSFORM_AFFINE ? 3 * (size_t)n : 1);
    zg_tf::Work<T> work;
    zg_tf::Serial x;
    zg_tf::find<T>(x, kind, from, to, (int)n, big.data(), &work);
    zg_tf::to_record(kind, work.status, n, work.converged, work.m, out);
}
bool count_ok(int kind, uint32_t n, zg_tf::Record *out) {
    if (n >= (uint32_t)zg_tf::min_points(kind) && n <= (uint32_t)zg_tf::max_points(kind)) return true;
    zg_tf::failed_record(kind, zg_tf::FIT_BAD_COUNT, n, out);
    return false;
}

template <typename T> void fit_matches_serial(int kind, const zg_keypoint *q, uint32_t nq, const zg_keypoint *t, uint32_t nt, const zg_match *m, uint32_t n, int train_to_query,
                                              zg_tf::Record *out) {
    std::vector<T> from(2 * (size_t)n), to(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        if (m[i].query_idx >= nq || m[i].train_idx >= nt) {
            zg_tf::failed_record(kind, zg_tf::FIT_BAD_INPUT, n, out);
            return;
        }
        const zg_keypoint *kq = q + m[i].query_idx, *kt = t + m[i].train_idx;
        const zg_keypoint *kf = train_to_query ? kt : kq, *ko = train_to_query ? kq : kt;
        from[2 * (size_t)i] = (T)kf->x;
        from[2 * (size_t)i + 1] = (T)kf->y;
        to[2 * (size_t)i] = (T)ko->x;
        to[2 * (size_t)i + 1] = (T)ko->y;
    }
    fit_serial<T>(kind, from.data(), to.data(), n, out);
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

size_t zg_transform_sizeof_fit(void) { return sizeof(zg_transform_fit); }
uint32_t zg_transform_chunk(void) { return CHUNK; }

int zg_transform_fit_points(int kind, int scalar, const void *from, const void *to, uint32_t capacity, const uint32_t *count, zg_transform_fit *out,
                            zg_stream stream) {
    int rc;
    if ((rc = check_kind_scalar(kind, scalar, "transform_fit_points")) || (rc = check_points(from, to, capacity, out, "transform_fit_points"))) return rc;
    FitArgs a{};
    a.from = from;
    a.to = to;
    a.capacity = capacity;
    a.count = count;
    a.out = out;
    return launch_fit(kind, scalar, a, as_stream(stream));
}

int zg_transform_fit_matches(int kind, int scalar, const zg_keypoint *query_kps, uint32_t n_query, const zg_keypoint *train_kps, uint32_t n_train,
                             const zg_match *matches, uint32_t capacity, const uint32_t *count, int train_to_query, zg_transform_fit *out, zg_stream stream) {
    int rc;
    if ((rc = check_kind_scalar(kind, scalar, "transform_fit_matches")) ||
        (rc = check_matches(query_kps, n_query, train_kps, n_train, matches, capacity, out, "transform_fit_matches")))
        return rc;
    FitArgs a{};
    a.query_kps = query_kps;
    a.train_kps = train_kps;
    a.matches = matches;
    a.n_query = n_query;
    a.n_train = n_train;
    a.capacity = matches ? capacity : 0; // no list: no points, and the record says ZG_FIT_BAD_COUNT
    a.train_to_query = train_to_query ? 1 : 0;
    a.count = count;
    a.out = out;
    return launch_fit(kind, scalar, a, as_stream(stream));
}

int zg_transform_fit_points_host(int kind, int scalar, const void *from, const void *to, uint32_t capacity, const uint32_t *count, zg_transform_fit *out) {
    int rc;
    if ((rc = check_kind_scalar(kind, scalar, "transform_fit_points_host")) || (rc = check_points(from, to, capacity, out, "transform_fit_points_host"))) return rc;
    const uint32_t n = count ? std::min(*count, capacity) : capacity;
    zg_tf::Record *r = (zg_tf::Record *)out;
    if (!count_ok(kind, n, r)) return ZG_OK;
    if (scalar == ZG_SCALAR_F32) fit_serial<float>(kind, (const float *)from, (const float *)to, n, r);
    else fit_serial<double>(kind, (const double *)from, (const double *)to, n, r);
    return ZG_OK;
}

int zg_transform_fit_matches_host(int kind, int scalar, const zg_keypoint *query_kps, uint32_t n_query, const zg_keypoint *train_kps, uint32_t n_train,
                                  const zg_match *matches, uint32_t capacity, const uint32_t *count, int train_to_query, zg_transform_fit *out) {
    int rc;
    if ((rc = check_kind_scalar(kind, scalar, "transform_fit_matches_host")) ||
        (rc = check_matches(query_kps, n_query, train_kps, n_train, matches, capacity, out, "transform_fit_matches_host")))
        return rc;
    if (!matches) capacity = 0;
    const uint32_t n = count ? std::min(*count, capacity) : capacity;
    zg_tf::Record *r = (zg_tf::Record *)out;
    if (!count_ok(kind, n, r)) return ZG_OK;
    if (scalar == ZG_SCALAR_F32) fit_matches_serial<float>(kind, query_kps, n_query, train_kps, n_train, matches, n, train_to_query, r);
    else fit_matches_serial<double>(kind, query_kps, n_query, train_kps, n_train, matches, n, train_to_query, r);
    return ZG_OK;
}

int zg_transform_project_points(const zg_transform_fit *fit, int scalar, const void *in, void *out, uint32_t n, zg_stream stream) {
    ZG_REQUIRE(fit != nullptr, ZG_ERR_INVALID_ARGUMENT, "transform_project_points: null record");
    ZG_REQUIRE(scalar == ZG_SCALAR_F32 || scalar == ZG_SCALAR_F64, ZG_ERR_INVALID_ARGUMENT, "transform_project_points: invalid scalar type %d", scalar);
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(in != nullptr && out != nullptr, ZG_ERR_INVALID_ARGUMENT, "transform_project_points: null points");
    const dim3 grid(ceil_div(n, (unsigned)THREADS));
    if (scalar == ZG_SCALAR_F32) hipLaunchKernelGGL((k_project<float>), grid, dim3(THREADS), 0, as_stream(stream), fit, (const float *)in, (float *)out, n);
    else hipLaunchKernelGGL((k_project<double>), grid, dim3(THREADS), 0, as_stream(stream), fit, (const double *)in, (double *)out, n);
    return launch_ok("k_project");
}

int zg_transform_project_points_host(const zg_transform_fit *fit, int scalar, const void *in, void *out, uint32_t n) {
    ZG_REQUIRE(fit != nullptr, ZG_ERR_INVALID_ARGUMENT, "transform_project_points_host: null record");
    ZG_REQUIRE(scalar == ZG_SCALAR_F32 || scalar == ZG_SCALAR_F64, ZG_ERR_INVALID_ARGUMENT, "transform_project_points_host: invalid scalar type %d", scalar);
    ZG_REQUIRE(n == 0 || (in != nullptr && out != nullptr), ZG_ERR_INVALID_ARGUMENT, "transform_project_points_host: null points");
    const zg_tf::Record *r = (const zg_tf::Record *)fit;
    for (size_t i = 0; i < n; ++i) {
        if (scalar == ZG_SCALAR_F32) {
            const float *p = (const float *)in + 2 * i;
            float ox, oy;
            zg_tf::project_record<float>(r, p[0], p[1], ox, oy);
            ((float *)out)[2 * i] = ox;
            ((float *)out)[2 * i + 1] = oy;
        } else {
            const double *p = (const double *)in + 2 * i;
            double ox, oy;
            zg_tf::project_record<double>(r, p[0], p[1], ox, oy);
            ((double *)out)[2 * i] = ox;
            ((double *)out)[2 * i + 1] = oy;
        }
    }
    return ZG_OK;
}

int zg_transform_invert(const zg_transform_fit *fit, int scalar, zg_transform_fit *out, zg_stream stream) {
    ZG_REQUIRE(fit != nullptr && out != nullptr, ZG_ERR_INVALID_ARGUMENT, "transform_invert: null record");
    ZG_REQUIRE(scalar == ZG_SCALAR_F32 || scalar == ZG_SCALAR_F64, ZG_ERR_INVALID_ARGUMENT, "transform_invert: invalid scalar type %d", scalar);
    if (scalar == ZG_SCALAR_F32) hipLaunchKernelGGL((k_invert<float>), dim3(1), dim3(64), 0, as_stream(stream), fit, out);
    else hipLaunchKernelGGL((k_invert<double>), dim3(1), dim3(64), 0, as_stream(stream), fit, out);
    return launch_ok("k_invert");
}

int zg_transform_invert_host(const zg_transform_fit *fit, int scalar, zg_transform_fit *out) {
    ZG_REQUIRE(fit != nullptr && out != nullptr, ZG_ERR_INVALID_ARGUMENT, "transform_invert_host: null record");
    ZG_REQUIRE(scalar == ZG_SCALAR_F32 || scalar == ZG_SCALAR_F64, ZG_ERR_INVALID_ARGUMENT, "transform_invert_host: invalid scalar type %d", scalar);
    zg_tf::Record r;
    if (scalar == ZG_SCALAR_F32) zg_tf::invert_record<float>((const zg_tf::Record *)fit, &r);
    else zg_tf::invert_record<double>((const zg_tf::Record *)fit, &r);
    std::memcpy(out, &r, sizeof r);
    return ZG_OK;
}

} // extern "C"
