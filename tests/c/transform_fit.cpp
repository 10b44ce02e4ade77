// A stand-alone driver of zignal_amd/csrc/zg_transform_fit.h on the CPU: built with plain g++ (the two HIP qualifiers defined away,
// -ffp-contract=off, -fsanitize=address,undefined) by tests/test_transform_fit_host.py, which writes the cases and compares the bits printed
// here with tests/transform_ref.py's. Every scalar travels as the hexadecimal of its bit pattern (16 digits for f64, 8 for f32). One case a
// line on stdin:
//   F kind scalar n from[2n] to[2n]   -> "R kind status n_points svd_converged m64[9] m32[9]"
//   I scalar m[9]                      -> the same for ProjectiveTransform.inv of that matrix
//   P kind scalar m[9] x y             -> "P x y": project
#include "../../zignal_amd/csrc/zg_transform_fit.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

template <typename T> static bool read_scalars(T *out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint64_t u;
        if (std::scanf("%" SCNx64, &u) != 1) return false;
        if (sizeof(T) == 4) {
            const uint32_t w = (uint32_t)u;
            std::memcpy(out + i, &w, 4);
        } else {
            std::memcpy(out + i, &u, 8);
        }
    }
    return true;
}
static void print_record(const zg_tf::Record &r) {
    std::printf("R %d %d %u %u", r.kind, r.status, r.n_points, r.svd_converged);
    for (int i = 0; i < 9; ++i) {
        uint64_t u;
        std::memcpy(&u, r.m64 + i, 8);
        std::printf(" %016" PRIx64, u);
    }
    for (int i = 0; i < 9; ++i) {
        uint32_t u;
        std::memcpy(&u, r.m32 + i, 4);
        std::printf(" %08" PRIx32, u);
    }
    std::printf("\n");
}

template <typename T> static bool fit_case(int kind, size_t n) {
    std::vector<T> from(2 * n), to(2 * n), big(3 * n + 3);
    if (!read_scalars(from.data(), 2 * n) || !read_scalars(to.data(), 2 * n)) return false;
    zg_tf::Record r;
    if ((int)n < zg_tf::min_points(kind) || (int)n > zg_tf::max_points(kind)) {
        zg_tf::failed_record(kind, zg_tf::FIT_BAD_COUNT, (uint32_t)n, &r);
    } else {
        zg_tf::Serial x;
        zg_tf::Work<T> w;
        zg_tf::find(x, kind, (const T *)from.data(), (const T *)to.data(), (int)n, big.data(), &w);
        zg_tf::to_record(kind, w.status, (uint32_t)n, w.converged, w.m, &r);
    }
    print_record(r);
    return true;
}

template <typename T> static bool matrix_record(int kind, zg_tf::Record *r) {
    T m[9];
    if (!read_scalars(m, 9)) return false;
    zg_tf::to_record(kind, zg_tf::FIT_OK, 0u, 0, m, r);
    return true;
}

template <typename T> static bool project_case(const zg_tf::Record &r) {
    T p[2], o[2];
    if (!read_scalars(p, 2)) return false;
    zg_tf::project_record(&r, p[0], p[1], o[0], o[1]);
    std::printf("P");
    for (int i = 0; i < 2; ++i) {
        if (sizeof(T) == 4) {
            uint32_t u;
            std::memcpy(&u, o + i, 4);
            std::printf(" %08" PRIx32, u);
        } else {
            uint64_t u;
            std::memcpy(&u, o + i, 8);
            std::printf(" %016" PRIx64, u);
        }
    }
    std::printf("\n");
    return true;
}

int main() {
    char what[4];
    unsigned long cases = 0;
    while (std::scanf("%3s", what) == 1) {
        int kind = zg_tf::KIND_PROJECTIVE, scalar;
        zg_tf::Record r, o;
        if (what[0] == 'F') {
            unsigned long n;
            if (std::scanf("%d %d %lu", &kind, &scalar, &n) != 3 || kind < 0 || kind > 2 || n > 100000) return 2;
            if (!(scalar == 0 ? fit_case<float>(kind, n) : fit_case<double>(kind, n))) return 2;
        } else if (what[0] == 'I') {
            if (std::scanf("%d", &scalar) != 1) return 2;
            if (!(scalar == 0 ? matrix_record<float>(kind, &r) : matrix_record<double>(kind, &r))) return 2;
            if (scalar == 0) zg_tf::invert_record<float>(&r, &o);
            else zg_tf::invert_record<double>(&r, &o);
            print_record(o);
        } else if (what[0] == 'P') {
            if (std::scanf("%d %d", &kind, &scalar) != 2 || kind < 0 || kind > 2) return 2;
            if (!(scalar == 0 ? matrix_record<float>(kind, &r) : matrix_record<double>(kind, &r))) return 2;
            if (!(scalar == 0 ? project_case<float>(r) : project_case<double>(r))) return 2;
        } else {
            return 3;
        }
        ++cases;
    }
    std::printf("transform fit ok %lu\n", cases);
    return 0;
}
