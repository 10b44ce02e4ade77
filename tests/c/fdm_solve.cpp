// A stand-alone driver of zignal_amd/csrc/zg_fdm_solve.h on the CPU: built with plain g++ (the two HIP qualifiers defined away,
// -ffp-contract=off, -fsanitize=address,undefined) by tests/test_fdm_solve_host.py, which writes the cases and compares the bits printed
// here with tests/fdm_ref.py's. Every f64 travels as the hexadecimal of its bit pattern. One case a line on stdin:
//   P pixel is_gray tmean[3] tcov[9] smean[3] scov[9]   -> "T status u[9] s[3]" and "X route status w[9] bias[3] scale offset"
//   C n sx sy sxy   (decimal)                            -> "C cov"
//   A n sx          (decimal)                            -> "A mean"
#include "../../zignal_amd/csrc/zg_fdm_solve.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

static double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}
static uint64_t to_bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
static bool read_f64(double *out, int n) {
    for (int i = 0; i < n; ++i) {
        uint64_t u;
        if (std::scanf("%" SCNx64, &u) != 1) return false;
        out[i] = from_bits(u);
    }
    return true;
}
static void print_f64(const double *v, int n) {
    for (int i = 0; i < n; ++i) std::printf(" %016" PRIx64, to_bits(v[i]));
}

int main() {
    char kind[4];
    unsigned long cases = 0;
    while (std::scanf("%3s", kind) == 1) {
        if (kind[0] == 'P') {
            int pixel, gray;
            double tmean[3], tcov[9], smean[3], scov[9];
            if (std::scanf("%d %d", &pixel, &gray) != 2 || !read_f64(tmean, 3) || !read_f64(tcov, 9) || !read_f64(smean, 3) || !read_f64(scov, 9)) return 2;
            zg_fdm::Target t;
            zg_fdm::Transform x;
            zg_fdm::Scratch k;
            zg_fdm::target_from_stats(tmean, tcov, gray, &t, &k);
            zg_fdm::transform_from_stats(pixel, &t, smean, scov, &x, &k);
            std::printf("T %d", t.status);
            print_f64(t.u, 9);
            print_f64(t.s, 3);
            std::printf("\nX %d %d", x.route, x.status);
            print_f64(x.w, 9);
            print_f64(x.bias, 3);
            print_f64(&x.scale, 1);
            print_f64(&x.offset, 1);
            std::printf("\n");
        } else if (kind[0] == 'C') {
            uint64_t n, sx, sy, sxy;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &n, &sx, &sy, &sxy) != 4) return 2;
            const double c = zg_fdm::cov_from_moments(n, sx, sy, sxy);
            std::printf("C");
            print_f64(&c, 1);
            std::printf("\n");
        } else if (kind[0] == 'A') {
            uint64_t n, sx;
            if (std::scanf("%" SCNu64 " %" SCNu64, &n, &sx) != 2) return 2;
            const double m = zg_fdm::mean_from_moments(n, sx);
            std::printf("A");
            print_f64(&m, 1);
            std::printf("\n");
        } else {
            return 3;
        }
        ++cases;
    }
    std::printf("fdm solve ok %lu\n", cases);
    return 0;
}
