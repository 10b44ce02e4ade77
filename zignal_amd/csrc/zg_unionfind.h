// zg_unionfind.h — the lock-free union-find that edges.hip's hysteresis and flood.hip's fill label connected components with, in LDS
// (a tile) and in global memory (across tiles). label[x] is x's parent, a root is its own parent, and a union hangs the larger root
// under the smaller one with atomicMin: parents only ever move to smaller indices, so the structure stays a forest whatever the
// interleaving, and a stale read still names an ancestor.
#pragma once
#include "zg_common.h"

namespace zg {

__device__ inline int cc_find(int *label, int x) {
    int p = label[x];
    while (p != x) { // path halving (plain stores: another lane can only have written a smaller ancestor)
        const int gp = label[p];
        if (gp != p) label[x] = gp;
        x = p;
        p = gp;
    }
    return x;
}
template <bool PAIRED>
__device__ inline void cc_unite_t(int *label, int a, int b) {
    for (;;) {
        if constexpr (PAIRED) { // cc_find of both at once: through global memory the two walks are independent chains of loads, and a union's
                                // time is their latency (k_cc_border 91 -> 74 us on noise; in LDS the extra instructions cost more than they hide)
            int pa = label[a], pb = label[b];
            while (pa != a || pb != b) {
                const int ga = label[pa], gb = label[pb];
                if (pa != a) { if (ga != pa) label[a] = ga; a = pa; pa = ga; }
                if (pb != b) { if (gb != pb) label[b] = gb; b = pb; pb = gb; }
            }
        } else {
            a = cc_find(label, a);
            b = cc_find(label, b);
        }
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; } // a > b: hang a under b
        const int old = atomicMin(&label[a], b);
        if (old == a) return; // a was still a root: linked
        a = old;              // someone re-rooted a in the meantime: retry from its new parent
    }
}
__device__ inline void cc_unite(int *label, int a, int b) { cc_unite_t<false>(label, a, b); }        // LDS
__device__ inline void cc_unite_global(int *label, int a, int b) { cc_unite_t<true>(label, a, b); }

} // namespace zg
