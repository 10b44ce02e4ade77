// zg_tracer_step.h — the two pieces of Tracer (reference src/features/Tracer.zig) that are arithmetic: which neighbour followPath steps
// to (:118-170), and Point.distanceToSegment (src/geometry/Point.zig:177-195) that douglasPeucker ranks points by. Plain
// __host__ __device__ functions of integers and f32 with no other header of this library under them: tracer.hip's kernels run them on
// the device, tests/c/tracer_step.cpp compiles them with g++ (-D__host__= -D__device__= -ffp-contract=off) and runs them on the CPU.
// Every f32 operation is the reference's, in its order, one rounding each: no FMA may be formed from them.
#pragma once
#include <math.h>
#include <stdint.h>

namespace zg {

// Tracer.neighbors (:88-105): neighbour k of a pixel, as (row, col) offsets in the order the reference tests them
//   0 (-1,-1)  1 (-1,0)  2 (-1,1)  3 (0,-1)  4 (0,1)  5 (1,-1)  6 (1,0)  7 (1,1)
__host__ __device__ inline int tracer_drow(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }
__host__ __device__ inline int tracer_dcol(int k) { return k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6)); }

// prev_dir . neighbors[k].dir (:130, :152) for a path whose last step was neighbour prev_k: (p_curr - p_prev).scale(1.0 / norm) dotted
// with (dx / len, dy / len). A point is (x = col, y = row), so component 0 is the column offset.
__host__ __device__ inline float tracer_score(int prev_k, int k) {
    const float px = (float)tracer_dcol(prev_k), py = (float)tracer_drow(prev_k);
    const float n = sqrtf(px * px + py * py); // never 0: a step moves
    const float s = 1.0f / n;
    const float ux = px * s, uy = py * s;
    const float dx = (float)tracer_dcol(k), dy = (float)tracer_drow(k);
    const float len = sqrtf(dx * dx + dy * dy);
    const float vx = dx / len, vy = dy / len;
    return ux * vx + uy * vy;
}

// The neighbour followPath moves to, or -1 when the path ends. prev_k: the neighbour index of the step that reached the current point,
// -1 for a path of one point (no history: the first open neighbour wins, :145-149). open: bit k set iff neighbour k is inside the
// image, an edge, and not visited. With history the strictly largest score wins (best_score starts at -2), the first among equals.
__host__ __device__ inline int tracer_choose(int prev_k, uint32_t open) {
    open &= 0xffu;
    if (open == 0) return -1;
    int best = -1;
    float best_score = -2.0f;
    for (int k = 0; k < 8; ++k) {
        if (!((open >> k) & 1u)) continue;
        if (prev_k < 0) return k;
        const float score = tracer_score(prev_k, k);
        if (score > best_score) {
            best_score = score;
            best = k;
        }
    }
    return best;
}

// Point(2, f32).distanceToSegment (Point.zig:177-195): p to the segment a b, with its three returns and the ab_len_sq == 0 case.
__host__ __device__ inline float tracer_distance_to_segment(float px, float py, float ax, float ay, float bx, float by) {
    const float abx = bx - ax, aby = by - ay;
    const float apx = px - ax, apy = py - ay;
    const float ab_len_sq = abx * abx + aby * aby;
    if (ab_len_sq == 0.0f) return sqrtf(apx * apx + apy * apy);
    const float t = (apx * abx + apy * aby) / ab_len_sq;
    if (t <= 0.0f) return sqrtf(apx * apx + apy * apy);
    if (t >= 1.0f) {
        const float dx = px - bx, dy = py - by;
        return sqrtf(dx * dx + dy * dy);
    }
    const float ex = apx - abx * t, ey = apy - aby * t; // ap.distance(ab.scale(t))
    return sqrtf(ex * ex + ey * ey);
}

} // namespace zg
