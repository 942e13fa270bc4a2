// HoleReacher's geometry and reward pieces as __device__ functions, shared by k_hole_rollout (mpk_hole.hip) and k_reacher_env_step
// (mpk_env_step.hip): one text of the link-crossing test, of the wall test as exact index intervals and of the reward terms that
// depend on numpy's dtypes, so the rollout and the one-launch environment step give the same bits by construction.
#pragma once
#include "mpk_dev.h"

namespace mpk {

constexpr int kHolePoints = 100;     // np.linspace(0, 1, 100) points per link (hole_reacher.py:149)

// np.linspace(0, 1, 100)[j]: j * (1 / 99), the last point exactly 1
__device__ __forceinline__ double hole_t(int j) { return j == kHolePoints - 1 ? 1.0 : (double)j * (1.0 / 99.0); }

// ccw / intersect of envs/classic_control/utils.py:1-9
__device__ __forceinline__ bool hole_ccw(double ax, double ay, double bx, double by, double cx, double cy) {
    return (cy - ay) * (bx - ax) - (by - ay) * (cx - ax) > 1e-12;
}
__device__ __forceinline__ bool hole_intersect(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
    return hole_ccw(ax, ay, cx, cy, dx, dy) != hole_ccw(bx, by, cx, cy, dx, dy) &&
           hole_ccw(ax, ay, bx, by, cx, cy) != hole_ccw(ax, ay, bx, by, dx, dy);
}

// The point coordinates of a link are v_j = fl(fl(a * t_j) + b), monotone in j (t_j increases, rounding is monotone), so
// {j : v_j < h} (LESS) and {j : v_j > h} are a prefix or a suffix of [0, 100).  The crossing index comes from one division; the
// exact predicate at the neighbouring indices then moves it to the true boundary (a step or two; any start would do).
template <bool LESS>
__device__ __forceinline__ void hole_interval(double a, double b, double h, int& lo, int& hi) {
    auto pred = [&](int j) {
        const double v = a * hole_t(j) + b;
        return LESS ? v < h : v > h;
    };
    if (!(a > 0.0) && !(a < 0.0)) {                  // a constant coordinate, or NaN (no comparison holds)
        const bool all = pred(0);
        lo = 0; hi = all ? kHolePoints : 0;
        return;
    }
    const double x = fmin(fmax((h - b) / a * 99.0, 0.0), (double)kHolePoints);   // NaN -> 0
    int g = (int)ceil(x);
    if ((a > 0.0) == LESS) {                        // true, then false: [0, g)
        while (g > 0 && !pred(g - 1)) --g;
        while (g < kHolePoints && pred(g)) ++g;
        lo = 0; hi = g;
    } else {                                        // false, then true: [g, 100)
        while (g > 0 && pred(g - 1)) --g;
        while (g < kHolePoints && !pred(g)) ++g;
        lo = g; hi = kHolePoints;
    }
}

// check_wall_collision (hole_reacher.py:151-179) for the link from (x0, y0) along (c, s): any point left of the hole and below 0,
// right of the hole and below 0, or over the hole and below -depth
template <bool SAMPLED>
__device__ __forceinline__ bool hole_link_hits_wall(double c, double s, double x0, double y0, double hl, double hr, double floor_y) {
    if constexpr (SAMPLED) {
        bool hit = false;
        for (int j = 0; j < kHolePoints; ++j) {
            const double t = hole_t(j);
            const double px = c * t + x0, py = s * t + y0;
            hit |= (px < hl && py < 0.0) || (px > hr && py < 0.0) || (px > hl && px < hr && py < floor_y);
        }
        return hit;
    } else {
        int l0, l1, r0, r1, a0, a1, b0, b1, y0l, y0h, yd0, yd1;
        hole_interval<true>(s, y0, 0.0, y0l, y0h);
        hole_interval<true>(c, x0, hl, l0, l1);
        if (max(l0, y0l) < min(l1, y0h)) return true;
        hole_interval<false>(c, x0, hr, r0, r1);
        if (max(r0, y0l) < min(r1, y0h)) return true;
        hole_interval<true>(s, y0, floor_y, yd0, yd1);
        hole_interval<false>(c, x0, hl, a0, a1);
        hole_interval<true>(c, x0, hr, b0, b1);
        return max(max(a0, b0), yd0) < min(min(a1, b1), yd1);
    }
}

// vel_acc's sum(qd^2) (hr_dist_vel_acc_reward.py:54) in numpy's dtypes: qd is the action, float32 for the velocity / position
// controllers from the first step on (f32), float64 for the motor controller; in numpy's order of additions (np_sum, mpk_dev.h)
template <int MD>
__device__ __forceinline__ double hole_vel_cost(bool f32, int D, const double* qd) {
    if (f32)
        return (double)np_sum<MD, float>(D, [&](int d) { const float v = (float)qd[d]; return v * v; });
    return np_sum<MD, double>(D, [&](int d) { return qd[d] * qd[d]; });
}

// vel_acc's np.dot(reward_features, reward_factors) (hr_dist_vel_acc_reward.py:57-58) over (dist_cost, vel_cost, acc_cost,
// collision_cost, time_cost) x (-1, -1e-4, -1e-6, -penalty, 0).  np.dot of five float64 entries is the BLAS's ddot, whose loop over
// so short a vector is `dot += x[i] * y[i]` compiled to fused multiply-adds: ONE rounding per entry, in index order.  A step without
// a distance term still has two non-zero products here (velocity and acceleration), so the fusing shows in the last bit: every such
// reward of the reference fixtures (3 .. 16 links) is this chain's, and one in five to eight of them is not the sum of separately
// rounded products.  (simple and unbounded have one non-zero product on such a step: either way of adding gives their bits.)
__device__ __forceinline__ double hole_vel_acc_reward(double dist_cost, double vel_cost, double acc_cost, double coll_cost,
                                                      double penalty) {
    double r = dist_cost * -1.0;
    r = fma(vel_cost, -1e-4, r);
    r = fma(acc_cost, -1e-6, r);
    return fma(coll_cost, -penalty, r);     // (the fifth feature, time_cost, has factor 0 and is 0)
}

__device__ __noinline__ double hole_unbounded_dist_reward(double dist, bool hit, bool up, double ey) {
    return hit ? 0.25 * exp(-dist) : (up ? exp(-dist) : 1.0 - ey);
}

}  // namespace mpk
