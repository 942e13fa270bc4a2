// One step of the reacher plants, shared by the rollout kernels and the step-observation replay (mpk_obs.hip): the replay runs the
// same operations on the same state and so reproduces the rollout's states bit for bit.  float64 without FMA contraction
// (-ffp-contract=off), except where the reference's numpy flow is float32 (hole_plant_step).
#pragma once
#include "mpk_dev.h"

namespace mpk {

// SimpleReacher (base_reacher_torque.py:20-37) for one DoF: tracking controller + clip (black_box_wrapper.py:176-179), then the
// torque double integrator.  Returns the clipped action.
__device__ __forceinline__ double torque_step(int ctrl, double pg, double dg, double lo, double hi, double dt, double dp, double dv,
                                              double& q, double& qd) {
    double u;
    if (ctrl == MPK_CTRL_MOTOR) u = pg * (dp - q) + dg * (dv - qd);
    else if (ctrl == MPK_CTRL_POSITION) u = dp;
    else u = dv;
    u = fmin(fmax(u, lo), hi);
    qd = qd + dt * u;
    q = q + dt * qd;
    return u;
}

// HoleReacher's tracking controller + clip for all DoFs of an episode; g = {p gains, d gains, low, high} at stride kMaxD
template <int MD>
__device__ __forceinline__ void hole_control(int ctrl, int D, const double* g, const float* dpos, const float* dvel, const double* q,
                                             const double* qd, double* u) {
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        if (d >= D) { u[d] = 0.0; continue; }
        double v;
        if (ctrl == MPK_CTRL_VELOCITY) v = (double)dvel[d];
        else if (ctrl == MPK_CTRL_POSITION) v = (double)dpos[d];
        else v = g[d] * ((double)dpos[d] - q[d]) + g[kMaxD + d] * ((double)dvel[d] - qd[d]);
        u[d] = fmin(fmax(v, g[2 * kMaxD + d]), g[3 * kMaxD + d]);
    }
}

// the direct-velocity plant (base_reacher_direct.py:26-28) and its control cost sum(acc^2), in numpy's dtypes: the velocity / position
// controllers hand over a float32 action, which becomes the state qd -- from the episode's second step on (f32: env step > 0)
// acc = (a - qd) / dt and dt * qd are float32 operations (numpy casts the Python float dt to float32), and np.sum(acc ** 2) adds in
// float32; the first step subtracts from the float64 start velocity.  The motor controller's action is float64 throughout.  Either
// sum in numpy's order of additions (np_sum, mpk_dev.h).
template <int MD>
__device__ __forceinline__ double hole_plant_step(int ctrl, bool f32, int D, double dt, float dt32, const double* u, double* q,
                                                  double* qd) {
    // (the sums read u and the velocity the step found: before the state moves)
    if (f32) {
        const float c32 = np_sum<MD, float>(D, [&](int d) {
            const float acc = ((float)u[d] - (float)qd[d]) / dt32;
            return acc * acc;
        });
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            if (d >= D) continue;
            const float a32 = (float)u[d];
            qd[d] = (double)a32;
            q[d] = q[d] + (double)(dt32 * a32);
        }
        return (double)c32;
    }
    const double acc_cost = np_sum<MD, double>(D, [&](int d) {
        const double acc = (u[d] - qd[d]) / dt;
        return acc * acc;
    });
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        if (d >= D) continue;
        qd[d] = u[d];
        q[d] = ctrl == MPK_CTRL_MOTOR ? q[d] + dt * qd[d] : q[d] + (double)(dt32 * (float)u[d]);
    }
    return acc_cost;
}

}  // namespace mpk
