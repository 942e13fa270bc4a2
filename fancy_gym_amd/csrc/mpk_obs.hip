// k_reacher_obs / k_reacher_step_obs: the observations of the reference's reacher envs for B device-resident episodes
// (mpk_reacher_observation, mpk_reacher_step_observations).
//   SimpleReacher _get_obs (simple_reacher.py:75-83): [cos q, sin q, qd, ee - goal, steps]
//   HoleReacher   _get_obs (hole_reacher.py:114-124): [cos q, sin q, qd, width, ee - goal, steps], goal = (x, -depth)
// plus, optionally, TimeAwareObservation's t / max_episode_steps (utils/wrappers.py:49-63).  A row is computed in float64 and cast
// to float32 once, as .astype(np.float32) does; the end effector follows _update_joints (base_reacher.py:95-103): the cumulative
// angles and the joints as sequential sums, numpy's order.  A column mask selects the written columns (the MP wrappers'
// context_mask); selected columns keep their order.
//
// Rows are assembled in LDS in output order and leave as contiguous runs: k_reacher_obs stores the [n_b, n_out] block of its
// workgroup's episodes, k_reacher_step_obs the S-step pieces [S, n_out] of its wave's 64 episodes, one piece after the other.
#include "mpk_reacher_env.h"
#include "mpk_plant.h"

namespace mpk {

constexpr int kObsBlock = 128;           // k_reacher_obs: episodes (= lanes) per workgroup
constexpr int kStepObsLds = 8192;        // k_reacher_step_obs: floats of row image per wave (32 KB)

struct ObsArgs {
    ObsLayout L;
    const double* q;
    const double* qd;
    const double* task;
    const int32_t* steps;
    float* out;                          // [B, n_out]
    int B;
};

template <int MD>
__global__ void __launch_bounds__(kObsBlock) k_reacher_obs(const ObsArgs a) {
    extern __shared__ float s_rows[];    // [kObsBlock, n_out]
    __shared__ int s_pos[kObsCols];
    const ObsLayout& L = a.L;
    obs_positions(L, s_pos);
    __syncthreads();
    const int b0 = blockIdx.x * kObsBlock;
    const int nb = min(kObsBlock, a.B - b0);
    const int n_out = L.n_out;
    if ((int)threadIdx.x < nb) {
        const int b = b0 + threadIdx.x, D = L.D;
        double q[MD], qd[MD];
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            q[d] = d < D ? a.q[(size_t)b * D + d] : 0.0;
            qd[d] = d < D ? a.qd[(size_t)b * D + d] : 0.0;
        }
        double gx, gy, width;
        obs_task(L, a.task, b, gx, gy, width);
        obs_row<MD>(L, s_pos, q, qd, gx, gy, width, a.steps[b], s_rows + threadIdx.x * n_out);
    }
    __syncthreads();
    float* dst = a.out + (size_t)b0 * n_out;
    for (int j = threadIdx.x; j < nb * n_out; j += kObsBlock) dst[j] = s_rows[j];
}

struct StepObsArgs {
    ObsLayout L;
    RolloutDev rc;
    const float* des_pos;
    const float* des_vel;
    const double* q0;
    const double* qd0;
    const double* task;
    const int32_t* n_exec;
    const int32_t* step0;
    float* out;                          // [B, T, n_out]
    double* q_end;                       // [B, D] or nullptr
    double* qd_end;
    int B, T, S;                         // S: steps per LDS piece
};

// One wave per workgroup, one lane per episode: the replay of the executed steps from the plan-start state on the stored plan,
// with the controller + plant code of the rollout kernels (mpk_plant.h: same operations, same bits), one observation row per step
// into the wave's LDS image; rows past n_exec are 0.  Every S steps the wave stores the 64 pieces [S, n_out] (contiguous in `out`
// per episode) with consecutive lanes on consecutive floats.
template <int MD>
__global__ void __launch_bounds__(64) k_reacher_step_obs(const StepObsArgs a) {
    extern __shared__ float s_img[];     // [64, S, n_out]
    __shared__ int s_pos[kObsCols];
    __shared__ double s_g[4 * kMaxD];
    const ObsLayout& L = a.L;
    const int D = MD < kMaxD ? MD : L.D;
    obs_positions(L, s_pos);
    if (threadIdx.x < (unsigned)D) {
        s_g[threadIdx.x] = a.rc.pg[threadIdx.x];
        s_g[kMaxD + threadIdx.x] = a.rc.dg[threadIdx.x];
        s_g[2 * kMaxD + threadIdx.x] = a.rc.lo[threadIdx.x];
        s_g[3 * kMaxD + threadIdx.x] = a.rc.hi[threadIdx.x];
    }
    __syncthreads();
    const int b0 = blockIdx.x * 64;
    const int nb = min(64, a.B - b0);
    const bool on = (int)threadIdx.x < nb;
    const int b = b0 + (on ? (int)threadIdx.x : 0);
    const int T = a.T, S = a.S, n_out = L.n_out;
    const int ctrl = a.rc.controller_type;
    const bool hole = L.env == MPK_RESET_HOLE_REACHER;
    int n = on ? a.n_exec[b] : 0;
    n = n < 0 ? 0 : (n > T ? T : n);
    const int s0 = on ? a.step0[b] : 0;
    double q[MD], qd[MD];
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        q[d] = (on && d < D) ? a.q0[(size_t)b * D + d] : 0.0;
        qd[d] = (on && d < D) ? a.qd0[(size_t)b * D + d] : 0.0;
    }
    double gx = 0.0, gy = 0.0, width = 0.0;
    if (on) obs_task(L, a.task, b, gx, gy, width);
    const double dt = a.rc.dt;
    const float dt32 = (float)dt;
    float* img = s_img + threadIdx.x * S * n_out;
    const int piece = S * n_out;
    for (int t0 = 0; t0 < T; t0 += S) {
        const int se = min(S, T - t0);
        for (int s = 0; s < se; ++s) {
            const int t = t0 + s;
            float* r = img + s * n_out;
            if (t < n) {
                const size_t row = ((size_t)b * T + t) * D;
                if (hole) {
                    double u[MD];
                    hole_control<MD>(ctrl, D, s_g, a.des_pos ? a.des_pos + row : nullptr, a.des_vel ? a.des_vel + row : nullptr, q, qd, u);
                    (void)hole_plant_step<MD>(ctrl, ctrl != MPK_CTRL_MOTOR && s0 + t > 0, D, dt, dt32, u, q, qd);
                } else {
#pragma unroll
                    for (int d = 0; d < MD; ++d) {
                        if (d >= D) continue;
                        const double dp = a.des_pos ? (double)a.des_pos[row + d] : 0.0;
                        const double dv = a.des_vel ? (double)a.des_vel[row + d] : 0.0;
                        (void)torque_step(ctrl, s_g[d], s_g[kMaxD + d], s_g[2 * kMaxD + d], s_g[3 * kMaxD + d], dt, dp, dv, q[d], qd[d]);
                    }
                }
                obs_row<MD>(L, s_pos, q, qd, gx, gy, width, s0 + t + 1, r);
            } else {
                for (int k = 0; k < n_out; ++k) r[k] = 0.0f;
            }
        }
        __syncthreads();
        // episode i's piece: se * n_out floats at out[(b0 + i) T + t0, 0 ..); j -> (i, k) by a float reciprocal (exact: j < 2^16,
        // and (j + 0.5) / len stays >= 0.5 / len away from an integer)
        const int len = se * n_out;
        const float inv = 1.0f / (float)len;
        for (int j = threadIdx.x; j < nb * len; j += 64) {
            const int i = (int)(((float)j + 0.5f) * inv);
            const int k = j - i * len;
            a.out[((size_t)(b0 + i) * T + t0) * n_out + k] = s_img[i * piece + k];
        }
        __syncthreads();
    }
    if (on && a.q_end) {
#pragma unroll
        for (int d = 0; d < MD; ++d)
            if (d < D) { a.q_end[(size_t)b * D + d] = q[d]; a.qd_end[(size_t)b * D + d] = qd[d]; }
    }
}

#ifndef MPK_DEVICE_ONLY
int launch_reacher_obs(const ObsLaunch& l, const double* q, const double* qd, const double* task, const int32_t* steps, float* out,
                       int B, void* stream) {
    ObsArgs a;
    a.L = obs_layout(l); a.q = q; a.qd = qd; a.task = task; a.steps = steps; a.out = out; a.B = B;
    const dim3 grid((unsigned)((B + kObsBlock - 1) / kObsBlock)), block(kObsBlock);
    const size_t lds = (size_t)kObsBlock * l.n_out * sizeof(float);
    if (l.D == 2) hipLaunchKernelGGL(k_reacher_obs<2>, grid, block, lds, (hipStream_t)stream, a);
    else if (l.D == 5) hipLaunchKernelGGL(k_reacher_obs<5>, grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_reacher_obs<kMaxD>, grid, block, lds, (hipStream_t)stream, a);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}

int launch_reacher_step_obs(const ObsLaunch& l, const RolloutDev& rc, const float* des_pos, const float* des_vel, const double* q0,
                            const double* qd0, const double* task, const int32_t* n_exec, const int32_t* step0, float* out,
                            double* q_end, double* qd_end, int B, int T, void* stream) {
    StepObsArgs a;
    a.L = obs_layout(l); a.rc = rc; a.des_pos = des_pos; a.des_vel = des_vel; a.q0 = q0; a.qd0 = qd0; a.task = task;
    a.n_exec = n_exec; a.step0 = step0; a.out = out; a.q_end = q_end; a.qd_end = qd_end; a.B = B; a.T = T;
    const int S = kStepObsLds / (64 * l.n_out);
    a.S = S < 1 ? 1 : (S > 16 ? 16 : S);
    const dim3 grid((unsigned)((B + 63) / 64)), block(64);
    const size_t lds = (size_t)64 * a.S * l.n_out * sizeof(float);
    if (l.D == 2) hipLaunchKernelGGL(k_reacher_step_obs<2>, grid, block, lds, (hipStream_t)stream, a);
    else if (l.D == 5) hipLaunchKernelGGL(k_reacher_step_obs<5>, grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_reacher_step_obs<kMaxD>, grid, block, lds, (hipStream_t)stream, a);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
