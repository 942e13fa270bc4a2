// k_reacher_autoreset: the per-episode autoreset of a vector step in one launch (mpk_reacher_autoreset), one lane per episode:
//   final_obs[b] = the observation of the state the step left (k_reacher_obs's row);
//   a selected episode (mask[b] != 0, or without a mask done[b] != 0) runs its reset (k_reacher_reset's row: the draw program on the
//   episode's own generator, plant state, counters, goal / hole, fp32 image) and obs[b] = the new episode's first observation;
//   every other episode keeps all of its state and obs[b] = final_obs[b].
// The draw program and the observation row are the functions of mpk_reacher_env.h that k_reacher_reset and k_reacher_obs run: the
// same bits as the three launches (observation, masked reset, observation) this one replaces.
//
// Rows are assembled in LDS in output order, as k_reacher_obs does, and the [n_b, n_out] blocks of final_obs and obs leave as
// contiguous runs with consecutive lanes on consecutive floats; the state rows of a reset episode (D doubles, 40 bytes of generator)
// are written by its lane, as k_reacher_reset writes them.
#include "mpk_reacher_env.h"

namespace mpk {

constexpr int kAutoresetBlock = 128;     // episodes (= lanes) per workgroup

struct AutoresetArgs {
    ResetArgs r;
    ObsLayout L;                         // read only with obs != nullptr
    const uint8_t* mask;                 // [B] or nullptr: the done bytes select
    uint8_t* reset_mask;                 // [B] or nullptr
    float* final_obs;                    // [B, n_out] or nullptr (with obs)
    float* obs;                          // [B, n_out] or nullptr
};

template <int MD>
__global__ void __launch_bounds__(kAutoresetBlock) k_reacher_autoreset(const AutoresetArgs a) {
    extern __shared__ float s_rows[];    // [2, kAutoresetBlock, n_out] with observations, else nothing
    __shared__ int s_pos[kObsCols];
    const ObsLayout& L = a.L;
    const bool with_obs = a.obs != nullptr;          // uniform over the launch
    const int b0 = blockIdx.x * kAutoresetBlock;
    const int nb = min(kAutoresetBlock, a.r.B - b0);
    const int n_out = with_obs ? L.n_out : 0;
    float* s_final = s_rows;
    float* s_obs = s_rows + kAutoresetBlock * n_out;
    if (with_obs) {
        obs_positions(L, s_pos);
        __syncthreads();
    }
    if ((int)threadIdx.x < nb) {
        const int b = b0 + threadIdx.x, D = a.r.D;
        float* rf = s_final + threadIdx.x * n_out;
        float* ro = s_obs + threadIdx.x * n_out;
        if (with_obs) {
            double q[MD], qd[MD];
#pragma unroll
            for (int d = 0; d < MD; ++d) {
                q[d] = d < D ? a.r.q[(size_t)b * D + d] : 0.0;
                qd[d] = d < D ? a.r.qd[(size_t)b * D + d] : 0.0;
            }
            double gx, gy, width;
            obs_task(L, a.r.task_out, b, gx, gy, width);
            obs_row<MD>(L, s_pos, q, qd, gx, gy, width, a.r.traj_steps[b], rf);
        }
        const bool sel = (a.mask ? a.mask[b] : a.r.done[b]) != 0;
        if (sel) {
            double t0, t1, t2;
            const double q0 = reset_episode(a.r, b, t0, t1, t2);
            if (with_obs) {
                // the new episode's row from the values just written: first joint q0, the others 0, at rest, step counter 0
                double q[MD], qd[MD];
#pragma unroll
                for (int d = 0; d < MD; ++d) { q[d] = d == 0 ? q0 : 0.0; qd[d] = 0.0; }
                const bool hole = L.env == MPK_RESET_HOLE_REACHER;
                obs_row<MD>(L, s_pos, q, qd, t0, hole ? -t2 : t1, hole ? t1 : 0.0, 0, ro);
            }
        } else if (with_obs) {
            for (int k = 0; k < n_out; ++k) ro[k] = rf[k];
        }
        if (a.reset_mask) a.reset_mask[b] = sel ? 1 : 0;
    }
    if (!with_obs) return;
    __syncthreads();
    float* dst_f = a.final_obs + (size_t)b0 * n_out;
    float* dst_o = a.obs + (size_t)b0 * n_out;
    for (int j = threadIdx.x; j < nb * n_out; j += kAutoresetBlock) {
        dst_f[j] = s_final[j];
        dst_o[j] = s_obs[j];
    }
}

#ifndef MPK_DEVICE_ONLY
int launch_reacher_autoreset(const ResetLaunch& l, const ObsLaunch* o, const uint8_t* mask, uint8_t* reset_mask, float* final_obs,
                             float* obs, int B, int D, void* stream, int* fault) {
    AutoresetArgs a;
    a.r = reset_args(l, B, D, fault);
    a.L = ObsLayout{};
    if (o) a.L = obs_layout(*o);
    a.mask = mask; a.reset_mask = reset_mask; a.final_obs = o ? final_obs : nullptr; a.obs = o ? obs : nullptr;
    const dim3 grid((unsigned)((B + kAutoresetBlock - 1) / kAutoresetBlock)), block(kAutoresetBlock);
    const size_t lds = o ? (size_t)2 * kAutoresetBlock * o->n_out * sizeof(float) : 0;
    if (D == 2) hipLaunchKernelGGL(k_reacher_autoreset<2>, grid, block, lds, (hipStream_t)stream, a);
    else if (D == 5) hipLaunchKernelGGL(k_reacher_autoreset<5>, grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_reacher_autoreset<kMaxD>, grid, block, lds, (hipStream_t)stream, a);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
