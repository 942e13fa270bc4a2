// k_reacher_reset: the seeded resets of the reference's reacher envs for B device-resident episodes, one lane per episode
// (mpk_reacher_reset).  Each lane (re)seeds or continues its episode's numpy generator (mpk_nprng.h), runs the env's draw program
// and writes what mpk_episode_reset writes (k_episode_reset, mpk_misc.hip) plus the goal / hole and the advanced generator state.
//   HoleReacher   hole_reacher.py:60-71,79-101, base_reacher.py:73-93: [reseed] width, direction + x, depth, first joint
//   SimpleReacher simple_reacher.py:46-54,85-96, base_reacher.py:73-93: goal (discarded), [reseed] first joint, goal, [reseed]
//                 first joint
#include "mpk_reacher_env.h"

namespace mpk {

__global__ void __launch_bounds__(256) k_reacher_reset(const ResetArgs a) {
    const long bl = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= a.B) return;
    const int b = (int)bl;
    double t0, t1, t2;
    (void)reset_episode(a, b, t0, t1, t2);       // mpk_reacher_env.h: the draw program and the row's writes
}

#ifndef MPK_DEVICE_ONLY
int launch_reacher_reset(const ResetLaunch& l, int B, int D, void* stream, int* fault) {
    const ResetArgs a = reset_args(l, B, D, fault);
    hipLaunchKernelGGL(k_reacher_reset, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
