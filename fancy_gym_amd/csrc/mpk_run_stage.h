// One episode's contiguous run of T * D floats, HBM -> a wave's LDS image, shared by k_traj_vjp_tile (mpk_traj_vjp.hip: the gradient
// rows) and k_traj_fit_tile (mpk_traj_fit.hip: the demonstrated positions).
//   run_shift   floats by which the run starts past a 16-byte boundary.
//   stage_run   the wave copies the run with 16-byte loads into an image SHIFTED by run_shift, so aligned HBM chunks land on aligned
//               LDS chunks whatever the pointer and T * D; up to three floats at either end go as dwords; the (TP - T) * D <= 48 floats
//               behind the run are zero-filled, so a tail chunk contracts zeros and nothing is read past T.  Element f of the run is at
//               img[run_shift + f].  The values an image holds, and the order they are contracted in, do not depend on the alignment.
#pragma once
#include "mpk_dev.h"

namespace mpk {

__device__ __forceinline__ int run_shift(const float* g, int b, int TD) {
    return (int)((reinterpret_cast<uintptr_t>(g + (size_t)b * TD) >> 2) & 3u);
}

// img: the episode's image (before the shift); src: the array's base; TPD = TP * D
__device__ __forceinline__ void stage_run(float* img, const float* src, int bb, int TD, int TPD, int lane) {
    const float* s = src + (size_t)bb * TD;
    const int shift = run_shift(src, bb, TD);
    float* dst = img + shift;                                           // element f of the run at dst[f]
    const int head = min((4 - shift) & 3, TD);
    const int n4 = (TD - head) >> 2;
    const int tail0 = head + 4 * n4;
    if (lane < head) dst[lane] = s[lane];
    for (int i0 = lane; i0 < n4; i0 += 256) {                           // four 16-byte loads in flight per lane
        f32x4 r4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 64 * u < n4) r4[u] = *reinterpret_cast<const f32x4*>(s + head + 4 * (i0 + 64 * u));
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 64 * u < n4) *reinterpret_cast<f32x4*>(dst + head + 4 * (i0 + 64 * u)) = r4[u];
    }
    if (tail0 + lane < TD) dst[tail0 + lane] = s[tail0 + lane];
    if (TD + lane < TPD) dst[TD + lane] = 0.0f;                         // (TP - T) * D <= 48 floats
}

// floats between the images of a group's episodes: the shifted, zero-filled run rounded to 32 banks, then 32 / NTW banks apart so the
// two 32-lane halves of a fragment read do not collide
inline long run_image_stride(int TP, int D, int NTW) {
    const long need = (long)TP * D + 3;
    return (need + 31) / 32 * 32 + (NTW == 1 ? 0 : (32 / NTW > 4 ? 32 / NTW : 4));
}

}  // namespace mpk
