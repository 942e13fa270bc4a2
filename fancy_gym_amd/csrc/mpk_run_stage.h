// One episode's contiguous run of T * D floats, HBM -> a wave's LDS image, shared by k_traj_vjp_tile (mpk_traj_vjp.hip: the gradient
// rows) and k_traj_fit_tile (mpk_traj_fit.hip: the demonstrated positions).
//   run_shift   floats by which the run starts past a 16-byte boundary.
//   stage_run   the wave copies the run with 16-byte loads into an image SHIFTED by run_shift, so aligned HBM chunks land on aligned
//               LDS chunks whatever the pointer and T * D; up to three floats at either end go as dwords; the (TP - T) * D <= 48 floats
//               behind the run are zero-filled, so a tail chunk contracts zeros and nothing is read past T.  Element f of the run is at
//               img[run_shift + f].  The values an image holds, and the order they are contracted in, do not depend on the alignment.
//   store_run   the reverse for an output run (k_traj_std_tile, mpk_traj_std.hip): LDS image -> HBM with 16-byte stores.
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

// the way back (k_traj_std_tile, mpk_traj_std.hip): an image the wave built at img[run_shift + f] leaves as the episode's contiguous run --
// 16-byte stores for the aligned body, up to three dwords at either end; nothing outside the run's T * D floats is written.  SQRT: the
// image holds squares and their roots leave (one sqrt per stored element, taken by all 64 lanes here instead of by the few that
// write an image element)
template <bool SQRT>
__device__ __forceinline__ void store_run(float* dst, const float* img, int bb, int TD, int lane) {
    float* g = dst + (size_t)bb * TD;
    const int shift = run_shift(dst, bb, TD);
    const float* s = img + shift;
    const int head = min((4 - shift) & 3, TD);
    const int n4 = (TD - head) >> 2;
    const int tail0 = head + 4 * n4;
    if (lane < head) g[lane] = SQRT ? sqrtf(s[lane]) : s[lane];
    for (int i = lane; i < n4; i += 64) {
        f32x4 v = *reinterpret_cast<const f32x4*>(s + head + 4 * i);
        if (SQRT) { v[0] = sqrtf(v[0]); v[1] = sqrtf(v[1]); v[2] = sqrtf(v[2]); v[3] = sqrtf(v[3]); }
        *reinterpret_cast<f32x4*>(g + head + 4 * i) = v;
    }
    if (tail0 + lane < TD) g[tail0 + lane] = SQRT ? sqrtf(s[tail0 + lane]) : s[tail0 + lane];
}

// floats between the images of a group's episodes: the shifted, zero-filled run rounded to 32 banks, then 32 / NTW banks apart so the
// two 32-lane halves of a fragment read do not collide
inline long run_image_stride(int TP, int D, int NTW) {
    const long need = (long)TP * D + 3;
    return (need + 31) / 32 * 32 + (NTW == 1 ? 0 : (32 / NTW > 4 ? 32 / NTW : 4));
}

}  // namespace mpk
