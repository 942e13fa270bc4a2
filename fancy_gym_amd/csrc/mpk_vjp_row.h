// The rows of the shared-phase map's transpose and the transposed input gather, shared by mpk_traj_vjp.hip (mpk_trajectory_vjp) and
// mpk_episode_vjp.hip (mpk_episode_return_vjp).  With a phase all episodes share, pos / vel are linear in a DoF's extended parameter
// column x,  pos[b, t, d] = sum_k R0[k][t] x[b, d][k],  vel[b, t, d] = sum_k R1[k][t] x[b, d][k]  (mpk_traj_vjp.hip has the whole story).
//   vjp_row      R0 / R1 of one (column, step) from the k-major table A [n_out][KP][TS] of k_build_shared.  prodmp / dmp response: the
//                table's rows.  promp: the forward's velocity is the forward difference of its positions times the reciprocal fp32 time
//                step (aux), last row repeating -- R1 = (R0[th] - R0[tl]) aux[t] from the position rows alone, which is all a lean
//                (k_traj_wide) table holds.
//   vjp_row_sm   the same two values from ONE row of the table's step-major copy At [TS][n_out * KP] (k_build_shared: prodmp rows
//                interleaved (pos_k, vel_k); promp rows [R0[.][t] | R0[.][th] | R0[.][tl]], the operands of the forward's difference).
//   vjp_scatter  the transposed gather of one element (x_kind, mpk_tile.h: the forward's own function).
//   vjp_zero_uncovered  inputs no column reads (promp: init_vel always, init_pos unless the basis is zero-padded) get an exact 0.
#pragma once
#include "mpk_tile.h"

namespace mpk {

template <int MP>
__device__ __forceinline__ float vjp_row(const DevCfg& c, const float* A, const float* aux, int TS, int o, int k, int t) {
    if (MP == MPK_MP_PROMP) {
        const float* r = A + (size_t)k * TS;
        if (o == 0) return r[t];
        const int th = t < c.T - 1 ? t + 1 : c.T - 1, tl = t < c.T - 1 ? t : c.T - 2;
        return (r[th] - r[tl]) * aux[t];
    }
    return A[((size_t)o * c.KP + k) * TS + t];
}

// a, h, l: the row's entries of column k -- prodmp [2 k], [2 k + 1], unused; promp [k], [KP + k], [2 KP + k]; aux_t: aux[t] (promp)
template <int MP>
__device__ __forceinline__ void vjp_row_sm(float a, float h, float l, float aux_t, float* r0, float* r1) {
    *r0 = a;
    *r1 = MP == MPK_MP_PROMP ? (h - l) * aux_t : h;
}

template <int MP>
__device__ __forceinline__ void vjp_scatter(const DevCfg& c, int k, int b, int d, float v, float* g_params, float* g_init_pos,
                                            float* g_init_vel) {
    int loc;
    const int kind = x_kind<MP>(c, k, &loc);
    if (kind == XK_PARAM) {
        if (g_params) g_params[(size_t)b * c.P + c.off + d * c.Kloc + loc] = v;
    } else if (kind == XK_IPOS) {
        if (g_init_pos) g_init_pos[(size_t)b * c.D + d] = v;
    } else if (kind == XK_IVEL) {
        if (g_init_vel) g_init_vel[(size_t)b * c.D + d] = v;
    }
}

template <int MP>
__device__ __forceinline__ void vjp_zero_uncovered(const DevCfg& c, int b, int d, float* g_init_pos, float* g_init_vel) {
    if (MP == MPK_MP_PROMP) {
        if (g_init_vel) g_init_vel[(size_t)b * c.D + d] = 0.0f;
        if (g_init_pos && c.KT <= c.nb) g_init_pos[(size_t)b * c.D + d] = 0.0f;
    }
}

}  // namespace mpk
