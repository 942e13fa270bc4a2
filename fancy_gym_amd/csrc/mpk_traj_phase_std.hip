// k_traj_phase_std: the trajectory's standard deviation under a Gaussian over the non-phase parameters at a PER-EPISODE tau / delay
// (mpk_trajectory_phase_std)
#include "mpk_tile.h"
#include "mpk_cond_rows.h"
#include "mpk_phase_rows.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// With a learned tau / delay every episode has its own rows, so there is no table k_traj_std_tile's matrix tiles could share.  The
// arithmetic is the factor form all the same (mpk_traj_std.hip has the story): with row_{t,d} the position (velocity) row of episode b at
// step t -- e[k] (ev[k]) of mpk_phase_rows.h in DoF d's block, zero elsewhere --
//     std[b, t, d] = | row_{t,d} tril(L_b) | = sqrt(sum_{j < (d + 1) Kloc} (sum_k e[k] L[d Kloc + k][j])^2)
// L L^T is never formed: L = 0 gives exact zeros, a rank-deficient covariance keeps its zeros, and the strict upper triangle is never
// read (the entries j > row of the diagonal block are skipped, not multiplied by a stored zero).  init_pos / init_vel are deterministic
// and contribute nothing, so of params only the phase columns are read.
// k_traj_phase_std<MP>: one wave per episode, `waves` of them a workgroup (sized at launch from the LDS the triangle needs).
//   * The row constants and base times once per workgroup (phase_rows_stage); the episode's lower triangle once from HBM into the wave's
//     LDS as packed float32, row i at i (i + 1) / 2 -- the input's own precision, half the LDS of a float64 image (Pl = 160: 52 KB, three
//     waves on a CU).
//   * lane <-> step, 64 steps a round: the lane evaluates its step's e / ev in float64 (phase_rows_eval, phase_rows_eval_vel) and keeps
//     them in registers.  Per DoF and column j every lane reads the same LDS word (a broadcast: no bank conflict), widens it and feeds the
//     position and the velocity chain; float64 sums, one rounding on the way out.
//   * A round's [64][D] roots leave through an LDS tile as one contiguous run (b, t0 .. t0 + 63, :), lane <-> consecutive floats; a
//     lane-per-step store would stride by D.
// No atomics on results, an episode never leaves its wave, nothing depends on an address: the same bits from run to run, for any
// alignment of the pointers, alone or in a batch.  A ProDMP step beyond the pre-computed range raises the handle's range flag.
// LDS: waves x 4 (Pl (Pl + 1) / 2 + 128 D) bytes + the row constants and 4 T.
// ------------------------------------------------------------------------------------------------------------
struct PhaseStdArgs {
    DevCfg c;
    const float* params;   // [B, P]; the phase columns are read
    const float* L;        // [B, Pl, Pl]; the lower triangle is read
    float* pos_std;        // [B, T, D] or nullptr
    float* vel_std;
    float init_time;
    int B, Pl;
    int waves;             // per workgroup
    int wave_floats;       // floats of LDS per wave
    int c_pad;             // floats of the workgroup's row constants (phase_rows_const_floats)
    int32_t* flag;         // prodmp: raised beyond the pre-computed range (k_phase_fit's)
};

template <int MP>
__global__ void __launch_bounds__(256) k_traj_phase_std(const PhaseStdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pstd_smem[];
    constexpr int KS = kPhaseRowSlots;
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int D = c.D, Kloc = c.Kloc, Pl = a.Pl, T = c.T;
    float* sK = pstd_smem;                                          // the row constants (8-byte aligned), then
    float* sBT = sK + a.c_pad;                                      // [T] the base times
    float* tri = pstd_smem + ((a.c_pad + T + 1) & ~1) + (size_t)wave * a.wave_floats;   // packed lower triangle
    float* tile = tri + Pl * (Pl + 1) / 2;                          // [2][64][D] a round's roots
    phase_rows_stage<MP>(c, sK, sBT, tid, blockDim.x);
    __syncthreads();
    const bool wp = a.pos_std != nullptr, wv = a.vel_std != nullptr;
    for (int b = blockIdx.x * a.waves + wave; b < a.B; b += gridDim.x * a.waves) {
        const float* Lb = a.L + (size_t)b * Pl * Pl;
        for (int i = 0; i < Pl; ++i)
            for (int j = lane; j <= i; j += 64) tri[i * (i + 1) / 2 + j] = Lb[(size_t)i * Pl + j];
        const PhaseEpisode ep = phase_rows_episode<MP>(c, a.params + (size_t)b * c.P, a.init_time);
        cond_wave_sync();
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int nout = T - t0 < 64 ? T - t0 : 64;
            const int t = t0 + lane < T ? t0 + lane : T - 1;        // the lanes beyond the horizon repeat its last step; they store nothing
            double e[KS], ev[KS], ca, cb, cg;
#pragma unroll
            for (int k = 0; k < KS; ++k) { e[k] = 0.0; ev[k] = 0.0; }
            if (wp) phase_rows_eval<MP>(c, ep, sK, sBT[t], a.flag, e, ca, cb, cg);
            if (wv) phase_rows_eval_vel<MP>(c, ep, sK, sBT, t, a.flag, ev, ca, cb, cg);
            for (int d = 0; d < D; ++d) {
                double sp = 0.0, sv = 0.0;
                for (int j = 0; j < (d + 1) * Kloc; ++j) {          // (wave-uniform)
                    const int k0 = j - d * Kloc;                    // the diagonal block: rows k >= k0 reach column j
                    double ap = 0.0, av = 0.0;
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        if (k < Kloc && k >= k0) {
                            const int row = d * Kloc + k;
                            const double l = (double)tri[row * (row + 1) / 2 + j];
                            ap = __builtin_fma(e[k], l, ap);
                            av = __builtin_fma(ev[k], l, av);
                        }
                    }
                    sp = __builtin_fma(ap, ap, sp);
                    sv = __builtin_fma(av, av, sv);
                }
                tile[lane * D + d] = (float)sqrt(sp);
                tile[64 * D + lane * D + d] = (float)sqrt(sv);
            }
            cond_wave_sync();
            const size_t at = ((size_t)b * T + t0) * D;
            for (int i = lane; i < nout * D; i += 64) {
                if (wp) a.pos_std[at + i] = tile[i];
                if (wv) a.vel_std[at + i] = tile[64 * D + i];
            }
            cond_wave_sync();                                       // the tile is free again
        }
    }
}

#ifndef MPK_DEVICE_ONLY
// the shapes the kernel takes; MPK_ENOTIMPL with the limit in the message otherwise (no HIP call)
int traj_phase_std_limits(const DevCfg& c, size_t* lds_out, int* waves_out, int* wave_floats_out) {
    const std::string name("mpk_trajectory_phase_std");
    if (const int rc = gauss_common_limits(c, name.c_str())) return rc;
    if (const int rc = gauss_phase_row_limits(c, kPhaseRowSlots, name.c_str())) return rc;
    const size_t Pl = (size_t)c.D * c.Kloc;
    const size_t wave_floats = (Pl * (Pl + 1) / 2 + (size_t)2 * 64 * c.D + 1) / 2 * 2;
    const size_t shared = ((size_t)phase_rows_const_floats(c) + c.T + 1) / 2 * 2 * sizeof(float);
    if (wave_floats * sizeof(float) + shared > kLdsPerCu) {
        set_error(name + ": the float32 triangle of " + std::to_string(Pl) + " parameters and the base times of " + std::to_string(c.T) +
                  " steps (" + std::to_string(wave_floats * sizeof(float) + shared) + " bytes with one wave per workgroup) do not fit the CU's " +
                  std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    // gauss_wave_plan counts float64 words per wave
    const WavePlan plan = gauss_wave_plan(wave_floats / 2, shared);
    if (lds_out) *lds_out = plan.lds;
    if (waves_out) *waves_out = plan.waves;
    if (wave_floats_out) *wave_floats_out = (int)wave_floats;
    return MPK_OK;
}

int launch_traj_phase_std(const DevCfg& c, const float* params, const float* params_L, float init_time, float* pos_std, float* vel_std,
                          int32_t* range_flag, int B, int num_cu, void* stream, const char** kernel_name) {
    PhaseStdArgs sa{};
    size_t lds = 0;
    const int rc = traj_phase_std_limits(c, &lds, &sa.waves, &sa.wave_floats);
    if (rc != MPK_OK) return rc;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    if (promp && vel_std && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    sa.c = c; sa.params = params; sa.L = params_L; sa.pos_std = pos_std; sa.vel_std = vel_std; sa.init_time = init_time;
    sa.B = B; sa.Pl = c.D * c.Kloc; sa.c_pad = phase_rows_const_floats(c); sa.flag = range_flag;
    const int blocks = gauss_blocks(B, sa.waves, lds, num_cu);
    *kernel_name = promp ? "k_traj_phase_std<promp>" : "k_traj_phase_std<prodmp>";
    return dispatch_mp(promp, [&](auto mp) {
        return launch_kernel(k_traj_phase_std<mp.value>, dim3(blocks), dim3(64 * sa.waves), lds, stream, sa);
    });
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
