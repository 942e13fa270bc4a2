// What the kernels that read scalar observations of the parameters share (mpk_traj_condition.hip, mpk_traj_log_prob.hip): the wave-level
// ordering of LDS traffic and a ProMP's velocity row in float64.  The observed steps' table rows are staged in float64 from the launch's
// own float32 table (vjp_row, mpk_vjp_row.h) -- but for a ProMP's velocity rows, which cond_promp_vel_row re-evaluates
// (profiles/r20_traj_condition.md says why).
#pragma once
#include "mpk_tile.h"
#include "mpk_vjp_row.h"

namespace mpk {

// what lanes of the wave wrote to LDS is read by other lanes: a wave's LDS operations complete in issue order, so only the compiler has
// to be kept from moving them across
__device__ __forceinline__ void cond_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a ProMP's velocity row (column k < nb, step t) in float64: ws (phi_k(x_th) - phi_k(x_tl)) aux[t] with the forward's fp32 reciprocal
// time step aux and k_build_shared's phase and normalised RBFs (direct exponentials: its recurrence only saves time)
__device__ __forceinline__ double cond_promp_vel_row(const DevCfg& c, const float* aux, float init_time, int k, int t) {
    const int th = t < c.T - 1 ? t + 1 : c.T - 1, tl = t < c.T - 1 ? t : c.T - 2;
    const double* cen = c.tab;
    const double* bw = c.tab + c.n_total;
    double phi[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const double x = phase_f64(c, c.base_times[e ? tl : th] + init_time, c.tau, c.delay, ExpLiteral());
        double sum = 0.0;
        for (int i = 0; i < c.n_total; ++i) {
            const double dx = x - cen[i];
            sum += exp_nonpos(-(dx * dx * bw[i]) * 0.5);
        }
        const double dx = x - cen[c.zs + k];
        const double ek = exp_nonpos(-(dx * dx * bw[c.zs + k]) * 0.5);
        phi[e] = c.n_total > 1 ? div_pos(ek, sum) : 1.0;
    }
    return (phi[0] - phi[1]) * (double)c.ws * (double)aux[t];
}

// the observed table row entry (o = 0 position / 1 velocity, column k, step t) as the staging of both kernels evaluates it
template <int MP>
__device__ __forceinline__ double cond_obs_row(const DevCfg& c, const float* A, const float* aux, int TS, float init_time, int o, int k,
                                               int t) {
    if (MP == MPK_MP_PROMP && o == 1) return k < c.nb ? cond_promp_vel_row(c, aux, init_time, k, t) : 0.0;
    return (double)vjp_row<MP>(c, A, aux, TS, o, k, t);
}

}  // namespace mpk
