// The position row of ONE episode at ONE step for a per-episode phase (learned tau / delay), regrouped by parameter: what k_phase_fit
// (mpk_traj_fit.hip) evaluates per lane, as device functions the kernels of the information form (mpk_demo_gram.h) share.  One row width:
// 16 slots, the basis count at run time.
//   promp   phase_f64 and rbf_row: the forward's row values (weights_scale folded in); a zero-padded basis adds init_pos (given).
//   prodmp  the clipped tau / delay, div_exact and the rintf index of k_traj_phase -- the very table row the forward reads.  The
//           forward contracts [Psi_k .. | xi1 xi2] with [wg_k .. | y_b - sum Psi_k(t_b) wg_k, tau v_b - sum dPsi_k(t_b) wg_k]; regrouped
//           by parameter the row of wg_k is Psi_k - xi1 Psi_k(t_b) - xi2 dPsi_k(t_b), times the column's scale; init_pos gets xi1 (plus
//           the goal's row under relative_goal), init_vel tau xi2, the goal offset the goal's row: the given part
//           c = ca init_pos + cb init_vel + cc.  The values come from the handle's FLOAT64 tables (c.tab), not from the float32 row
//           table the forward gathers, and xi1 / xi2 are not rounded to float32: a likelihood at sigma = 1e-3 multiplies a row's error
//           by 1 / sigma, and the three float32 roundings of Psi_k, Psi_k(t_b) xi1 and dPsi_k(t_b) xi2 -- each relative to its own
//           term, not to their difference -- do not belong in it.  The column scales are the float64 products of the table behind the forward's
//           float32 products: a scale that is 4e-8 off shifts a whole column coherently, and at TableTennis' 350 steps that alone put
//           g_params 1e-4 of its scale off the float64 reference (profiles/r24_demo_phase.md).
#pragma once
#include "mpk_tile.h"

namespace mpk {

constexpr int kPhaseRowSlots = 16;

// the floats of the workgroup's constants in front of the base times: promp [2 n_total + 3] doubles centres | bandwidths | recurrence
// constants; prodmp [16] float64 column scales (0: not fitted) | the goal scale
__host__ __device__ inline int phase_rows_const_floats(const DevCfg& c) {
    return c.mp_type == MPK_MP_PRODMP ? 2 * (kPhaseRowSlots + 2) : (4 * c.n_total + 6 + 3) / 4 * 4;
}

// the workgroup's constants: `consts` (8-byte aligned, phase_rows_const_floats(c) floats) and the base times sBT [T]; the caller
// synchronises the workgroup
template <int MP>
__device__ __forceinline__ void phase_rows_stage(const DevCfg& c, float* consts, float* sBT, int tid, int nthreads) {
    for (int t = tid; t < c.T; t += nthreads) sBT[t] = c.base_times[t];
    if (MP == MPK_MP_PRODMP) {
        // the float64 products of the column scales, behind the forward's float32 products (mpk_create)
        const double* S = c.tab + 4 * (size_t)c.n_pc + 2 * (size_t)c.n_pc * (c.nb + 1) + (c.nb + 1);
        double* sc = reinterpret_cast<double*>(consts);
        if (tid < kPhaseRowSlots) {
            const bool off = tid < c.nb ? c.disable_weights != 0 : (tid == c.nb ? c.disable_goal != 0 : true);
            sc[tid] = off ? 0.0 : S[tid];
        }
        if (tid == kPhaseRowSlots) sc[kPhaseRowSlots] = S[c.nb];
    } else {
        double* sCen = reinterpret_cast<double*>(consts);
        for (int k = tid; k < 2 * c.n_total + 3; k += nthreads) sCen[k] = c.tab[k];
    }
}

// what an episode's rows share: the clipped tau / delay (np.clip(action, low, high) as the forward) and, for a ProDMP, the boundary row
// at the episode's start
struct PhaseEpisode {
    float tau, delay, it;
    ExactDiv dtau, dsdt;
    PosDiv taud;
    const double *pb, *vb;       // prodmp: Psi_k(t_b), dPsi_k(t_b), k <= nb
    double bca, bcb, bcc, bcd;
};

// phase: the tau / delay of the episode as they stand at the front of its params row
template <int MP>
__device__ __forceinline__ PhaseEpisode phase_rows_episode(const DevCfg& c, const float* phase, float init_time) {
    PhaseEpisode ep;
    ep.tau = c.tau; ep.delay = c.delay; ep.it = init_time;
    if (c.learn_tau) ep.tau = fminf(fmaxf(phase[0], c.tau_lo), c.tau_hi);
    if (c.learn_delay) ep.delay = fminf(fmaxf(phase[c.learn_tau ? 1 : 0], c.delay_lo), c.delay_hi);
    ep.dtau = make_exact_div(ep.tau);
    ep.dsdt = make_exact_div(c.scaled_dt);
    ep.taud = make_pos_div((double)ep.tau);
    ep.pb = ep.vb = c.tab;
    ep.bca = ep.bcb = ep.bcc = ep.bcd = 0.0;
    if (MP == MPK_MP_PRODMP) {
        // c.tab: y1 | y2 | dy1 | dy2 [n_pc] each, pos_basis | vel_basis [n_pc][nb + 1] each, the column scales [nb + 1]
        const size_t n_pc = (size_t)c.n_pc, K = (size_t)c.nb + 1;
        const float sbl = fmaxf(div_exact(init_time - ep.delay, ep.dtau), 0.0f);
        const size_t ib = (size_t)max(min((int)rintf(div_exact(sbl, ep.dsdt)), c.n_pc - 1), 0);
        ep.pb = c.tab + 4 * n_pc + ib * K;
        ep.vb = ep.pb + n_pc * K;
        const double y1b = c.tab[ib], y2b = c.tab[n_pc + ib], dy1b = c.tab[2 * n_pc + ib], dy2b = c.tab[3 * n_pc + ib];
        const double idet = div_pos(1.0, y1b * dy2b - y2b * dy1b);
        ep.bca = dy2b * idet; ep.bcb = dy1b * idet; ep.bcc = y1b * idet; ep.bcd = y2b * idet;
    }
    return ep;
}

// the row of the step at base time bt: e[k] the entry of LOCAL parameter k (< Kloc; exact 0 beyond), and the given part
// c[t, d] = ca init_pos[d] + cb init_vel[d] + cc.  flag: raised by a ProDMP step beyond the pre-computed range (k_phase_fit's)
template <int MP>
__device__ __forceinline__ void phase_rows_eval(const DevCfg& c, const PhaseEpisode& ep, const float* consts, float bt, int32_t* flag,
                                                double (&e)[kPhaseRowSlots], double& ca, double& cb, double& cc) {
    constexpr int KS = kPhaseRowSlots;
    const float time = bt + ep.it;
    ca = 0.0; cb = 0.0; cc = 0.0;
    if (MP == MPK_MP_PRODMP) {
        const double* sc = reinterpret_cast<const double*>(consts);
        const size_t n_pc = (size_t)c.n_pc, K = (size_t)c.nb + 1;
        const float s = fmaxf(div_exact(time - ep.delay, ep.dtau), 0.0f);
        if (s > (float)c.len_factor) atomicOr(flag, 1);
        const size_t idx = (size_t)max(min((int)rintf(div_exact(s, ep.dsdt)), c.n_pc - 1), 0);
        const double* row = c.tab + 4 * n_pc + idx * K;
        const double y1 = c.tab[idx], y2 = c.tab[n_pc + idx];
        const double xi1 = fma(ep.bca, y1, -(ep.bcb * y2)), xi2 = fma(ep.bcc, y2, -(ep.bcd * y1));
        const int nw = c.disable_weights ? 0 : c.nb;
        double eg = 0.0, egs = 0.0;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            e[k] = 0.0;
            if (k <= c.nb) {
                const double raw = row[k] - xi1 * ep.pb[k] - xi2 * ep.vb[k];
                const double scaled = raw * sc[k];
                if (k == c.nb) { eg = raw; egs = scaled; }
                else if (k < nw) e[k] = scaled;
            }
        }
        if (!c.disable_goal) {
#pragma unroll
            for (int k = 0; k < KS; ++k)
                if (k == nw) e[k] = egs;
        }
        ca = xi1 + (c.relative_goal ? (c.relgoal_before_scale ? eg * sc[KS] : eg) : 0.0);
        cb = xi2 * (double)ep.tau;
        cc = c.goal_off_on ? eg * (double)c.goal_offset : 0.0;
    } else {
        const double* sCen = reinterpret_cast<const double*>(consts);
        const double x = phase_f64(c, time, ep.taud, ep.delay, ExpLiteral());
        float h[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) h[k] = 0.0f;
        rbf_row<KS>(c, sCen, sCen + c.n_total, x, (double)c.ws, h, ExpLiteral());
#pragma unroll
        for (int k = 0; k < KS; ++k) e[k] = k < c.nb ? (double)h[k] : 0.0;
        ca = c.KT > c.nb ? 1.0 : 0.0;
    }
}

// a ProMP's normalised RBF row at phase x in float64 (weights_scale folded in; exact 0 beyond nb): rbf_row's direct-exponential
// arithmetic without its rounding to float32 -- for rows that are DIFFERENCED (cond_promp_vel_row says why)
__device__ __forceinline__ void phase_rows_rbf64(const DevCfg& c, const double* cen, const double* bw, double x,
                                                 double (&e)[kPhaseRowSlots]) {
    double sum = 0.0;
    for (int i = 0; i < c.n_total; ++i) {
        const double dx = x - cen[i];
        sum += exp_nonpos(-(dx * dx * bw[i]) * 0.5);
    }
    const double scale = c.n_total > 1 ? div_pos((double)c.ws, sum) : (double)c.ws;
#pragma unroll
    for (int k = 0; k < kPhaseRowSlots; ++k) {
        e[k] = 0.0;
        if (k < c.nb) {
            const double dx = x - cen[c.zs + k];
            e[k] = exp_nonpos(-(dx * dx * bw[c.zs + k]) * 0.5) * scale;
        }
    }
}

// the VELOCITY row of step t (sBT: the base times phase_rows_stage staged), regrouped as phase_rows_eval regroups the position row:
// ev[k] the entry of local parameter k, and the given part cv[t, d] = cva init_pos[d] + cvb init_vel[d] + cvc -- the row of the
// velocity the forward returns for this episode at this step.
//   promp   the forward difference of the position rows of steps (t, t + 1) -- (T - 2, T - 1) at the last step, which repeats the
//           difference before it -- times the forward's float32 reciprocal time step.  Two FLOAT64 rows are differenced
//           (phase_rows_rbf64): the difference of two float32-rounded rows carries their rounding amplified by |row| / |difference|
//           (profiles/r20_traj_condition.md).  A zero-padded basis' init_pos is constant over the steps: cva = 0.
//   prodmp  phase_rows_eval's regrouping on the derivative tables: dPsi_k (vel_basis) for Psi_k and (dy1, dy2) for (y1, y2) at the
//           step, the boundary row and the column scales as they are, everything times the forward's float32 1 / tau.
template <int MP>
__device__ __forceinline__ void phase_rows_eval_vel(const DevCfg& c, const PhaseEpisode& ep, const float* consts, const float* sBT, int t,
                                                    int32_t* flag, double (&ev)[kPhaseRowSlots], double& cva, double& cvb, double& cvc) {
    constexpr int KS = kPhaseRowSlots;
    cva = 0.0; cvb = 0.0; cvc = 0.0;
    if (MP == MPK_MP_PRODMP) {
        const double* sc = reinterpret_cast<const double*>(consts);
        const size_t n_pc = (size_t)c.n_pc, K = (size_t)c.nb + 1;
        const float time = sBT[t] + ep.it;
        const float s = fmaxf(div_exact(time - ep.delay, ep.dtau), 0.0f);
        if (s > (float)c.len_factor) atomicOr(flag, 1);
        const size_t idx = (size_t)max(min((int)rintf(div_exact(s, ep.dsdt)), c.n_pc - 1), 0);
        const double* row = c.tab + 4 * n_pc + n_pc * K + idx * K;          // dPsi_k at the step
        const double dy1 = c.tab[2 * n_pc + idx], dy2 = c.tab[3 * n_pc + idx];
        const double xi3 = fma(ep.bca, dy1, -(ep.bcb * dy2)), xi4 = fma(ep.bcc, dy2, -(ep.bcd * dy1));
        const double itau = (double)ep.dtau.r;
        const int nw = c.disable_weights ? 0 : c.nb;
        double eg = 0.0, egs = 0.0;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            ev[k] = 0.0;
            if (k <= c.nb) {
                const double raw = (row[k] - xi3 * ep.pb[k] - xi4 * ep.vb[k]) * itau;
                const double scaled = raw * sc[k];
                if (k == c.nb) { eg = raw; egs = scaled; }
                else if (k < nw) ev[k] = scaled;
            }
        }
        if (!c.disable_goal) {
#pragma unroll
            for (int k = 0; k < KS; ++k)
                if (k == nw) ev[k] = egs;
        }
        cva = xi3 * itau + (c.relative_goal ? (c.relgoal_before_scale ? eg * sc[KS] : eg) : 0.0);
        cvb = xi4 * (double)ep.tau * itau;
        cvc = c.goal_off_on ? eg * (double)c.goal_offset : 0.0;
    } else {
        const double* sCen = reinterpret_cast<const double*>(consts);
        const int th = t < c.T - 1 ? t + 1 : c.T - 1, tl = t < c.T - 1 ? t : c.T - 2;
        const float rdt = 1.0f / ((sBT[th] + ep.it) - (sBT[tl] + ep.it));
        double lo[KS];
        phase_rows_rbf64(c, sCen, sCen + c.n_total, phase_f64(c, sBT[th] + ep.it, ep.taud, ep.delay, ExpLiteral()), ev);
        phase_rows_rbf64(c, sCen, sCen + c.n_total, phase_f64(c, sBT[tl] + ep.it, ep.taud, ep.delay, ExpLiteral()), lo);
#pragma unroll
        for (int k = 0; k < KS; ++k) ev[k] = (ev[k] - lo[k]) * (double)rdt;
    }
}

}  // namespace mpk
