// k_demo_log_prob: the log-likelihood of WHOLE demonstrations [B, T, D] under a Gaussian over the MP parameters, and its gradient
// (mpk_demonstration_log_prob, mpk_demonstration_log_prob_vjp) -- the information (Pl x Pl) form, for n >> Pl
#include "mpk_demo_gram.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// Notation is mpk_traj_log_prob.hip's: w ~ N(mu, L L^T) over the Pl = D Kloc non-phase parameters; the observation (t, d) reads
// y = psi_t . w_d + c_td + eps, eps ~ N(0, sigma_td^2), psi_t the POSITION table row of step t on the parameter columns (the values
// cond_obs_row<MP>(.., o = 0, k, t) gives k_traj_log_prob), c what init_pos / init_vel / the goal offset contribute.  An observation is
// kept when 0 < sigma < +inf (+inf, NaN, negative: removed -- missing samples, prefixes).  With w = 1 / sigma^2 on kept entries and 0
// elsewhere, n the number kept, r = y - c - psi . mu_d:
//     G_d = sum_t w_td psi_t psi_t^T  [Kloc x Kloc]    q_d = sum_t w_td psi_t r_td    s = sum w r^2    lsig = sum over kept of log sigma^2
//     M = I + tril(L)^T blockdiag(G_d) tril(L) = C C^T      v = tril(L)^T q      z = C^-1 v
//     log_prob = -1/2 (s - z.z) - 1/2 (lsig + 2 sum log C_ii) - n / 2 log 2 pi
// which is log N(y; H mu + c, A A^T + diag(sigma^2)), A = H tril(L), by the Woodbury identity and the determinant lemma: the n x n
// covariance (700 x 700 for 7 DoF x 100 steps) is never formed, and neither is L L^T.  Gradients for an upstream g, with x = M^-1 v,
// X = G tril(L), gm = q - X x (= H^T S^-1 r):
//     g_params[off + .] = g gm        g_params_L = g tril(gm (tril(L)^T gm)^T - X M^-1)
// k_demo_log_prob<MP, NS, GRAD>: one wave per episode, `waves` of them a workgroup (sized at launch from the LDS the images need), all
// float64, NS = ceil(Pl / 64) rows or columns per lane.
//   * The T position rows [T][KT] are staged once per workgroup (cond_obs_row, o = 0), and the table column of every local parameter
//     (kof, the inverse of x_kind), as k_traj_log_prob stages them.
//   * In chunks of tc steps: lane <-> (t, d), pos and obs_std read coalesced; w and r go to an LDS image [tc][D] each, s / lsig / n stay
//     in the lane (summed over the wave by a fixed xor ladder at the end).  Then lane <-> packed entry (d, k >= l) of the Gram matrices and
//     lane <-> row of q, each a chain over the chunk's steps in ascending t.
//   * Per DoF d: the Kloc rows of tril(L)'s block d to a float32 LDS image (entries j <= row only: the strict upper triangle is never
//     read); X_d = G_d tril(L)[rows of d] [Kloc][ld] with lane <-> column; v += that block's part of tril(L)^T q; the rank-Kloc update
//     of the packed lower triangle of M, row by row with lane <-> column.  A DoF with nothing kept is skipped: G_d = 0, q_d = 0.
//   * A left-looking Cholesky in place (lane <-> row), the forward substitution with z in registers, two xor-ladder sums.  GRAD = false
//     ends here.
//   * GRAD: back substitution -> x; tril(L) x row by row (lane <-> column, an xor-ladder sum per row); gm; u = tril(L)^T gm (lane <->
//     column); then per DoF X_d again, its Kloc rows solved against C (forward, backward; lane <-> row of the system, the Kloc right-hand
//     sides in the LDS image), and that DoF's rows of g_params_L leave: g (gm_row u_j - W[k][j]) for j <= row, exact 0 for j > row, exact
//     0 for the rows of a DoF with nothing kept.  There is never a Pl x Pl image besides the packed C, so the backward fits wherever the
//     forward does; nothing is kept from the forward launch.
// n = 0: exactly 0.0 and zero gradients.  A sigma == 0 cannot be expressed in this form: the episode's log_prob, its g_params local block
// and the lower triangle of its g_params_L are NaN (mpk_trajectory_log_prob takes exact observations); so is an episode with a pivot that is
// not > 0 (non-finite input).  No atomics, an episode never leaves its wave, nothing depends on an address, and no index depends on a value
// that is read: the same bits from run to run, for any alignment, alone or in a batch; non-finite inputs never fault.
// LDS per wave: 8 (Pl (Pl + 1) / 2 + D Kloc^2 + 2 Pl + max(Kloc ld, 2 tc D)) + 4 Kloc ld + 64 bytes, ld = Pl | 1; per workgroup 8 T KT + 64.
// ------------------------------------------------------------------------------------------------------------
// the arguments both kernels of the information form read (mpk_demo_gram.h), and this one's own
struct DemoLogProbArgs : DemoGramArgs {
    double* log_prob;      // [B] out (forward)
    const double* g;       // [B] the upstream gradient (GRAD)
    float* g_params;       // [B, P] out or nullptr (GRAD)
    float* g_L;            // [B, Pl, Pl] out or nullptr (GRAD)
};

template <int MP, int NS, bool GRAD, bool PHASE>
__global__ void __launch_bounds__(256) k_demo_log_prob(const DemoLogProbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double demo_smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int D = c.D, Kloc = c.Kloc, Pl = a.Pl, ld = a.ld;
    const int KK = Kloc * Kloc;
    const DemoImages im = demo_images(a, demo_smem, wave);
    double* sC = im.sC;                                             // packed lower triangle: M, then its Cholesky factor C
    double* sG = im.sG;                                             // [D][Kloc][Kloc] the Gram matrices
    double* sq = im.sq;                                             // [Pl] q
    double* sy = im.sy;                                             // [Pl] mu, then tril(L) x, then gm
    double* sX = im.sX;                                             // [Kloc][ld] X_d, then X_d M^-1; the accumulation's w | r [tc][D]
    float* sL = im.sL;                                              // [Kloc][ld] the rows of tril(L)'s block d
    int* snd = im.snd;                                              // [D] kept observations per DoF
    if (PHASE) {                                                    // row constants, base times [T]
        phase_rows_stage<MP>(c, im.sK, im.sBT, tid, (int)blockDim.x);
        __syncthreads();
    } else {
        demo_stage_tables<MP>(a, im, tid);                          // rows [T][KT], kof [Kloc]
    }
    const double nan = __builtin_nan("");
    for (int b = blockIdx.x * a.waves + wave; b < a.B; b += gridDim.x * a.waves) {
        const float* Lb = a.L + (size_t)b * Pl * Pl;
        // ---- w, r, then G, q over the steps, a chunk at a time (mpk_demo_gram.h)
        const DemoSums sm = demo_accumulate<MP, true, PHASE>(a, im, b, lane);
        const double ssum = sm.s, lsig = sm.lsig;
        const int n = sm.n;
        bool bad = sm.zero;                                         // (wave-uniform) a sigma == 0, or a pivot that was not > 0
        double rr[NS], dg[NS];                                      // lane + 64 s <-> row i: v_i -> z_i -> x_i; C[i][i]
#pragma unroll
        for (int s = 0; s < NS; ++s) { rr[s] = 0.0; dg[s] = 1.0; }
        if (n > 0 && !bad) {
            // ---- M = I + sum_d tril(L)_d^T G_d tril(L)_d (packed lower triangle), v = tril(L)^T q
            demo_build_M<NS>(a, im, Lb, lane, rr);
            // ---- M = C C^T in place, left-looking (lane + 64 s <-> row)
            for (int jc = 0; jc < Pl; ++jc) {
                const double* cj = sC + jc * (jc + 1) / 2;
                double sv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    sv[s] = 0.0;
                    if (i >= jc && i < Pl) {
                        const int mine = i * (i + 1) / 2;
                        // four accumulators in a fixed order: with one wave on a CU a single chain waits out every LDS round trip
                        double x0 = sC[mine + jc], x1 = 0.0, x2 = 0.0, x3 = 0.0;
                        int k = 0;
                        for (; k + 3 < jc; k += 4) {
                            x0 = __builtin_fma(-sC[mine + k], cj[k], x0);
                            x1 = __builtin_fma(-sC[mine + k + 1], cj[k + 1], x1);
                            x2 = __builtin_fma(-sC[mine + k + 2], cj[k + 2], x2);
                            x3 = __builtin_fma(-sC[mine + k + 3], cj[k + 3], x3);
                        }
                        for (; k < jc; ++k) x0 = __builtin_fma(-sC[mine + k], cj[k], x0);
                        sv[s] = (x0 + x1) + (x2 + x3);
                    }
                }
                const double piv = demo_bcast<NS>(sv, jc);
                const bool ok = piv > 0.0;                          // (wave-uniform) a NaN is not
                bad = bad || !ok;
                const double root = ok ? sqrt(piv) : nan;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    if (i >= jc && i < Pl) sC[i * (i + 1) / 2 + jc] = i == jc ? root : sv[s] / root;
                }
                cond_wave_sync();
            }
            // ---- z = C^-1 v (column by column)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int i = lane + 64 * s;
                if (i < Pl) dg[s] = sC[i * (i + 1) / 2 + i];
            }
            for (int j = 0; j < Pl; ++j) {
                const double zj = demo_bcast<NS>(rr, j) / demo_bcast<NS>(dg, j);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    if (i == j) rr[s] = zj;
                    else if (i > j && i < Pl) rr[s] = __builtin_fma(-sC[i * (i + 1) / 2 + j], zj, rr[s]);
                }
            }
        }
        const bool live = n > 0 && !bad;                            // (wave-uniform)
        if (!GRAD) {
            double zz = 0.0, lg = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int i = lane + 64 * s;
                if (i < Pl) { zz = __builtin_fma(rr[s], rr[s], zz); lg += log(dg[s]); }
            }
            const double quad = ssum - demo_wave_sum(zz);
            const double logs = demo_wave_sum(lg);
            double lp = 0.0;
            if (bad) lp = nan;
            else if (n > 0) lp = -0.5 * quad - 0.5 * lsig - logs - (double)n * 0.91893853320467274178;   // 1/2 log 2 pi
            if (lane == 0) a.log_prob[b] = lp;
        } else {
            const double gb = a.g[b];
            double u[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) u[s] = 0.0;
            if (live) {
                // ---- x = C^-T z (row by row from the last)
                for (int j = Pl - 1; j >= 0; --j) {
                    const double xj = demo_bcast<NS>(rr, j) / demo_bcast<NS>(dg, j);
                    const double* cj = sC + j * (j + 1) / 2;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int i = lane + 64 * s;
                        if (i == j) rr[s] = xj;
                        else if (i < j) rr[s] = __builtin_fma(-cj[i], xj, rr[s]);
                    }
                }
                // ---- tril(L) x, row by row (lane <-> column), over mu's place
                for (int row = 0; row < Pl; ++row) {
                    double part = 0.0;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = lane + 64 * s;
                        if (j <= row) part = __builtin_fma((double)Lb[(size_t)row * Pl + j], rr[s], part);
                    }
                    const double tot = demo_wave_sum(part);
                    if (lane == 0) sy[row] = tot;
                }
                cond_wave_sync();
                // ---- gm = q - G (tril(L) x), in its place
                double gm[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int row = lane + 64 * s;
                    gm[s] = 0.0;
                    if (row < Pl) {
                        const int d = row / Kloc, k = row - d * Kloc;
                        double acc = 0.0;
                        for (int l = 0; l < Kloc; ++l) acc = __builtin_fma(sG[d * KK + k * Kloc + l], sy[d * Kloc + l], acc);
                        gm[s] = sq[row] - acc;
                    }
                }
                cond_wave_sync();
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int row = lane + 64 * s;
                    if (row < Pl) sy[row] = gm[s];
                }
                cond_wave_sync();
                // ---- u = tril(L)^T gm (lane <-> column)
                for (int row = 0; row < Pl; ++row) {
                    const double gr = sy[row];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = lane + 64 * s;
                        if (j <= row) u[s] = __builtin_fma((double)Lb[(size_t)row * Pl + j], gr, u[s]);
                    }
                }
            }
            if (a.g_params) {
                for (int p = lane; p < c.P; p += 64) {
                    const int row = p - c.off;
                    float out = 0.0f;
                    if (row >= 0 && row < Pl) {
                        if (bad) out = (float)nan;
                        else if (n > 0 && snd[row / Kloc] > 0) out = (float)(gb * sy[row]);
                    }
                    a.g_params[(size_t)b * c.P + p] = out;
                }
            }
            if (a.g_L) {
                float* Go = a.g_L + (size_t)b * Pl * Pl;
                for (int d = 0; d < D; ++d) {
                    const bool any = live && __builtin_amdgcn_readfirstlane(snd[d]) > 0;   // (wave-uniform)
                    if (any) {
                        // ---- W = X_d M^-1: the Kloc rows of X_d against C, forward then backward (lane + 64 s <-> row of the system)
                        demo_stage_block<NS>(Lb, sG + d * KK, sL, sX, d, Kloc, Pl, ld, lane);
                        for (int j = 0; j < Pl; ++j) {
                            const double cjj = sC[j * (j + 1) / 2 + j];
                            if (lane < Kloc) sX[lane * ld + j] = sX[lane * ld + j] / cjj;
                            cond_wave_sync();
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const int i = lane + 64 * s;
                                if (i > j && i < Pl) {
                                    const double cij = sC[i * (i + 1) / 2 + j];
                                    for (int k = 0; k < Kloc; ++k) sX[k * ld + i] = __builtin_fma(-cij, sX[k * ld + j], sX[k * ld + i]);
                                }
                            }
                            cond_wave_sync();
                        }
                        for (int j = Pl - 1; j >= 0; --j) {
                            const double* cj = sC + j * (j + 1) / 2;
                            const double cjj = cj[j];
                            if (lane < Kloc) sX[lane * ld + j] = sX[lane * ld + j] / cjj;
                            cond_wave_sync();
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const int i = lane + 64 * s;
                                if (i < j) {
                                    const double cji = cj[i];
                                    for (int k = 0; k < Kloc; ++k) sX[k * ld + i] = __builtin_fma(-cji, sX[k * ld + j], sX[k * ld + i]);
                                }
                            }
                            cond_wave_sync();
                        }
                    }
                    // ---- this DoF's rows leave, rounded once
                    for (int k = 0; k < Kloc; ++k) {
                        const int row = d * Kloc + k;
                        const double gr = any ? sy[row] : 0.0;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int j = lane + 64 * s;
                            if (j < Pl) {
                                float out = 0.0f;
                                if (j <= row) {
                                    if (bad) out = (float)nan;
                                    else if (any) out = (float)(gb * (gr * u[s] - sX[k * ld + j]));
                                }
                                Go[(size_t)row * Pl + j] = out;
                            }
                        }
                    }
                    cond_wave_sync();
                }
            }
        }
        cond_wave_sync();                                           // the images are free again
    }
}

#ifndef MPK_DEVICE_ONLY
// the shapes the kernels of the information form take; MPK_ENOTIMPL with the limit in the message, under the entry's name fn, otherwise
// (no HIP call)
static int demo_limits(const DevCfg& c, bool phase, DemoPlan* plan, const char* fn) {
    if (const int rc = gauss_common_limits(c, fn)) return rc;
    const std::string name(fn);
    const size_t Pl = (size_t)c.D * c.Kloc;
    if (Pl > (size_t)64 * kDemoSlots) {
        set_error(name + ": at most " + std::to_string(64 * kDemoSlots) + " non-phase parameters (this handle: " +
                  std::to_string(c.D) + " DoF x " + std::to_string(c.Kloc) + " = " + std::to_string(Pl) + ")");
        return MPK_ENOTIMPL;
    }
    if (phase) {
        // the row evaluation of mpk_phase_rows.h: 16 slots (a ProDMP: weights, goal and the two boundary columns, as k_traj_phase)
        const bool prodmp = c.mp_type == MPK_MP_PRODMP;
        const int need = prodmp ? c.nb + 3 : c.KT;
        if (need > kPhaseRowSlots || c.Kloc > kPhaseRowSlots || c.D < 1 || !c.tab) {
            set_error(name + ": at most " + std::to_string(kMaxD) + " DoF and " + std::to_string(kMaxKP) +
                      " table columns (this handle: " + std::to_string(c.D) + " DoF, " + std::to_string(need) +
                      " columns); the per-episode rows are those of the wave kernel k_traj_phase");
            return MPK_ENOTIMPL;
        }
    }
    const size_t ld = Pl | 1;
    size_t tc = (size_t)c.Kloc * ld / (2 * (size_t)(c.D > 0 ? c.D : 1));
    if (tc < 32) tc = 32;
    if (tc > (size_t)c.T) tc = c.T > 0 ? c.T : 1;
    const size_t xw = (size_t)c.Kloc * ld, ch = 2 * tc * c.D;
    const size_t scratch = xw > ch ? xw : ch;
    // the per-episode route: a chunk image [tc][sl] per wave; the workgroup keeps row constants and base times, no [T][KT] image
    const size_t sl = phase ? (size_t)(c.Kloc + 3) | 1 : 0, chunk = tc * sl;
    const size_t c_pad = phase ? (size_t)phase_rows_const_floats(c) : 0, t_pad = ((size_t)c.T + 3) / 4 * 4;
    const size_t wave_doubles = Pl * (Pl + 1) / 2 + (size_t)c.D * c.Kloc * c.Kloc + 2 * Pl + scratch + (xw + 1) / 2 + 8 + chunk;
    const size_t shared = phase ? (c_pad + t_pad) * sizeof(float) + 64 : (size_t)c.T * c.KT * sizeof(double) + 64;
    if (wave_doubles * sizeof(double) + shared > kLdsPerCu) {
        set_error(name + ": the float64 images of " + std::to_string(Pl) + " parameters and " + std::to_string(c.T) +
                  " steps (" + std::to_string(wave_doubles * sizeof(double) + shared) + " bytes with one wave per workgroup) do not "
                  "fit the CU's " + std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    if (plan) {
        const WavePlan wp = gauss_wave_plan(wave_doubles, shared);
        plan->lds = wp.lds;
        plan->waves = wp.waves; plan->wave_doubles = (int)wave_doubles; plan->tc = (int)tc; plan->scratch = (int)scratch;
        plan->sl = (int)sl; plan->chunk = (int)chunk; plan->c_pad = (int)c_pad;
    }
    return MPK_OK;
}

int demo_log_prob_limits(const DevCfg& c, DemoPlan* plan, const char* fn) { return demo_limits(c, false, plan, fn); }

// the per-episode-phase route's limits: the same images plus the chunk image per wave, row constants and base times per workgroup
int demo_phase_limits(const DevCfg& c, DemoPlan* plan, const char* fn) { return demo_limits(c, true, plan, fn); }

void demo_plan_args(const DemoPlan& plan, DemoGramArgs* la) {
    la->waves = plan.waves; la->wave_doubles = plan.wave_doubles; la->tc = plan.tc; la->scratch = plan.scratch;
    la->sl = plan.sl; la->chunk = plan.chunk; la->c_pad = plan.c_pad;
}

int launch_demo_log_prob(const DevCfg& c, const SharedTables& st, const DemoLogProbLaunch& q, int num_cu, void* stream,
                         const char** kernel_name) {
    DemoLogProbArgs la{};
    DemoPlan plan;
    const bool phase = q.obs.phase, grad = q.out.grad;
    const int rc = phase ? demo_phase_limits(c, &plan, grad ? "mpk_demonstration_phase_log_prob_vjp" : "mpk_demonstration_phase_log_prob")
                         : demo_log_prob_limits(c, &plan);
    if (rc != MPK_OK) return rc;
    demo_plan_args(plan, &la);
    const size_t lds = plan.lds;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    la.flag = q.obs.range_flag;
    la.c = c; la.A = st.A; la.aux = st.aux; la.TS = st.TS; la.init_time = q.in.init_time;
    la.params = q.in.params; la.L = q.in.params_L; la.init_pos = q.in.init_pos; la.init_vel = q.in.init_vel;
    la.pos = q.obs.pos; la.sd = q.obs.obs_std;
    la.log_prob = q.out.log_prob; la.g = q.out.g; la.g_params = q.out.g_params; la.g_L = q.out.g_params_L;
    la.B = q.in.B; la.Pl = c.D * c.Kloc; la.ld = la.Pl | 1;
    const int blocks = gauss_blocks(q.in.B, la.waves, lds, num_cu);
    static const char* const names[2][2][2] = {
        {{"k_demo_log_prob<prodmp>", "k_demo_log_prob<promp>"}, {"k_demo_log_prob<prodmp, grad>", "k_demo_log_prob<promp, grad>"}},
        {{"k_demo_log_prob<prodmp, phase>", "k_demo_log_prob<promp, phase>"},
         {"k_demo_log_prob<prodmp, phase, grad>", "k_demo_log_prob<promp, phase, grad>"}}};
    *kernel_name = names[phase][grad][promp];
    return dispatch_flag(phase, [&](auto ph) {
        return dispatch_flag(grad, [&](auto gr) {
            return dispatch_mp(promp, [&](auto mp) {
                return dispatch_ns((la.Pl + 63) / 64, [&](auto ns) {
                    // (Pl > 192 passes neither route's LDS limit; the per-episode route does not carry the instantiation)
                    if constexpr (ph.value && ns.value == 4) {
                        set_error("mpk_demonstration_phase_log_prob: internal: more than 192 non-phase parameters passed the LDS limit");
                        return (int)MPK_ENOTIMPL;
                    } else {
                        return launch_kernel(k_demo_log_prob<mp.value, ns.value, gr.value, ph.value>, dim3(blocks), dim3(64 * la.waves), lds,
                                             stream, la);
                    }
                });
            });
        });
    });
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
