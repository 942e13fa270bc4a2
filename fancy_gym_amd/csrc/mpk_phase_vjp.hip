// k_phase_vjp: the vector-Jacobian product of the per-episode-phase trajectory map (learned tau / delay, per-episode init_time) for
// ProMP and ProDMP, one launch (include/mpk.h: mpk_trajectory_phase_vjp).  Gradient convention: the pathwise gradient with ProDMP's
// integer table indices held (g_delay = 0 exactly), torch.clamp's mask on tau / delay (1 inside the closed bounds, 0 outside) and the
// one-sided masks of the phase clips.
#include "mpk_dev.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// One WAVE per episode, lane <-> time step, 64 steps a round -- k_traj_phase's map, so a lane recomputes ITS row with the forward's
// device functions and nothing of the forward launch is stored:
//   prodmp  the clipped tau / delay, div_exact, the rintf index and the rows32 gather of k_traj_phase; the row is the forward's
//           [(Psi_k, dPsi_k) .. | (xi1, xi3) (xi2, xi4)] and the episode's columns are its [wg_k .. | r1 r2] (regrouped form)
//   promp   the float64 phase and RBF evaluation (rbf_row's operations in rbf_row's order: the forward's row values) plus the row's
//           derivative w.r.t. the phase, phi'_k = phi_k (u_k - sum_j phi_j u_j) over all n_total columns of the normalisation
// Per lane and DoF the products row[k] * g[t, d] are summed over the rounds into KS fp32 accumulators (a lane sees ceil(T / 64) terms),
// for at most DG = 64 / KS DoF at a time (more DoF: further passes over the horizon, rows recomputed); the lane sums of the 64
// accumulators then meet in a float64 halving butterfly (wave_transpose_sum: a fixed tree) that leaves accumulator i in lane i, and the
// episode's outputs leave through an LDS image of [g_params | g_init_pos | g_init_vel] as plain coalesced stores.  The gradient rows are read as dwords, t * D + d: the same
// loads, the same order and the same bits whatever the alignment of g_pos / g_vel.  An episode never leaves its wave; no atomics but
// the forward's range flag.  Outputs no column reads (a disabled block, the delay of a ProDMP, init_vel of a ProMP) are the image's
// zeros.
// ------------------------------------------------------------------------------------------------------------
struct PhaseVjpArgs {
    DevCfg c;
    const float* params;
    const float* init_pos;
    const float* init_vel;
    const float* init_time;
    float init_time_shared;
    const float* g_pos;     // [B, T, D] or nullptr
    const float* g_vel;     // [B, T, D] or nullptr
    float* g_params;        // [B, P] or nullptr
    float* g_init_pos;      // [B, D] or nullptr
    float* g_init_vel;      // [B, D] or nullptr
    int32_t* flag;          // prodmp: raised beyond the pre-computed range
    int B;
    int c_pad, t_pad, wave_floats;      // floats: centres | base times (per workgroup), columns + output image (per wave)
};

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the row of rbf_row (same operations, same order: same bits) and its derivative w.r.t. the phase value x, both times weights_scale;
// column nb of a zero-padded basis: 1 and 0
template <int KS, class CF>
__device__ __forceinline__ void rbf_row_grad(const DevCfg& c, const double* cen, const double* bw, const double x, float (&h)[KS],
                                             float (&hd)[KS], const CF& cf) {
    const double mul = (double)c.ws;
    double sum = 0.0, su = 0.0;
    if (c.rbf_uniform) {
        RbfRecur s1(cen, bw, c.n_total, x, cf);
        for (int k = 0; k < c.n_total; ++k) {
            const double e = s1.next();
            sum += e;
            su += e * (-bw[k] * (x - cen[k]));
        }
    } else {
        for (int k = 0; k < c.n_total; ++k) {
            const double dx = x - cen[k];
            const double e = exp_nonpos(-(dx * dx * bw[k]) * 0.5, cf);
            sum += e;
            su += e * (-bw[k] * dx);
        }
    }
    const bool norm = c.rbf_uniform || c.n_total > 1;
    const double scale = norm ? div_pos(mul, sum) : mul;
    const double ubar = norm ? div_pos(su, sum) : 0.0;
    double re = 0.0, rr = 0.0, rq = 0.0;                    // the second recurrence, at column zs
    if (c.rbf_uniform) {
        RbfRecur s2(cen, bw, c.n_total, x, cf);
        for (int k = 0; k < c.zs; ++k) (void)s2.next();
        re = s2.e; rr = s2.r; rq = s2.q;
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        h[k] = 0.0f; hd[k] = 0.0f;
        if (k < c.nb) {
            const double dx = x - cen[c.zs + k];
            double e = re;
            if (c.rbf_uniform) { re *= rr; rr *= rq; }
            else e = exp_nonpos(-(dx * dx * bw[c.zs + k]) * 0.5, cf);
            const double v = e * scale;
            h[k] = (float)v;
            hd[k] = (float)(v * (-bw[c.zs + k] * dx - ubar));
        } else if (k == c.nb && c.KT > c.nb) {
            h[k] = 1.0f;
        }
    }
}

// 64 per-lane accumulators -> the wave total of accumulator i in lane i: a butterfly that HALVES what a lane carries at every stage
// (the lane keeps the half its bit selects, sends the other half to its partner and adds what the partner sends: 32 + 16 + .. + 1
// exchanges instead of 64 x 6).  The first exchange moves the fp32 lane sums, every addition is float64; a + b is commutative, so the
// total does not depend on which lane formed it: a fixed summation tree.
template <int M>
__device__ __forceinline__ void halve_stage(double (&w)[32], const int lane) {
    const bool hi = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const double keep = hi ? w[i + M] : w[i], send = hi ? w[i] : w[i + M];
        w[i] = keep + __shfl_xor(send, M, 64);
    }
}
__device__ __forceinline__ double wave_transpose_sum(const float (&v)[64], const int lane) {
    double w[32];
    const bool hi = (lane & 32) != 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float keep = hi ? v[i + 32] : v[i], send = hi ? v[i] : v[i + 32];
        w[i] = (double)keep + (double)__shfl_xor(send, 32, 64);
    }
    halve_stage<16>(w, lane); halve_stage<8>(w, lane); halve_stage<4>(w, lane); halve_stage<2>(w, lane); halve_stage<1>(w, lane);
    return w[0];
}

template <int MP, int KQ>
__global__ void __launch_bounds__(256) k_phase_vjp(const PhaseVjpArgs a) {
    static_assert(MP == MPK_MP_PROMP || MP == MPK_MP_PRODMP, "promp / prodmp");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevCfg& c = a.c;
    constexpr int KS = KQ * 4, DG = 64 / KS, kRow = 2 * KS + 4;
    constexpr bool PRODMP = MP == MPK_MP_PRODMP;
    const int lane = threadIdx.x & 63;
    const int wave = wave_of(threadIdx.x);
    const int wpb = (int)(blockDim.x >> 6);
    const int D = c.D, T = c.T, P = c.P, TD = T * D;
    double* sCen = reinterpret_cast<double*>(smem);         // promp: [2 n_total + 3] centres | bandwidths | recurrence constants
    float* sWgs = smem;                                     // prodmp: [KS] column scales (0: no parameter) | the goal scale
    float* sBT = smem + a.c_pad;                            // [t_pad] base times
    float* sX = sBT + a.t_pad + (size_t)wave * a.wave_floats;   // [D][KS] the episode's columns
    float* sOut = sX + D * KS;                              // [P | D | D] g_params, g_init_pos, g_init_vel of the episode
    for (int t = threadIdx.x; t < T; t += blockDim.x) sBT[t] = c.base_times[t];
    if (PRODMP) {
        const double* S = c.tab + 4 * (size_t)c.n_pc + 2 * (size_t)c.n_pc * (c.nb + 1);
        const int tid = (int)threadIdx.x;
        if (tid < KS) {
            const bool off = tid < c.nb ? c.disable_weights != 0 : (tid == c.nb ? c.disable_goal != 0 : true);
            sWgs[tid] = off ? 0.0f : (float)S[tid];
        }
        if (tid == KS) sWgs[KS] = (float)S[c.nb];
    } else {
        for (int k = threadIdx.x; k < 2 * c.n_total + 3; k += blockDim.x) sCen[k] = c.tab[k];
    }
    __syncthreads();
    const float* const rows = c.rows32;
    const int row_max = c.n_pc - 1;
    const ExactDiv dsdt = make_exact_div(c.scaled_dt);
    const int nw = PRODMP ? (c.disable_weights ? 0 : c.nb) : c.nb;
    const int n_out = P + 2 * D;

    for (int b = (int)blockIdx.x * wpb + wave; b < a.B; b += (int)gridDim.x * wpb) {
        const float* prm = a.params + (size_t)b * P;
        // np.clip(action, low, high) as the forward; the mask is torch.clamp's: 1 on the closed interval
        float tau = c.tau, delay = c.delay;
        bool m_tau = false, m_delay = false;
        if (c.learn_tau) {
            const float raw = prm[0];
            tau = fminf(fmaxf(raw, c.tau_lo), c.tau_hi);
            m_tau = raw >= c.tau_lo && raw <= c.tau_hi;
        }
        if (c.learn_delay) {
            const float raw = prm[c.learn_tau ? 1 : 0];
            delay = fminf(fmaxf(raw, c.delay_lo), c.delay_hi);
            m_delay = raw >= c.delay_lo && raw <= c.delay_hi;
        }
        const float it = a.init_time ? a.init_time[b] : a.init_time_shared;
        const ExactDiv dtau = make_exact_div(tau);
        const float inv_tau = dtau.r;
        for (int i = lane; i < n_out; i += 64) sOut[i] = 0.0f;
        // ---- the episode's columns (prodmp: the forward's per-(episode, DoF) block, one lane per DoF)
        const float* rb = rows;
        if (PRODMP) {
            const float sbl = fmaxf(div_exact(it - delay, dtau), 0.0f);
            rb = rows + (size_t)min((int)rintf(div_exact(sbl, dsdt)), row_max) * kRow;
            if (lane < D) {
                const float yb = a.init_pos[(size_t)b * D + lane], ydb = a.init_vel[(size_t)b * D + lane];
                const float* loc = prm + c.off + lane * c.Kloc;
                const float rawg = c.disable_goal ? 0.0f : loc[nw];
                float wgg = c.disable_goal ? 0.0f : rawg * sWgs[KS];
                if (c.relative_goal) wgg = c.relgoal_before_scale ? (rawg + yb) * sWgs[KS] : wgg + yb;
                if (c.goal_off_on) wgg = wgg + c.goal_offset;
                double pb = 0.0, vb = 0.0;
                float* xf = sX + lane * KS;
#pragma unroll
                for (int k = 0; k < KS - 2; ++k) {
                    float wg = k < nw ? loc[k] * sWgs[k] : 0.0f;
                    wg = k == c.nb ? wgg : wg;
                    pb += (double)rb[2 * k] * (double)wg;
                    vb += (double)rb[2 * k + 1] * (double)wg;
                    xf[k] = wg;
                }
                xf[KS - 2] = (float)((double)yb - pb);
                xf[KS - 1] = (float)((double)(tau * ydb) - vb);
            }
        } else {
            for (int i = lane; i < D * KS; i += 64) {
                const int dd = i / KS, k = i - dd * KS;
                sX[i] = k < c.nb ? prm[c.off + dd * c.Kloc + k] : 0.0f;
            }
        }
        __builtin_amdgcn_wave_barrier();
        double bca = 0.0, bcb = 0.0, bcc = 0.0, bcd = 0.0;
        if (PRODMP) {
            const double* yb4 = reinterpret_cast<const double*>(rb + 2 * KS - 4);
            const double y1b = yb4[0], y2b = yb4[1], dy1b = yb4[2], dy2b = yb4[3];
            const double idet = div_pos(1.0, y1b * dy2b - y2b * dy1b);
            bca = dy2b * idet; bcb = dy1b * idet; bcc = y1b * idet; bcd = y2b * idet;
        }
        const PosDiv taud = make_pos_div((double)tau);
        const float* gp0 = a.g_pos ? a.g_pos + (size_t)b * TD : nullptr;
        const float* gv0 = a.g_vel ? a.g_vel + (size_t)b * TD : nullptr;
        // per lane: prodmp sum_t,d g_vel / tau * (tau vel); promp sum_t g_x dx/ds (-s / tau) and sum_t g_x dx/ds (-1 / tau)
        double s_tau = 0.0, s_delay = 0.0;
        double g_tau_bc = 0.0;                              // prodmp: ydot_b[d] G2[d] in the lane that holds G2[d]

        for (int d0 = 0; d0 < D; d0 += DG) {
            float acc[64];                                  // [DG][KS]
#pragma unroll
            for (int i = 0; i < 64; ++i) acc[i] = 0.0f;
            for (int r0 = 0; r0 < T; r0 += 64) {
                const bool live = r0 + lane < T;
                const int t = live ? r0 + lane : T - 1;
                const float time = sBT[t] + it;
                float h[KS], hv[KS];       // prodmp: (Psi_k .. xi1 xi2), (dPsi_k .. xi3 xi4); promp: the RBF row, its derivative
                double dxds_tau = 0.0, dxds_delay = 0.0;
                float rdt0 = 0.0f, rdt1 = 0.0f;
                if (PRODMP) {
                    const float s = fmaxf(div_exact(time - delay, dtau), 0.0f);
                    if (s > (float)c.len_factor) atomicOr(a.flag, 1);
                    const int idx = min((int)rintf(div_exact(s, dsdt)), row_max);
                    const float4* row = reinterpret_cast<const float4*>(rows + (size_t)idx * kRow);
#pragma unroll
                    for (int j = 0; j < (2 * KS - 4) / 4; ++j) {
                        const float4 q4 = row[j];
                        h[2 * j] = q4.x; hv[2 * j] = q4.y; h[2 * j + 1] = q4.z; hv[2 * j + 1] = q4.w;
                    }
                    const double* y4 = reinterpret_cast<const double*>(row + (2 * KS - 4) / 4);
                    const double y1 = y4[0], y2 = y4[1], dy1 = y4[2], dy2 = y4[3];
                    h[KS - 2] = (float)fma(bca, y1, -(bcb * y2));
                    hv[KS - 2] = (float)fma(bca, dy1, -(bcb * dy2));
                    h[KS - 1] = (float)fma(bcc, y2, -(bcd * y1));
                    hv[KS - 1] = (float)fma(bcc, dy2, -(bcd * dy1));
                } else {
                    const double s = div_pos((double)time - (double)delay, taud);
                    double x, dxds;
                    if (c.phase_type == MPK_PHASE_LINEAR) {
                        x = fmin(fmax(s, 0.0), 1.0);
                        dxds = s > 0.0 && s < 1.0 ? 1.0 : 0.0;
                    } else {
                        x = exp_nonpos(-(double)c.alpha_phase * fmax(s, 0.0), ExpLiteral());
                        dxds = s > 0.0 ? -(double)c.alpha_phase * x : 0.0;
                    }
                    rbf_row_grad<KS>(c, sCen, sCen + c.n_total, x, h, hv, ExpLiteral());
                    dxds_tau = -(dxds * s) * taud.y;
                    dxds_delay = -dxds * taud.y;
                    // the forward's 1 / (time[t + 1] - time[t]) of the differences that end and start at this step
                    if (t >= 1) rdt0 = 1.0f / (time - (sBT[t - 1] + it));
                    if (t <= T - 2) rdt1 = 1.0f / ((sBT[t + 1] + it) - time);
                }
                double gx = 0.0;
                float sv = 0.0f;
#pragma unroll
                for (int j = 0; j < DG; ++j) {
                    const int d = d0 + j;
                    if (d >= D) continue;                  // (uniform)
                    float gp = 0.0f, gv = 0.0f;
                    if (live) {
                        if (gp0) gp = gp0[t * D + d];
                        if (gv0) {
                            if (PRODMP) {
                                gv = gv0[t * D + d] * inv_tau;
                            } else {
                                // transpose of vel[t] = (pos[t + 1] - pos[t]) rdt, vel[T - 1] = vel[T - 2]
                                if (t >= 1) {
                                    float u = gv0[(t - 1) * D + d];
                                    if (t == T - 1) u += gv0[t * D + d];
                                    gp += u * rdt0;
                                }
                                if (t <= T - 2) {
                                    float u = gv0[t * D + d];
                                    if (t == T - 2) u += gv0[(t + 1) * D + d];
                                    gp -= u * rdt1;
                                }
                            }
                        }
                    }
                    float x[KS];
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        const float4 v = *reinterpret_cast<const float4*>(sX + d * KS + 4 * q);
                        x[4 * q + 0] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
                    }
                    float vn = 0.0f;        // prodmp: tau vel[t, d]; promp: d pos[t, d] / d x
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        acc[j * KS + k] = fmaf(h[k], gp, acc[j * KS + k]);
                        if (PRODMP) acc[j * KS + k] = fmaf(hv[k], gv, acc[j * KS + k]);
                        vn = fmaf(hv[k], x[k], vn);
                    }
                    if (PRODMP) sv = fmaf(gv, vn, sv);
                    else gx += (double)gp * (double)vn;
                }
                if (PRODMP) {
                    s_tau += (double)sv;
                } else {
                    s_tau += gx * dxds_tau;
                    s_delay += gx * dxds_delay;
                }
            }
            // ---- the lane sums -> wave totals, lane j KS + k holds (DoF d0 + j, column k) and writes it into the episode's output image
            const double tot = wave_transpose_sum(acc, lane);
            const int k = lane & (KS - 1), d = d0 + lane / KS;
            float* gl = sOut + c.off + d * c.Kloc;
            if (PRODMP) {
                const int first = lane & ~(KS - 1);
                const double G1 = __shfl(tot, first + KS - 2, 64), G2 = __shfl(tot, first + KS - 1, 64);
                if (d < D && k < KS - 2) {
                    const double gwg = tot - (double)rb[2 * k] * G1 - (double)rb[2 * k + 1] * G2;
                    if (k < nw) gl[k] = (float)(gwg * (double)sWgs[k]);
                    if (k == c.nb) {
                        if (!c.disable_goal) gl[nw] = (float)(gwg * (double)sWgs[KS]);
                        double gip = G1;
                        if (c.relative_goal) gip += c.relgoal_before_scale ? gwg * (double)sWgs[KS] : gwg;
                        sOut[P + d] = (float)gip;
                    }
                }
                if (d < D && k == KS - 1) {
                    sOut[P + D + d] = (float)((double)tau * G2);
                    g_tau_bc += (double)a.init_vel[(size_t)b * D + d] * G2;
                }
            } else if (d < D) {
                if (k < c.nb) gl[k] = (float)tot;
                else if (k == c.nb && c.KT > c.nb) sOut[P + d] = (float)tot;
            }
        }
        // prodmp: d / d tau of r2 = tau ydot_b - .. and of the 1 / tau of vel; the table indices are held: nothing reaches the delay
        const double t_tau = wave_sum64(PRODMP ? g_tau_bc - s_tau * (double)inv_tau : s_tau), t_delay = wave_sum64(s_delay);
        if (lane == 0) {
            if (c.learn_tau) sOut[0] = m_tau ? (float)t_tau : 0.0f;
            if (c.learn_delay && !PRODMP) sOut[c.learn_tau ? 1 : 0] = m_delay ? (float)t_delay : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        if (a.g_params)
            for (int i = lane; i < P; i += 64) a.g_params[(size_t)b * P + i] = sOut[i];
        if (a.g_init_pos && lane < D) a.g_init_pos[(size_t)b * D + lane] = sOut[P + lane];
        if (a.g_init_vel && lane < D) a.g_init_vel[(size_t)b * D + lane] = sOut[P + D + lane];
        __builtin_amdgcn_wave_barrier();
    }
}

#ifndef MPK_DEVICE_ONLY
// ---- launch_phase_vjp: the route (plan_phase_vjp: arithmetic only, no HIP call) and ONE launch of what it names
struct PhaseVjpRoute {
    int mp, kq;
    long blocks;
    int threads;
    size_t lds;
    const char* name;       // what mpk_last_kernel reports: static storage
};
constexpr int kPhaseVjpWaves = 4;       // waves per workgroup
constexpr int kPhaseVjpPerCu = 8;       // resident workgroups per CU the grid is cut to

// the shapes of the wave kernel k_traj_phase (plan_traj_phase's rules) with <= kMaxD DoF; MPK_ENOTIMPL with the error text set otherwise
static int plan_phase_vjp(const DevCfg& c, int num_cu, PhaseVjpArgs& pa, PhaseVjpRoute& r) {
    if (c.mp_type == MPK_MP_DMP) {
        set_error("mpk_trajectory_phase_vjp: a DMP with a per-episode phase is an Euler recurrence in the scaled time, which this "
                  "kernel does not transpose (promp / prodmp only)");
        return MPK_ENOTIMPL;
    }
    const bool prodmp = c.mp_type == MPK_MP_PRODMP;
    if (!prodmp && c.T < 2) {
        set_error("mpk_trajectory_phase_vjp: promp with one time step has no finite-difference velocity");
        return MPK_ENOTIMPL;
    }
    const int need = prodmp ? c.nb + 3 : c.KT;
    const int KQ = need <= 4 && !prodmp ? 1 : (need <= 8 ? 2 : 4), KS = KQ * 4;
    const bool rows_ok = !prodmp || (c.rows32 && c.rows32_stride == 2 * KS + 4);
    if (need > 16 || c.D > kMaxD || c.D * KS > 256 || !rows_ok || c.P > 320) {
        set_error("mpk_trajectory_phase_vjp: the shapes of the wave kernel k_traj_phase only (<= 16 DoF, DoF x padded columns <= 256, "
                  "<= 16 columns, <= 320 parameters per episode)");
        return MPK_ENOTIMPL;
    }
    pa.t_pad = (c.T + 3) / 4 * 4;
    pa.c_pad = prodmp ? KS + 4 : (4 * c.n_total + 6 + 3) / 4 * 4;
    pa.wave_floats = (c.D * KS + c.P + 2 * c.D + 3) / 4 * 4;
    r = PhaseVjpRoute{};
    r.mp = c.mp_type; r.kq = KQ;
    r.threads = 64 * kPhaseVjpWaves;
    r.lds = (size_t)(pa.c_pad + pa.t_pad + kPhaseVjpWaves * pa.wave_floats) * sizeof(float);
    if (r.lds > kLdsPerCu) {
        set_error("mpk_trajectory_phase_vjp: the horizon's time grid does not fit the LDS");
        return MPK_ENOTIMPL;
    }
    int per_cu = (int)(kLdsPerCu / r.lds);
    per_cu = per_cu > kPhaseVjpPerCu ? kPhaseVjpPerCu : per_cu;
    const long units = ((long)pa.B + kPhaseVjpWaves - 1) / kPhaseVjpWaves;
    r.blocks = units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu;
    r.name = prodmp ? "k_phase_vjp<prodmp>" : "k_phase_vjp<promp>";
    return MPK_OK;
}

static int launch_phase_vjp_route(const PhaseVjpArgs& pa, const PhaseVjpRoute& r, void* stream, const char** kernel_name) {
    auto go = [&](auto kern) { return launch_kernel(kern, dim3((unsigned)r.blocks), dim3(r.threads), r.lds, stream, pa); };
    *kernel_name = r.name;
    if (r.mp == MPK_MP_PROMP) {
        if (r.kq == 1) return go(k_phase_vjp<MPK_MP_PROMP, 1>);
        return r.kq == 2 ? go(k_phase_vjp<MPK_MP_PROMP, 2>) : go(k_phase_vjp<MPK_MP_PROMP, 4>);
    }
    return r.kq == 2 ? go(k_phase_vjp<MPK_MP_PRODMP, 2>) : go(k_phase_vjp<MPK_MP_PRODMP, 4>);
}

int launch_phase_vjp(const DevCfg& c, const PhaseVjpLaunch& q, int num_cu, void* stream, const char** kernel_name) {
    PhaseVjpArgs pa{};
    pa.c = c;
    pa.params = q.params; pa.init_pos = q.init_pos; pa.init_vel = q.init_vel; pa.init_time = q.init_time;
    pa.init_time_shared = q.init_time_shared;
    pa.g_pos = q.g_pos; pa.g_vel = q.g_vel; pa.g_params = q.g_params; pa.g_init_pos = q.g_init_pos; pa.g_init_vel = q.g_init_vel;
    pa.flag = q.range_flag; pa.B = q.B;
    PhaseVjpRoute r;
    const int rc = plan_phase_vjp(c, num_cu, pa, r);
    return rc != MPK_OK ? rc : launch_phase_vjp_route(pa, r, stream, kernel_name);
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
