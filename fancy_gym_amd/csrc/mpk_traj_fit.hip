// k_traj_fit_tile / k_phase_fit: the regularised least-squares fit of the trajectory map to demonstrated positions, for a shared phase
// (mpk_trajectory_fit) and for a per-episode phase (mpk_trajectory_phase_fit)
#include "mpk_tile.h"
#include "mpk_run_stage.h"
#include "mpk_vjp_row.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// With a phase all episodes share, pos[b, t, d] = sum_k R0[k][t] x[b, d][k] (mpk_traj_vjp.hip has the whole story).  x_kind (mpk_tile.h, the
// forward's own gather) splits the columns of x into FITTED ones -- those that are read from params: p, in the user's units, the
// scales, the relative goal and the zero padding are folded into the table's rows -- and GIVEN ones: init_pos, init_vel and the
// constant goal-offset column.  Columns that are neither (a disabled block, padding) do not exist.  With G = R0 R0^T the Gram matrix
// of the rows the forward kernels read (float32 values, summed in float64 on the host: fit_factor_build), the fit of one (episode,
// DoF) is
//   (G_ff + reg I) p = R0_f y - G_fg x_g
// k_traj_fit_tile<MP>: k_traj_vjp_tile's contraction with the demonstration in the gradient's place, accumulated in float64
// (v_mfma_f64_16x16x4_f64: M = column, K = four time steps, N = (episode, DoF); C / D layout row = (lane >> 4) + 4 reg, column = lane & 15),
// then, inside the launch,
//   * the four lanes of a tile column exchange their rows (each holds the column's 16 sums),
//   * subtract the given-columns cross term G_fg x_g,
//   * solve with the Cholesky factor L of G_ff + reg I -- L z = r, L^T p = z -- in float64 (the factor is written in the table's own
//     16 column slots, identity where a column is not fitted, so no index map is needed; its diagonal is stored inverted),
//   * scatter p through the transpose of x_kind into params (vjp_scatter), rounded to float32 once.
// The factor is the same for the whole batch: 320 doubles [L 16 x 16 | G_fg 16 x 3 | fitted 16] built once per (handle, init_time,
// reg) and staged into LDS per workgroup.  Deterministic: an episode never leaves its wave, a tile column depends on no other
// column, plain stores, no atomics; the image staging (mpk_run_stage.h) makes the bits independent of the alignment of pos.
// LDS per workgroup: 2560 + 64 TP + 16 NTW stride bytes (cfg2: 2.5 + 6.4 + 23 KB).
// ------------------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kFitL = 0, kFitG = 256, kFitMask = 304, kFitFac = 320;      // doubles

struct FitArgs {
    DevCfg c;
    const float* A;        // [n_out][KP][TS] (k_build_shared); the position rows are read
    const float* aux;
    int TS;
    const float* pos;      // [B, T, D] the demonstrations
    const float* init_pos; // [B, D] or nullptr (no column reads it)
    const float* init_vel; // [B, D] or nullptr
    float* params;         // [B, P] out
    const double* fac;     // [kFitFac]
    int B, sh, G;
    int TP;                // T rounded up to 4
    int stride;            // floats per episode image in LDS
};

template <int MP>
__global__ void __launch_bounds__(256) k_traj_fit_tile(const FitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int T = c.T, D = c.D, TD = T * D, TP = a.TP, NCH = TP >> 2;
    const int NTW = 16 >> a.sh, DP = 1 << a.sh;
    double* sFac = reinterpret_cast<double*>(smem);                 // [kFitFac]
    float* sAt = smem + 2 * kFitFac;                                // [TP][16]
    float* img = sAt + TP * 16 + wave * (NTW * a.stride);           // [NTW][stride]
    for (int i = tid; i < kFitFac; i += 256) sFac[i] = a.fac[i];
    for (int i = tid; i < 16 * TP; i += 256) {                      // t fastest: coalesced table reads
        const int k = i / TP, t = i - k * TP;
        sAt[t * 16 + k] = (t < T && k < c.KT) ? vjp_row<MP>(a.c, a.A, a.aux, a.TS, 0, k, t) : 0.0f;
    }
    __syncthreads();
    const int col = lane & 15, q = lane >> 4;
    const int bl = col >> a.sh, d = col & (DP - 1);
    const bool dvalid = d < D;
    const float* at = sAt + q * 16 + col;
    const double* sL = sFac + kFitL;
    const int KT = c.KT;
    for (int g = blockIdx.x * 4 + wave; g < a.G; g += gridDim.x * 4) {
        const int b0 = g * NTW;
        for (int e = 0; e < NTW; ++e) {
            const int bb = b0 + e;
            if (bb >= a.B) break;
            stage_run(img + e * a.stride, a.pos, bb, TD, TP * D, lane);
        }
        // (a wave's LDS operations complete in issue order: the barrier keeps the compiler from moving the reads above the writes)
        __builtin_amdgcn_wave_barrier();
        const int bb = b0 + bl;
        const bool lv = dvalid && bb < a.B;
        const int bs = lv ? bb : b0;
        const float* ip = img + (lv ? bl * a.stride + q * D + d : 0) + run_shift(a.pos, bs, TD);
        // ---- contraction over time, float64, two independent chains
        f64x4 s0 = {0.0, 0.0, 0.0, 0.0}, s1 = s0;
        const int D4 = 4 * D;
        int ch = 0;
        for (; ch + 1 < NCH; ch += 2) {
            const float x0 = lv ? ip[ch * D4] : 0.0f, x1 = lv ? ip[(ch + 1) * D4] : 0.0f;
            s0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)at[ch * 64], (double)x0, s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)at[(ch + 1) * 64], (double)x1, s1, 0, 0, 0);
        }
        if (ch < NCH) s0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)at[ch * 64], (double)(lv ? ip[ch * D4] : 0.0f), s0, 0, 0, 0);
        const f64x4 acc = s0 + s1;                                  // rows q + 4 r of this lane's (episode, DoF) column
        // ---- all 16 rows of the column in each of its four lanes
        double v[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) v[qq + 4 * r] = __shfl(acc[r], qq * 16 + col, 64);
        // ---- the given columns' cross term; columns that are not fitted carry 0
        const double yb = (lv && a.init_pos) ? (double)a.init_pos[(size_t)bb * D + d] : 0.0;
        const double vb = (lv && a.init_vel) ? (double)a.init_vel[(size_t)bb * D + d] : 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double* gk = sFac + kFitG + 3 * k;
            const double cross = fma(gk[0], yb, fma(gk[1], vb, gk[2]));
            v[k] = sFac[kFitMask + k] != 0.0 ? v[k] - cross : 0.0;
        }
        // ---- L z = r
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < KT) {
                double s = v[i];
#pragma unroll
                for (int j = 0; j < i; ++j) s = fma(-sL[i * 16 + j], v[j], s);
                v[i] = s * sL[i * 16 + i];
            }
        }
        // ---- L^T p = z
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            if (i < KT) {
                double s = v[i];
#pragma unroll
                for (int j = i + 1; j < 16; ++j) s = fma(-sL[j * 16 + i], v[j], s);
                v[i] = s * sL[i * 16 + i];
            }
        }
        // ---- transposed gather: the column's four lanes store four rows each
        if (lv) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((k & 3) == q && k < KT) vjp_scatter<MP>(c, k, bb, d, (float)v[k], a.params, nullptr, nullptr);
        }
        // the images are free again (in-order completion of a wave's LDS operations keeps the next group's writes behind these reads)
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_phase_fit<MP, KQ>: the same fit for a PER-EPISODE phase (learned tau / delay, per-episode init_time) of a ProMP or a ProDMP
// (mpk_trajectory_phase_fit).  Every episode has its own Psi, hence its own Gram matrix: one WAVE per episode, lane <-> time step,
// 64 steps a round -- k_phase_vjp's map, the lane's row recomputed with the forward's device functions:
//   promp   phase_f64 and rbf_row: the forward's row values (weights_scale folded in); a zero-padded basis adds init_pos (given).
//   prodmp  the clipped tau / delay, div_exact, the rintf index and the rows32 gather of k_traj_phase.  The forward contracts
//           [Psi_k .. | xi1 xi2] with [wg_k .. | y_b - sum Psi_k(t_b) wg_k, tau v_b - sum dPsi_k(t_b) wg_k]; regrouped by parameter the
//           row of wg_k is Psi_k - xi1 Psi_k(t_b) - xi2 dPsi_k(t_b), times the column's scale; init_pos gets xi1 (plus the goal's row
//           under relative_goal), init_vel tau xi2, the goal offset the goal's row: the given part c.
// A round's rows [64][KS] and residuals y - c [64][D] go to the wave's LDS in float64; then lane <-> OUTPUT ENTRY: each lane owns up to
// three entries of the lower Gram triangle (KS (KS + 1) / 2 <= 136) and up to four of Psi^T (y - c) (KS D <= 256) and adds the round's
// 64 terms to them in float64 in ascending step order -- a fixed order, no atomics, nothing leaves the wave.  Then, in the wave: the
// Cholesky factor of Gram + reg I column by column (lane <-> row; slots that are not fitted carry the identity), the D pairs of
// triangular solves (lane <-> DoF), and plain stores of the episode's params row: the phase_params as given in front (unclipped; the
// fit is the one at the clipped values), then p.  An episode whose pivot is not positive in float64 gets a NaN row and sets *status.
// ------------------------------------------------------------------------------------------------------------
struct PhaseFitArgs {
    DevCfg c;
    const float* pos;           // [B, T, D]
    const float* phase;         // [B, n_phase] tau / delay as they stand at the front of params, or nullptr (n_phase = 0)
    const float* init_pos;      // [B, D] or nullptr (promp)
    const float* init_vel;      // [B, D] or nullptr (promp)
    const float* init_time;     // [B] or nullptr: init_time_shared
    float init_time_shared;
    double reg;
    float* params;              // [B, P] out
    int32_t* flag;              // prodmp: raised beyond the pre-computed range
    int32_t* status;            // set to 1 by an episode whose Gram + reg I is not positive definite
    int B;
    int c_pad, t_pad, wave_doubles;
};

template <int MP, int KQ>
__global__ void __launch_bounds__(256) k_phase_fit(const PhaseFitArgs a) {
    static_assert(MP == MPK_MP_PROMP || MP == MPK_MP_PRODMP, "promp / prodmp");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevCfg& c = a.c;
    constexpr int KS = KQ * 4, kRow = 2 * KS + 4, RS = KS + 1;
    constexpr int NG = (KS * (KS + 1) / 2 + 63) / 64;       // Gram entries a lane owns
    constexpr bool PRODMP = MP == MPK_MP_PRODMP;
    const int lane = threadIdx.x & 63;
    const int wave = wave_of(threadIdx.x);
    const int wpb = (int)(blockDim.x >> 6);
    const int D = c.D, T = c.T, P = c.P, TD = T * D;
    double* sCen = reinterpret_cast<double*>(smem);         // promp: [2 n_total + 3] centres | bandwidths | recurrence constants
    float* sWgs = smem;                                     // prodmp: [KS] column scales (0: not fitted) | the goal scale
    float* sBT = smem + a.c_pad;                            // [t_pad] base times
    double* sW = reinterpret_cast<double*>(sBT + a.t_pad) + (size_t)wave * a.wave_doubles;
    double* sE = sW;                                        // [64][KS] the round's rows
    double* sR = sE + 64 * KS;                              // [64][D] the round's residuals y - c
    double* sM = sR + 64 * D;                               // [KS][KS] Gram, then its factor (diagonal inverted)
    double* sP = sM + KS * KS;                              // [16][KS + 1] Psi^T (y - c), then p
    double* sY = sP + 16 * RS;                              // [2][16] init_pos | init_vel
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
    // the output entries of this lane: Gram (gi, gj), gj <= gi, and right-hand side (DoF rd, slot rk)
    int gi[NG], gj[NG];
#pragma unroll
    for (int m = 0; m < NG; ++m) {
        const int e = lane + 64 * m;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        gi[m] = i < KS ? i : -1;
        gj[m] = e - i * (i + 1) / 2;
    }
    const int n_rhs = D * KS;
    // (entries this lane does not own accumulate element 0 and are never written: the round loop stays free of branches)
    int gis[NG], gjs[NG], rks[4], rds[4];
#pragma unroll
    for (int m = 0; m < NG; ++m) { gis[m] = gi[m] >= 0 ? gi[m] : 0; gjs[m] = gi[m] >= 0 ? gj[m] : 0; }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int idx = lane + 64 * m;
        rks[m] = idx < n_rhs ? idx % KS : 0;
        rds[m] = idx < n_rhs ? idx / KS : 0;
    }

    for (int b = (int)blockIdx.x * wpb + wave; b < a.B; b += (int)gridDim.x * wpb) {
        // np.clip(action, low, high) as the forward
        float tau = c.tau, delay = c.delay;
        if (c.learn_tau) tau = fminf(fmaxf(a.phase[(size_t)b * c.off], c.tau_lo), c.tau_hi);
        if (c.learn_delay) delay = fminf(fmaxf(a.phase[(size_t)b * c.off + (c.learn_tau ? 1 : 0)], c.delay_lo), c.delay_hi);
        const float it = a.init_time ? a.init_time[b] : a.init_time_shared;
        const ExactDiv dtau = make_exact_div(tau);
        const float* rb = rows;
        double bca = 0.0, bcb = 0.0, bcc = 0.0, bcd = 0.0;
        if (PRODMP) {
            const float sbl = fmaxf(div_exact(it - delay, dtau), 0.0f);
            rb = rows + (size_t)min((int)rintf(div_exact(sbl, dsdt)), row_max) * kRow;
            const double* yb4 = reinterpret_cast<const double*>(rb + 2 * KS - 4);
            const double y1b = yb4[0], y2b = yb4[1], dy1b = yb4[2], dy2b = yb4[3];
            const double idet = div_pos(1.0, y1b * dy2b - y2b * dy1b);
            bca = dy2b * idet; bcb = dy1b * idet; bcc = y1b * idet; bcd = y2b * idet;
        }
        if (lane < 16) {
            sY[lane] = (lane < D && a.init_pos) ? (double)a.init_pos[(size_t)b * D + lane] : 0.0;
            sY[16 + lane] = (lane < D && a.init_vel) ? (double)a.init_vel[(size_t)b * D + lane] : 0.0;
        }
        const PosDiv taud = make_pos_div((double)tau);
        const float* y0 = a.pos + (size_t)b * TD;
        double accG[NG], accR[4];
#pragma unroll
        for (int m = 0; m < NG; ++m) accG[m] = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) accR[m] = 0.0;
        __builtin_amdgcn_wave_barrier();

        for (int r0 = 0; r0 < T; r0 += 64) {
            const bool live = r0 + lane < T;
            const int t = live ? r0 + lane : T - 1;
            const float time = sBT[t] + it;
            double e[KS];
            double ca = 0.0, cb = 0.0, cc = 0.0;    // c[t, d] = ca init_pos[d] + cb init_vel[d] + cc
            if (PRODMP) {
                const float s = fmaxf(div_exact(time - delay, dtau), 0.0f);
                if (s > (float)c.len_factor) atomicOr(a.flag, 1);
                const int idx = min((int)rintf(div_exact(s, dsdt)), row_max);
                const float4* row = reinterpret_cast<const float4*>(rows + (size_t)idx * kRow);
                float h[KS];
#pragma unroll
                for (int j = 0; j < (2 * KS - 4) / 4; ++j) {
                    const float4 q4 = row[j];
                    h[2 * j] = q4.x; h[2 * j + 1] = q4.z;
                }
                const double* y4 = reinterpret_cast<const double*>(row + (2 * KS - 4) / 4);
                const double y1 = y4[0], y2 = y4[1];
                const double xi1 = (double)(float)fma(bca, y1, -(bcb * y2)), xi2 = (double)(float)fma(bcc, y2, -(bcd * y1));
                double eg = 0.0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    e[k] = 0.0;
                    if (k < KS - 2) {
                        const double raw = (double)h[k] - xi1 * (double)rb[2 * k] - xi2 * (double)rb[2 * k + 1];
                        e[k] = raw * (double)sWgs[k];
                        if (k == c.nb) eg = raw;
                    }
                }
                ca = xi1 + (c.relative_goal ? (c.relgoal_before_scale ? eg * (double)sWgs[KS] : eg) : 0.0);
                cb = xi2 * (double)tau;
                cc = c.goal_off_on ? eg * (double)c.goal_offset : 0.0;
            } else {
                const double x = phase_f64(c, time, taud, delay, ExpLiteral());
                float h[KS];
#pragma unroll
                for (int k = 0; k < KS; ++k) h[k] = 0.0f;
                rbf_row<KS>(c, sCen, sCen + c.n_total, x, (double)c.ws, h, ExpLiteral());
#pragma unroll
                for (int k = 0; k < KS; ++k) e[k] = k < c.nb ? (double)h[k] : 0.0;
                ca = c.KT > c.nb ? 1.0 : 0.0;
            }
#pragma unroll
            for (int k = 0; k < KS; ++k) sE[lane * KS + k] = live ? e[k] : 0.0;
            for (int d = 0; d < D; ++d)
                sR[lane * D + d] = live ? (double)y0[t * D + d] - fma(ca, sY[d], fma(cb, sY[16 + d], cc)) : 0.0;
            __builtin_amdgcn_wave_barrier();
            // lane <-> output entry: the round's 64 terms in ascending step order
#pragma unroll 4
            for (int s = 0; s < 64; ++s) {
                const double* es = sE + s * KS;
#pragma unroll
                for (int m = 0; m < NG; ++m) accG[m] = fma(es[gis[m]], es[gjs[m]], accG[m]);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (64 * m >= n_rhs) break;             // (uniform)
                    accR[m] = fma(es[rks[m]], sR[s * D + rds[m]], accR[m]);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- Gram + reg I in the table's slots (identity where a slot is not fitted), right-hand sides
#pragma unroll
        for (int m = 0; m < NG; ++m) {
            if (gi[m] < 0) continue;
            const int i = gi[m], j = gj[m];
            const bool fit_i = PRODMP ? sWgs[i] != 0.0f && i <= c.nb : i < c.nb;
            double v = accG[m];
            if (i == j) v = fit_i ? v + a.reg : 1.0;
            sM[i * KS + j] = v;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int idx = lane + 64 * m;
            if (idx < n_rhs) sP[(idx / KS) * RS + idx % KS] = accR[m];
        }
        __builtin_amdgcn_wave_barrier();
        // ---- Cholesky, column by column: lane <-> row
        bool bad = false;
        for (int j = 0; j < KS; ++j) {
            double s = 0.0;
            if (lane < KS && lane >= j) {
                s = sM[lane * KS + j];
                for (int k = 0; k < j; ++k) s = fma(-sM[lane * KS + k], sM[j * KS + k], s);
            }
            const double piv = __shfl(s, j, 64);
            bad = bad || !(piv > 0.0);
            const double ljj = sqrt(piv);
            __builtin_amdgcn_wave_barrier();
            if (lane == j) sM[j * KS + j] = 1.0 / ljj;
            else if (lane > j && lane < KS) sM[lane * KS + j] = s / ljj;
            __builtin_amdgcn_wave_barrier();
        }
        // ---- L z = r, L^T p = z: lane <-> DoF
        if (lane < D) {
            double* r = sP + lane * RS;
            for (int i = 0; i < KS; ++i) {
                double s = r[i];
                for (int j = 0; j < i; ++j) s = fma(-sM[i * KS + j], r[j], s);
                r[i] = s * sM[i * KS + i];
            }
            for (int i = KS - 1; i >= 0; --i) {
                double s = r[i];
                for (int j = i + 1; j < KS; ++j) s = fma(-sM[j * KS + i], r[j], s);
                r[i] = s * sM[i * KS + i];
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the episode's params row: the phase parameters as given, then p through the forward's packing
        float* out = a.params + (size_t)b * P;
        if (lane < c.off) out[lane] = a.phase[(size_t)b * c.off + lane];
        for (int idx = lane; idx < n_rhs; idx += 64) {
            const int d = idx / KS, k = idx - d * KS;
            int loc = -1;
            if (PRODMP) {
                if (k < c.nb && !c.disable_weights) loc = k;
                else if (k == c.nb && !c.disable_goal) loc = nw;
            } else if (k < c.nb) {
                loc = k;
            }
            if (loc >= 0) out[c.off + d * c.Kloc + loc] = bad ? __builtin_nanf("") : (float)sP[d * RS + k];
        }
        if (bad && lane == 0) *a.status = 1;
        __builtin_amdgcn_wave_barrier();
    }
}

#ifndef MPK_DEVICE_ONLY
template <int MP>
static void fit_kinds(const DevCfg& c, int (&kind)[16]) {
    for (int k = 0; k < 16; ++k) {
        int loc;
        kind[k] = k < c.KT ? x_kind<MP>(c, k, &loc) : XK_ZERO;
    }
}

// rows: the position rows [KP][TS] of the launch's table as the device holds them (float32).  fac: [kFitFac] out.
int fit_factor_build(const DevCfg& c, const float* rows, int TS, double reg, double* fac) {
    int kind[16];
    if (c.mp_type == MPK_MP_PROMP) fit_kinds<MPK_MP_PROMP>(c, kind);
    else fit_kinds<MPK_MP_PRODMP>(c, kind);
    double G[16][16] = {};
    for (int i = 0; i < c.KT; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int t = 0; t < c.T; ++t) s += (double)rows[(size_t)i * TS + t] * (double)rows[(size_t)j * TS + t];
            G[i][j] = G[j][i] = s;
        }
    for (int i = 0; i < kFitFac; ++i) fac[i] = 0.0;
    double M[16][16] = {};
    int n_fit = 0;
    for (int i = 0; i < 16; ++i) {
        const bool fi = kind[i] == XK_PARAM;
        n_fit += fi ? 1 : 0;
        fac[kFitMask + i] = fi ? 1.0 : 0.0;
        for (int j = 0; j < 16; ++j) {
            const bool fj = kind[j] == XK_PARAM;
            M[i][j] = (fi && fj) ? G[i][j] + (i == j ? reg : 0.0) : (i == j ? 1.0 : 0.0);
            if (fi && kind[j] != XK_PARAM && kind[j] != XK_ZERO) {
                const int slot = kind[j] == XK_IPOS ? 0 : (kind[j] == XK_IVEL ? 1 : 2);
                fac[kFitG + 3 * i + slot] += G[i][j];
            }
        }
    }
    if (n_fit != c.Kloc) {
        set_error("mpk_trajectory_fit: internal: the table's parameter columns do not cover the local parameter block");
        return MPK_EINVAL;
    }
    // Cholesky, lower, float64
    double L[16][16] = {};
    for (int j = 0; j < 16; ++j) {
        double s = M[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0)) {
            set_error("mpk_trajectory_fit: the Gram matrix plus reg * I is not positive definite in float64 (pivot " + std::to_string(j) +
                      " = " + std::to_string(s) + "): reg = " + std::to_string(reg) + " is too small for this basis, raise reg");
            return MPK_EINVAL;
        }
        const double ljj = std::sqrt(s);
        L[j][j] = ljj;
        for (int i = j + 1; i < 16; ++i) {
            double u = M[i][j];
            for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k];
            L[i][j] = u / ljj;
        }
    }
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j <= i; ++j) fac[kFitL + i * 16 + j] = i == j ? 1.0 / L[i][i] : L[i][j];
    return MPK_OK;
}

int fit_factor_doubles() { return kFitFac; }

// the shapes the tile route takes; MPK_ENOTIMPL with the limit in the message otherwise (no HIP call)
int traj_fit_limits(const DevCfg& c, size_t* lds_out, int* sh_out, int* stride_out) {
    if (c.mp_type == MPK_MP_DMP) {
        set_error("mpk_trajectory_fit: a DMP handle is fitted through its response rows only (<= 16 DoF, <= 13 basis functions, alpha ds "
                  "<= 1, dmp_first_sample = init, option \"dmp_response\" not 0)");
        return MPK_ENOTIMPL;
    }
    if (c.D > kMaxD || c.KP > kMaxKP) {
        set_error("mpk_trajectory_fit: at most " + std::to_string(kMaxD) + " DoF and " + std::to_string(kMaxKP) + " table columns (this handle: " +
                  std::to_string(c.D) + " DoF, " + std::to_string(c.KT) + " columns); the k_traj_wide shapes have no fit kernel");
        return MPK_ENOTIMPL;
    }
    int sh = 0;
    while ((1 << sh) < c.D) ++sh;
    const int NTW = 16 >> sh, TP = (c.T + 3) / 4 * 4;
    const long st_ = run_image_stride(TP, c.D, NTW);
    const size_t bytes = (size_t)kFitFac * sizeof(double) + ((size_t)TP * 16 + (size_t)4 * NTW * st_) * sizeof(float);
    if (bytes > kLdsPerCu) {
        set_error("mpk_trajectory_fit: the horizon's demonstration images (" + std::to_string(bytes) + " bytes for " + std::to_string(c.T) +
                  " steps x " + std::to_string(c.D) + " DoF) do not fit the CU's " + std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    if (lds_out) *lds_out = bytes;
    if (sh_out) *sh_out = sh;
    if (stride_out) *stride_out = (int)st_;
    return MPK_OK;
}

int launch_traj_fit(const DevCfg& c, const SharedTables& st, const double* fac, const float* pos, const float* init_pos,
                    const float* init_vel, float* params, int B, int num_cu, void* stream, const char** kernel_name) {
    FitArgs fa{};
    size_t lds = 0;
    const int rc = traj_fit_limits(c, &lds, &fa.sh, &fa.stride);
    if (rc != MPK_OK) return rc;
    fa.c = c; fa.A = st.A; fa.aux = st.aux; fa.TS = st.TS;
    fa.pos = pos; fa.init_pos = init_pos; fa.init_vel = init_vel; fa.params = params; fa.fac = fac;
    fa.B = B;
    const int NTW = 16 >> fa.sh;
    fa.G = (B + NTW - 1) / NTW;
    fa.TP = (c.T + 3) / 4 * 4;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    const int per_cu = (int)(kLdsPerCu / lds) < 1 ? 1 : ((int)(kLdsPerCu / lds) > 8 ? 8 : (int)(kLdsPerCu / lds));
    const long units = ((long)fa.G + 3) / 4;
    const int blocks = (int)(units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu);
    auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(256), lds, stream, fa); };
    *kernel_name = c.dmp_resp ? "k_traj_fit_tile<dmp_resp>" : (promp ? "k_traj_fit_tile<promp>" : "k_traj_fit_tile<prodmp>");
    return promp ? go(k_traj_fit_tile<MPK_MP_PROMP>) : go(k_traj_fit_tile<MPK_MP_PRODMP>);
}

// ---- launch_phase_fit: k_phase_vjp's shapes (plan_phase_vjp's rules; a ProMP with one step is fine here: no velocity is involved)
constexpr int kPhaseFitWaves = 4;
int phase_fit_limits(const DevCfg& c, int* kq_out, PhaseFitArgs* pa, size_t* lds_out) {
    if (c.mp_type == MPK_MP_DMP) {
        set_error("mpk_trajectory_phase_fit: a DMP with a per-episode phase is an Euler recurrence in the scaled time, which is not a "
                  "table this kernel could invert (promp / prodmp only)");
        return MPK_ENOTIMPL;
    }
    const bool prodmp = c.mp_type == MPK_MP_PRODMP;
    const int need = prodmp ? c.nb + 3 : c.KT;
    const int KQ = need <= 4 && !prodmp ? 1 : (need <= 8 ? 2 : 4), KS = KQ * 4;
    const bool rows_ok = !prodmp || (c.rows32 && c.rows32_stride == 2 * KS + 4);
    if (need > 16 || c.D > kMaxD || c.D < 1 || c.D * KS > 256 || !rows_ok || c.P > 320) {
        set_error("mpk_trajectory_phase_fit: the shapes of the wave kernel k_traj_phase only (<= 16 DoF, DoF x padded columns <= 256, "
                  "<= 16 columns, <= 320 parameters per episode)");
        return MPK_ENOTIMPL;
    }
    const int t_pad = (c.T + 3) / 4 * 4, c_pad = prodmp ? KS + 4 : (4 * c.n_total + 6 + 3) / 4 * 4;
    const int wave_doubles = 64 * KS + 64 * c.D + KS * KS + 16 * (KS + 1) + 32;
    const size_t lds = (size_t)(c_pad + t_pad) * sizeof(float) + (size_t)kPhaseFitWaves * wave_doubles * sizeof(double);
    if (lds > kLdsPerCu) {
        set_error("mpk_trajectory_phase_fit: the horizon's time grid (" + std::to_string(c.T) + " steps) does not fit the LDS");
        return MPK_ENOTIMPL;
    }
    if (kq_out) *kq_out = KQ;
    if (pa) { pa->t_pad = t_pad; pa->c_pad = c_pad; pa->wave_doubles = wave_doubles; }
    if (lds_out) *lds_out = lds;
    return MPK_OK;
}
int phase_fit_limits(const DevCfg& c) { return phase_fit_limits(c, nullptr, nullptr, nullptr); }

int launch_phase_fit(const DevCfg& c, const PhaseFitLaunch& q, int num_cu, void* stream, const char** kernel_name) {
    PhaseFitArgs pa{};
    pa.c = c;
    pa.pos = q.pos; pa.phase = q.phase; pa.init_pos = q.init_pos; pa.init_vel = q.init_vel; pa.init_time = q.init_time;
    pa.init_time_shared = q.init_time_shared; pa.reg = q.reg; pa.params = q.params; pa.flag = q.range_flag; pa.status = q.status;
    pa.B = q.B;
    int KQ = 0;
    size_t lds = 0;
    const int rc = phase_fit_limits(c, &KQ, &pa, &lds);
    if (rc != MPK_OK) return rc;
    int per_cu = (int)(kLdsPerCu / lds);
    per_cu = per_cu > 8 ? 8 : per_cu;
    const long units = ((long)q.B + kPhaseFitWaves - 1) / kPhaseFitWaves;
    const long blocks = units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu;
    auto go = [&](auto kern) { return launch_kernel(kern, dim3((unsigned)blocks), dim3(64 * kPhaseFitWaves), lds, stream, pa); };
    if (c.mp_type == MPK_MP_PROMP) {
        *kernel_name = "k_phase_fit<promp>";
        if (KQ == 1) return go(k_phase_fit<MPK_MP_PROMP, 1>);
        return KQ == 2 ? go(k_phase_fit<MPK_MP_PROMP, 2>) : go(k_phase_fit<MPK_MP_PROMP, 4>);
    }
    *kernel_name = "k_phase_fit<prodmp>";
    return KQ == 2 ? go(k_phase_fit<MPK_MP_PRODMP, 2>) : go(k_phase_fit<MPK_MP_PRODMP, 4>);
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
