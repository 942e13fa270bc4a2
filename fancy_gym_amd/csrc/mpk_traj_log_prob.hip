// k_traj_log_prob: the log-likelihood of observed trajectory points under a Gaussian over the MP parameters, and its gradient
// (mpk_trajectory_log_prob, mpk_trajectory_log_prob_vjp)
#include "mpk_tile.h"
#include "mpk_vjp_row.h"
#include "mpk_cond_rows.h"
#include "mpk_phase_rows.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// The scalar observations (o, m, d) are mpk_trajectory_condition's (mpk_traj_condition.hip has the whole story): of the non-phase
// parameters w ~ N(mu, L L^T) an observation reads y = h . w + c + eps, eps ~ N(0, sigma^2), h the table row R_o[.][t_m] placed in DoF
// d's block, c what init_pos / init_vel / the goal offset contribute; sigma +inf, NaN or negative removes it.  With the n that remain, in
// conditioning's order (m ascending; positions by DoF, then velocities by DoF):
//     A = H tril(L)  [n, Pl]   (row i = L^T h_i; zero from column (d_i + 1) Kloc on),   S = A A^T + diag(sigma^2),   r = y - c - H mu
//     log_prob = -1/2 r^T S^-1 r - 1/2 log det S - n / 2 log 2 pi
//     alpha = S^-1 r,   g_params[off + .] = g H^T alpha,   g_params_L = g tril(H^T (alpha alpha^T - S^-1) A)
// all in float64: a DENSE factorisation S = C C^T of the n x n observation covariance -- another algorithm than conditioning's sequential
// update, and never through L L^T.  A pivot that is not > 0 makes the episode's log_prob and gradient rows NaN (S singular is an input
// property); nothing else of the batch changes.
// k_traj_log_prob<MP, NS, GRAD>: one wave per episode, `waves` of them a workgroup (sized at launch from the LDS the images need).
//   * The table rows of the M observed steps, [2][M][KT] float64, are staged once per workgroup exactly as k_traj_condition stages them
//     (cond_obs_row: the launch's float32 table, a ProMP's velocity rows re-evaluated in float64), and the table column of every local
//     parameter (kof, the inverse of x_kind).
//   * lane <-> candidate observation q = (m narr + array) D + d (at most 64): its sigma decides whether it counts; a ballot compacts the
//     kept ones to i = 0 .. n - 1 in order.  n = 0: log_prob = 0.0 and zero gradients, exactly.
//   * lane <-> column j (NS = ceil(Pl / 64) per lane): row i of A straight from the float32 rows of L in HBM -- the Kloc rows of DoF d_i's
//     block, entries j <= row only: the strict upper triangle is never read -- into a float64 LDS image [n][ld], ld odd (rows of the
//     image then fall on different banks).  r_i: every lane, the same fixed order.
//   * lane <-> j2 <= i, row by row: S[i][j2] = sum_j A[i][j] A[j2][j] over the columns both rows have, packed lower triangle; then a
//     left-looking Cholesky in place, lane <-> row; forward substitution with lane <-> row (z in a register); the two sums by a fixed
//     xor ladder.  GRAD = false ends here: log_prob.
//   * GRAD: back substitution -> alpha; u = A^T alpha (lane <-> column); W = S^-1 A in place, two triangular solves per column with
//     lane <-> column, so no lane reads another's column; then row by row of the output, row = d Kloc + l:
//         g_params_L[row][j] = g sum_{i: d_i = d} h_i[k(l)] (alpha_i u_j - W[i][j])   for j <= row, exact 0 for j > row
//     -- a gather: every entry is written once by one lane, a row no kept observation touches is an exact 0 -- and g_params the same
//     with alpha_i alone.  Float64 sums, rounded to float32 once.  Nothing is kept from the forward launch: A, S and C are recomputed.
// No atomics, an episode never leaves its wave, and nothing depends on an address: the same bits from run to run, for any alignment of
// the pointers, alone or in a batch.  No index depends on a value that is read: non-finite inputs give non-finite outputs, never a fault.
// LDS: waves x 8 (nmax ld + nmax (nmax + 1) / 2 + 3 nmax) + 16 M KT + 64 bytes, nmax = M D narr, ld = Pl | 1 (Pl = 160, n = 64: 101 KB).
// k_traj_log_prob<MP, NS, GRAD, PHASE = true> (mpk_trajectory_phase_log_prob / _vjp; last_kernel "k_traj_log_prob<.., phase>"): the same text
// with k_traj_condition's PER-EPISODE row source, for handles that learn tau / delay: every wave evaluates its own episode's [2][M]
// rows at the tau / delay in front of its params row (mpk_phase_rows.h, float64) into an image of its own, [2][M][Kloc + 3], regrouped
// by local parameter (kof is the identity) with ca | cb | cc of the given part behind.  The phase columns of g_params are exact zeros:
// the timing is an input.  LDS: 16 M (Kloc + 3) more per wave; the row constants and base times per workgroup instead of [2][M][KT].
// ------------------------------------------------------------------------------------------------------------
constexpr int kLpMaxObs = MPK_LOGPROB_MAX_OBS;                      // scalar observations per episode: one lane each
constexpr int kLpSlots = 4;                                         // columns per lane at most (NS = ceil(Pl / 64))
static_assert(kLpMaxObs == 64, "one lane per candidate observation");

struct LogProbArgs {
    DevCfg c;
    const float* A;        // [n_out][KP][TS] (k_build_shared)
    const float* aux;      // [TS]
    int TS;
    float init_time;       // the tables' (init_time_shared)
    const float* params;   // [B, P]
    const float* L;        // [B, Pl, Pl]; the lower triangle is read
    const float* init_pos; // [B, D] or nullptr (promp: zeros)
    const float* init_vel;
    const float* obs[2];   // [B, M, D] position / velocity values, or nullptr
    const float* sd[2];    // [B, M, D] their standard deviations
    double* log_prob;      // [B] out (forward)
    const double* g;       // [B] the upstream gradient (GRAD)
    float* g_params;       // [B, P] out or nullptr (GRAD)
    float* g_L;            // [B, Pl, Pl] out or nullptr (GRAD)
    int B, Pl, M;
    int narr;              // observation arrays given: 1 or 2
    int nmax;              // M D narr <= 64: the candidate observations
    int ld;                // float64 words between the rows of the A image (odd)
    int waves;             // per workgroup
    int wave_doubles;      // float64 words of LDS per wave
    int steps[MPK_COND_MAX_STEPS];
};
static_assert(sizeof(LogProbArgs) <= 4096, "kernel arguments");

// the sum over the wave by a fixed xor ladder: the same bits in every lane
__device__ __forceinline__ double lp_wave_sum(double x) {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x += __shfl_xor(x, sh, 64);
    return x;
}

// the per-episode row source's arguments behind the shared ones (A, aux, TS are not read)
struct LogProbPhaseArgs : LogProbArgs {
    int sl;                // words between the rows of a wave's row image: Kloc + 3
    int c_pad;             // floats of the workgroup's row constants (phase_rows_const_floats)
    int32_t* flag;         // prodmp: raised beyond the pre-computed range (k_phase_fit's)
};
static_assert(sizeof(LogProbPhaseArgs) <= 4096, "kernel arguments");

// PHASE: the per-episode row source ("k_traj_log_prob<.., phase>")
template <int MP, int NS, bool GRAD, bool PHASE = false>
__global__ void __launch_bounds__(256) k_traj_log_prob(const std::conditional_t<PHASE, LogProbPhaseArgs, LogProbArgs> a) {
    extern __shared__ __attribute__((aligned(16))) double lp_smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int D = c.D, Kloc = c.Kloc, Pl = a.Pl, M = a.M, KT = c.KT, ld = a.ld, nmax = a.nmax, narr = a.narr;
    double* sA = lp_smem + (size_t)wave * a.wave_doubles;           // [nmax][ld] A, then W = S^-1 A
    double* sS = sA + nmax * ld;                                    // packed lower triangle: S, then its Cholesky factor C
    double* sal = sS + nmax * (nmax + 1) / 2;                       // [nmax] y, then r, then alpha
    double* ssg = sal + nmax;                                       // [nmax] sigma^2
    int* cidx = (int*)(ssg + nmax);                                 // [nmax] candidate -> its index among the kept ones, or -1
    int* sdof = cidx + nmax;                                        // [nmax] kept -> its DoF
    double* rows = lp_smem + (size_t)a.waves * a.wave_doubles;      // [2][M][KT]
    int* kof = (int*)(rows + (PHASE ? 0 : 2 * M * KT));             // [Kloc] the table column read from local parameter l, or -1
    double* prow = ssg + 2 * nmax;                                  // PHASE: [2][M][sl] this episode's rows
    float* sK = (float*)(rows + 8);                                 // PHASE: behind kof the row constants, then the base times [T]
    int sl = 0;
    const float* sBT = nullptr;
    bool use_ip = false, use_iv = false;
    if constexpr (PHASE) {
        sl = a.sl;
        sBT = sK + a.c_pad;
        phase_rows_stage<MP>(c, sK, sK + a.c_pad, tid, blockDim.x);
        // which of the given columns exist: a ProDMP's init_pos / init_vel, a zero-padded ProMP's init_pos
        use_ip = a.init_pos && (MP == MPK_MP_PRODMP || KT > c.nb);
        use_iv = a.init_vel && MP == MPK_MP_PRODMP;
    }
    for (int i = tid; !PHASE && i < 2 * M * KT; i += blockDim.x) {
        const int o = i / (M * KT), r = i - o * M * KT;
        const int m = r / KT, k = r - m * KT;
        rows[i] = a.obs[o] ? cond_obs_row<MP>(c, a.A, a.aux, a.TS, a.init_time, o, k, a.steps[m]) : 0.0;
    }
    if (tid < Kloc) {
        int found = -1;
        for (int k = 0; k < KT; ++k) {
            int loc;
            if (x_kind<MP>(c, k, &loc) == XK_PARAM && loc == tid) found = k;
        }
        kof[tid] = PHASE ? tid : found;
    }
    __syncthreads();
    const int o_first = a.obs[0] ? 0 : 1;                           // the array candidate `array 0` belongs to
    const double nan = __builtin_nan("");
    for (int b = blockIdx.x * a.waves + wave; b < a.B; b += gridDim.x * a.waves) {
        const float* Lb = a.L + (size_t)b * Pl * Pl;
        if constexpr (PHASE) {                                      // lane <-> (array, step): this episode's rows
            const PhaseEpisode ep = phase_rows_episode<MP>(c, a.params + (size_t)b * c.P, a.init_time);
            const int o = lane >= M ? 1 : 0, m = lane - o * M;
            if (lane < 2 * M && a.obs[o]) {
                double e[kPhaseRowSlots], ca, cb, cg;
                if (o) phase_rows_eval_vel<MP>(c, ep, sK, sBT, a.steps[m], a.flag, e, ca, cb, cg);
                else phase_rows_eval<MP>(c, ep, sK, sBT[a.steps[m]], a.flag, e, ca, cb, cg);
                double* er = prow + (o * M + m) * sl;
#pragma unroll
                for (int k = 0; k < kPhaseRowSlots; ++k)
                    if (k < Kloc) er[k] = e[k];
                er[Kloc] = ca; er[Kloc + 1] = cb; er[Kloc + 2] = cg;
            }
        }
        // ---- which observations count (lane <-> candidate)
        bool keep = false;
        double sig = 0.0, yv = 0.0;
        int d_l = 0;
        if (lane < nmax) {
            const int m = lane / (narr * D), rem = lane - m * narr * D;
            const int oi = rem / D;
            d_l = rem - oi * D;
            const int o = oi ? 1 : o_first;
            const size_t at = ((size_t)b * M + m) * D + d_l;
            sig = (double)(o ? a.sd[1] : a.sd[0])[at];
            yv = (double)(o ? a.obs[1] : a.obs[0])[at];
            keep = sig >= 0.0 && sig != __builtin_inf();            // +inf, NaN, negative: not observed
        }
        const unsigned long long kept = __ballot(keep);
        const int n = __builtin_amdgcn_readfirstlane(__popcll(kept));
        const int idx = __popcll(kept & ((1ull << lane) - 1ull));
        if (lane < nmax) cidx[lane] = keep ? idx : -1;
        if (keep) { ssg[idx] = sig * sig; sdof[idx] = d_l; sal[idx] = yv; }
        cond_wave_sync();
        bool bad = false;                                           // (wave-uniform) a pivot was not > 0
        double rr = 0.0, dg = 1.0;                                  // lane <-> row i: r_i -> z_i -> alpha_i; C[i][i]
        if (n > 0) {
            // ---- A and r: the candidates of DoF d, each from the Kloc rows of L's block d (lane <-> column)
            for (int d = 0; d < D; ++d) {
                for (int mo = 0; mo < M * narr; ++mo) {
                    const int i = __builtin_amdgcn_readfirstlane(cidx[mo * D + d]);
                    if (i < 0) continue;
                    const int m = mo / narr, o = (mo - m * narr) ? 1 : o_first;
                    const double* hr = PHASE ? prow + (o * M + m) * sl : rows + (o * M + m) * KT;
                    double cc = 0.0, hmu = 0.0;
                    double acc[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
                    if constexpr (PHASE) {
                        for (int l = 0; l < Kloc; ++l) {
                            const int row = d * Kloc + l;
                            const double hk = hr[l];
                            hmu = __builtin_fma(hk, (double)a.params[(size_t)b * c.P + c.off + row], hmu);
                            const float* lr = Lb + (size_t)row * Pl;
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const int j = lane + 64 * s;
                                if (j <= row) acc[s] = __builtin_fma(hk, (double)lr[j], acc[s]);
                            }
                        }
                        cc = hr[Kloc + 2];
                        if (use_iv) cc = __builtin_fma(hr[Kloc + 1], (double)a.init_vel[(size_t)b * D + d], cc);
                        if (use_ip) cc = __builtin_fma(hr[Kloc], (double)a.init_pos[(size_t)b * D + d], cc);
                    }
                    for (int k = 0; !PHASE && k < KT; ++k) {
                        int loc;
                        const int kind = x_kind<MP>(c, k, &loc);
                        const double hk = hr[k];
                        if (kind == XK_PARAM) {
                            const int row = d * Kloc + loc;
                            hmu = __builtin_fma(hk, (double)a.params[(size_t)b * c.P + c.off + row], hmu);
                            const float* lr = Lb + (size_t)row * Pl;
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const int j = lane + 64 * s;
                                if (j <= row) acc[s] = __builtin_fma(hk, (double)lr[j], acc[s]);
                            }
                        } else if (kind == XK_IPOS) {
                            if (a.init_pos) cc = __builtin_fma(hk, (double)a.init_pos[(size_t)b * D + d], cc);
                        } else if (kind == XK_IVEL) {
                            if (a.init_vel) cc = __builtin_fma(hk, (double)a.init_vel[(size_t)b * D + d], cc);
                        } else if (kind == XK_ONE) {
                            cc += hk;
                        }
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = lane + 64 * s;
                        if (j < Pl) sA[i * ld + j] = acc[s];
                    }
                    if (lane == 0) sal[i] = sal[i] - cc - hmu;
                }
            }
            cond_wave_sync();
            // ---- S = A A^T + diag(sigma^2), row by row (lane <-> j2 <= i), over the columns both rows have
            for (int i = 0; i < n; ++i) {
                if (lane <= i) {
                    const double* ai = sA + i * ld;
                    const double* aj = sA + lane * ld;
                    const int di = sdof[i], dj = sdof[lane];
                    const int jm = ((di < dj ? di : dj) + 1) * Kloc;
                    double s0 = 0.0, s1 = 0.0;
                    int j = 0;
                    for (; j + 1 < jm; j += 2) {
                        s0 = __builtin_fma(ai[j], aj[j], s0);
                        s1 = __builtin_fma(ai[j + 1], aj[j + 1], s1);
                    }
                    if (j < jm) s0 = __builtin_fma(ai[j], aj[j], s0);
                    double s = s0 + s1;
                    if (lane == i) s += ssg[i];
                    sS[i * (i + 1) / 2 + lane] = s;
                }
            }
            cond_wave_sync();
            // ---- S = C C^T in place, left-looking (lane <-> row)
            const int mine = lane * (lane + 1) / 2;
            for (int jc = 0; jc < n; ++jc) {
                const double* cj = sS + jc * (jc + 1) / 2;
                double s = 0.0;
                if (lane >= jc && lane < n) {
                    s = sS[mine + jc];
                    for (int k = 0; k < jc; ++k) s = __builtin_fma(-sS[mine + k], cj[k], s);
                }
                const double piv = __shfl(s, jc, 64);
                const bool ok = piv > 0.0;                          // (wave-uniform) a NaN is not
                bad = bad || !ok;
                const double root = ok ? sqrt(piv) : nan;
                if (lane >= jc && lane < n) sS[mine + jc] = lane == jc ? root : s / root;
                cond_wave_sync();
            }
            // ---- z = C^-1 r (lane <-> row; column by column)
            if (lane < n) { rr = sal[lane]; dg = sS[mine + lane]; }
            for (int j = 0; j < n; ++j) {
                const double zj = __shfl(rr, j, 64) / __shfl(dg, j, 64);
                if (lane == j) rr = zj;
                else if (lane > j && lane < n) rr = __builtin_fma(-sS[mine + j], zj, rr);
            }
        }
        if (!GRAD) {
            const double quad = lp_wave_sum(lane < n ? rr * rr : 0.0);
            const double logs = lp_wave_sum(lane < n ? log(dg) : 0.0);
            double lp = 0.0;
            if (n > 0) lp = bad ? nan : -0.5 * quad - logs - (double)n * 0.91893853320467274178;   // 1/2 log 2 pi
            if (lane == 0) a.log_prob[b] = lp;
        } else {
            const double gb = a.g[b];
            double u[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) u[s] = 0.0;
            if (n > 0) {
                // ---- alpha = C^-T z (lane <-> row; row by row from the last)
                for (int j = n - 1; j >= 0; --j) {
                    const double aj = __shfl(rr, j, 64) / __shfl(dg, j, 64);
                    if (lane == j) rr = aj;
                    else if (lane < j) rr = __builtin_fma(-sS[j * (j + 1) / 2 + lane], aj, rr);
                }
                if (lane < n) sal[lane] = rr;
                cond_wave_sync();
                // ---- u = A^T alpha, then W = S^-1 A in place (lane <-> column: a lane touches its own columns only)
                for (int i = 0; i < n; ++i) {
                    const double al = sal[i];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = lane + 64 * s;
                        if (j < Pl) u[s] = __builtin_fma(sA[i * ld + j], al, u[s]);
                    }
                }
                for (int i = 0; i < n; ++i) {                       // C x = a
                    const double* ci = sS + i * (i + 1) / 2;
                    double x[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; x[s] = j < Pl ? sA[i * ld + j] : 0.0; }
                    for (int k = 0; k < i; ++k) {
                        const double ck = ci[k];
#pragma unroll
                        for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; if (j < Pl) x[s] = __builtin_fma(-ck, sA[k * ld + j], x[s]); }
                    }
                    const double cii = ci[i];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; if (j < Pl) sA[i * ld + j] = x[s] / cii; }
                }
                for (int i = n - 1; i >= 0; --i) {                  // C^T w = x
                    double x[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; x[s] = j < Pl ? sA[i * ld + j] : 0.0; }
                    for (int k = i + 1; k < n; ++k) {
                        const double ck = sS[k * (k + 1) / 2 + i];
#pragma unroll
                        for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; if (j < Pl) x[s] = __builtin_fma(-ck, sA[k * ld + j], x[s]); }
                    }
                    const double cii = sS[i * (i + 1) / 2 + i];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { const int j = lane + 64 * s; if (j < Pl) sA[i * ld + j] = x[s] / cii; }
                }
            }
            // ---- the gradients leave, rounded once: a gather over the kept observations of the row's DoF
            if (a.g_L) {
                float* Go = a.g_L + (size_t)b * Pl * Pl;
                for (int row = 0; row < Pl; ++row) {
                    const int d = row / Kloc, k = kof[row - d * Kloc];
                    double acc[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
                    bool any = false;                               // (wave-uniform)
                    if (n > 0 && k >= 0) {
                        for (int mo = 0; mo < M * narr; ++mo) {
                            const int i = __builtin_amdgcn_readfirstlane(cidx[mo * D + d]);
                            if (i < 0) continue;
                            const int m = mo / narr, o = (mo - m * narr) ? 1 : o_first;
                            const double hk = PHASE ? prow[(o * M + m) * sl + k] : rows[(o * M + m) * KT + k], al = sal[i];
                            any = true;
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const int j = lane + 64 * s;
                                if (j <= row) acc[s] = __builtin_fma(hk, __builtin_fma(al, u[s], -sA[i * ld + j]), acc[s]);
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = lane + 64 * s;
                        if (j < Pl) {
                            float out = 0.0f;
                            if (j <= row && n > 0) out = bad ? (float)nan : (any ? (float)(gb * acc[s]) : 0.0f);
                            Go[(size_t)row * Pl + j] = out;
                        }
                    }
                }
            }
            if (a.g_params) {
                for (int p = lane; p < c.P; p += 64) {
                    const int row = p - c.off;
                    float out = 0.0f;
                    if (row >= 0 && row < Pl && n > 0) {
                        const int d = row / Kloc, k = kof[row - d * Kloc];
                        double acc = 0.0;
                        bool any = false;
                        if (k >= 0) {
                            for (int mo = 0; mo < M * narr; ++mo) {
                                const int i = cidx[mo * D + d];
                                if (i < 0) continue;
                                const int m = mo / narr, o = (mo - m * narr) ? 1 : o_first;
                                acc = __builtin_fma(PHASE ? prow[(o * M + m) * sl + k] : rows[(o * M + m) * KT + k], sal[i], acc);
                                any = true;
                            }
                        }
                        out = bad ? (float)nan : (any ? (float)(gb * acc) : 0.0f);
                    }
                    a.g_params[(size_t)b * c.P + p] = out;
                }
            }
        }
        cond_wave_sync();                                           // the images are free again
    }
}

#ifndef MPK_DEVICE_ONLY
// the shapes the kernels take; MPK_ENOTIMPL with the limit in the message, under the entry's name fn, otherwise (no HIP call).  M: the
// observed steps of the call, narr: the observation arrays given (1 or 2).  phase: the per-episode row source -- [2][M][Kloc + 3] more
// per wave, the row constants and base times per workgroup where the shared route has [2][M][KT]; rows beyond the 16 slots are refused
static int log_prob_limits(const DevCfg& c, int M, int narr, bool phase, const char* fn, size_t* lds_out, int* waves_out,
                           int* wave_doubles_out) {
    if (const int rc = gauss_common_limits(c, fn)) return rc;
    const std::string name(fn);
    if (phase)
        if (const int rc = gauss_phase_row_limits(c, kPhaseRowSlots, fn)) return rc;
    const size_t nmax = (size_t)M * c.D * narr;
    if (nmax > (size_t)kLpMaxObs) {
        set_error(name + ": at most " + std::to_string(kLpMaxObs) + " scalar observations per episode (M x D x the "
                  "observation arrays given = " + std::to_string(M) + " x " + std::to_string(c.D) + " x " + std::to_string(narr) + " = " +
                  std::to_string(nmax) + "); the whole-trajectory likelihood wants the Pl x Pl form, which has no kernel here");
        return MPK_ENOTIMPL;
    }
    const size_t Pl = (size_t)c.D * c.Kloc;
    const size_t wave_doubles = nmax * (Pl | 1) + nmax * (nmax + 1) / 2 + 3 * nmax + (phase ? (size_t)2 * M * (c.Kloc + 3) : 0);
    const size_t shared = phase ? 64 + ((size_t)phase_rows_const_floats(c) + c.T + 1) / 2 * 2 * sizeof(float)
                                : (size_t)2 * M * c.KT * sizeof(double) + 64;
    if (wave_doubles * sizeof(double) + shared > kLdsPerCu || Pl > 64 * kLpSlots) {
        set_error(name + ": the float64 images of " + std::to_string(nmax) + " observations of " + std::to_string(Pl) +
                  " parameters (" + std::to_string(wave_doubles * sizeof(double) + shared) + " bytes with one wave per workgroup) do not "
                  "fit the CU's " + std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    const WavePlan plan = gauss_wave_plan(wave_doubles, shared);
    if (lds_out) *lds_out = plan.lds;
    if (waves_out) *waves_out = plan.waves;
    if (wave_doubles_out) *wave_doubles_out = (int)wave_doubles;
    return MPK_OK;
}

int traj_log_prob_limits(const DevCfg& c, int M, int narr, size_t* lds_out, int* waves_out, int* wave_doubles_out) {
    return log_prob_limits(c, M, narr, false, "mpk_trajectory_log_prob", lds_out, waves_out, wave_doubles_out);
}

int traj_log_prob_phase_limits(const DevCfg& c, int M, int narr, const char* fn, size_t* lds_out, int* waves_out, int* wave_doubles_out) {
    return log_prob_limits(c, M, narr, true, fn, lds_out, waves_out, wave_doubles_out);
}

int launch_traj_log_prob(const DevCfg& c, const SharedTables& st, const LogProbLaunch& q, int num_cu, void* stream,
                         const char** kernel_name) {
    LogProbPhaseArgs la{};
    size_t lds = 0;
    const bool phase = q.phase;
    const char* fn = !phase ? "mpk_trajectory_log_prob" : (q.out.grad ? "mpk_trajectory_phase_log_prob_vjp" : "mpk_trajectory_phase_log_prob");
    const int M = q.obs.M, narr = (q.obs.obs_pos ? 1 : 0) + (q.obs.obs_vel ? 1 : 0);
    if (M < 1 || M > MPK_COND_MAX_STEPS || narr < 1) {
        set_error(std::string(fn) + ": internal: the observed steps are outside 1.." + std::to_string(MPK_COND_MAX_STEPS) +
                  " or no observation array is given");
        return MPK_EINVAL;
    }
    const int rc = phase ? traj_log_prob_phase_limits(c, M, narr, fn, &lds, &la.waves, &la.wave_doubles)
                         : traj_log_prob_limits(c, M, narr, &lds, &la.waves, &la.wave_doubles);
    if (rc != MPK_OK) return rc;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    if (promp && q.obs.obs_vel && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    la.c = c; la.A = st.A; la.aux = st.aux; la.TS = st.TS; la.init_time = q.in.init_time;
    la.params = q.in.params; la.L = q.in.params_L; la.init_pos = q.in.init_pos; la.init_vel = q.in.init_vel;
    la.obs[0] = q.obs.obs_pos; la.sd[0] = q.obs.obs_pos_std; la.obs[1] = q.obs.obs_vel; la.sd[1] = q.obs.obs_vel_std;
    la.log_prob = q.out.log_prob; la.g = q.out.g; la.g_params = q.out.g_params; la.g_L = q.out.g_params_L;
    la.B = q.in.B; la.Pl = c.D * c.Kloc; la.M = M; la.narr = narr; la.nmax = M * c.D * narr; la.ld = la.Pl | 1;
    for (int m = 0; m < M; ++m) la.steps[m] = q.obs.steps[m];
    const int blocks = gauss_blocks(q.in.B, la.waves, lds, num_cu);
    static const char* const names[2][2][2] = {
        {{"k_traj_log_prob<prodmp>", "k_traj_log_prob<promp>"}, {"k_traj_log_prob<prodmp, grad>", "k_traj_log_prob<promp, grad>"}},
        {{"k_traj_log_prob<prodmp, phase>", "k_traj_log_prob<promp, phase>"},
         {"k_traj_log_prob<prodmp, phase, grad>", "k_traj_log_prob<promp, phase, grad>"}}};
    *kernel_name = names[phase][q.out.grad][promp];
    if (phase) {
        la.sl = c.Kloc + 3; la.c_pad = phase_rows_const_floats(c); la.flag = q.range_flag;
        return dispatch_flag(q.out.grad, [&](auto grad) {
            return dispatch_mp(promp, [&](auto mp) {
                return dispatch_ns((la.Pl + 63) / 64, [&](auto ns) {
                    return launch_kernel(k_traj_log_prob<mp.value, ns.value, grad.value, true>, dim3(blocks), dim3(64 * la.waves), lds,
                                         stream, la);
                });
            });
        });
    }
    return dispatch_flag(q.out.grad, [&](auto grad) {
        return dispatch_mp(promp, [&](auto mp) {
            return dispatch_ns((la.Pl + 63) / 64, [&](auto ns) {
                return launch_kernel(k_traj_log_prob<mp.value, ns.value, grad.value>, dim3(blocks), dim3(64 * la.waves), lds, stream,
                                     static_cast<const LogProbArgs&>(la));
            });
        });
    });
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
