// k_traj_condition: a Gaussian over the MP parameters conditioned on observed trajectory points (mpk_trajectory_condition)
#include "mpk_tile.h"
#include "mpk_vjp_row.h"
#include "mpk_cond_rows.h"
#include "mpk_phase_rows.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// With a phase all episodes share, pos[b, t, d] = sum_k R0[k][t] x[b, d][k] and vel the same with R1 (mpk_traj_vjp.hip has the whole
// story), and x_kind (mpk_tile.h, the forward's own gather) says which columns k of x are read from params, at
// params[off + d Kloc + loc(k)].  So a scalar observation (o, m, d) -- o = 0 position / 1 velocity, step t_m, DoF d -- of the non-phase
// parameters w ~ N(mu, L L^T) (Pl = D Kloc of them, user's units) reads
//     y = h . w + c + eps,   eps ~ N(0, sigma^2),   h[d Kloc + loc(k)] = R_o[k][t_m] for the parameter columns k, 0 elsewhere,
//     c = what the other columns give: R_o[k_ipos][t_m] init_pos[b, d] + R_o[k_ivel][t_m] init_vel[b, d] + R_o[k_one][t_m].
// The posterior is again Gaussian.  The update is Carlson's square-root measurement update in its lower-triangular form, one scalar
// observation after the other, in float64 -- the FACTOR form: L L^T is never formed, no two covariances are subtracted, L stays lower
// triangular with a non-negative diagonal, and sigma = 0 (exact conditioning) is defined:
//     v = L^T h                                  (v_j = 0 for j >= n = (d + 1) Kloc: h lives in block d and L is lower triangular)
//     b_n = sigma^2;  b_j = b_{j+1} + v_j^2  (j = n - 1 .. 0);  s = b_0
//     skip the observation when sigma is +inf, NaN or negative, or when s == 0
//     r = y - c - h . mu
//     w = 0;  for j = n - 1 .. 0:  L'[:, j] = L[:, j] sqrt(b_{j+1} / b_j) - w v_j / sqrt(b_{j+1} b_j);  w += L[:, j] v_j
//             (b_j == 0: the column stays;  b_{j+1} == 0 < b_j: the column becomes 0;  sqrt(b_{j+1} b_j) is evaluated as the product
//              of the two roots: the b of far-off RBF columns are ~1e-200 and their product underflows)
//     mu' = mu + w (r / s)
// Order: m ascending; within a step the positions, d ascending, then the velocities, d ascending.
// k_traj_condition<MP>: one wave per episode, `waves` of them a workgroup (sized at launch from the LDS the triangle needs).
//   * The table rows of the M observed steps, [2][M][KT], are staged once per workgroup as float64: the launch's own float32 table
//     (vjp_row) -- but for a ProMP's velocity rows.  Those are the forward difference of two position rows times 1 / dt, and the
//     difference of two float32-ROUNDED rows carries their rounding amplified by |row| / |difference| (20 to 50 at dt = 0.02): at
//     sigma = 1e-3 the posterior mean was measured 2 x the project rule off.  The staging recomputes the two normalised-RBF rows in
//     float64 with the table builder's own functions (phase_f64, exp_nonpos: 2e-10) and differences those (cond_promp_vel_row).
//   * The episode's lower triangle goes once from HBM into the wave's LDS as packed float64, row i at i (i + 1) / 2; mu beside it.
//     The strict upper triangle of the input is never read.
//   * Per observation: (1) lane <-> column j: v_j, a sum over the <= Kloc parameter columns in table order; (2) lane <-> a block of
//     ceil(n / 64) consecutive j: the suffix sums b_j -- inside the lane, then across the lanes by a fixed shuffle ladder -- and from
//     them the two coefficients of every column, sqrt(b_{j+1} / b_j) and v_j / sqrt(b_{j+1} b_j), ONCE per observation; (3) lane <->
//     rows i, i + 64, ...: the column sweep j = n - 1 .. 0 over its rows' entries j <= i, two multiply-adds per entry and no sqrt or
//     division, four columns' loads in flight; (4) mu_i += w_i (r / s).  c and h . mu: every lane, the same fixed order.
//   * The float64 image is rounded to float32 once, on the way out, with plain stores; the strict upper triangle of params_L_out is
//     written as exact zeros.  An episode is read completely before anything of it is written: the outputs may be the inputs.
// No atomics, an episode never leaves its wave, and nothing depends on an address: the same bits from run to run, for any alignment of
// the pointers, alone or in a batch.  A skipped observation touches nothing: float32 -> float64 -> float32 is the identity.
// LDS: waves x 8 (Pl (Pl + 1) / 2 + 4 Pl) bytes + 16 M KT; traj_cond_limits refuses a Pl that one wave cannot hold (Pl = 160: 108 KB).
// k_traj_condition<MP, NS, PHASE = true> (mpk_trajectory_phase_condition; last_kernel "k_traj_condition<.., phase>"): the same text with a
// PER-EPISODE row source, for handles that learn tau / delay -- the tau / delay of episode b stand at the front of its params row
// (phase_rows_episode reads and clips them as the forward does).  No workgroup-wide row image: before the sweep every wave evaluates its
// own episode's [2][M] rows, lane <-> (array, step), with mpk_phase_rows.h in float64 into an image of its own, [2][M][Kloc + 3]: the
// entries regrouped by local parameter, then ca | cb | cc of the given part c = ca init_pos + cb init_vel + cc.  The workgroup shares
// the row constants and the base times.  The phase columns leave as they came, unclipped.  LDS: 16 M (Kloc + 3) more per wave.
// ------------------------------------------------------------------------------------------------------------
constexpr int kCondMaxObs = MPK_COND_MAX_STEPS;                     // observed steps per call (mpk.h)
constexpr int kCondSlots = 4;                                       // rows per lane at most (NS = ceil(Pl / 64)): Pl <= 256 whatever the LDS allows
constexpr int kCondAhead = 4;                                       // columns of the sweep whose loads are in flight together

struct CondArgs {
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
    float* params_out;     // [B, P]
    float* L_out;          // [B, Pl, Pl]
    int B, Pl, M;
    int waves;             // per workgroup
    int wave_doubles;      // float64 words of LDS per wave
    int steps[kCondMaxObs];
};

// (i, j) of the packed lower triangle's entry p = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ void cond_unpack(int p, int* i_out, int* j_out) {
    int i = (int)((__builtin_sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > p) --i;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    *i_out = i; *j_out = p - i * (i + 1) / 2;
}

// the per-episode row source's arguments behind the shared ones (A, aux, TS are not read)
struct CondPhaseArgs : CondArgs {
    int sl;                // words between the rows of a wave's row image: Kloc + 3
    int c_pad;             // floats of the workgroup's row constants (phase_rows_const_floats)
    int32_t* flag;         // prodmp: raised beyond the pre-computed range (k_phase_fit's)
};

// NS: rows per lane, ceil(Pl / 64); PHASE: the per-episode row source ("k_traj_condition<.., phase>")
template <int MP, int NS, bool PHASE = false>
__global__ void __launch_bounds__(256) k_traj_condition(const std::conditional_t<PHASE, CondPhaseArgs, CondArgs> a) {
    extern __shared__ __attribute__((aligned(16))) double cond_smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int D = c.D, Kloc = c.Kloc, Pl = a.Pl, M = a.M, KT = c.KT;
    const int tri_n = Pl * (Pl + 1) / 2;
    double* tri = cond_smem + (size_t)wave * a.wave_doubles;        // packed lower triangle
    double* smu = tri + tri_n;                                      // [Pl] the mean
    double* sv = smu + Pl;                                          // [Pl] v = L^T h
    double* sa = sv + Pl;                                           // [Pl] sqrt(b_{j+1} / b_j)
    double* sb = sa + Pl;                                           // [Pl] v_j / sqrt(b_{j+1} b_j)
    double* rows = cond_smem + (size_t)a.waves * a.wave_doubles;    // [2][M][KT]
    double* prow = sb + Pl;                                         // PHASE: [2][M][sl] this episode's rows
    float* sK = (float*)rows;                                       // PHASE: the row constants, then the base times [T]
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
        double x = 0.0;
        if (a.obs[o]) {
            if (MP == MPK_MP_PROMP && o == 1) x = k < c.nb ? cond_promp_vel_row(c, a.aux, a.init_time, k, a.steps[m]) : 0.0;
            else x = (double)vjp_row<MP>(a.c, a.A, a.aux, a.TS, o, k, a.steps[m]);
        }
        rows[i] = x;
    }
    __syncthreads();
    int rowbase[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { const int i = lane + 64 * s; rowbase[s] = i * (i + 1) / 2; }
    for (int b = blockIdx.x * a.waves + wave; b < a.B; b += gridDim.x * a.waves) {
        // ---- the episode: HBM -> float64 LDS image
        const float* Lb = a.L + (size_t)b * Pl * Pl;
#pragma unroll 8
        for (int p = lane; p < tri_n; p += 64) {                    // independent loads, consecutive inside a row
            int i, j;
            cond_unpack(p, &i, &j);
            tri[p] = (double)Lb[(size_t)i * Pl + j];
        }
        for (int i = lane; i < Pl; i += 64) smu[i] = (double)a.params[(size_t)b * c.P + c.off + i];
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
        cond_wave_sync();
        for (int m = 0; m < M; ++m) {
            for (int od = 0; od < 2 * D; ++od) {
                const int o = od >= D ? 1 : 0, d = od - o * D;      // (wave-uniform)
                if (!a.obs[o]) continue;
                const size_t at = ((size_t)b * M + m) * D + d;
                const double sigma = (double)__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.sd[o][at])));
                if (!(sigma >= 0.0) || sigma == __builtin_inf()) continue;    // +inf, NaN, negative: not observed (wave-uniform)
                const double* hr = PHASE ? prow + (o * M + m) * sl : rows + (o * M + m) * KT;
                const int n = (d + 1) * Kloc;
                // ---- c and h . mu (every lane, table order), v (lane <-> column)
                double cc = 0.0, hmu = 0.0;
                double vj[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) vj[s] = 0.0;
                if constexpr (PHASE) {
                    for (int l = 0; l < Kloc; ++l) {
                        const int row = d * Kloc + l;
                        const double hk = hr[l];
                        hmu = __builtin_fma(hk, smu[row], hmu);
                        const double* lr = tri + row * (row + 1) / 2;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int j = lane + 64 * s;
                            if (j <= row) vj[s] = __builtin_fma(hk, lr[j], vj[s]);
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
                        hmu = __builtin_fma(hk, smu[row], hmu);
                        const double* lr = tri + row * (row + 1) / 2;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int j = lane + 64 * s;
                            if (j <= row) vj[s] = __builtin_fma(hk, lr[j], vj[s]);
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
                    if (j < n) sv[j] = vj[s];
                }
                cond_wave_sync();
                // ---- suffix sums and the columns' coefficients (lane <-> the C consecutive columns from lane C)
                const int C = (n + 63) >> 6;                        // <= NS
                double vq[NS], bq[NS + 1];
                double tot = 0.0;
#pragma unroll
                for (int q = NS - 1; q >= 0; --q) {
                    const int j = lane * C + q;
                    vq[q] = (q < C && j < n) ? sv[j] : 0.0;
                    tot = __builtin_fma(vq[q], vq[q], tot);
                }
                double incl = tot;                                  // sum over this lane and the lanes above it
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) {
                    const double up = __shfl_down(incl, sh, 64);
                    if (lane + sh < 64) incl += up;
                }
                const double above = __shfl_down(incl, 1, 64);
                bq[NS] = sigma * sigma + (lane < 63 ? above : 0.0);
#pragma unroll
                for (int q = NS - 1; q >= 0; --q) bq[q] = __builtin_fma(vq[q], vq[q], bq[q + 1]);
                const double s_all = __shfl(bq[0], 0, 64);          // b_0
                // s == 0: nothing to learn from it (a NaN: left alone); wave-uniform
                if (!__builtin_amdgcn_readfirstlane(s_all > 0.0 ? 1 : 0)) { cond_wave_sync(); continue; }
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const int j = lane * C + q;
                    if (q < C && j < n) {
                        const double bj = bq[q], bn = bq[q + 1];
                        double al = 1.0, be = 0.0;
                        if (bj > 0.0) {
                            if (bn > 0.0) { al = sqrt(bn / bj); be = vq[q] / (sqrt(bn) * sqrt(bj)); }
                            else al = 0.0;
                        }
                        sa[j] = al; sb[j] = be;
                    }
                }
                const double gain = ((double)a.obs[o][at] - cc - hmu) / s_all;
                cond_wave_sync();
                // ---- the column sweep (lane <-> rows lane + 64 s)
                double w[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) w[s] = 0.0;
                for (int j0 = n - 1; j0 >= 0; j0 -= kCondAhead) {
                    double al[kCondAhead], be[kCondAhead], vv[kCondAhead], l[NS][kCondAhead];
#pragma unroll
                    for (int u = 0; u < kCondAhead; ++u) {
                        const int j = j0 - u;
                        const bool on = j >= 0;                     // (wave-uniform)
                        al[u] = on ? sa[j] : 1.0; be[u] = on ? sb[j] : 0.0; vv[u] = on ? sv[j] : 0.0;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int i = lane + 64 * s;
                            l[s][u] = (on && i < Pl && i >= j) ? tri[rowbase[s] + j] : 0.0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kCondAhead; ++u) {
                        const int j = j0 - u;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int i = lane + 64 * s;
                            if (j >= 0 && i < Pl && i >= j) tri[rowbase[s] + j] = l[s][u] * al[u] - w[s] * be[u];
                            w[s] = __builtin_fma(l[s][u], vv[u], w[s]);
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    if (i < Pl) smu[i] = __builtin_fma(w[s], gain, smu[i]);
                }
                cond_wave_sync();
            }
        }
        // ---- the posterior leaves, rounded once
        float* Lo = a.L_out + (size_t)b * Pl * Pl;
        for (int i = 0; i < Pl; ++i)
            for (int j = lane; j < Pl; j += 64) Lo[(size_t)i * Pl + j] = j <= i ? (float)tri[i * (i + 1) / 2 + j] : 0.0f;
        for (int p = lane; p < c.P; p += 64) {                      // what is not in the local block travels through unchanged
            const int i = p - c.off;
            a.params_out[(size_t)b * c.P + p] = (i >= 0 && i < Pl) ? (float)smu[i] : a.params[(size_t)b * c.P + p];
        }
        cond_wave_sync();                                           // the image is free again
    }
}

#ifndef MPK_DEVICE_ONLY
// the shapes the kernels take; MPK_ENOTIMPL with the limit in the message, under the entry's name fn, otherwise (no HIP call).  M: the
// observed steps of the call.  phase: the per-episode row source -- [2][M][Kloc + 3] more per wave, and the row constants and base times
// per workgroup where the shared route has [2][M][KT]; rows beyond mpk_phase_rows.h's 16 slots are refused
static int cond_limits(const DevCfg& c, int M, bool phase, const char* fn, size_t* lds_out, int* waves_out, int* wave_doubles_out) {
    if (const int rc = gauss_common_limits(c, fn)) return rc;
    const std::string name(fn);
    if (phase)
        if (const int rc = gauss_phase_row_limits(c, kPhaseRowSlots, fn)) return rc;
    const size_t Pl = (size_t)c.D * c.Kloc;
    const size_t wave_doubles = Pl * (Pl + 1) / 2 + 4 * Pl + (phase ? (size_t)2 * M * (c.Kloc + 3) : 0);
    const size_t shared = phase ? ((size_t)phase_rows_const_floats(c) + c.T + 1) / 2 * 2 * sizeof(float) : (size_t)2 * M * c.KT * sizeof(double);
    if (wave_doubles * sizeof(double) + shared > kLdsPerCu || Pl > 64 * kCondSlots) {
        set_error(name + ": the float64 triangle and work vectors of " + std::to_string(Pl) + " parameters (" +
                  std::to_string(wave_doubles * sizeof(double) + shared) + " bytes with one wave per workgroup) do not fit the CU's " +
                  std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    const WavePlan plan = gauss_wave_plan(wave_doubles, shared);
    if (lds_out) *lds_out = plan.lds;
    if (waves_out) *waves_out = plan.waves;
    if (wave_doubles_out) *wave_doubles_out = (int)wave_doubles;
    return MPK_OK;
}

int traj_cond_limits(const DevCfg& c, int M, size_t* lds_out, int* waves_out, int* wave_doubles_out) {
    return cond_limits(c, M, false, "mpk_trajectory_condition", lds_out, waves_out, wave_doubles_out);
}

int traj_cond_phase_limits(const DevCfg& c, int M, size_t* lds_out, int* waves_out, int* wave_doubles_out) {
    return cond_limits(c, M, true, "mpk_trajectory_phase_condition", lds_out, waves_out, wave_doubles_out);
}

int launch_traj_condition(const DevCfg& c, const SharedTables& st, const CondLaunch& q, int num_cu, void* stream, const char** kernel_name) {
    CondPhaseArgs ca{};
    size_t lds = 0;
    const int M = q.obs.M;
    const bool phase = q.phase;
    const std::string name(phase ? "mpk_trajectory_phase_condition" : "mpk_trajectory_condition");
    const int rc = phase ? traj_cond_phase_limits(c, M, &lds, &ca.waves, &ca.wave_doubles)
                         : traj_cond_limits(c, M, &lds, &ca.waves, &ca.wave_doubles);
    if (rc != MPK_OK) return rc;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    if (promp && q.obs.obs_vel && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    if (M < 1 || M > kCondMaxObs) {
        set_error(name + ": internal: the number of observed steps is outside 1.." + std::to_string(kCondMaxObs));
        return MPK_EINVAL;
    }
    ca.c = c; ca.A = st.A; ca.aux = st.aux; ca.TS = st.TS; ca.init_time = q.in.init_time;
    ca.params = q.in.params; ca.L = q.in.params_L; ca.init_pos = q.in.init_pos; ca.init_vel = q.in.init_vel;
    ca.obs[0] = q.obs.obs_pos; ca.sd[0] = q.obs.obs_pos_std; ca.obs[1] = q.obs.obs_vel; ca.sd[1] = q.obs.obs_vel_std;
    ca.params_out = q.out.params_out; ca.L_out = q.out.params_L_out;
    ca.B = q.in.B; ca.Pl = c.D * c.Kloc; ca.M = M;
    for (int m = 0; m < M; ++m) ca.steps[m] = q.obs.steps[m];
    const int blocks = gauss_blocks(q.in.B, ca.waves, lds, num_cu);
    if (phase) {
        ca.sl = c.Kloc + 3; ca.c_pad = phase_rows_const_floats(c); ca.flag = q.range_flag;
        *kernel_name = promp ? "k_traj_condition<promp, phase>" : "k_traj_condition<prodmp, phase>";
        return dispatch_mp(promp, [&](auto mp) {
            return dispatch_ns((ca.Pl + 63) / 64, [&](auto ns) {
                return launch_kernel(k_traj_condition<mp.value, ns.value, true>, dim3(blocks), dim3(64 * ca.waves), lds, stream, ca);
            });
        });
    }
    *kernel_name = promp ? "k_traj_condition<promp>" : "k_traj_condition<prodmp>";
    return dispatch_mp(promp, [&](auto mp) {
        return dispatch_ns((ca.Pl + 63) / 64, [&](auto ns) {
            return launch_kernel(k_traj_condition<mp.value, ns.value>, dim3(blocks), dim3(64 * ca.waves), lds, stream,
                                 static_cast<const CondArgs&>(ca));
        });
    });
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
