// k_demo_condition: the Gaussian N(mu, L L^T) over the MP parameters conditioned on WHOLE demonstrations [B, T, D]
// (mpk_demonstration_condition) -- the information (Pl x Pl) form of mpk_demo_log_prob.hip, leaving as a valid scale_tril
#include "mpk_demo_gram.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// Notation is mpk_demo_log_prob.hip's: an entry (t, d) is kept when 0 < sigma < +inf; w = 1 / sigma^2 on kept entries, r = y - c - psi . mu_d,
//     G_d = sum_t w_td psi_t psi_t^T      q = H^T W r      M = I + tril(L)^T blockdiag(G_d) tril(L)      v = tril(L)^T q.
// The posterior of w ~ N(mu, L L^T) given the kept entries is Sigma' = tril(L) M^-1 tril(L)^T, mu' = mu + tril(L) M^-1 v.  M is factored
// from the bottom-right corner (the reverse, UL Cholesky: the left-looking loop over reversed indices), M = K^T K with K lower
// triangular, so M^-1 = K^-1 K^-T and
//     L' = tril(L) K^-1          mu' = mu + L' t,   t = K^-T v
// L' is lower triangular times lower triangular: lower triangular with diag L'_ii = L_ii / K_ii, no second factorisation; L L^T and no
// difference of covariances is ever formed.
// k_demo_condition<MP, NS>: k_demo_log_prob's layout -- one wave per episode, `waves` of them a workgroup, all float64, NS = ceil(Pl / 64)
// columns per lane -- and its accumulation, the same text (mpk_demo_gram.h): w, r, G_d, q, the per-DoF counts, M in the packed triangle.
// After M, in this order (the packed row k starts at k (k + 1) / 2, so lane <-> column reads consecutive words in every step below):
//   1. K in place, row jc = Pl - 1 .. 0 (lane <-> column i <= jc): K[jc][i] = (M[jc][i] - sum_{k > jc} K[k][i] K[k][jc]) / K[jc][jc],
//      four accumulators in a fixed order as in k_demo_log_prob's Cholesky; a pivot that is not > 0 marks the episode.
//   2. t = K^-T v, row by row from the last, t in registers (lane <-> row).
//   3. K^-1 in place, row j = 0 .. Pl - 1 (lane <-> column c < j): Kinv[j][c] = -(sum_{k = c .. j - 1} K[j][k] Kinv[k][c]) / K[j][j],
//      Kinv[j][j] = 1 / K[j][j]; the row is read completely before it is written.
//   4. Row i of L' (lane <-> column j <= i): sum_{k = j .. i} L[i][k] Kinv[k][j], row i of L in a float32 LDS image (the next row is
//      already on its way from memory), and
//   5. mu'_i = mu_i + sum_j L'[i][j] t_j from the float64 row by a fixed xor ladder,
//   6. each rounded to float32 once: the row of L' leaves at once, mu' after the last row.
// Row i of the output depends on row i of L only and is read before it is written; params is read before the first write: the outputs
// may be the inputs.  The strict upper triangle of params_L is never read and is written as exact zeros; params outside the local block is
// copied.  Nothing kept: params and tril(L) are copied bit for bit.  A sigma == 0 cannot be expressed in this form: the episode's local
// block of params_out and the lower triangle of its params_L_out are NaN (mpk_trajectory_condition takes exact observations); so is an
// episode with a pivot that is not > 0 or a t that is not finite (non-finite input).  An exactly zero column j of tril(L) makes row and
// column j of M, of K and of K^-1 those of the identity in floating point too, so column j of L' is exactly zero.  No atomics, an episode
// never leaves its wave, nothing depends on an address, and no index depends on a value that is read: the same bits from run to run,
// for any alignment, alone or in a batch; non-finite inputs never fault.
// LDS: k_demo_log_prob's images and nothing else -- per wave 8 (Pl (Pl + 1) / 2 + D Kloc^2 + 2 Pl + max(Kloc ld, 2 tc D)) + 4 Kloc ld + 64
// bytes, ld = Pl | 1; per workgroup 8 T KT + 64 (demo_log_prob_limits).  After M the q image holds mu' and the first Pl words of the
// float32 image hold the row of L: the kernel fits wherever the forward k_demo_log_prob does.
// ------------------------------------------------------------------------------------------------------------
struct DemoCondArgs : DemoGramArgs {
    float* params_out;     // [B, P]; may be params
    float* L_out;          // [B, Pl, Pl]; may be L
};

// sum_{k = lo .. hi} x[k] T[k][col], T the packed lower triangle, x a float32 or float64 LDS vector: four accumulators in a fixed order
template <typename X>
__device__ __forceinline__ double demo_row_dot(const X* x, const double* sC, int col, int lo, int hi) {
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
    int k = lo;
    int base = lo * (lo + 1) / 2 + col;                             // of T[k][col]
    for (; k + 3 <= hi; k += 4) {
        const int b1 = base + k + 1, b2 = b1 + k + 2, b3 = b2 + k + 3;
        x0 = __builtin_fma((double)x[k], sC[base], x0);
        x1 = __builtin_fma((double)x[k + 1], sC[b1], x1);
        x2 = __builtin_fma((double)x[k + 2], sC[b2], x2);
        x3 = __builtin_fma((double)x[k + 3], sC[b3], x3);
        base = b3 + k + 4;
    }
    for (; k <= hi; ++k) {
        x0 = __builtin_fma((double)x[k], sC[base], x0);
        base += k + 1;
    }
    return (x0 + x1) + (x2 + x3);
}

template <int MP, int NS, bool PHASE>
__global__ void __launch_bounds__(256) k_demo_condition(const DemoCondArgs a) {
    extern __shared__ __attribute__((aligned(16))) double demo_cond_smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int Pl = a.Pl;
    const DemoImages im = demo_images(a, demo_cond_smem, wave);
    double* sC = im.sC;                                             // packed lower triangle: M, then K, then K^-1
    double* smu = im.sq;                                            // [Pl] q, then mu'
    const double* sy = im.sy;                                       // [Pl] mu
    float* srow = im.sL;                                            // [Pl] row i of tril(L)
    if (PHASE) {
        phase_rows_stage<MP>(c, im.sK, im.sBT, tid, (int)blockDim.x);
        __syncthreads();
    } else {
        demo_stage_tables<MP>(a, im, tid);
    }
    const double nan = __builtin_nan("");
    for (int b = blockIdx.x * a.waves + wave; b < a.B; b += gridDim.x * a.waves) {
        const float* Lb = a.L + (size_t)b * Pl * Pl;
        float* Lo = a.L_out + (size_t)b * Pl * Pl;
        const DemoSums sm = demo_accumulate<MP, false, PHASE>(a, im, b, lane);
        const int n = sm.n;
        bool bad = sm.zero;                                         // (wave-uniform) a sigma == 0, a pivot that was not > 0, a t not finite
        double rr[NS], dg[NS];                                      // lane + 64 s <-> row i: v_i -> t_i; K[i][i]
#pragma unroll
        for (int s = 0; s < NS; ++s) { rr[s] = 0.0; dg[s] = 1.0; }
        if (n > 0 && !bad) {
            demo_build_M<NS>(a, im, Lb, lane, rr);
            // ---- 1. M = K^T K in place, from the last row (lane + 64 s <-> column)
            for (int jc = Pl - 1; jc >= 0; --jc) {
                double* rj = sC + jc * (jc + 1) / 2;
                double sv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    sv[s] = 0.0;
                    if (i <= jc) {
                        double x0 = rj[i], x1 = 0.0, x2 = 0.0, x3 = 0.0;
                        int k = jc + 1;
                        int base = k * (k + 1) / 2;                 // of row k
                        for (; k + 3 < Pl; k += 4) {
                            const int b1 = base + k + 1, b2 = b1 + k + 2, b3 = b2 + k + 3;
                            x0 = __builtin_fma(-sC[base + i], sC[base + jc], x0);
                            x1 = __builtin_fma(-sC[b1 + i], sC[b1 + jc], x1);
                            x2 = __builtin_fma(-sC[b2 + i], sC[b2 + jc], x2);
                            x3 = __builtin_fma(-sC[b3 + i], sC[b3 + jc], x3);
                            base = b3 + k + 4;
                        }
                        for (; k < Pl; ++k) {
                            x0 = __builtin_fma(-sC[base + i], sC[base + jc], x0);
                            base += k + 1;
                        }
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
                    if (i <= jc) rj[i] = i == jc ? root : sv[s] / root;
                }
                cond_wave_sync();
            }
            // ---- 2. t = K^-T v (row by row from the last)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int i = lane + 64 * s;
                if (i < Pl) dg[s] = sC[i * (i + 1) / 2 + i];
            }
            for (int j = Pl - 1; j >= 0; --j) {
                const double tj = demo_bcast<NS>(rr, j) / demo_bcast<NS>(dg, j);
                const double* kj = sC + j * (j + 1) / 2;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i = lane + 64 * s;
                    if (i == j) rr[s] = tj;
                    else if (i < j) rr[s] = __builtin_fma(-kj[i], tj, rr[s]);
                }
            }
            bool fin = true;
#pragma unroll
            for (int s = 0; s < NS; ++s) fin = fin && __builtin_fabs(rr[s]) < __builtin_inf();
            bad = bad || __ballot(!fin) != 0ull;
            // ---- 3. K^-1 in place, row by row (lane + 64 s <-> column)
            for (int j = 0; j < Pl; ++j) {
                double* kj = sC + j * (j + 1) / 2;
                const double inv = 1.0 / kj[j];
                double nv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int col = lane + 64 * s;
                    nv[s] = inv;
                    if (col < j) nv[s] = (0.0 - demo_row_dot(kj, sC, col, col, j - 1)) * inv;
                }
                cond_wave_sync();                                   // the row is read before it is written
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int col = lane + 64 * s;
                    if (col <= j) kj[col] = nv[s];
                }
                cond_wave_sync();
            }
        }
        const bool live = n > 0 && !bad;                            // (wave-uniform)
        // ---- 4. - 6. the rows of L' leave one by one; mu' to the q image
        float cur[NS], nxt[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = lane + 64 * s;
            cur[s] = j <= 0 ? Lb[j] : 0.0f;
            nxt[s] = 0.0f;
        }
        for (int i = 0; i < Pl; ++i) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                if (j < Pl) srow[j] = cur[s];
            }
            cond_wave_sync();
            if (i + 1 < Pl) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int j = lane + 64 * s;
                    nxt[s] = j <= i + 1 ? Lb[(size_t)(i + 1) * Pl + j] : 0.0f;
                }
            }
            float outv[NS];
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                float o = 0.0f;
                if (j <= i) {
                    if (bad) {
                        o = (float)nan;
                    } else if (!live) {
                        o = cur[s];
                    } else {
                        const double acc = demo_row_dot(srow, sC, j, j, i);
                        part = __builtin_fma(acc, rr[s], part);
                        o = (float)acc;
                    }
                }
                outv[s] = o;
            }
            cond_wave_sync();                                       // the image is read before the next row takes it
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                if (j < Pl) Lo[(size_t)i * Pl + j] = outv[s];
            }
            if (live) {
                const double tot = demo_wave_sum(part);
                if (lane == 0) smu[i] = sy[i] + tot;
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) cur[s] = nxt[s];
        }
        cond_wave_sync();
        for (int p = lane; p < c.P; p += 64) {
            const int row = p - c.off;
            float o = a.params[(size_t)b * c.P + p];
            if (row >= 0 && row < Pl) {
                if (bad) o = (float)nan;
                else if (live) o = (float)smu[row];
            }
            a.params_out[(size_t)b * c.P + p] = o;
        }
        cond_wave_sync();                                           // the images are free again
    }
}

#ifndef MPK_DEVICE_ONLY
// the launch plan: k_demo_log_prob's images (its limits, refusing under the entry's name fn) and workgroups
static int demo_condition_plan(const DevCfg& c, bool phase, const char* fn, int B, int num_cu, DemoPlan* plan, int* blocks_out) {
    const int rc = phase ? demo_phase_limits(c, plan, fn) : demo_log_prob_limits(c, plan, fn);
    if (rc != MPK_OK) return rc;
    *blocks_out = gauss_blocks(B, plan->waves, plan->lds, num_cu);
    return MPK_OK;
}

int demo_condition_launch_plan(const DevCfg& c, int B, int num_cu, bool phase, int32_t* blocks_out, int32_t* waves_out,
                               int32_t* lds_bytes_out) {
    DemoPlan plan;
    int blocks = 0;
    const int rc = demo_condition_plan(c, phase, phase ? "mpk_demonstration_phase_plan" : "mpk_demonstration_condition", B, num_cu, &plan,
                                       &blocks);
    if (rc != MPK_OK) return rc;
    if (blocks_out) *blocks_out = blocks;
    if (waves_out) *waves_out = plan.waves;
    if (lds_bytes_out) *lds_bytes_out = (int32_t)plan.lds;
    return MPK_OK;
}

int launch_demo_condition(const DevCfg& c, const SharedTables& st, const DemoCondLaunch& q, int num_cu, void* stream,
                          const char** kernel_name) {
    DemoCondArgs la{};
    DemoPlan plan;
    int blocks = 0;
    const bool phase = q.obs.phase;
    const int rc = demo_condition_plan(c, phase, phase ? "mpk_demonstration_phase_condition" : "mpk_demonstration_condition", q.in.B, num_cu,
                                       &plan, &blocks);
    if (rc != MPK_OK) return rc;
    demo_plan_args(plan, &la);
    const size_t lds = plan.lds;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    la.flag = q.obs.range_flag;
    la.c = c; la.A = st.A; la.aux = st.aux; la.TS = st.TS; la.init_time = q.in.init_time;
    la.params = q.in.params; la.L = q.in.params_L; la.init_pos = q.in.init_pos; la.init_vel = q.in.init_vel;
    la.pos = q.obs.pos; la.sd = q.obs.obs_std;
    la.params_out = q.out.params_out; la.L_out = q.out.params_L_out;
    la.B = q.in.B; la.Pl = c.D * c.Kloc; la.ld = la.Pl | 1;
    static const char* const names[2][2] = {{"k_demo_condition<prodmp>", "k_demo_condition<promp>"},
                                            {"k_demo_condition<prodmp, phase>", "k_demo_condition<promp, phase>"}};
    *kernel_name = names[phase][promp];
    return dispatch_flag(phase, [&](auto ph) {
        return dispatch_mp(promp, [&](auto mp) {
            return dispatch_ns((la.Pl + 63) / 64, [&](auto ns) {
                // (Pl > 192 passes neither route's LDS limit; the per-episode route does not carry the instantiation)
                if constexpr (ph.value && ns.value == 4) {
                    set_error("mpk_demonstration_phase_condition: internal: more than 192 non-phase parameters passed the LDS limit");
                    return (int)MPK_ENOTIMPL;
                } else {
                    return launch_kernel(k_demo_condition<mp.value, ns.value, ph.value>, dim3(blocks), dim3(64 * la.waves), lds, stream, la);
                }
            });
        });
    });
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
