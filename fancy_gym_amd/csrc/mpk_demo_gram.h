// What the two kernels of the information (Pl x Pl) form share (mpk_demo_log_prob.hip: the likelihood of whole demonstrations and its
// gradient; mpk_demo_condition.hip: the posterior given them): the launch arguments both read, the LDS images of one wave, the staging of
// the position rows, the accumulation of w, r, G_d, q and the per-DoF counts over the steps, and the packed lower triangle of
// M = I + tril(L)^T blockdiag(G_d) tril(L) with v = tril(L)^T q.  Both kernels compile this text, so what they accumulate is the same
// bits.  Notation and the LDS formula: mpk_demo_log_prob.hip.
// Two row sources, a template flag PHASE on the accumulation and on both kernels.  PHASE = false: the phase all episodes share, the T rows
// [T][KT] staged once per workgroup from the launch's table.  PHASE = true: a per-episode phase (tau / delay given at the front of the
// episode's params row): no workgroup-wide row image; for each chunk of tc steps the wave evaluates its own episode's rows, lane <-> step,
// with the forward's device functions (mpk_phase_rows.h, what k_phase_fit evaluates) into a per-wave float64 chunk image [tc][sl]:
// Kloc entries regrouped by local parameter, then ca | cb | cc of the step's given part c[t, d] = ca init_pos[d] + cb init_vel[d] + cc.
// The accumulation reads the chunk image where it reads rows + t KT otherwise; after G_d, q, the counts and the sums nothing knows where
// the rows came from.
#pragma once
#include "mpk_tile.h"
#include "mpk_vjp_row.h"
#include "mpk_cond_rows.h"
#include "mpk_phase_rows.h"

namespace mpk {

constexpr int kDemoSlots = 4;                                       // rows / columns per lane at most (NS = ceil(Pl / 64))

struct DemoGramArgs {
    DevCfg c;
    const float* A;        // [n_out][KP][TS] (k_build_shared)
    const float* aux;      // [TS]
    int TS;
    float init_time;       // the tables' (init_time_shared)
    const float* params;   // [B, P]
    const float* L;        // [B, Pl, Pl]; the lower triangle is read
    const float* init_pos; // [B, D] or nullptr (promp: zeros)
    const float* init_vel;
    const float* pos;      // [B, T, D] the demonstrations
    const float* sd;       // [B, T, D] their standard deviations
    int B, Pl;
    int ld;                // words between the rows of the X and L images (odd)
    int tc;                // steps per chunk of the accumulation
    int scratch;           // float64 words of the X image / the chunk's w and r images: max(Kloc ld, 2 tc D)
    int waves;             // per workgroup
    int wave_doubles;      // float64 words of LDS per wave
    // PHASE only (0 / nullptr otherwise)
    int sl;                // words between the rows of the chunk image: Kloc + 3, odd
    int chunk;             // float64 words of the chunk image: tc sl
    int c_pad;             // floats of the workgroup's row constants (phase_rows_const_floats)
    int32_t* flag;         // prodmp: raised beyond the pre-computed range (k_phase_fit's)
};

#ifndef MPK_DEVICE_ONLY
void demo_plan_args(const DemoPlan& plan, DemoGramArgs* la);    // mpk_demo_log_prob.hip
#endif

// the LDS images of one wave, and the two the workgroup shares
struct DemoImages {
    double* sC;            // packed lower triangle: M, then its factor
    double* sG;            // [D][Kloc][Kloc] the Gram matrices
    double* sq;            // [Pl] q
    double* sy;            // [Pl] mu
    double* sX;            // [Kloc][ld] X_d; the accumulation's w | r [tc][D]
    float* sL;             // [Kloc][ld] the rows of tril(L)'s block d
    int* snd;              // [D] kept observations per DoF
    double* rows;          // [T][KT] the position rows (per workgroup)
    int* kof;              // [Kloc] the table column read from local parameter l, or -1 (per workgroup)
    double* sE;            // PHASE: [tc][sl] the chunk's rows by local parameter | ca cb cc (per wave)
    float* sK;             // PHASE: the row constants (per workgroup; 8-byte aligned), then
    float* sBT;            // PHASE: [T] the base times (per workgroup)
};

__device__ __forceinline__ DemoImages demo_images(const DemoGramArgs& a, double* smem, int wave) {
    const DevCfg& c = a.c;
    DemoImages im;
    im.sE = smem + (size_t)wave * a.wave_doubles;
    im.sC = im.sE + a.chunk;
    im.sG = im.sC + a.Pl * (a.Pl + 1) / 2;
    im.sq = im.sG + c.D * c.Kloc * c.Kloc;
    im.sy = im.sq + a.Pl;
    im.sX = im.sy + a.Pl;
    im.sL = (float*)(im.sX + a.scratch);
    im.snd = (int*)(im.sL + ((c.Kloc * a.ld + 1) & ~1));
    im.rows = smem + (size_t)a.waves * a.wave_doubles;
    im.kof = (int*)(im.rows + c.T * c.KT);
    im.sK = (float*)im.rows;
    im.sBT = im.sK + a.c_pad;
    return im;
}

// the sum over the wave by a fixed xor ladder: the same bits in every lane
__device__ __forceinline__ double demo_wave_sum(double x) {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x += __shfl_xor(x, sh, 64);
    return x;
}

// element j (wave-uniform) of a vector held as lane + 64 s: every lane gets it
template <int NS>
__device__ __forceinline__ double demo_bcast(const double (&x)[NS], int j) {
    const int sj = j >> 6;
    double v = x[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) v = sj == s ? x[s] : v;
    return __shfl(v, j & 63, 64);
}

// the rows of tril(L)'s block d as a float32 LDS image [Kloc][ld] (entries j <= row; exact 0 beyond), and X_d = G_d tril(L)[rows of d]
// [Kloc][ld] in float64 (columns < (d + 1) Kloc; exact 0 beyond): lane <-> column
template <int NS>
__device__ __forceinline__ void demo_stage_block(const float* Lb, const double* Gd, float* sL, double* sX, int d, int Kloc, int Pl, int ld,
                                                 int lane) {
    for (int l = 0; l < Kloc; ++l) {
        const int row = d * Kloc + l;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = lane + 64 * s;
            if (j < Pl) sL[l * ld + j] = j <= row ? Lb[(size_t)row * Pl + j] : 0.0f;
        }
    }
    cond_wave_sync();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = lane + 64 * s;
        if (j < Pl) {
            for (int k = 0; k < Kloc; ++k) {
                double acc = 0.0;
                for (int l = 0; l < Kloc; ++l) acc = __builtin_fma(Gd[k * Kloc + l], (double)sL[l * ld + j], acc);
                sX[k * ld + j] = acc;
            }
        }
    }
    cond_wave_sync();
}

// the T position rows [T][KT] (cond_obs_row, o = 0) and the table column of every local parameter, once per workgroup
template <int MP>
__device__ __forceinline__ void demo_stage_tables(const DemoGramArgs& a, const DemoImages& im, int tid) {
    const DevCfg& c = a.c;
    const int T = c.T, KT = c.KT;
    for (int i = tid; i < T * KT; i += blockDim.x) {
        const int t = i / KT, k = i - t * KT;
        im.rows[i] = cond_obs_row<MP>(c, a.A, a.aux, a.TS, a.init_time, 0, k, t);
    }
    if (tid < c.Kloc) {
        int found = -1;
        for (int k = 0; k < KT; ++k) {
            int loc;
            if (x_kind<MP>(c, k, &loc) == XK_PARAM && loc == tid) found = k;
        }
        im.kof[tid] = found;
    }
    __syncthreads();
}

// what the accumulation leaves besides the images (wave-uniform): s = sum w r^2, lsig = sum over kept of log sigma^2 (SUMS only; 0
// otherwise), n the entries kept, zero: a sigma == 0 was read
struct DemoSums {
    double s, lsig;
    int n;
    bool zero;
};

// episode b: mu to sy; w, r, then G_d, q and the per-DoF counts over the steps, a chunk at a time
template <int MP, bool SUMS, bool PHASE>
__device__ __forceinline__ DemoSums demo_accumulate(const DemoGramArgs& a, const DemoImages& im, int b, int lane) {
    const DevCfg& c = a.c;
    const int D = c.D, Kloc = c.Kloc, Pl = a.Pl, T = c.T, KT = c.KT, tc = a.tc;
    const int KK = Kloc * Kloc, Kt2 = Kloc * (Kloc + 1) / 2;
    double* sG = im.sG;
    double* sq = im.sq;
    double* sy = im.sy;
    int* snd = im.snd;
    const double* rows = im.rows;
    const int* kof = im.kof;
    for (int i = lane; i < D * KK; i += 64) sG[i] = 0.0;
    for (int i = lane; i < Pl; i += 64) {
        sq[i] = 0.0;
        sy[i] = (double)a.params[(size_t)b * c.P + c.off + i];
    }
    if (lane < D) snd[lane] = 0;
    cond_wave_sync();
    double s_l = 0.0, lsig_l = 0.0;
    int n_l = 0;
    bool zero_l = false;
    double* sw = im.sX;
    double* sr = im.sX + tc * D;
    double* sE = im.sE;
    const int sl = a.sl;
    PhaseEpisode ep{};
    if (PHASE) ep = phase_rows_episode<MP>(c, a.params + (size_t)b * c.P, a.init_time);
    // (PHASE) which of the given columns exist: a ProDMP's init_pos / init_vel, a zero-padded ProMP's init_pos
    const bool use_ip = a.init_pos && (MP == MPK_MP_PRODMP || KT > c.nb), use_iv = a.init_vel && MP == MPK_MP_PRODMP;
    for (int t0 = 0; t0 < T; t0 += tc) {
        const int nt = T - t0 < tc ? T - t0 : tc;
        if (PHASE) {                                            // lane <-> step: this episode's rows of the chunk
            for (int tt = lane; tt < nt; tt += 64) {
                double e[kPhaseRowSlots], ca, cb, cg;
                phase_rows_eval<MP>(c, ep, im.sK, im.sBT[t0 + tt], a.flag, e, ca, cb, cg);
                double* er = sE + tt * sl;
#pragma unroll
                for (int k = 0; k < kPhaseRowSlots; ++k)
                    if (k < Kloc) er[k] = e[k];
                er[Kloc] = ca; er[Kloc + 1] = cb; er[Kloc + 2] = cg;
            }
            cond_wave_sync();
        }
        for (int e = lane; e < nt * D; e += 64) {               // lane <-> (t, d): coalesced
            const int tt = e / D, d = e - tt * D;
            const size_t at = ((size_t)b * T + t0) * D + e;
            const double sig = (double)a.sd[at], yv = (double)a.pos[at];
            const bool keep = sig > 0.0 && sig != __builtin_inf();   // +inf, NaN, negative: not observed
            zero_l = zero_l || sig == 0.0;
            const double* hr = PHASE ? sE + tt * sl : rows + (t0 + tt) * KT;
            double cc = 0.0, hmu = 0.0;
            if (PHASE) {
                for (int l = 0; l < Kloc; ++l) hmu = __builtin_fma(hr[l], sy[d * Kloc + l], hmu);
                cc = hr[Kloc + 2];
                if (use_iv) cc = __builtin_fma(hr[Kloc + 1], (double)a.init_vel[(size_t)b * D + d], cc);
                if (use_ip) cc = __builtin_fma(hr[Kloc], (double)a.init_pos[(size_t)b * D + d], cc);
            }
            for (int k = 0; !PHASE && k < KT; ++k) {
                int loc;
                const int kind = x_kind<MP>(c, k, &loc);
                const double hk = hr[k];
                if (kind == XK_PARAM) {
                    hmu = __builtin_fma(hk, sy[d * Kloc + loc], hmu);
                } else if (kind == XK_IPOS) {
                    if (a.init_pos) cc = __builtin_fma(hk, (double)a.init_pos[(size_t)b * D + d], cc);
                } else if (kind == XK_IVEL) {
                    if (a.init_vel) cc = __builtin_fma(hk, (double)a.init_vel[(size_t)b * D + d], cc);
                } else if (kind == XK_ONE) {
                    cc += hk;
                }
            }
            const double r = keep ? yv - cc - hmu : 0.0;
            const double w = keep ? 1.0 / (sig * sig) : 0.0;
            sw[e] = w;
            sr[e] = r;
            if (keep) {
                if (SUMS) {
                    s_l = __builtin_fma(w * r, r, s_l);
                    lsig_l += log(sig * sig);
                }
                ++n_l;
            }
        }
        cond_wave_sync();
        for (int e = lane; e < D * Kt2; e += 64) {              // lane <-> (d, k >= l)
            const int d = e / Kt2, rem = e - d * Kt2;
            int k = 0;
            while ((k + 1) * (k + 2) / 2 <= rem) ++k;
            const int l = rem - k * (k + 1) / 2;
            const int ck = PHASE ? k : kof[k], cl = PHASE ? l : kof[l];
            double acc = sG[d * KK + k * Kloc + l];
            if (ck >= 0 && cl >= 0) {
                for (int tt = 0; tt < nt; ++tt) {
                    const double* hr = PHASE ? sE + tt * sl : rows + (t0 + tt) * KT;
                    acc = __builtin_fma(sw[tt * D + d] * hr[ck], hr[cl], acc);
                }
            }
            sG[d * KK + k * Kloc + l] = acc;
            sG[d * KK + l * Kloc + k] = acc;
        }
        for (int row = lane; row < Pl; row += 64) {             // lane <-> row of q
            const int d = row / Kloc, ck = PHASE ? row - d * Kloc : kof[row - d * Kloc];
            double acc = sq[row];
            if (ck >= 0) {
                for (int tt = 0; tt < nt; ++tt)
                    acc = __builtin_fma(sw[tt * D + d] * sr[tt * D + d], PHASE ? sE[tt * sl + ck] : rows[(t0 + tt) * KT + ck], acc);
            }
            sq[row] = acc;
        }
        if (lane < D) {
            int cnt = snd[lane];
            for (int tt = 0; tt < nt; ++tt) cnt += sw[tt * D + lane] > 0.0 ? 1 : 0;
            snd[lane] = cnt;
        }
        cond_wave_sync();
    }
    DemoSums out;
    out.s = SUMS ? demo_wave_sum(s_l) : 0.0;
    out.lsig = SUMS ? demo_wave_sum(lsig_l) : 0.0;
    int n = n_l;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) n += __shfl_xor(n, sh, 64);
    out.n = __builtin_amdgcn_readfirstlane(n);
    out.zero = __ballot(zero_l) != 0ull;
    return out;
}

// M = I + sum_d tril(L)_d^T G_d tril(L)_d to the packed lower triangle sC, and rr (lane + 64 s <-> row, zero on entry) += v = tril(L)^T q.
// A DoF with nothing kept is skipped: G_d = 0, q_d = 0
template <int NS>
__device__ __forceinline__ void demo_build_M(const DemoGramArgs& a, const DemoImages& im, const float* Lb, int lane, double (&rr)[NS]) {
    const int D = a.c.D, Kloc = a.c.Kloc, Pl = a.Pl, ld = a.ld;
    const int KK = Kloc * Kloc;
    double* sC = im.sC;
    const double* sq = im.sq;
    const double* sX = im.sX;
    const float* sL = im.sL;
    for (int i = lane; i < Pl * (Pl + 1) / 2; i += 64) sC[i] = 0.0;
    cond_wave_sync();
    for (int i = lane; i < Pl; i += 64) sC[i * (i + 1) / 2 + i] = 1.0;
    cond_wave_sync();
    for (int d = 0; d < D; ++d) {
        if (__builtin_amdgcn_readfirstlane(im.snd[d]) == 0) continue;
        const int jm = (d + 1) * Kloc;
        demo_stage_block<NS>(Lb, im.sG + d * KK, im.sL, im.sX, d, Kloc, Pl, ld, lane);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = lane + 64 * s;
            if (j < jm) {
                for (int l = 0; l < Kloc; ++l) rr[s] = __builtin_fma((double)sL[l * ld + j], sq[d * Kloc + l], rr[s]);
            }
        }
        for (int i = 0; i < jm; ++i) {
            const int base = i * (i + 1) / 2;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                if (j <= i) {
                    double acc = sC[base + j];
                    for (int l = 0; l < Kloc; ++l) acc = __builtin_fma((double)sL[l * ld + i], sX[l * ld + j], acc);
                    sC[base + j] = acc;
                }
            }
        }
        cond_wave_sync();
    }
}

}  // namespace mpk
