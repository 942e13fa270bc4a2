// k_traj_std_tile: the standard deviation of the shared-phase trajectory under a Gaussian over the parameters (mpk_trajectory_std)
#include "mpk_tile.h"
#include "mpk_run_stage.h"
#include "mpk_vjp_row.h"
#include "mpk_gauss_launch.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// With a phase all episodes share, pos[b, t, d] = sum_k R0[k][t] x[b, d][k] (mpk_traj_vjp.hip has the whole story), and x_kind (mpk_tile.h,
// the forward's own gather) says which columns k of x are read from params, at params[off + d Kloc + loc(k)].  With the parameters
// Gaussian, covariance L L^T (L lower triangular, [Pl, Pl], Pl = D Kloc, in the user's units -- the scales, the relative goal and the zero
// padding are folded into the table's rows), the trajectory's standard deviation is the norm of the table row times L,
//   pos_std[b, t, d] = sqrt(sum_j (sum_k R0[k][t] X[k][j])^2),   X[k][j] = L[d Kloc + loc(k), j] for the parameter columns, else 0,
// and vel_std the same with R1: the FACTOR form, a sum of squares, never the quadratic form r^T (L L^T) r, which cancels where the
// covariance is rank deficient and goes negative.
// k_traj_std_tile<MP, KM>: v_mfma_f32_16x16x4_f32 with M = 16 columns j of L, K = the 4 KM table columns in chunks of four, N = 16 time
// steps -- the forward's tile with L's columns in the episodes' place and transposed, so that the sum over j is the sum over the ROWS of
// the C tile: a lane adds the squares of its four rows in registers, across the j tiles too, and only the four lane quarters are left to
// add up (M = time would leave the sixteen lanes of a quarter, per row).  Those partial sums S[quarter][step] sit in the lanes exactly
// as the B operand of one more MFMA wants them, so ones[16 x 4] . S puts the total of every step into every row: one instruction per
// row tile and output instead of cross-lane exchanges, the same hardware sum every time.
//   * One wave per episode, four waves a workgroup; an episode never leaves its wave, plain stores, no atomics.
//   * Tables: staged once per workgroup as [2][KP][pitch], t fastest, t >= T and k >= KT zero: the B fragment of (chunk m, row tile)
//     is R[4 m + (lane >> 4)][16 rt + (lane & 15)] -- 16 consecutive floats per lane quarter, the quarters `pitch` apart (pitch = 16 mod
//     32: the two quarters of a 32-lane half land on different banks).  An output that is not asked for is neither staged nor computed.
//   * Loop order: passes of kStdTiles row tiles; inside a pass the (DoF, j tile) pairs in sequence.  The pass's B fragments depend on
//     neither and are read from LDS ONCE per pass into registers (2 kStdTiles KM of them), and the sums of a pass are one register per
//     (row tile, output): the horizon costs no registers.  A horizon beyond 16 kStdTiles steps re-reads L from the cache once per pass.
//   * A fragment of (DoF d, j tile, chunk m): L[d Kloc + loc(4 m + (lane >> 4)), 16 jt + (lane & 15)] straight from HBM / L2, 64
//     consecutive bytes per lane quarter; the fragments of the next TWO pairs of the sequence are in flight while one is contracted
//     (across the DoF boundary too).  0 without a load where the column is no parameter or j exceeds the row index: the strict upper
//     triangle is never read.  L is lower triangular, so DoF d needs the j tiles below (d + 1) Kloc only.
//   * At a DoF's last j tile: the quarter sums through the ones-MFMA into the wave's LDS image of the episode's [T, D] block, shifted
//     by the block's offset from a 16-byte boundary (run_shift); the image -- variances -- leaves as the episode's contiguous run of
//     T D floats with 16-byte stores, the square root taken on the way out (store_run<true>: one sqrt per element, by all 64 lanes).
// The values and the order they are added in depend on nothing but the episode's own L: the same bits from run to run, for any
// alignment of the three pointers, alone or in a batch, with one output or both.
// LDS per workgroup: 8 KP pitch + 32 image bytes (cfg2: 7 KB + 22 KB); traj_std_limits refuses what exceeds a CU's.
// ------------------------------------------------------------------------------------------------------------
constexpr int kStdTiles = 8;

struct StdArgs {
    DevCfg c;
    const float* A;        // [n_out][KP][TS] (k_build_shared)
    const float* aux;      // [TS]
    int TS;
    const float* L;        // [B, Pl, Pl]; the lower triangle is read
    float* pos_std;        // [B, T, D] or nullptr
    float* vel_std;        // [B, T, D] or nullptr
    int B, Pl;
    int pitch;             // floats per table row in LDS
    int image;             // floats per (wave, output) image in LDS
};

// s + the squares of a lane's four C-tile rows: four dependent FMAs (explicit: the build does not contract)
__device__ __forceinline__ float sum_squares(const f32x4& acc, float s) {
    return __builtin_fmaf(acc[3], acc[3], __builtin_fmaf(acc[2], acc[2], __builtin_fmaf(acc[1], acc[1], __builtin_fmaf(acc[0], acc[0], s))));
}

template <int MP, int KM>
__global__ void __launch_bounds__(256) k_traj_std_tile(const StdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int T = c.T, D = c.D, TD = T * D, Kloc = c.Kloc, Pl = a.Pl;
    constexpr int KP = 4 * KM;
    const int pitch = a.pitch, NRT = (T + 15) >> 4;
    const bool wp = a.pos_std != nullptr, wv = a.vel_std != nullptr;
    float* sR = smem;                                               // [2][KP][pitch]
    float* img = smem + 2 * KP * pitch + wave * (2 * a.image);      // [pos | vel][image]
    for (int i = tid; i < 2 * KP * pitch; i += 256) {               // t fastest: coalesced table reads
        const int o = i / (KP * pitch), r = i - o * KP * pitch;
        const int k = r / pitch, t = r - k * pitch;
        sR[i] = ((o ? wv : wp) && t < T && k < c.KT) ? vjp_row<MP>(a.c, a.A, a.aux, a.TS, o, k, t) : 0.0f;
    }
    __syncthreads();
    const int col = lane & 15, q = lane >> 4;
    // the lane's table column of every chunk: is it a parameter, and which of the DoF's local block
    bool isp[KM];
    int loc[KM];
#pragma unroll
    for (int m = 0; m < KM; ++m) {
        const int k = 4 * m + q;
        int l;
        const int kind = x_kind<MP>(c, k, &l);
        isp[m] = k < c.KT && kind == XK_PARAM;
        loc[m] = l;
    }
    const float* rq = sR + q * pitch + col;
    // j tiles of DoF d: the columns up to its last row (at least one, so that a DoF without parameters still writes its zeros)
    auto njt = [&](int d) { const int n = ((d + 1) * Kloc + 15) >> 4; return n > 0 ? n : 1; };
    for (int b = blockIdx.x * 4 + wave; b < a.B; b += gridDim.x * 4) {
        const float* Lb = a.L + (size_t)b * Pl * Pl;
        float* ip = img + (wp ? run_shift(a.pos_std, b, TD) : 0);
        float* iv = img + a.image + (wv ? run_shift(a.vel_std, b, TD) : 0);
        // the A fragment of (DoF d, j tile jt); zeros behind the last DoF
        auto load_frag = [&](int d, int jt, float (&f)[KM]) {
            const int j = jt * 16 + col;
#pragma unroll
            for (int m = 0; m < KM; ++m) {
                const int row = d * Kloc + loc[m];
                f[m] = (d < D && isp[m] && j <= row) ? Lb[(size_t)row * Pl + j] : 0.0f;
            }
        };
        auto advance = [&](int& d, int& jt) {
            if (d < D && ++jt >= njt(d)) { jt = 0; ++d; }
        };
        for (int rt0 = 0; rt0 < NRT; rt0 += kStdTiles) {
            // ---- the pass's B fragments, once
            float bp[kStdTiles][KM], bv[kStdTiles][KM];
#pragma unroll
            for (int u = 0; u < kStdTiles; ++u) {
                const bool on = rt0 + u < NRT;                      // (wave-uniform)
#pragma unroll
                for (int m = 0; m < KM; ++m) {
                    bp[u][m] = (on && wp) ? rq[(rt0 + u) * 16 + 4 * m * pitch] : 0.0f;
                    bv[u][m] = (on && wv) ? rq[(rt0 + u) * 16 + (KP + 4 * m) * pitch] : 0.0f;
                }
            }
            float sp[kStdTiles], sv[kStdTiles];
#pragma unroll
            for (int u = 0; u < kStdTiles; ++u) { sp[u] = 0.0f; sv[u] = 0.0f; }
            // ---- the (DoF, j tile) pairs in sequence, two fragments ahead
            int d0 = 0, j0 = 0, d1 = 0, j1 = 0;
            advance(d1, j1);
            int d2 = d1, j2 = j1;
            advance(d2, j2);
            float f0[KM], f1[KM];
            load_frag(d0, j0, f0);
            load_frag(d1, j1, f1);
            while (d0 < D) {
                float f2[KM];
                load_frag(d2, j2, f2);
#pragma unroll
                for (int u = 0; u < kStdTiles; ++u) {
                    if (rt0 + u >= NRT) break;                      // (wave-uniform)
                    if (wp) {
                        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int m = 0; m < KM; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f0[m], bp[u][m], acc, 0, 0, 0);
                        sp[u] = sum_squares(acc, sp[u]);
                    }
                    if (wv) {
                        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int m = 0; m < KM; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f0[m], bv[u][m], acc, 0, 0, 0);
                        sv[u] = sum_squares(acc, sv[u]);
                    }
                }
                if (j0 + 1 >= njt(d0)) {                            // (wave-uniform) the DoF's last j tile
                    // rows 4 q + r of the C tiles are summed in the lane; the four lane quarters: ones[16 x 4] . S[quarter][step]
#pragma unroll
                    for (int u = 0; u < kStdTiles; ++u) {
                        if (rt0 + u >= NRT) break;                  // (wave-uniform)
                        const int t = (rt0 + u) * 16 + col;
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        if (wp) {
                            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, sp[u], zero, 0, 0, 0);
                            if (q == 0 && t < T) ip[t * D + d0] = s[0];
                        }
                        if (wv) {
                            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, sv[u], zero, 0, 0, 0);
                            if (q == 0 && t < T) iv[t * D + d0] = s[0];
                        }
                        sp[u] = 0.0f; sv[u] = 0.0f;
                    }
                }
#pragma unroll
                for (int m = 0; m < KM; ++m) { f0[m] = f1[m]; f1[m] = f2[m]; }
                d0 = d1; j0 = j1; d1 = d2; j1 = j2;
                advance(d2, j2);
            }
        }
        // (lanes read what OTHER lanes of the wave wrote: a wave's LDS operations complete in issue order, so the barrier only has to
        // keep the compiler from moving the reads above the writes -- the idiom of the forward kernels' staging)
        __builtin_amdgcn_wave_barrier();
        if (wp) store_run<true>(a.pos_std, img, b, TD, lane);       // mpk_run_stage.h: the roots leave
        if (wv) store_run<true>(a.vel_std, img + a.image, b, TD, lane);
        // the images are free again: the next episode's ds_writes are issued behind these ds_reads
        __builtin_amdgcn_wave_barrier();
    }
}

#ifndef MPK_DEVICE_ONLY
// the shapes the kernel takes; MPK_ENOTIMPL with the limit in the message otherwise (no HIP call)
int traj_std_limits(const DevCfg& c, size_t* lds_out, int* pitch_out, int* image_out) {
    if (const int rc = gauss_common_limits(c, "mpk_trajectory_std")) return rc;
    const int T16 = (c.T + 15) / 16 * 16;
    const int pitch = T16 % 32 == 16 ? T16 : T16 + 16;
    const int image = (c.T * c.D + 3 + 3) / 4 * 4;                  // the run shifted by up to three floats, whole 16-byte chunks
    const size_t bytes = ((size_t)2 * c.KP * pitch + (size_t)4 * 2 * image) * sizeof(float);
    if (bytes > kLdsPerCu) {
        set_error("mpk_trajectory_std: the tables and the four waves' output images (" + std::to_string(bytes) + " bytes for " +
                  std::to_string(c.T) + " steps x " + std::to_string(c.D) + " DoF, " + std::to_string(c.KP) + " columns) do not fit the CU's " +
                  std::to_string(kLdsPerCu) + " bytes of LDS");
        return MPK_ENOTIMPL;
    }
    if (lds_out) *lds_out = bytes;
    if (pitch_out) *pitch_out = pitch;
    if (image_out) *image_out = image;
    return MPK_OK;
}

template <int MP>
static int launch_traj_std_mp(const StdArgs& sa, int km, int blocks, size_t lds, void* stream) {
    auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(256), lds, stream, sa); };
    switch (km) {
        case 1: return go(k_traj_std_tile<MP, 1>);
        case 2: return go(k_traj_std_tile<MP, 2>);
        case 3: return go(k_traj_std_tile<MP, 3>);
        default: return go(k_traj_std_tile<MP, 4>);
    }
}

int launch_traj_std(const DevCfg& c, const SharedTables& st, const float* params_L, float* pos_std, float* vel_std, int B, int num_cu,
                    void* stream, const char** kernel_name) {
    StdArgs sa{};
    size_t lds = 0;
    const int rc = traj_std_limits(c, &lds, &sa.pitch, &sa.image);
    if (rc != MPK_OK) return rc;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    if (promp && vel_std && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    if (c.KP < 4 || c.KP % 4) {
        set_error("mpk_trajectory_std: internal: the table's padded column count is no positive multiple of four");
        return MPK_EINVAL;
    }
    sa.c = c; sa.A = st.A; sa.aux = st.aux; sa.TS = st.TS;
    sa.L = params_L; sa.pos_std = pos_std; sa.vel_std = vel_std;
    sa.B = B; sa.Pl = c.D * c.Kloc;
    const int per_cu = (int)(kLdsPerCu / lds) < 1 ? 1 : ((int)(kLdsPerCu / lds) > 8 ? 8 : (int)(kLdsPerCu / lds));
    const long units = ((long)B + 3) / 4;
    const int blocks = (int)(units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu);
    *kernel_name = promp ? "k_traj_std_tile<promp>" : "k_traj_std_tile<prodmp>";
    return promp ? launch_traj_std_mp<MPK_MP_PROMP>(sa, c.KP / 4, blocks, lds, stream)
                 : launch_traj_std_mp<MPK_MP_PRODMP>(sa, c.KP / 4, blocks, lds, stream);
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
