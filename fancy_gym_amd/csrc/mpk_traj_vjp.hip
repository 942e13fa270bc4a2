// k_traj_vjp_tile / k_traj_vjp_generic: the vector-Jacobian product of the shared-phase trajectory map (mpk_trajectory_vjp)
#include "mpk_tile.h"
#include "mpk_run_stage.h"
#include "mpk_vjp_row.h"

namespace mpk {

// ------------------------------------------------------------------------------------------------------------
// With a phase all episodes share, pos / vel are LINEAR in a DoF's extended parameter column x = (weights, goal, y_b, v_b [, 1]):
//   pos[b, t, d] = sum_k R0[k][t] x[b, d][k],   vel[b, t, d] = sum_k R1[k][t] x[b, d][k]
// with R the k_build_shared table of the launch (weights_scale, goal_scale, tau, the relative goal and the zero-padded basis are folded
// into its rows at build time; a DMP handle's response rows are the same two-output table).  So the gradient w.r.t. x is the SAME table
// contracted over time instead of over columns,
//   gx[b, k, d] = sum_t R0[k][t] g_pos[b, t, d] + R1[k][t] g_vel[b, t, d],
// followed by the transpose of the forward kernels' input gather (x_kind, mpk_tile.h -- the forward's own function, so the packing and
// its transpose cannot drift apart): column k of DoF d goes to params[b, off + d Kloc + loc], init_pos[b, d] or init_vel[b, d]; the
// constant goal-offset column and the padding columns go nowhere.
// (vjp_row, vjp_scatter, vjp_zero_uncovered: mpk_vjp_row.h, shared with mpk_episode_vjp.hip.)
// Two routes, one arithmetic recipe each (deterministic: an episode's reduction never leaves its workgroup, plain stores, no atomics):
//   k_traj_vjp_tile     D <= 16, <= 16 columns, on the matrix cores (below).
//   k_traj_vjp_generic  everything else (the k_traj_wide shapes): one workgroup per episode, one thread per (column, DoF), float64 sum.
// ------------------------------------------------------------------------------------------------------------
struct VjpArgs {
    DevCfg c;
    const float* A;        // [n_out][KP][TS] (k_build_shared)
    const float* aux;      // [TS]
    int TS;
    const float* g_pos;    // [B, T, D] or nullptr
    const float* g_vel;    // [B, T, D] or nullptr
    float* g_params;       // [B, P] or nullptr
    float* g_init_pos;     // [B, D] or nullptr
    float* g_init_vel;     // [B, D] or nullptr
    int B, sh, G;          // tile route: log2 of the DoF padded to a power of two, episode groups of 16 >> sh
    int TP;                // T rounded up to 4: the time chunks of the tile route
    int stride;            // floats per (array, episode) gradient image in LDS
};

// ------------------------------------------------------------------------------------------------------------
// k_traj_vjp_tile<MP>: v_mfma_f32_16x16x4_f32 with M = contraction column, K = four time steps, N = (episode, DoF) -- the forward's tile
// with the roles of column and time exchanged.  A workgroup is four waves; a wave walks episode groups of NTW = 16 >> sh episodes (the
// forward's grouping: 7 DoF -> 2 episodes, 14 of the 16 tile columns used).
//   * Tables: staged once per workgroup, TRANSPOSED to [2][TP][16] (column fastest), t >= T and k >= KT zero: the A fragment of a chunk
//     (lane <-> column lane & 15, step lane >> 4) is 64 consecutive floats -- ds_read_b32 without bank conflicts.
//   * Gradients: each episode's T * D floats of g_pos (then g_vel) are one contiguous run in HBM: the wave copies them into its LDS
//     image with 16-byte loads (stage_run, mpk_run_stage.h) -- the image is shifted by the run's offset from a 16-byte boundary, so aligned HBM chunks
//     land on aligned LDS chunks whatever the pointer and T * D; up to three floats at either end go as dwords -- and zero-fills the
//     (TP - T) * D floats behind the run: the tail chunk contracts zeros, nothing is read past T.  A null array is not read at all.
//     The B fragment of a chunk is (step lane >> 4, tile column) = image[(4 ch + q) D + d] of the lane's episode; images of the
//     episodes of a group start 32 / NTW banks apart (stride), so the two 32-lane halves of a read do not collide.
//   * Accumulators [16 x 16] per array and chunk parity (four independent MFMA chains of depth T / 8), summed in a fixed order;
//     rows 4 q + r of a lane's column leave through vjp_scatter as plain dword stores (224 bytes per episode at cfg2's shape against
//     5.6 KB read).
// LDS per workgroup: 128 TP + 32 NTW stride bytes (cfg2: 12.8 + 47 KB -> two workgroups per CU).
// ------------------------------------------------------------------------------------------------------------
template <int MP>
__global__ void __launch_bounds__(256) k_traj_vjp_tile(const VjpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevCfg& c = a.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_of(tid);
    const int T = c.T, D = c.D, TD = T * D, TP = a.TP, NCH = TP >> 2;
    const int NTW = 16 >> a.sh, DP = 1 << a.sh;
    float* sAt = smem;                                              // [2][TP][16]
    float* img = smem + 2 * TP * 16 + wave * (2 * NTW * a.stride);  // [pos | vel][NTW][stride]
    for (int i = tid; i < 2 * 16 * TP; i += 256) {                  // t fastest: coalesced table reads
        const int o = i / (16 * TP), r = i - o * 16 * TP;
        const int k = r / TP, t = r - k * TP;
        sAt[(o * TP + t) * 16 + k] = (t < T && k < c.KT) ? vjp_row<MP>(a.c, a.A, a.aux, a.TS, o, k, t) : 0.0f;
    }
    __syncthreads();
    const int col = lane & 15, q = lane >> 4;
    const int bl = col >> a.sh, d = col & (DP - 1);
    const bool dvalid = d < D;
    const float* at = sAt + q * 16 + col;
    for (int g = blockIdx.x * 4 + wave; g < a.G; g += gridDim.x * 4) {
        const int b0 = g * NTW;
        // ---- gradient rows of the group -> LDS images ----
        for (int e = 0; e < NTW; ++e) {
            const int bb = b0 + e;
            if (bb >= a.B) break;
#pragma unroll
            for (int arr = 0; arr < 2; ++arr) {
                const float* src = arr ? a.g_vel : a.g_pos;
                if (!src) continue;
                stage_run(img + (arr * NTW + e) * a.stride, src, bb, TD, TP * D, lane);      // mpk_run_stage.h
            }
        }
        // (lanes read what OTHER lanes of the wave wrote: a wave's LDS operations complete in issue order, so the barrier only has to
        // keep the compiler from moving the reads above the writes -- the idiom of the forward kernels' staging)
        __builtin_amdgcn_wave_barrier();
        // ---- contraction over time ----
        const int bb = b0 + bl;
        const bool lv = dvalid && bb < a.B;
        const int bs = lv ? bb : b0;
        const float* ip = img + (lv ? bl * a.stride + q * D + d : 0);
        const float* iv = ip + NTW * a.stride;
        if (a.g_pos) ip += run_shift(a.g_pos, bs, TD);
        if (a.g_vel) iv += run_shift(a.g_vel, bs, TD);
        f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0, v0 = p0, v1 = p0;
        const int D4 = 4 * D;
        int ch = 0;
        for (; ch + 1 < NCH; ch += 2) {
            if (a.g_pos) {
                const float x0 = lv ? ip[ch * D4] : 0.0f, x1 = lv ? ip[(ch + 1) * D4] : 0.0f;
                p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[ch * 64], x0, p0, 0, 0, 0);
                p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[(ch + 1) * 64], x1, p1, 0, 0, 0);
            }
            if (a.g_vel) {
                const float x0 = lv ? iv[ch * D4] : 0.0f, x1 = lv ? iv[(ch + 1) * D4] : 0.0f;
                v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[TP * 16 + ch * 64], x0, v0, 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[TP * 16 + (ch + 1) * 64], x1, v1, 0, 0, 0);
            }
        }
        if (ch < NCH) {
            if (a.g_pos) p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[ch * 64], lv ? ip[ch * D4] : 0.0f, p0, 0, 0, 0);
            if (a.g_vel) v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[TP * 16 + ch * 64], lv ? iv[ch * D4] : 0.0f, v0, 0, 0, 0);
        }
        const f32x4 acc = (p0 + p1) + (v0 + v1);
        // ---- transposed gather: rows 4 q + r of this lane's (episode, DoF) column ----
        if (lv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) vjp_scatter<MP>(c, 4 * q + r, bb, d, acc[r], a.g_params, a.g_init_pos, a.g_init_vel);
            if (q == 0) vjp_zero_uncovered<MP>(c, bb, d, a.g_init_pos, a.g_init_vel);
        }
        // the images are free again: the next group's ds_writes are issued behind this group's ds_reads, and in-order completion of a
        // wave's LDS operations keeps them behind
        __builtin_amdgcn_wave_barrier();
    }
}

// one workgroup per episode, thread <-> (column, DoF) pairs, ascending t, float64 accumulation rounded once
template <int MP>
__global__ void __launch_bounds__(256) k_traj_vjp_generic(const VjpArgs a) {
    const DevCfg& c = a.c;
    const int T = c.T, D = c.D, tid = threadIdx.x;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const size_t base = (size_t)b * T * D;
        for (int idx = tid; idx < c.KT * D; idx += 256) {
            const int k = idx / D, d = idx - k * D;
            double s = 0.0;
            if (a.g_pos) {
                const float* g = a.g_pos + base + d;
                for (int t = 0; t < T; ++t) s = fma((double)vjp_row<MP>(a.c, a.A, a.aux, a.TS, 0, k, t), (double)g[(size_t)t * D], s);
            }
            if (a.g_vel) {
                const float* g = a.g_vel + base + d;
                for (int t = 0; t < T; ++t) s = fma((double)vjp_row<MP>(a.c, a.A, a.aux, a.TS, 1, k, t), (double)g[(size_t)t * D], s);
            }
            vjp_scatter<MP>(c, k, b, d, (float)s, a.g_params, a.g_init_pos, a.g_init_vel);
        }
        for (int d = tid; d < D; d += 256) vjp_zero_uncovered<MP>(c, b, d, a.g_init_pos, a.g_init_vel);
    }
}

#ifndef MPK_DEVICE_ONLY
int launch_traj_vjp(const DevCfg& c, const SharedTables& st, const float* g_pos, const float* g_vel, float* g_params, float* g_init_pos,
                    float* g_init_vel, int B, int num_cu, void* stream, const char** kernel_name, const Tuning& tune) {
    if (c.mp_type == MPK_MP_DMP) {
        set_error("mpk_trajectory_vjp: a DMP handle is differentiated through its response rows only");
        return MPK_ENOTIMPL;
    }
    if (c.mp_type == MPK_MP_PROMP && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    VjpArgs va{};
    va.c = c; va.A = st.A; va.aux = st.aux; va.TS = st.TS;
    va.g_pos = g_pos; va.g_vel = g_vel; va.g_params = g_params; va.g_init_pos = g_init_pos; va.g_init_vel = g_init_vel;
    va.B = B;
    const bool promp = c.mp_type == MPK_MP_PROMP;
    bool tile = c.D >= 1 && c.D <= kMaxD && c.KP <= kMaxKP && tune.vjp_generic != 1;
    size_t lds = 0;
    if (tile) {
        int sh = 0;
        while ((1 << sh) < c.D) ++sh;
        const int NTW = 16 >> sh;
        va.sh = sh;
        va.G = (B + NTW - 1) / NTW;
        va.TP = (c.T + 3) / 4 * 4;
        // a run of T * D floats shifted by up to 3, zero-filled to TP * D; images of a group's episodes 32 / NTW banks apart
        const long st_ = run_image_stride(va.TP, c.D, NTW);
        const size_t bytes = ((size_t)2 * va.TP * 16 + (size_t)4 * 2 * NTW * st_) * sizeof(float);
        if (bytes > kLdsPerCu) tile = false;        // long horizons: the generic route
        va.stride = (int)st_;
        lds = bytes;
    }
    if (tile) {
        const int per_cu = (int)(kLdsPerCu / lds) < 1 ? 1 : ((int)(kLdsPerCu / lds) > 8 ? 8 : (int)(kLdsPerCu / lds));
        const long units = ((long)va.G + 3) / 4;
        const int blocks = (int)(units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu);
        auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(256), lds, stream, va); };
        *kernel_name = c.dmp_resp ? "k_traj_vjp_tile<dmp_resp>" : (promp ? "k_traj_vjp_tile<promp>" : "k_traj_vjp_tile<prodmp>");
        return promp ? go(k_traj_vjp_tile<MPK_MP_PROMP>) : go(k_traj_vjp_tile<MPK_MP_PRODMP>);
    }
    const int blocks = B < num_cu * 8 ? B : num_cu * 8;
    *kernel_name = c.dmp_resp ? "k_traj_vjp_generic<dmp_resp>" : (promp ? "k_traj_vjp_generic<promp>" : "k_traj_vjp_generic<prodmp>");
    if (promp) hipLaunchKernelGGL(k_traj_vjp_generic<MPK_MP_PROMP>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, va);
    else hipLaunchKernelGGL(k_traj_vjp_generic<MPK_MP_PRODMP>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, va);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
