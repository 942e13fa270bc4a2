// k_reacher_rollout_vjp: the adjoint of mpk_reacher_rollout (k_pd_rollout_tiles<.., reward> / k_reacher_rollout, mpk_rollout.hip) --
// controller, clip, torque double integrator and SimpleReacher's reward transposed: upstream gradients of the step rewards and of the
// final state -> gradients w.r.t. the desired (pos, vel), the plan-start state and the goal (include/mpk.h: mpk_reacher_rollout_vjp).
#include "mpk_reward.h"

namespace mpk {

struct RvjpArgs {
    RolloutDev rc;
    const float* des_pos;
    const float* des_vel;
    const double* q0;
    const double* qd0;
    const int32_t* n_steps;
    const int32_t* step0;
    const double* goal;
    const double* g_rewards;
    const double* g_q;
    const double* g_qd;
    const float* g_cond_pos;         // [B, D] or nullptr: upstream of the forward's condition output (row tcond of the plan)
    const float* g_cond_vel;
    float* g_des_pos;
    float* g_des_vel;
    double* g_q0;
    double* g_qd0;
    double* g_goal;
    int D, B, T, NRT, steps_before_reward;
};

// LDS of one wave, in doubles then floats (the launcher sizes the same carve): checkpoints [NRT][2][64] | a [16][64] | q' [16][64] |
// (-sin, cos) [2][64] | g_r [E][16] | staging pos, vel [E * (16 D + 1)] floats each, rounded up to 4
__host__ __device__ inline size_t rvjp_stage_floats(int D) { return ((size_t)(64 / D) * (16 * D + 1) + 3) & ~(size_t)3; }
__host__ __device__ inline size_t rvjp_lds_bytes(int D, int NRT) {
    return ((size_t)NRT * 128 + 2 * 1024 + 128 + (size_t)(64 / D) * 16) * sizeof(double) + 2 * rvjp_stage_floats(D) * sizeof(float);
}

// The forward's lane map: one lane per (episode, DoF), E = 64 / D episodes per wave (k_reacher_rollout's grouping), one wave per
// workgroup, an episode never leaves its wave; float64 without contraction, the forward's operations for u, clip and plant, so the
// replayed a_t and q'_t are the forward's bits.  The adjoint needs a_t and m_t of every step and q'_t of the paid ones, the forward
// recurrence yields them first to last and the adjoint consumes them last to first: a forward sweep leaves (q, qd) at every 16-step
// tile boundary in LDS (1 KB per tile and wave), then the tiles are walked backwards -- restore the checkpoint, replay the tile into a
// 16-step float64 image of (a, q') in LDS (m as 16 bits in a register), run the reverse chain over the image.  Three serial chains of
// T steps in all (sweep, replay, reverse).  The link sums of a paid step are cross-lane within the episode's D lanes: each lane takes
// the sin / cos of its own cumulative angle, leaves (-sin, cos) in LDS and reads its episode's D pairs back -- behind ONE wave-uniform
// branch per step, skipped altogether in a tile without a paid item (the registered envs pay one step in 200).  The desired (pos, vel)
// of a tile are requested one tile ahead of their use (registers -> LDS staging); g_des_pos / g_des_vel of a tile are staged in the
// same LDS rows and leave as float4 stores on 16-byte boundaries with dword stores for the up to three floats at either end of an
// episode's run, so any pointer alignment takes the same path and gives the same bits.  No atomics, no waits on other waves.
// CT: the controller, DC: the DoF count compiled in (0: run time), GC: an upstream gradient of the condition output is given
// (mpk_reacher_rollout_vjp_cond with g_cond_pos or g_cond_vel; without one the instantiation is the code it was before the term existed).
template <int CT, int DC, bool GC>
__global__ void __launch_bounds__(64) k_reacher_rollout_vjp(const RvjpArgs a) {
    extern __shared__ __attribute__((aligned(16))) double rvjp_smem[];
    const int D = DC > 0 ? DC : a.D, T = a.T, B = a.B, NRT = a.NRT;
    const int E = 64 / D, SEGN = 16 * D, SEGS = SEGN + 1;
    double* const ck = rvjp_smem;
    double* const aimg = ck + (size_t)NRT * 128;
    double* const qimg = aimg + 1024;
    double* const sc = qimg + 1024;
    double* const grs = sc + 128;
    float* const stP = reinterpret_cast<float*>(grs + E * 16);
    float* const stV = stP + rvjp_stage_floats(D);
    const int lane = threadIdx.x;
    const int el = lane / D, d = lane - el * D;
    const long b0 = (long)blockIdx.x * E;
    const int Eon = (int)((long)B - b0 < (long)E ? (long)B - b0 : (long)E);
    const bool on = el < Eon;
    const int elc = on ? el : 0;                 // an idle lane reads its wave's first episode and writes nothing
    const long b = b0 + elc;
    const int ebase = elc * D;                   // first lane of the episode
    int n = a.n_steps ? a.n_steps[b] : T;
    n = !on ? 0 : (n < 0 ? 0 : (n < T ? n : T));
    int nmax = n;
    for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, __shfl_xor(nmax, m));
    const int NT = __builtin_amdgcn_readfirstlane((nmax + 15) >> 4);      // tiles with an executed step
    const int s0 = a.step0 ? a.step0[b] : 0;
    const bool have_gr = a.g_rewards != nullptr;
    const double gx = a.goal[2 * b], gy = a.goal[2 * b + 1];
    double pg = 0.0, dg = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll
    for (int dd = 0; dd < kMaxD; ++dd)
        if (dd == d) { pg = a.rc.pg[dd]; dg = a.rc.dg[dd]; lo = a.rc.lo[dd]; hi = a.rc.hi[dd]; }
    const double dt = a.rc.dt;
    const size_t sidx = (size_t)b * D + d;
    double q = a.q0[sidx], qd = a.qd0[sidx];
    double lq = a.g_q ? a.g_q[sidx] : 0.0, lqd = a.g_qd ? a.g_qd[sidx] : 0.0;
    // the condition output's upstream: the forward copied row tcond = clamp(n - 1, 0, T - 1) of the plan (nothing executed -> row 0),
    // whatever the controller reads, so g_cond_* joins that row of g_des_* in float64 before the one rounding; it is loaded where the
    // chain reaches the row: nothing of it is live across the replay
    constexpr bool have_gc = GC;

    // ---- the desired (pos, vel) of a tile: item = lane + 64 k over the wave's E runs of 16 D floats, registers, then LDS ----
    constexpr int KL = DC > 0 ? ((64 / (DC > 0 ? DC : 1)) * 16 * DC + 63) / 64 : 16;
    constexpr int KG = DC > 0 ? (64 / (DC > 0 ? DC : 1) + 3) / 4 : 16;
    float rp[KL], rv[KL];
    double rg[KG];
    const size_t wbase = (size_t)b0 * T * D;
    auto fetch = [&](const int rt) {
        const int nrow = min(16, T - rt * 16) * D;
#pragma unroll
        for (int k = 0; k < KL; ++k) {
            const int i = lane + 64 * k, e = i / SEGN, w = i - e * SEGN;
            const bool ok = rt >= 0 && e < Eon && w < nrow;
            const size_t off = wbase + (size_t)e * T * D + (size_t)(rt < 0 ? 0 : rt) * SEGN + w;
            rp[k] = (ok && CT != MPK_CTRL_VELOCITY) ? a.des_pos[off] : 0.0f;
            rv[k] = (ok && CT != MPK_CTRL_POSITION) ? a.des_vel[off] : 0.0f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int k = 0; k < KL; ++k) {
            const int i = lane + 64 * k, e = i / SEGN, w = i - e * SEGN;
            if (e < E) { stP[e * SEGS + w] = rp[k]; stV[e * SEGS + w] = rv[k]; }
        }
    };
    // upstream reward gradients of a tile: item = lane + 64 k -> (episode i / 16, step i % 16)
    auto fetch_gr = [&](const int rt) {
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            const int i = lane + 64 * k, e = i >> 4, t = rt * 16 + (i & 15);
            rg[k] = (e < Eon && t < T) ? a.g_rewards[(size_t)(b0 + e) * T + t] : 0.0;
        }
    };
    auto stage_gr = [&]() {
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            const int i = lane + 64 * k;
            if (i < E * 16) grs[i] = rg[k];
        }
    };
    // one step of the forward (k_pd_rollout's operations): u, a = clip(u), qd' = qd + dt a, q' = q + dt qd'
    auto step = [&](const int i, double& u, double& av, double& qn, double& qdn) {
        const double dp = (double)stP[elc * SEGS + i * D + d], dv = (double)stV[elc * SEGS + i * D + d];
        if (CT == MPK_CTRL_MOTOR) u = pg * (dp - q) + dg * (dv - qd);
        else if (CT == MPK_CTRL_POSITION) u = dp;
        else u = dv;
        av = fmin(fmax(u, lo), hi);
        qdn = qd + dt * av;
        qn = q + dt * qdn;
    };
    // a tile's staged gradient rows -> global: per episode a run of nrow floats; 16-byte stores on 16-byte boundaries, dwords at the ends
    auto store_tile = [&](float* const g, const float* const st, const int rt) {
        const int nrow = min(16, T - rt * 16) * D;
        const int CH = (nrow + 3) / 4 + 1;
        for (int it = lane; it < Eon * CH; it += 64) {
            const int e = it / CH, c = it - e * CH;
            float* const seg = g + wbase + (size_t)e * T * D + (size_t)rt * SEGN;
            const int ae = (int)((reinterpret_cast<uintptr_t>(seg) >> 2) & 3);
            const int w0 = 4 * c - ae;
            const float* const s = st + e * SEGS;
            if (w0 >= 0 && w0 + 4 <= nrow) {
                const f32x4 v = {s[w0], s[w0 + 1], s[w0 + 2], s[w0 + 3]};
                *reinterpret_cast<f32x4*>(seg + w0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int w = w0 + j;
                    if (w >= 0 && w < nrow) seg[w] = s[w];
                }
            }
        }
    };
    auto store_both = [&](const int rt) {
        __syncthreads();
        if (a.g_des_pos) store_tile(a.g_des_pos, stP, rt);
        if (a.g_des_vel) store_tile(a.g_des_vel, stV, rt);
        __syncthreads();
    };
    const bool want_rows = a.g_des_pos != nullptr || a.g_des_vel != nullptr;

    // ---- forward sweep: (q, qd) at the start of every tile that executes a step ----
    fetch(NT > 0 ? 0 : -1);
    for (int rt = 0; rt + 1 < NT; ++rt) {
        stage();
        fetch(rt + 1);
        ck[(rt * 2) * 64 + lane] = q;
        ck[(rt * 2 + 1) * 64 + lane] = qd;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            double u, av, qn, qdn;
            step(i, u, av, qn, qdn);
            const bool live = rt * 16 + i < n;
            q = live ? qn : q;
            qd = live ? qdn : qd;
        }
        __syncthreads();
    }
    if (NT > 0) {
        ck[((NT - 1) * 2) * 64 + lane] = q;
        ck[((NT - 1) * 2 + 1) * 64 + lane] = qd;
    }

    // ---- rows of the tiles nobody executes: exact zeros ----
    if (want_rows) {
        for (int rt = NRT - 1; rt >= NT; --rt) {
            if (on) {
#pragma unroll
                for (int i = 0; i < 16; ++i) { stP[elc * SEGS + i * D + d] = 0.0f; stV[elc * SEGS + i * D + d] = 0.0f; }
                if (have_gc && rt == 0) {                     // (a wave that executed nothing: every episode's tcond is row 0)
                    stP[elc * SEGS + d] = a.g_cond_pos ? a.g_cond_pos[sidx] : 0.0f;
                    stV[elc * SEGS + d] = a.g_cond_vel ? a.g_cond_vel[sidx] : 0.0f;
                }
            }
            store_both(rt);
        }
    }

    // ---- the tiles backwards: restore, replay into the (a, q') image, reverse chain ----
    double ggx = 0.0, ggy = 0.0;
    for (int rt = NT - 1; rt >= 0; --rt) {
        stage();                                  // (the registers hold tile rt: the sweep's last fetch, or the previous tile's)
        fetch(rt - 1);
        if (have_gr) fetch_gr(rt);
        __syncthreads();
        q = ck[(rt * 2) * 64 + lane];
        qd = ck[(rt * 2 + 1) * 64 + lane];
        unsigned mm = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            double u, av, qn, qdn;
            step(i, u, av, qn, qdn);
            const bool live = rt * 16 + i < n;
            // the derivative of clip: 1 inside and AT a bound (torch.clamp's convention)
            mm |= (live && lo <= u && u <= hi) ? (1u << i) : 0u;
            aimg[i * 64 + lane] = live ? av : 0.0;
            qimg[i * 64 + lane] = qn;
            q = live ? qn : q;
            qd = live ? qdn : qd;
        }
        if (have_gr) stage_gr();
        __syncthreads();
        // (wave-uniform, conservative: the tile's last step against every episode's step offset; the step decides exactly)
        const bool tile_paid = have_gr && __any(on && n > rt * 16 && s0 + rt * 16 + 15 >= a.steps_before_reward) != 0;
#pragma unroll 1
        for (int i = 15; i >= 0; --i) {
            const int t = rt * 16 + i;
            const bool live = t < n;
            const double av = aimg[i * 64 + lane];
            const double gr = (have_gr && live) ? grs[elc * 16 + i] : 0.0;
            const bool paid = have_gr && live && s0 + t >= a.steps_before_reward;
            if (tile_paid && __any(paid) != 0) {
                // cumulative joint angle of this lane's link, left to right as np.cumsum; then the episode's (-sin, cos) pairs
                double c = 0.0;
                for (int j = 0; j < D; ++j) {
                    const double v = qimg[i * 64 + ebase + j];
                    c = j == 0 ? v : (j <= d ? c + v : c);
                }
                double sn, cs;
                sincos_lean(c, &sn, &cs);
                sc[lane] = 0.0 - sn;
                sc[64 + lane] = cs;
                __syncthreads();
                double ex = 0.0, ey = 0.0, sx = 0.0, sy = 0.0;
                for (int l = 0; l < D; ++l) {
                    const double ms = sc[ebase + l], cc = sc[64 + ebase + l];
                    ex = l == 0 ? cc : ex + cc;
                    ey = l == 0 ? 0.0 - ms : ey - ms;
                    sx = l >= d ? sx + ms : sx;
                    sy = l >= d ? sy + cc : sy;
                }
                const double dx = ex - gx, dy = ey - gy;
                const double dist = sqrt(dx * dx + dy * dy);
                if (paid && dist > 0.0) {
                    lq = lq - gr * (dx * sx + dy * sy) / dist;
                    ggx = ggx + gr * dx / dist;
                    ggy = ggy + gr * dy / dist;
                }
                __syncthreads();
            }
            const double lqd_n = lqd + dt * lq;
            const double la = dt * lqd_n - 2.0 * av * gr;
            const double lu = (live && ((mm >> i) & 1u)) ? la : 0.0;
            lqd = live ? lqd_n : lqd;
            float gp, gv;
            if (CT == MPK_CTRL_MOTOR) {
                const double kp = pg * lu, kd = dg * lu;
                gp = (float)kp; gv = (float)kd;
                lq = lq - kp;
                lqd = lqd - kd;
            } else if (CT == MPK_CTRL_POSITION) {
                gp = (float)lu; gv = 0.0f;
            } else {
                gp = 0.0f; gv = (float)lu;
            }
            if (have_gc && t == min(max(n - 1, 0), T - 1)) {
                const double gcp = a.g_cond_pos ? (double)a.g_cond_pos[sidx] : 0.0, gcv = a.g_cond_vel ? (double)a.g_cond_vel[sidx] : 0.0;
                const double kp = CT == MPK_CTRL_MOTOR ? pg * lu : (CT == MPK_CTRL_POSITION ? lu : 0.0);
                const double kd = CT == MPK_CTRL_MOTOR ? dg * lu : (CT == MPK_CTRL_POSITION ? 0.0 : lu);
                gp = (float)(kp + gcp); gv = (float)(kd + gcv);
            }
            if (on && want_rows) { stP[elc * SEGS + i * D + d] = gp; stV[elc * SEGS + i * D + d] = gv; }
        }
        if (want_rows) store_both(rt);
        else __syncthreads();
    }
    if (on) {
        if (a.g_q0) a.g_q0[sidx] = lq;
        if (a.g_qd0) a.g_qd0[sidx] = lqd;
        if (a.g_goal && d == 0) { a.g_goal[2 * b] = ggx; a.g_goal[2 * b + 1] = ggy; }
    }
}

#ifndef MPK_DEVICE_ONLY
int launch_reacher_rollout_vjp(const RolloutDev& rc, int D, const float* des_pos, const float* des_vel, const double* q0,
                               const double* qd0, const int32_t* n_steps, const int32_t* step0, const double* goal,
                               int steps_before_reward, const double* g_rewards, const double* g_q, const double* g_qd,
                               const float* g_cond_pos, const float* g_cond_vel, float* g_des_pos, float* g_des_vel, double* g_q0, double* g_qd0, double* g_goal, int B, int T,
                               void* stream, const char** kernel_name) {
    if (D < 1 || D > kMaxD) {
        set_error("mpk_reacher_rollout_vjp: at most 16 DoF (one lane per (episode, DoF), the links of a paid step summed inside a wave)");
        return MPK_ENOTIMPL;
    }
    if (rc.plant_type != MPK_PLANT_DOUBLE_INTEGRATOR) {
        set_error("mpk_reacher_rollout_vjp: the torque double integrator (MPK_PLANT_DOUBLE_INTEGRATOR) only");
        return MPK_ENOTIMPL;
    }
    RvjpArgs va{};
    va.rc = rc; va.des_pos = des_pos; va.des_vel = des_vel; va.q0 = q0; va.qd0 = qd0; va.n_steps = n_steps; va.step0 = step0;
    va.goal = goal; va.g_rewards = g_rewards; va.g_q = g_q; va.g_qd = g_qd; va.g_cond_pos = g_cond_pos;
    va.g_cond_vel = g_cond_vel; va.g_des_pos = g_des_pos; va.g_des_vel = g_des_vel;
    va.g_q0 = g_q0; va.g_qd0 = g_qd0; va.g_goal = g_goal;
    va.D = D; va.B = B; va.T = T; va.NRT = (T + 15) / 16; va.steps_before_reward = steps_before_reward;
    const size_t lds = rvjp_lds_bytes(D, va.NRT);
    if (lds > kLdsPerCu) {
        const long fixed = (long)rvjp_lds_bytes(D, 0);
        set_error("mpk_reacher_rollout_vjp: T = " + std::to_string(T) + " steps: the (q, qd) checkpoints of a wave, 1 KB of LDS per 16 "
                  "steps, do not fit the CU's 160 KB; at most " + std::to_string(((long)kLdsPerCu - fixed) / 1024 * 16) + " steps at " +
                  std::to_string(D) + " DoF");
        return MPK_ENOTIMPL;
    }
    const int E = 64 / D;
    const unsigned blocks = (unsigned)(((long)B + E - 1) / E);
    auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(64), lds, stream, va); };
    const bool gc = g_cond_pos != nullptr || g_cond_vel != nullptr;
    auto by_gc = [&](auto ct_tag, auto gc_tag, const char* n2, const char* n5, const char* n7, const char* n0) -> int {
        constexpr int CT = decltype(ct_tag)::value;
        constexpr bool GC = decltype(gc_tag)::value;
        if (D == 2) { *kernel_name = n2; return go(k_reacher_rollout_vjp<CT, 2, GC>); }
        if (D == 5) { *kernel_name = n5; return go(k_reacher_rollout_vjp<CT, 5, GC>); }
        if (D == 7) { *kernel_name = n7; return go(k_reacher_rollout_vjp<CT, 7, GC>); }
        *kernel_name = n0;
        return go(k_reacher_rollout_vjp<CT, 0, GC>);
    };
    // (the <.., cond> variants are named by appending " + cond" to the name of the plain instantiation)
    auto by_d = [&](auto ct_tag, const char* n2, const char* n5, const char* n7, const char* n0) -> int {
        if (!gc) return by_gc(ct_tag, std::false_type(), n2, n5, n7, n0);
        const int r = by_gc(ct_tag, std::true_type(), n2, n5, n7, n0);
        *kernel_name = cond_variant_name(*kernel_name);
        return r;
    };
    using std::integral_constant;
    switch (rc.controller_type) {
        case MPK_CTRL_MOTOR:
            return by_d(integral_constant<int, MPK_CTRL_MOTOR>(), "k_reacher_rollout_vjp<motor, 2>", "k_reacher_rollout_vjp<motor, 5>",
                        "k_reacher_rollout_vjp<motor, 7>", "k_reacher_rollout_vjp<motor>");
        case MPK_CTRL_POSITION:
            return by_d(integral_constant<int, MPK_CTRL_POSITION>(), "k_reacher_rollout_vjp<position, 2>", "k_reacher_rollout_vjp<position, 5>",
                        "k_reacher_rollout_vjp<position, 7>", "k_reacher_rollout_vjp<position>");
        default:
            return by_d(integral_constant<int, MPK_CTRL_VELOCITY>(), "k_reacher_rollout_vjp<velocity, 2>", "k_reacher_rollout_vjp<velocity, 5>",
                        "k_reacher_rollout_vjp<velocity, 7>", "k_reacher_rollout_vjp<velocity>");
    }
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
