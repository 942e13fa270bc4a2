// k_episode_return_vjp: the gradient of mpk_episode_return's aggregated SimpleReacher reward in ONE launch -- the composition of
// mpk_trajectory, mpk_reacher_rollout_vjp and mpk_trajectory_vjp with nothing per step in memory (include/mpk.h: mpk_episode_return_vjp).
// Upstream gradients of the return and of the final state -> gradients w.r.t. params, init_pos, init_vel, the plan-start state and the goal.
#include "mpk_reward.h"
#include "mpk_vjp_row.h"

#include <string>

namespace mpk {

struct EvjpArgs {
    DevCfg c;                  // the configuration the tables were built for (a DMP handle: its response configuration)
    RolloutDev rc;
    const float* At;           // [TS][RS] the step-major copy of the launch's table (k_build_shared), RS = n_out * KP
    const float* aux;          // [TS]
    const float* params;       // [B, P]
    const float* init_pos;     // [B, D]
    const float* init_vel;     // [B, D]
    const double* q0;
    const double* qd0;
    const int32_t* n_steps;
    const int32_t* step0;
    const double* goal;
    const double* g_ret;       // [B] or nullptr
    const double* g_q;
    const double* g_qd;
    const float* g_cond_pos;   // [B, D] or nullptr: upstream of the forward's condition output (row tcond of the plan)
    const float* g_cond_vel;
    float* g_params;
    float* g_init_pos;
    float* g_init_vel;
    double* g_q0;
    double* g_qd0;
    double* g_goal;
    double* q_end;
    double* qd_end;
    int B, NRT, RS, steps_before_reward, agg;
};

// LDS of one wave, in doubles then floats (the launcher sizes the same carve): checkpoints [NRT][2][64] | a [16][64] | q' [16][64] |
// (-sin, cos) [2][64] | table rows of one tile [16][RS] | aux of the tile [16]
__host__ __device__ inline size_t evjp_lds_bytes(int RS, int NRT) {
    return ((size_t)NRT * 128 + 2 * 1024 + 128) * sizeof(double) + ((size_t)16 * RS + 16) * sizeof(float);
}

// k_reacher_rollout_vjp (mpk_rollout_vjp.hip) with its two memory streams replaced by arithmetic: same lane map -- one lane per
// (episode, DoF), E = 64 / D episodes per wave, one wave per workgroup --, same forward sweep to 16-step checkpoints, same replay into
// the float64 (a, q') image and same reverse chain, float64 without contraction.
//   * The desired (pos, vel) of a step are not read, they are PLANNED: the lane gathers its DoF's extended parameter column x once
//     (x_kind, the forward's gather) and contracts it with the step's table row, fp32 fmaf chains from 0 in ascending k -- the order of
//     the fp32 MFMA k_episode_return plans with, so the bits are the forward's, and with them the replayed a_t, clip mask and q'_t.
//     ProMP's velocity is the forward's difference of two such chains times aux[t].
//   * g_des_pos / g_des_vel of a step never leave the lane: the reverse chain adds R0[k][t] gp_t + R1[k][t] gv_t (vjp_row_sm) to up to
//     16 float64 column accumulators, t descending as the chain runs; each is rounded to float once and scattered (vjp_scatter).
//   * The table: a row is the same for every lane of the wave.  The wave copies the 16 step-major rows of a tile (16 RS floats, 2 KB
//     for ProDMP with 16 columns, contiguous in At) from global memory -- the table is 25 KB and lives in the L2 -- into its LDS slice
//     with coalesced 16-byte loads one tile ahead of their use, and every step reads its row back with broadcast ds_read_b128: no
//     per-workgroup copy of the whole table, so a wave's LDS is the checkpoints plus 19 KB and the staging rows and the g_r image of
//     k_reacher_rollout_vjp are gone.
//   * An upstream gradient of the forward's condition output (g_cond_pos / g_cond_vel, mpk_episode_return_vjp_cond) is one more
//     g_des term of row tcond = clamp(n - 1, 0, T - 1): the condition is a copy of the PLAN, whatever the controller reads, so it goes
//     through R0 / R1 of step tcond into the same accumulators when the chain reaches that step -- its own block, compiled into the GC
//     instantiations only, outside the CT guards.  An episode that executed nothing still gets row 0.
// The step-reward gradient is the aggregation's: g_ret (sum), g_ret / n (mean), g_ret at t = n - 1 (last).  No atomics, no waits on
// other waves.  MP: promp or prodmp rows (a DMP handle arrives as its response rows), CT: the controller, DC: the DoF count compiled
// in (0: run time), GC: an upstream gradient of the condition output is given (mpk_episode_return_vjp_cond with g_cond_pos or g_cond_vel;
// without one the instantiation is the code it was before the term existed).
template <int MP, int CT, int DC, bool GC>
__global__ void __launch_bounds__(64) k_episode_return_vjp(const EvjpArgs a) {
    static_assert(MP != MPK_MP_DMP, "promp / prodmp rows (DMP arrives as its response rows)");
    extern __shared__ __attribute__((aligned(16))) double evjp_smem[];
    const DevCfg& c = a.c;
    const int D = DC > 0 ? DC : c.D, T = c.T, B = a.B, NRT = a.NRT, KP = c.KP, RS = a.RS;
    const int E = 64 / D;
    double* const ck = evjp_smem;
    double* const aimg = ck + (size_t)NRT * 128;
    double* const qimg = aimg + 1024;
    double* const sc = qimg + 1024;
    float* const sRow = reinterpret_cast<float*>(sc + 128);
    float* const sAux = sRow + 16 * RS;
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
    const bool have_gr = a.g_ret != nullptr;
    const double gx = a.goal[2 * b], gy = a.goal[2 * b + 1];
    double pg = 0.0, dg = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll
    for (int dd = 0; dd < kMaxD; ++dd)
        if (dd == d) { pg = a.rc.pg[dd]; dg = a.rc.dg[dd]; lo = a.rc.lo[dd]; hi = a.rc.hi[dd]; }
    const double dt = a.rc.dt;
    const size_t sidx = (size_t)b * D + d;
    double q = a.q0[sidx], qd = a.qd0[sidx];
    double lq = a.g_q ? a.g_q[sidx] : 0.0, lqd = a.g_qd ? a.g_qd[sidx] : 0.0;
    // the step-reward gradient of the aggregation: sum g_ret, mean g_ret / n, last g_ret at t = n - 1
    const double gret = have_gr ? a.g_ret[b] : 0.0;
    const double gevery = a.agg == MPK_AGG_MEAN ? gret / (double)(n > 1 ? n : 1) : (a.agg == MPK_AGG_LAST ? 0.0 : gret);
    const int tlast = a.agg == MPK_AGG_LAST ? n - 1 : -1;
    // the condition output's upstream goes to row tcond = clamp(n - 1, 0, T - 1) of the plan (the forward's rule: nothing executed ->
    // row 0); it is loaded where the chain reaches that row, so nothing of it is live across the sweep and the replay
    constexpr bool have_gc = GC;

    // ---- the lane's extended parameter column: the forward's gather (every load is requested before the first one is used) ----
    float x[kMaxKP];
    {
        const float* prm = a.params + (size_t)b * c.P + c.off + d * c.Kloc;
        const float ipv = a.init_pos[sidx];
        const float ivv = MP == MPK_MP_PRODMP ? a.init_vel[sidx] : 0.0f;
        int kinds[kMaxKP];
#pragma unroll
        for (int k = 0; k < kMaxKP; ++k) {
            int loc = 0;
            kinds[k] = k < KP ? x_kind<MP>(c, k, &loc) : XK_ZERO;          // wave-uniform
            x[k] = prm[k < KP ? loc : 0];
        }
#pragma unroll
        for (int k = 0; k < kMaxKP; ++k)
            x[k] = kinds[k] == XK_PARAM ? x[k] : (kinds[k] == XK_IPOS ? ipv : (kinds[k] == XK_IVEL ? ivv : (kinds[k] == XK_ONE ? 1.0f : 0.0f)));
    }

    // ---- the table rows of a tile: 16 RS contiguous floats of At, item = lane + 64 i, registers one tile ahead, then LDS ----
    constexpr int NRR = 16 * 3 * kMaxKP / 4 / 64;         // float4 per lane (promp with 16 columns: 3)
    f32x4 rr[NRR];
    float rx = 0.0f;
#pragma unroll
    for (int i = 0; i < NRR; ++i) rr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nr4 = 4 * RS;                               // float4 per tile
    auto fetch = [&](const int rt) {
        if (rt < 0) return;                               // (wave-uniform)
        const f32x4* src = reinterpret_cast<const f32x4*>(a.At + (size_t)rt * 16 * RS);
#pragma unroll
        for (int i = 0; i < NRR; ++i)
            if (lane + 64 * i < nr4) rr[i] = src[lane + 64 * i];
        if (MP == MPK_MP_PROMP && lane < 16) rx = a.aux[rt * 16 + lane];
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NRR; ++i)
            if (lane + 64 * i < nr4) reinterpret_cast<f32x4*>(sRow)[lane + 64 * i] = rr[i];
        if (MP == MPK_MP_PROMP && lane < 16) sAux[lane] = rx;
    };
    // four columns of step i's row (broadcast reads): prodmp (pos_k, vel_k) interleaved, promp [R0[.][t] | R0[.][th] | R0[.][tl]]
    struct Row4 { float r0[4], rh[4], rl[4]; };
    auto read_row4 = [&](const int i, const int k4) {
        Row4 r;
        const f32x4* row = reinterpret_cast<const f32x4*>(sRow + i * RS);
        if (MP == MPK_MP_PROMP) {
            const int kp4 = KP >> 2;
            const f32x4 p0 = row[k4], ph = row[kp4 + k4], pl = row[2 * kp4 + k4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { r.r0[j] = p0[j]; r.rh[j] = ph[j]; r.rl[j] = pl[j]; }
        } else {
            const f32x4 u0 = row[2 * k4], u1 = row[2 * k4 + 1];
            r.r0[0] = u0[0]; r.rh[0] = u0[1]; r.r0[1] = u0[2]; r.rh[1] = u0[3];
            r.r0[2] = u1[0]; r.rh[2] = u1[1]; r.r0[3] = u1[2]; r.rh[3] = u1[3];
#pragma unroll
            for (int j = 0; j < 4; ++j) r.rl[j] = 0.0f;
        }
        return r;
    };
    // the plan at step i of the staged tile: fp32 fmaf chains in ascending k (the MFMA's accumulation order)
    auto plan = [&](const int i, double& dp, double& dv) {
        float p = 0.0f, v = 0.0f, pl = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < kMaxKP / 4; ++k4) {
            if (4 * k4 < KP) {                            // (wave-uniform)
                const Row4 r = read_row4(i, k4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (CT != MPK_CTRL_VELOCITY) p = fmaf(r.r0[j], x[4 * k4 + j], p);
                    if (CT != MPK_CTRL_POSITION) {
                        v = fmaf(r.rh[j], x[4 * k4 + j], v);
                        if (MP == MPK_MP_PROMP) pl = fmaf(r.rl[j], x[4 * k4 + j], pl);
                    }
                }
            }
        }
        if (MP == MPK_MP_PROMP && CT != MPK_CTRL_POSITION) v = (v - pl) * sAux[i];      // forward difference of fp32 positions x (1 / dt)
        dp = (double)p;
        dv = (double)v;
    };
    // one step of the forward (k_pd_rollout's operations): u, a = clip(u), qd' = qd + dt a, q' = q + dt qd'
    auto step = [&](const int i, double& u, double& av, double& qn, double& qdn) {
        double dp, dv;
        plan(i, dp, dv);
        if (CT == MPK_CTRL_MOTOR) u = pg * (dp - q) + dg * (dv - qd);
        else if (CT == MPK_CTRL_POSITION) u = dp;
        else u = dv;
        av = fmin(fmax(u, lo), hi);
        qdn = qd + dt * av;
        qn = q + dt * qdn;
    };

    // ---- forward sweep: (q, qd) at the start of every tile that executes a step ----
    fetch(NT > 0 ? 0 : -1);
    for (int rt = 0; rt + 1 < NT; ++rt) {
        stage();
        fetch(rt + 1);
        ck[(rt * 2) * 64 + lane] = q;
        ck[(rt * 2 + 1) * 64 + lane] = qd;
        __syncthreads();
#pragma unroll 4
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

    // ---- the tiles backwards: restore, replay into the (a, q') image, reverse chain with the column accumulators ----
    double gxa[kMaxKP];
#pragma unroll
    for (int k = 0; k < kMaxKP; ++k) gxa[k] = 0.0;
    // d loss / d (cond_pos, cond_vel) times the staged tile's row i, for the lanes whose tcond this step is
    auto cond_term = [&](const int i, const bool mine) {
        const float auxt = MP == MPK_MP_PROMP ? sAux[i] : 0.0f;
        const double gcp = (mine && a.g_cond_pos) ? (double)a.g_cond_pos[sidx] : 0.0;
        const double gcv = (mine && a.g_cond_vel) ? (double)a.g_cond_vel[sidx] : 0.0;
#pragma unroll
        for (int k4 = 0; k4 < kMaxKP / 4; ++k4) {
            if (4 * k4 < KP) {                            // (wave-uniform)
                const Row4 r = read_row4(i, k4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float r0, r1;
                    vjp_row_sm<MP>(r.r0[j], r.rh[j], r.rl[j], auxt, &r0, &r1);
                    if (mine) {
                        gxa[4 * k4 + j] = fma((double)r0, gcp, gxa[4 * k4 + j]);
                        gxa[4 * k4 + j] = fma((double)r1, gcv, gxa[4 * k4 + j]);
                    }
                }
            }
        }
    };
    double ggx = 0.0, ggy = 0.0;
    double qe = q, qde = qd;                      // the state after n steps (no executed tile: the plan-start state)
    for (int rt = NT - 1; rt >= 0; --rt) {
        stage();                                  // (the registers hold tile rt: the sweep's last fetch, or the previous tile's)
        fetch(rt - 1);
        __syncthreads();
        q = ck[(rt * 2) * 64 + lane];
        qd = ck[(rt * 2 + 1) * 64 + lane];
        unsigned mm = 0;
#pragma unroll 4
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
        if (rt == NT - 1) { qe = q; qde = qd; }   // (the last executed tile is replayed first)
        __syncthreads();
        // (wave-uniform, conservative: the tile's last step against every episode's step offset; the step decides exactly)
        const bool tile_paid = have_gr && __any(on && n > rt * 16 && s0 + rt * 16 + 15 >= a.steps_before_reward) != 0;
#pragma unroll 1
        for (int i = 15; i >= 0; --i) {
            const int t = rt * 16 + i;
            const bool live = t < n;
            const double av = aimg[i * 64 + lane];
            const double gr = live ? (t == tlast ? gret : gevery) : 0.0;
            const bool paid = have_gr && live && s0 + t >= a.steps_before_reward;
            if (tile_paid && __any(paid) != 0) {
                // cumulative joint angle of this lane's link, left to right as np.cumsum; then the episode's (-sin, cos) pairs
                double cj = 0.0;
                for (int j = 0; j < D; ++j) {
                    const double v = qimg[i * 64 + ebase + j];
                    cj = j == 0 ? v : (j <= d ? cj + v : cj);
                }
                double sn, cs;
                sincos_lean(cj, &sn, &cs);
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
            double gp, gv;                        // d loss / d desired (pos, vel) of this step: consumed here, never stored
            if (CT == MPK_CTRL_MOTOR) {
                gp = pg * lu; gv = dg * lu;
                lq = lq - gp;
                lqd = lqd - gv;
            } else if (CT == MPK_CTRL_POSITION) {
                gp = lu; gv = 0.0;
            } else {
                gp = 0.0; gv = lu;
            }
            const float auxt = MP == MPK_MP_PROMP ? sAux[i] : 0.0f;
#pragma unroll
            for (int k4 = 0; k4 < kMaxKP / 4; ++k4) {
                if (4 * k4 < KP) {                        // (wave-uniform)
                    const Row4 r = read_row4(i, k4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float r0, r1;
                        vjp_row_sm<MP>(r.r0[j], r.rh[j], r.rl[j], auxt, &r0, &r1);
                        if (CT != MPK_CTRL_VELOCITY) gxa[4 * k4 + j] = fma((double)r0, gp, gxa[4 * k4 + j]);
                        if (CT != MPK_CTRL_POSITION) gxa[4 * k4 + j] = fma((double)r1, gv, gxa[4 * k4 + j]);
                    }
                }
            }
            if (have_gc) {                                // (wave-uniform)
                const bool mine = t == min(max(n - 1, 0), T - 1);
                if (__any(mine) != 0) cond_term(i, mine);
            }
        }
        __syncthreads();
    }
    if (have_gc && NT == 0 && T > 0) {            // (wave-uniform) nobody executed a step: the loop did not run, every tcond is row 0
        fetch(0);
        stage();
        __syncthreads();
        cond_term(0, true);
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < kMaxKP; ++k)
            if (k < KP) vjp_scatter<MP>(c, k, (int)b, d, (float)gxa[k], a.g_params, a.g_init_pos, a.g_init_vel);
        vjp_zero_uncovered<MP>(c, (int)b, d, a.g_init_pos, a.g_init_vel);
        if (a.g_q0) a.g_q0[sidx] = lq;
        if (a.g_qd0) a.g_qd0[sidx] = lqd;
        if (a.g_goal && d == 0) { a.g_goal[2 * b] = ggx; a.g_goal[2 * b + 1] = ggy; }
        if (a.q_end) a.q_end[sidx] = qe;
        if (a.qd_end) a.qd_end[sidx] = qde;
    }
}

#ifndef MPK_DEVICE_ONLY
// what the kernel cannot take, each with the limit named (the entry point asks before it does anything, the launcher again)
int episode_return_vjp_limits(const DevCfg& c) {
    if (c.D < 1 || c.D > kMaxD || c.KP > kMaxKP) {
        set_error("mpk_episode_return_vjp: " + std::to_string(c.D) + " DoF and " + std::to_string(c.KP) + " contraction columns, the kernel "
                  "takes at most 16 of each (one lane per (episode, DoF), a DoF's column gradient in 16 accumulators of its lane)");
        return MPK_ENOTIMPL;
    }
    int TS = 0, n_out = 0;
    (void)shared_tables_floats(c, &TS, &n_out);
    const int RS = n_out * c.KP;
    if (evjp_lds_bytes(RS, (c.T + 15) / 16) > kLdsPerCu) {
        const long fixed = (long)evjp_lds_bytes(RS, 0);
        set_error("mpk_episode_return_vjp: T = " + std::to_string(c.T) + " steps: the (q, qd) checkpoints of a wave, 1 KB of LDS per 16 "
                  "steps, do not fit the CU's 160 KB; at most " + std::to_string(((long)kLdsPerCu - fixed) / 1024 * 16) + " steps with " +
                  std::to_string(c.KP) + " contraction columns");
        return MPK_ENOTIMPL;
    }
    return MPK_OK;
}

int launch_episode_return_vjp(const DevCfg& c, const SharedTables& st, const RolloutDev& rc, const EpisodeVjpAsk& q, int B, void* stream,
                              std::string* kernel_name) {
    const int D = c.D;
    if (const int lim = episode_return_vjp_limits(c); lim != MPK_OK) return lim;
    if (rc.plant_type != MPK_PLANT_DOUBLE_INTEGRATOR) {
        set_error("mpk_episode_return_vjp: the torque double integrator (MPK_PLANT_DOUBLE_INTEGRATOR) only");
        return MPK_ENOTIMPL;
    }
    if (c.mp_type == MPK_MP_DMP || shared_tables_lean(c)) {
        set_error("internal: mpk_episode_return_vjp takes promp / prodmp rows with their step-major copy");
        return MPK_EINVAL;
    }
    if (c.mp_type == MPK_MP_PROMP && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    EvjpArgs va{};
    va.c = c; va.rc = rc;
    va.RS = st.n_out * c.KP;
    va.At = st.A + (size_t)va.RS * st.TS; va.aux = st.aux;
    va.params = q.params; va.init_pos = q.init_pos; va.init_vel = q.init_vel; va.q0 = q.q0; va.qd0 = q.qd0;
    va.n_steps = q.n_steps; va.step0 = q.step0; va.goal = q.goal; va.g_ret = q.g_ret; va.g_q = q.g_q; va.g_qd = q.g_qd;
    va.g_cond_pos = q.g_cond_pos; va.g_cond_vel = q.g_cond_vel;
    va.g_params = q.g_params; va.g_init_pos = q.g_init_pos; va.g_init_vel = q.g_init_vel;
    va.g_q0 = q.g_q0; va.g_qd0 = q.g_qd0; va.g_goal = q.g_goal; va.q_end = q.q_end; va.qd_end = q.qd_end;
    va.B = B; va.NRT = (c.T + 15) / 16; va.steps_before_reward = q.steps_before_reward; va.agg = q.agg;
    const size_t lds = evjp_lds_bytes(va.RS, va.NRT);
    const int E = 64 / D;
    const unsigned blocks = (unsigned)(((long)B + E - 1) / E);
    auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(64), lds, stream, va); };
    const bool promp = c.mp_type == MPK_MP_PROMP;
    const int ct = rc.controller_type;
    const int dc = (D == 2 || D == 5 || D == 7) ? D : 0;
    *kernel_name = std::string("k_episode_return_vjp<") + (c.dmp_resp ? "dmp_resp" : (promp ? "promp" : "prodmp")) + ", " +
                   (ct == MPK_CTRL_MOTOR ? "motor" : (ct == MPK_CTRL_POSITION ? "position" : "velocity")) +
                   (dc ? ", " + std::to_string(dc) : std::string()) + ">" + ((q.g_cond_pos || q.g_cond_vel) ? " + cond" : "");
    auto by_gc = [&](auto mp_tag, auto ct_tag, auto gc_tag) -> int {
        constexpr int MP = decltype(mp_tag)::value, CT = decltype(ct_tag)::value;
        constexpr bool GC = decltype(gc_tag)::value;
        if (dc == 2) return go(k_episode_return_vjp<MP, CT, 2, GC>);
        if (dc == 5) return go(k_episode_return_vjp<MP, CT, 5, GC>);
        if (dc == 7) return go(k_episode_return_vjp<MP, CT, 7, GC>);
        return go(k_episode_return_vjp<MP, CT, 0, GC>);
    };
    auto by_d = [&](auto mp_tag, auto ct_tag) -> int {
        return (q.g_cond_pos || q.g_cond_vel) ? by_gc(mp_tag, ct_tag, std::true_type()) : by_gc(mp_tag, ct_tag, std::false_type());
    };
    auto by_ct = [&](auto mp_tag) -> int {
        using std::integral_constant;
        if (ct == MPK_CTRL_MOTOR) return by_d(mp_tag, integral_constant<int, MPK_CTRL_MOTOR>());
        if (ct == MPK_CTRL_POSITION) return by_d(mp_tag, integral_constant<int, MPK_CTRL_POSITION>());
        return by_d(mp_tag, integral_constant<int, MPK_CTRL_VELOCITY>());
    };
    return promp ? by_ct(std::integral_constant<int, MPK_MP_PROMP>()) : by_ct(std::integral_constant<int, MPK_MP_PRODMP>());
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
