// k_hole_rollout_vjp: the adjoint of mpk_hole_reacher_rollout2 (k_hole_rollout, mpk_hole.hip) with the episode's end and collision
// verdict frozen -- controller, clip, direct-velocity plant (hole_control / hole_plant_step, mpk_plant.h, in numpy's dtypes), the squared
// distance to the hole's bottom and the acceleration / velocity costs transposed: upstream gradients of the step rewards, of their
// aggregate and of the final state -> gradients w.r.t. the desired (pos, vel), the plan-start state and the hole
// (include/mpk.h: mpk_hole_reacher_rollout_vjp).  The collision geometry is never evaluated: n_exec and collided are the forward's.
#include "mpk_reward.h"

namespace mpk {

struct HvjpArgs {
    RolloutDev rc;
    const float* des_pos;
    const float* des_vel;
    const double* q0;
    const double* qd0;
    const int32_t* n_exec;
    const int32_t* step0;
    const double* hole;              // [B, 3] (x, width, depth)
    const uint8_t* collided;         // [B] or nullptr (= 0)
    const double* g_ret;             // [B] or nullptr
    const double* g_rewards;         // [B, T] or nullptr
    const double* g_q;
    const double* g_qd;
    const float* g_cond_pos;         // [B, D] or nullptr: upstream of the forward's condition output (row tcond of the plan)
    const float* g_cond_vel;
    float* g_des_pos;
    float* g_des_vel;
    double* g_q0;
    double* g_qd0;
    double* g_hole;                  // [B, 3]
    double penalty;
    int D, B, T, NRT, steps_before_reward, agg;
};

// LDS of one wave, in doubles then floats (the launcher sizes the same carve): checkpoints [NRT][2][64] | acc [16][64] | qd' [16][64]
// (vel_acc only) | q' of the paid steps [2][64] (vel_acc: [1][64]) | (-sin, cos) [2][64] | g_r [E][16] | staging pos, vel
// [E * (16 D + 1)] floats each, rounded up to 4.  An episode pays the distance on at most two steps (vel_acc: one), so their q' rows
// stand in for a 16-step image: at T = 200, D = 5 both rewards stay at four workgroups per CU (32 864 and 40 544 bytes)
__host__ __device__ inline size_t hvjp_stage_floats(int D) { return ((size_t)(64 / D) * (16 * D + 1) + 3) & ~(size_t)3; }
__host__ __device__ inline size_t hvjp_lds_bytes(int D, int NRT, int rew) {
    const size_t images = rew == MPK_HOLE_REW_VEL_ACC ? 2 * 1024 + 64 : 1024 + 128;
    return ((size_t)NRT * 128 + images + 128 + (size_t)(64 / D) * 16) * sizeof(double) + 2 * hvjp_stage_floats(D) * sizeof(float);
}

// k_reacher_rollout_vjp's lane map and schedule (mpk_rollout_vjp.hip) around HoleReacher's plant and reward: one lane per (episode, DoF),
// E = 64 / D episodes per wave, one wave per workgroup, an episode never leaves its wave.  A forward sweep leaves (q, qd) at every
// 16-step tile boundary in LDS (1 KB per tile and wave); the tiles are then walked backwards -- restore the checkpoint, replay the tile
// with the forward's operations in the forward's dtypes (float32 action, acc and dt * a from the episode's second env step on for the
// velocity / position controllers, float64 for the motor controller) into a 16-step float64 image of acc (vel_acc: and qd') in LDS (the
// clip mask as 16 bits in a register, q' of the episode's paid steps in one LDS row each), run the reverse chain over the image.  A paid
// step -- the env step steps_before_reward, and the colliding step (simple) -- needs the episode's link sums: each lane takes the sin /
// cos of its own cumulative angle (its episode's q' row), leaves (-sin, cos) in LDS and reads its episode's D pairs back, behind ONE
// wave-uniform branch per step, skipped altogether in a tile without a paid item (an episode has at most two).  Desired rows are
// requested one tile ahead (registers -> LDS staging); g_des_pos / g_des_vel of a tile are staged in the same LDS rows and leave as
// float4 stores on 16-byte boundaries with dword stores for the up to three floats at either end of an episode's run: any pointer
// alignment takes the same path and gives the same bits.  No atomics, no waits on other waves.  CT: the controller, REW:
// MPK_HOLE_REW_SIMPLE / _VEL_ACC, DC: the DoF count compiled in (0: run time), GC: an upstream gradient of the condition output is given
// (mpk_hole_reacher_rollout_vjp_cond with g_cond_pos or g_cond_vel; without one the instantiation is the code it was before the term
// existed).
template <int CT, int REW, int DC, bool GC>
__global__ void __launch_bounds__(64) k_hole_rollout_vjp(const HvjpArgs a) {
    extern __shared__ __attribute__((aligned(16))) double hvjp_smem[];
    constexpr bool VA = REW == MPK_HOLE_REW_VEL_ACC;
    const int D = DC > 0 ? DC : a.D, T = a.T, B = a.B, NRT = a.NRT;
    const int E = 64 / D, SEGN = 16 * D, SEGS = SEGN + 1;
    double* const ck = hvjp_smem;
    double* const cimg = ck + (size_t)NRT * 128;             // acc_t
    double* const vimg = cimg + 1024;                        // qd'_t as the velocity cost reads it (vel_acc)
    double* const qrow = vimg + (VA ? 1024 : 0);             // q' of the step that pays at steps_before_reward | of the colliding step
    double* const sc = qrow + (VA ? 64 : 128);
    double* const grs = sc + 128;
    float* const stP = reinterpret_cast<float*>(grs + E * 16);
    float* const stV = stP + hvjp_stage_floats(D);
    const int lane = threadIdx.x;
    const int el = lane / D, d = lane - el * D;
    const long b0 = (long)blockIdx.x * E;
    const int Eon = (int)((long)B - b0 < (long)E ? (long)B - b0 : (long)E);
    const bool on = el < Eon;
    const int elc = on ? el : 0;                 // an idle lane reads its wave's first episode and writes nothing
    const long b = b0 + elc;
    const int ebase = elc * D;                   // first lane of the episode
    int n = a.n_exec ? a.n_exec[b] : T;
    n = !on ? 0 : (n < 0 ? 0 : (n < T ? n : T));
    int nmax = n;
    for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, __shfl_xor(nmax, m));
    const int NT = __builtin_amdgcn_readfirstlane((nmax + 15) >> 4);      // tiles with an executed step
    const int s0 = a.step0 ? a.step0[b] : 0;
    const bool coll = a.collided ? a.collided[b] != 0 : false;
    const bool have_grw = a.g_rewards != nullptr;
    const bool have_up = have_grw || a.g_ret != nullptr;
    // the aggregate's share of a step's reward gradient: g_ret w_t, w_t = 1 (sum), 1 / n (mean), [t == n - 1] (last)
    double gw = a.g_ret ? a.g_ret[b] : 0.0;
    if (a.agg == MPK_AGG_MEAN) gw = n > 0 ? gw / (double)n : 0.0;
    const bool agg_last = a.agg == MPK_AGG_LAST;
    // the paid steps of this episode (plan-local): the env step that pays the distance, and simple's colliding step
    const int tp_step = (VA ? 199 : a.steps_before_reward) - s0;
    const int tp_coll = (!VA && coll) ? n - 1 : -1;
    const double hx = a.hole[3 * b], floor_y = 0.0 - a.hole[3 * b + 2];
    double pg = 0.0, dg = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll
    for (int dd = 0; dd < kMaxD; ++dd)
        if (dd == d) { pg = a.rc.pg[dd]; dg = a.rc.dg[dd]; lo = a.rc.lo[dd]; hi = a.rc.hi[dd]; }
    const double dt = a.rc.dt;
    const float dt32 = (float)dt;
    const double dt32d = (double)dt32;
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
    // one step of the forward for this lane's DoF: hole_control, then hole_plant_step's operations in their dtypes
    auto step = [&](const int i, const int t, bool& m, double& acc, double& qn, double& qdn) {
        const double dp = (double)stP[elc * SEGS + i * D + d], dv = (double)stV[elc * SEGS + i * D + d];
        double u;
        if (CT == MPK_CTRL_MOTOR) u = pg * (dp - q) + dg * (dv - qd);
        else if (CT == MPK_CTRL_POSITION) u = dp;
        else u = dv;
        // the derivative of clip: 1 inside and AT a bound (torch.clamp's convention)
        m = lo <= u && u <= hi;
        const double av = fmin(fmax(u, lo), hi);
        if (CT == MPK_CTRL_MOTOR) {
            acc = (av - qd) / dt;
            qdn = av;
            qn = q + dt * qdn;
        } else if (s0 + t > 0) {
            const float a32 = (float)av;
            const float acc32 = (a32 - (float)qd) / dt32;
            acc = (double)acc32;
            qdn = (double)a32;
            qn = q + (double)(dt32 * a32);
        } else {
            acc = (av - qd) / dt;
            qdn = av;
            qn = q + (double)(dt32 * (float)av);
        }
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
            bool m;
            double acc, qn, qdn;
            step(i, rt * 16 + i, m, acc, qn, qdn);
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

    // ---- the tiles backwards: restore, replay into the acc (and qd') image and the paid q' rows, reverse chain ----
    constexpr double c_acc = VA ? -1e-6 : -5e-8;
    double ghx = 0.0, ghd = 0.0;
    for (int rt = NT - 1; rt >= 0; --rt) {
        stage();                                  // (the registers hold tile rt: the sweep's last fetch, or the previous tile's)
        fetch(rt - 1);
        if (have_grw) fetch_gr(rt);
        __syncthreads();
        q = ck[(rt * 2) * 64 + lane];
        qd = ck[(rt * 2 + 1) * 64 + lane];
        unsigned mm = 0;
        double qp_step = 0.0, qp_coll = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bool m;
            double acc, qn, qdn;
            step(i, rt * 16 + i, m, acc, qn, qdn);
            const bool live = rt * 16 + i < n;
            mm |= (live && m) ? (1u << i) : 0u;
            cimg[i * 64 + lane] = live ? acc : 0.0;
            qp_step = rt * 16 + i == tp_step ? qn : qp_step;
            if (!VA) qp_coll = rt * 16 + i == tp_coll ? qn : qp_coll;
            // (hole_vel_cost squares the float32 action of the velocity / position controllers)
            if (VA) vimg[i * 64 + lane] = !live ? 0.0 : (CT == MPK_CTRL_MOTOR ? qdn : (double)(float)qdn);
            q = live ? qn : q;
            qd = live ? qdn : qd;
        }
        // (a row is read in the tile of its paid step only, after that tile's replay wrote it: what the other tiles leave there is not read)
        qrow[lane] = qp_step;
        if (!VA) qrow[64 + lane] = qp_coll;
        if (have_grw) stage_gr();
        __syncthreads();
        // (wave-uniform: does a paid step of a live episode fall into this tile?)
        const int tlo = rt * 16, thi = rt * 16 + 15;
        const bool mine = (tp_step >= tlo && tp_step <= thi && tp_step < n) || (tp_coll >= tlo && tp_coll <= thi);
        const bool tile_paid = have_up && __any(on && mine) != 0;
#pragma unroll 1
        for (int i = 15; i >= 0; --i) {
            const int t = rt * 16 + i;
            const bool live = t < n;
            const bool last = coll && t == n - 1;
            double gr = 0.0;
            if (have_up && live) gr = (have_grw ? grs[elc * 16 + i] : 0.0) + ((!agg_last || t == n - 1) ? gw : 0.0);
            const bool paid = have_up && live && (t == tp_step || t == tp_coll);
            if (tile_paid && __any(paid) != 0) {
                // cumulative joint angle of this lane's link, left to right as np.cumsum; then the episode's (-sin, cos) pairs
                const double* const qr = qrow + ((VA || t == tp_step) ? 0 : 64) + ebase;
                double c = 0.0;
                for (int j = 0; j < D; ++j) {
                    const double v = qr[j];
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
                if (paid) {
                    const double dx = ex - hx, dy = ey - floor_y;
                    // the distance weight: simple 1; vel_acc 1 + penalty on a colliding step 199
                    const double w = VA ? 1.0 + a.penalty * (last ? 1.0 : 0.0) : 1.0;
                    const double k2 = 2.0 * gr * w;
                    lq = lq - k2 * (dx * sx + dy * sy);
                    ghx = ghx + k2 * dx;
                    ghd = ghd - k2 * dy;
                }
                __syncthreads();
            }
            // the operation's own dt: float64 for the motor controller and on the episode's first env step, else the float32 one
            const double del = (CT == MPK_CTRL_MOTOR || s0 + t == 0) ? dt : dt32d;
            const double delq = CT == MPK_CTRL_MOTOR ? dt : dt32d;
            const double acc = cimg[i * 64 + lane];
            double lqdn = lqd;
            if (VA) lqdn = lqdn + (-2e-4 * gr) * vimg[i * 64 + lane];
            const double lacc = 2.0 * c_acc * gr * acc;
            const double la = (delq * lq + lqdn) + lacc / del;
            const double lu = (live && ((mm >> i) & 1u)) ? la : 0.0;
            lqd = live ? 0.0 - lacc / del : lqd;
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
        if (a.g_hole && d == 0) { a.g_hole[3 * b] = ghx; a.g_hole[3 * b + 1] = 0.0; a.g_hole[3 * b + 2] = ghd; }
    }
}

#ifndef MPK_DEVICE_ONLY
// the largest horizon whose checkpoints fit beside the fixed carve
static long hvjp_max_steps(int D, int rew) { return ((long)kLdsPerCu - (long)hvjp_lds_bytes(D, 0, rew)) / 1024 * 16; }

int launch_hole_rollout_vjp(const HoleVjpLaunch& h, int B, int T, int D, void* stream, const char** kernel_name) {
    if (D < 1 || D > kMaxD) {
        set_error("mpk_hole_reacher_rollout_vjp: at most 16 DoF (one lane per (episode, DoF), the links of a paid step summed inside a wave)");
        return MPK_ENOTIMPL;
    }
    HvjpArgs va{};
    va.rc = h.rc; va.des_pos = h.des_pos; va.des_vel = h.des_vel; va.q0 = h.q0; va.qd0 = h.qd0; va.n_exec = h.n_exec; va.step0 = h.step0;
    va.hole = h.hole; va.collided = h.collided; va.g_ret = h.g_ret; va.g_rewards = h.g_rewards; va.g_q = h.g_q; va.g_qd = h.g_qd;
    va.g_cond_pos = h.g_cond_pos; va.g_cond_vel = h.g_cond_vel;
    va.g_des_pos = h.g_des_pos; va.g_des_vel = h.g_des_vel; va.g_q0 = h.g_q0; va.g_qd0 = h.g_qd0; va.g_hole = h.g_hole;
    va.penalty = h.penalty; va.D = D; va.B = B; va.T = T; va.NRT = (T + 15) / 16; va.steps_before_reward = h.steps_before_reward;
    va.agg = h.agg;
    const size_t lds = hvjp_lds_bytes(D, va.NRT, h.rew_fct);
    if (lds > kLdsPerCu) {
        set_error("mpk_hole_reacher_rollout_vjp: T = " + std::to_string(T) + " steps: the (q, qd) checkpoints of a wave, 1 KB of LDS per "
                  "16 steps, do not fit the CU's 160 KB; at most " + std::to_string(hvjp_max_steps(D, h.rew_fct)) + " steps at " +
                  std::to_string(D) + " DoF");
        return MPK_ENOTIMPL;
    }
    const int E = 64 / D;
    const unsigned blocks = (unsigned)(((long)B + E - 1) / E);
    auto go = [&](auto kern) { return launch_kernel(kern, dim3(blocks), dim3(64), lds, stream, va); };
    // names[rew][0: D = 5, 1: run-time D]
    const bool gc = h.g_cond_pos != nullptr || h.g_cond_vel != nullptr;
    auto by_gc = [&](auto ct_tag, auto gc_tag, const char* const (&names)[2][2]) -> int {
        constexpr int CT = decltype(ct_tag)::value;
        constexpr bool GC = decltype(gc_tag)::value;
        const bool va_rew = h.rew_fct == MPK_HOLE_REW_VEL_ACC;
        *kernel_name = names[va_rew ? 1 : 0][D == 5 ? 0 : 1];
        if (va_rew)
            return D == 5 ? go(k_hole_rollout_vjp<CT, MPK_HOLE_REW_VEL_ACC, 5, GC>) : go(k_hole_rollout_vjp<CT, MPK_HOLE_REW_VEL_ACC, 0, GC>);
        return D == 5 ? go(k_hole_rollout_vjp<CT, MPK_HOLE_REW_SIMPLE, 5, GC>) : go(k_hole_rollout_vjp<CT, MPK_HOLE_REW_SIMPLE, 0, GC>);
    };
    // (the <.., cond> variants are named by appending " + cond" to the name of the plain instantiation)
    auto by_rew = [&](auto ct_tag, const char* const (&names)[2][2]) -> int {
        if (!gc) return by_gc(ct_tag, std::false_type(), names);
        const int r = by_gc(ct_tag, std::true_type(), names);
        *kernel_name = cond_variant_name(*kernel_name);
        return r;
    };
    using std::integral_constant;
    static const char* const motor[2][2] = {{"k_hole_rollout_vjp<motor, simple, 5>", "k_hole_rollout_vjp<motor, simple>"},
                                            {"k_hole_rollout_vjp<motor, vel_acc, 5>", "k_hole_rollout_vjp<motor, vel_acc>"}};
    static const char* const position[2][2] = {{"k_hole_rollout_vjp<position, simple, 5>", "k_hole_rollout_vjp<position, simple>"},
                                               {"k_hole_rollout_vjp<position, vel_acc, 5>", "k_hole_rollout_vjp<position, vel_acc>"}};
    static const char* const velocity[2][2] = {{"k_hole_rollout_vjp<velocity, simple, 5>", "k_hole_rollout_vjp<velocity, simple>"},
                                               {"k_hole_rollout_vjp<velocity, vel_acc, 5>", "k_hole_rollout_vjp<velocity, vel_acc>"}};
    switch (h.rc.controller_type) {
        case MPK_CTRL_MOTOR: return by_rew(integral_constant<int, MPK_CTRL_MOTOR>(), motor);
        case MPK_CTRL_POSITION: return by_rew(integral_constant<int, MPK_CTRL_POSITION>(), position);
        default: return by_rew(integral_constant<int, MPK_CTRL_VELOCITY>(), velocity);
    }
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
