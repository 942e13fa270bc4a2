// k_hole_rollout: the step loop of BlackBoxWrapper.step (black_box_wrapper.py:175-203) around the reference's HoleReacher
// (envs/classic_control/hole_reacher/hole_reacher.py, base_reacher/base_reacher_direct.py:20-38, and the reward function of rew_fct:
// hr_simple_reward.py:19-53, hr_dist_vel_acc_reward.py:20-60, hr_unbounded_reward.py:17-60, one instantiation each):
// controller + clip, the direct-velocity plant, self / wall collision, reward, and the break on collision.  One lane per episode,
// serial in time; a wave leaves the loop once none of its lanes is live.  float64 without FMA contraction, except where the
// reference's own numpy flow is float32 (hole_plant_step, mpk_plant.h).
#include "mpk_dev.h"
#include "mpk_hole_geom.h"
#include "mpk_plant.h"
#include "mpk_reward.h"

namespace mpk {

struct HoleArgs {
    RolloutDev rc;
    const float* des_pos;
    const float* des_vel;
    double* Q;
    double* QD;
    const int32_t* n_steps;
    const int32_t* step0;
    const double* hole;              // [B, 3] (x, width, depth)
    float* actions;                  // [B, T, D] or nullptr
    double* rewards;                 // [B, T] or nullptr
    double* ret;                     // [B] or nullptr
    int32_t* n_exec;                 // [B] or nullptr
    uint8_t* collided;               // [B] or nullptr
    uint8_t* success;                // [B] or nullptr
    double* reward_state;            // [B, 2] unbounded's stored end effector (REW == MPK_HOLE_REW_UNBOUNDED only)
    ReplanDev rp;                    // traj_steps == nullptr: off
    double penalty;
    int allow_self, allow_wall, steps_before_reward, agg;
    int D, B, T;
};

constexpr int kHoleWpb = 4;          // waves per workgroup

// DC: link count compiled in (0: run time, <= kMaxD); REW: the reward function, MPK_HOLE_REW_*
template <int DC, bool SAMPLED, int REW>
__global__ void __launch_bounds__(64 * kHoleWpb) k_hole_rollout(const HoleArgs a) {
    constexpr int MD = DC > 0 ? DC : kMaxD;
    __shared__ double s_g[4 * kMaxD];
    __shared__ double s_slot[16 * 64 * kHoleWpb];     // ret: per step slot t mod 16, the order of k_reward_aggregate
    const int D = DC > 0 ? DC : a.D;
    if (threadIdx.x < (unsigned)D) {
        const double *pg = a.rc.pg, *dg = a.rc.dg, *lo = a.rc.lo, *hi = a.rc.hi;
        s_g[threadIdx.x] = pg[threadIdx.x];
        s_g[kMaxD + threadIdx.x] = dg[threadIdx.x];
        s_g[2 * kMaxD + threadIdx.x] = lo[threadIdx.x];
        s_g[3 * kMaxD + threadIdx.x] = hi[threadIdx.x];
    }
    __syncthreads();
    const long bl = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = bl < a.B;
    if (!__any(on)) return;
    const int b = on ? (int)bl : 0;
    const int T = a.T;
    const int ctrl = a.rc.controller_type;
    const bool with_rp = a.rp.traj_steps != nullptr;

    int n = 0, s0 = 0;
    ReplanVals rv{0, 0, 0, true};
    if (on) {
        if (with_rp) {
            rv = replan_eval(a.rp, b, T);
            n = rv.seg;
            s0 = rv.cur;
        } else {
            n = a.n_steps ? a.n_steps[b] : T;
            n = n < T ? (n < 0 ? 0 : n) : T;
            s0 = a.step0 ? a.step0[b] : 0;
        }
    }
    double q[MD], qd[MD];
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        q[d] = (on && d < D) ? a.Q[(size_t)b * D + d] : 0.0;
        qd[d] = (on && d < D) ? a.QD[(size_t)b * D + d] : 0.0;
    }
    const double hx = on ? a.hole[3 * (size_t)b] : 0.0, hw = on ? a.hole[3 * (size_t)b + 1] : 0.0;
    const double hdepth = on ? a.hole[3 * (size_t)b + 2] : 0.0;
    const double hl = hx - hw / 2.0, hr = hx + hw / 2.0, floor_y = -hdepth;     // hole_reacher.py:156,165,174
    const double dt = a.rc.dt;
    const float dt32 = (float)dt;
    double* slot = s_slot + threadIdx.x;
    if (a.ret) {
#pragma unroll
        for (int i = 0; i < 16; ++i) slot[i * 64 * kHoleWpb] = 0.0;
    }
    double last_r = 0.0;
    bool coll = false, succ = false;
    int t = 0;
    const size_t row0 = (size_t)b * T;
    for (;; ++t) {
        const bool live = t < n && !coll;
        if (!__any(live)) break;                      // wave-uniform exit
        if (!live) continue;
        const size_t row = (row0 + t) * D;
        // controller + clip (black_box_wrapper.py:176-179), then the direct-velocity plant in numpy's dtypes (mpk_plant.h)
        double u[MD];
        hole_control<MD>(ctrl, D, s_g, a.des_pos ? a.des_pos + row : nullptr, a.des_vel ? a.des_vel + row : nullptr, q, qd, u);
        const double acc_cost = hole_plant_step<MD>(ctrl, ctrl != MPK_CTRL_MOTOR && s0 + t > 0, D, dt, dt32, u, q, qd);
        // kinematics (base_reacher.py:95-103): unit links, cumulative angles, joints from the origin
        double jx[MD + 1], jy[MD + 1], cs[MD], sn[MD];
        jx[0] = 0.0; jy[0] = 0.0;
        double ang = 0.0;
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            if (d >= D) { cs[d] = sn[d] = 0.0; jx[d + 1] = jx[d]; jy[d + 1] = jy[d]; continue; }
            ang = d == 0 ? q[0] : ang + q[d];
            sincos_lean(ang, &sn[d], &cs[d]);
            jx[d + 1] = jx[d] + cs[d];
            jy[d + 1] = jy[d] + sn[d];
        }
        // self collision (base_reacher.py:105-119): joint limits, then non-adjacent links
        bool hit = false;
        if (!a.allow_self) {
#pragma unroll
            for (int d = 0; d < MD; ++d)
                if (d < D) hit |= q[d] > M_PI || q[d] < -M_PI;
            if (!hit) {
                for (int i = 0; i < D && !hit; ++i)
                    for (int k = i + 2; k < D && !hit; ++k)
                        hit = hole_intersect(jx[i], jy[i], jx[i + 1], jy[i + 1], jx[k], jy[k], jx[k + 1], jy[k + 1]);
            }
        }
        if (!a.allow_wall && !hit) {
            for (int i = 0; i < D && !hit; ++i) hit = hole_link_hits_wall<SAMPLED>(cs[i], sn[i], jx[i], jy[i], hl, hr, floor_y);
        }
        double r;
        if constexpr (REW == MPK_HOLE_REW_VEL_ACC) {
            // hr_dist_vel_acc_reward.py:40-58: the distance terms at step 199 only -- also after a collision, which ended the episode
            // before (the latch of :29-38 never sees a second step), so a collision before 199 pays velocity and acceleration alone
            const double vel_cost = hole_vel_cost<MD>(ctrl != MPK_CTRL_MOTOR, D, qd);
            double dist_cost = 0.0, coll_cost = 0.0;
            if (s0 + t == 199) {
                const double dx = jx[D] - hx, dy = jy[D] - floor_y;
                const double dist = sqrt(dx * dx + dy * dy);
                dist_cost = dist * dist;
                coll_cost = hit ? dist_cost : 0.0;          // collided * collision_dist^2, collision_dist = this step's dist
                succ = dist < 0.005 && !hit;
            }
            r = hole_vel_acc_reward(dist_cost, vel_cost, acc_cost, coll_cost, a.penalty);
        } else if constexpr (REW == MPK_HOLE_REW_UNBOUNDED) {
            // hr_unbounded_reward.py:32-58: store the end effector at step 180 or on collision, pay at step 199 or on collision.  The
            // stored one lives in reward_state, not in registers (the kernel is at the occupancy-2 limit): step 180 and step 199 may
            // fall into different plans; a collision pays on its own end effector
            double* e = a.reward_state + 2 * (size_t)b;
            const double cx = jx[D], cy = jy[D];
            if (s0 + t == 180 || hit) { e[0] = cx; e[1] = cy; }
            double dist_reward = 0.0;
            if (s0 + t == 199 || hit) {
                const double ex = hit ? cx : e[0], ey = hit ? cy : e[1];
                const double dx = ex - hx, dy = ey - floor_y;
                const double dist = sqrt(dx * dx + dy * dy);
                dist_reward = hole_unbounded_dist_reward(dist, hit, cy > 0.0, ey);
                succ = !hit;
            }
            r = dist_reward * 1.0 + acc_cost * -5e-6;
        } else {
            // reward (hr_simple_reward.py:36-53): the distance term at step steps_before_reward or on collision
            double dist_cost = 0.0;
            if (s0 + t == a.steps_before_reward || hit) {
                const double dx = jx[D] - hx, dy = jy[D] - floor_y;
                const double dist = sqrt(dx * dx + dy * dy);
                dist_cost = dist * dist;
                succ = dist < 0.005 && !hit;
            }
            r = (dist_cost * -1.0 + acc_cost * -5e-8) + (hit ? 1.0 : 0.0) * -a.penalty;
        }
        if (a.actions) {
#pragma unroll
            for (int d = 0; d < MD; ++d)
                if (d < D) a.actions[row + d] = (float)u[d];
        }
        if (a.rewards) a.rewards[row0 + t] = r;
        if (a.ret) slot[(t & 15) * 64 * kHoleWpb] += r;
        last_r = r;
        if (hit) { coll = true; n = t + 1; }      // terminated: the wrapper breaks (black_box_wrapper.py:197-203)
    }
    if (!on) return;
    // steps after the break
    for (int tt = n; tt < T; ++tt) {
        if (a.actions)
            for (int d = 0; d < D; ++d) a.actions[(row0 + tt) * D + d] = 0.0f;
        if (a.rewards) a.rewards[row0 + tt] = 0.0;
    }
#pragma unroll
    for (int d = 0; d < MD; ++d)
        if (d < D) { a.Q[(size_t)b * D + d] = q[d]; a.QD[(size_t)b * D + d] = qd[d]; }
    if (a.ret) {
        double sum = slot[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) sum = sum + slot[i * 64 * kHoleWpb];
        a.ret[b] = a.agg == MPK_AGG_LAST ? (n > 0 ? last_r : 0.0) : (a.agg == MPK_AGG_MEAN ? (n > 0 ? sum / (double)n : 0.0) : sum);
    }
    if (a.n_exec) a.n_exec[b] = n;
    if (a.collided) a.collided[b] = coll ? 1 : 0;
    if (a.success) a.success[b] = succ ? 1 : 0;
    if (with_rp) {
        // the break committed: the executed steps, the clock, and a collision finishes the episode
        const ReplanDev& rp = a.rp;
        rp.seg_len[b] = n;
        if (!rv.was_done) {
            const uint8_t dn = (coll || rv.cur + n >= rp.horizon) ? 1 : 0;
            rp.plan_steps[b] = rv.plan;
            rp.traj_steps[b] = rv.cur + n;
            rp.done[b] = dn;
            if (rp.done_out) rp.done_out[b] = dn;
        } else if (rp.done_out) {
            rp.done_out[b] = 1;
        }
        if (rp.cond_pos) {
            int tc = n - 1;
            tc = tc < 0 ? 0 : (tc > T - 1 ? T - 1 : tc);
            for (int d = 0; d < D; ++d) {
                rp.cond_pos[(size_t)b * D + d] = a.des_pos[(row0 + tc) * D + d];
                rp.cond_vel[(size_t)b * D + d] = a.des_vel[(row0 + tc) * D + d];
            }
        }
    }
}

#ifndef MPK_DEVICE_ONLY
template <int DC, bool SAMPLED>
static void launch_hole_rew(int rew_fct, dim3 grid, dim3 block, hipStream_t stream, const HoleArgs& a) {
    if (rew_fct == MPK_HOLE_REW_VEL_ACC) hipLaunchKernelGGL((k_hole_rollout<DC, SAMPLED, MPK_HOLE_REW_VEL_ACC>), grid, block, 0, stream, a);
    else if (rew_fct == MPK_HOLE_REW_UNBOUNDED)
        hipLaunchKernelGGL((k_hole_rollout<DC, SAMPLED, MPK_HOLE_REW_UNBOUNDED>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_hole_rollout<DC, SAMPLED, MPK_HOLE_REW_SIMPLE>), grid, block, 0, stream, a);
}

int launch_hole_rollout(const HoleLaunch& h, int B, int T, int D, void* stream, const Tuning& tune) {
    HoleArgs a;
    a.rc = h.rc; a.des_pos = h.des_pos; a.des_vel = h.des_vel; a.Q = h.q; a.QD = h.qd; a.n_steps = h.n_steps; a.step0 = h.step0;
    a.hole = h.hole; a.actions = h.actions; a.rewards = h.rewards; a.ret = h.ret; a.n_exec = h.n_exec; a.collided = h.collided;
    a.success = h.success; a.reward_state = h.reward_state; a.rp = h.rp; a.penalty = h.penalty; a.allow_self = h.allow_self; a.allow_wall = h.allow_wall;
    a.steps_before_reward = h.steps_before_reward; a.agg = h.agg; a.D = D; a.B = B; a.T = T;
    const bool sampled = tune.hole_sampled == 1;
    const dim3 grid((unsigned)((B + 64 * kHoleWpb - 1) / (64 * kHoleWpb))), block(64 * kHoleWpb);
    const hipStream_t s = (hipStream_t)stream;
    if (D == 5) {
        if (sampled) launch_hole_rew<5, true>(h.rew_fct, grid, block, s, a);
        else launch_hole_rew<5, false>(h.rew_fct, grid, block, s, a);
    } else {
        if (sampled) launch_hole_rew<0, true>(h.rew_fct, grid, block, s, a);
        else launch_hole_rew<0, false>(h.rew_fct, grid, block, s, a);
    }
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
