// k_reacher_env_step: one env.step(action) of the gymnasium-wrapped STEP-BASED reacher envs (fancy/SimpleReacher-v0,
// fancy/LongSimpleReacher-v0, fancy/HoleReacher-v0) for B device-resident episodes, followed by the same-step autoreset of a vector
// env, in one launch (mpk_reacher_env_step), one lane per episode:
//   the plant in numpy's dtypes for the float32 action of the env's action space, NOT clipped (the step-based envs do not clip:
//   base_reacher_torque.py:20-37, base_reacher_direct.py:20-38; only the black-box wrapper does)
//       SimpleReacher  qd = qd + dt * action with dt * action a float32 product, q = q + dt * qd in float64
//       HoleReacher    hole_plant_step (mpk_plant.h) with the action as the velocity controller's output
//   kinematics, collisions and the reward terms as k_hole_rollout has them (mpk_hole_geom.h; SimpleReacher's reward
//   simple_reacher.py:56-72), keyed on the env step counter before its increment; terminated = collided (HoleReacher), truncated =
//   gymnasium's TimeLimit on the incremented counter;
//   final_obs[b] = the full _get_obs row after the step; where terminated | truncated and the autoreset is on, reset_episode on the
//   episode's own generator and obs[b] = the new episode's reset observation, elsewhere obs[b] = final_obs[b] (mpk_reacher_env.h:
//   the functions k_reacher_autoreset runs).
// The lane keeps q, qd and the action in registers from the loads to the stores; the observation rows are assembled in LDS in output
// order and leave as contiguous runs, consecutive lanes on consecutive floats, as k_reacher_autoreset writes them.
#include "mpk_hole_geom.h"
#include "mpk_plant.h"
#include "mpk_reacher_env.h"
#include "mpk_reward.h"

namespace mpk {

constexpr int kEnvStepBlock = 128;       // episodes (= lanes) per workgroup

struct EnvStepArgs {
    ResetArgs r;                         // q, qd, traj_steps, rng, task_out = the task rows (read, written by a reset); no seeds
    ObsLayout L;                         // every column of the full row, no time column
    const float* actions;                // [B, D]
    double* reward_state;                // [B, 2], unbounded only
    double* reward;                      // [B]
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* collided;                   // HoleReacher (else nullptr)
    uint8_t* success;
    uint8_t* reset_mask;
    float* final_obs;                    // [B, n_out]
    float* obs;
    double dt, penalty;
    int allow_self, allow_wall, steps_before_reward, max_steps, autoreset;
};

constexpr int kEnvStepSimple = -1;       // KIND: SimpleReacher; otherwise HoleReacher's MPK_HOLE_REW_*

template <int MD, int KIND>
__global__ void __launch_bounds__(kEnvStepBlock) k_reacher_env_step(const EnvStepArgs a) {
    extern __shared__ float s_rows[];    // [2, kEnvStepBlock, n_out]
    __shared__ int s_pos[kObsCols];
    const ObsLayout& L = a.L;
    const int b0 = blockIdx.x * kEnvStepBlock;
    const int nb = min(kEnvStepBlock, a.r.B - b0);
    const int n_out = L.n_out;
    float* s_final = s_rows;
    float* s_obs = s_rows + kEnvStepBlock * n_out;
    obs_positions(L, s_pos);
    __syncthreads();
    if ((int)threadIdx.x < nb) {
        const int b = b0 + threadIdx.x;
        const int D = MD < kMaxD ? MD : a.r.D;
        const size_t row = (size_t)b * D;
        float* rf = s_final + threadIdx.x * n_out;
        float* ro = s_obs + threadIdx.x * n_out;
        double q[MD], qd[MD], u[MD];
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            q[d] = d < D ? a.r.q[row + d] : 0.0;
            qd[d] = d < D ? a.r.qd[row + d] : 0.0;
            u[d] = d < D ? (double)a.actions[row + d] : 0.0;
        }
        const int steps = a.r.traj_steps[b];
        double gx, gy, width;
        obs_task(L, a.r.task_out, b, gx, gy, width);
        const double dt = a.dt;
        const float dt32 = (float)dt;
        double r;
        bool hit = false, succ = false;
        if constexpr (KIND == kEnvStepSimple) {
            // base_reacher_torque.py:25-26 for a float32 action: numpy keeps the Python float dt weak, dt * action is float32;
            // reward_ctrl = (action ** 2).sum() adds in float32 in numpy's order (simple_reacher.py:68; np_sum, mpk_dev.h)
            const float c32 = np_sum<MD, float>(D, [&](int d) { const float a32 = (float)u[d]; return a32 * a32; });
#pragma unroll
            for (int d = 0; d < MD; ++d) {
                if (d >= D) continue;
                const float a32 = (float)u[d];
                qd[d] = qd[d] + (double)(dt32 * a32);
                q[d] = q[d] + dt * qd[d];
            }
            double rdist = 0.0;
            if (steps >= a.steps_before_reward) {
                // the end effector of reacher_reward_item (mpk_reward.h): cumulative angles, sums left to right
                double ex = 0.0, ey = 0.0, ang = 0.0;
#pragma unroll
                for (int d = 0; d < MD; ++d) {
                    if (d >= D) continue;
                    ang = d == 0 ? q[0] : ang + q[d];
                    double sn, cs;
                    sincos_lean(ang, &sn, &cs);
                    ex = d == 0 ? cs : ex + cs;
                    ey = d == 0 ? sn : ey + sn;
                }
                const double dx = ex - gx, dy = ey - gy;
                rdist = 0.0 - sqrt(dx * dx + dy * dy);
            }
            r = rdist - (double)c32;
        } else {
            const double hx = gx, floor_y = gy;                   // goal = (x, -depth)
            const double hl = hx - width / 2.0, hr = hx + width / 2.0;     // hole_reacher.py:156,165,174
            const double acc_cost = hole_plant_step<MD>(MPK_CTRL_VELOCITY, steps > 0, D, dt, dt32, u, q, qd);
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
                for (int i = 0; i < D && !hit; ++i) hit = hole_link_hits_wall<false>(cs[i], sn[i], jx[i], jy[i], hl, hr, floor_y);
            }
            if constexpr (KIND == MPK_HOLE_REW_VEL_ACC) {
                // hr_dist_vel_acc_reward.py:40-58: the distance terms at step 199 only
                const double vel_cost = hole_vel_cost<MD>(true, D, qd);
                double dist_cost = 0.0, coll_cost = 0.0;
                if (steps == 199) {
                    const double dx = jx[D] - hx, dy = jy[D] - floor_y;
                    const double dist = sqrt(dx * dx + dy * dy);
                    dist_cost = dist * dist;
                    coll_cost = hit ? dist_cost : 0.0;
                    succ = dist < 0.005 && !hit;
                }
                r = hole_vel_acc_reward(dist_cost, vel_cost, acc_cost, coll_cost, a.penalty);
            } else if constexpr (KIND == MPK_HOLE_REW_UNBOUNDED) {
                // hr_unbounded_reward.py:32-58: store the end effector at step 180 or on collision, pay at step 199 or on collision
                double* e = a.reward_state + 2 * (size_t)b;
                const double cx = jx[D], cy = jy[D];
                if (steps == 180 || hit) { e[0] = cx; e[1] = cy; }
                double dist_reward = 0.0;
                if (steps == 199 || hit) {
                    const double ex = hit ? cx : e[0], ey = hit ? cy : e[1];
                    const double dx = ex - hx, dy = ey - floor_y;
                    const double dist = sqrt(dx * dx + dy * dy);
                    dist_reward = hole_unbounded_dist_reward(dist, hit, cy > 0.0, ey);
                    succ = !hit;
                }
                r = dist_reward * 1.0 + acc_cost * -5e-6;
            } else {
                // hr_simple_reward.py:36-53: the distance term at step steps_before_reward or on collision
                double dist_cost = 0.0;
                if (steps == a.steps_before_reward || hit) {
                    const double dx = jx[D] - hx, dy = jy[D] - floor_y;
                    const double dist = sqrt(dx * dx + dy * dy);
                    dist_cost = dist * dist;
                    succ = dist < 0.005 && !hit;
                }
                r = (dist_cost * -1.0 + acc_cost * -5e-8) + (hit ? 1.0 : 0.0) * -a.penalty;
            }
        }
        const int steps_after = steps + 1;
        const bool trunc = steps_after >= a.max_steps;           // gymnasium's TimeLimit
        a.reward[b] = r;
        a.terminated[b] = hit ? 1 : 0;
        a.truncated[b] = trunc ? 1 : 0;
        if (a.collided) a.collided[b] = hit ? 1 : 0;
        if (a.success) a.success[b] = succ ? 1 : 0;
        obs_row<MD>(L, s_pos, q, qd, gx, gy, width, steps_after, rf);
        const bool sel = a.autoreset && (hit || trunc);
        if (sel) {
            double t0, t1, t2;
            const double q0 = reset_episode(a.r, b, t0, t1, t2);
            // the new episode's row from the values just written: first joint q0, the others 0, at rest, step counter 0
#pragma unroll
            for (int d = 0; d < MD; ++d) { q[d] = d == 0 ? q0 : 0.0; qd[d] = 0.0; }
            const bool hole = L.env == MPK_RESET_HOLE_REACHER;
            obs_row<MD>(L, s_pos, q, qd, t0, hole ? -t2 : t1, hole ? t1 : 0.0, 0, ro);
        } else {
#pragma unroll
            for (int d = 0; d < MD; ++d)
                if (d < D) { a.r.q[row + d] = q[d]; a.r.qd[row + d] = qd[d]; }
            a.r.traj_steps[b] = steps_after;
            for (int k = 0; k < n_out; ++k) ro[k] = rf[k];
        }
        a.reset_mask[b] = sel ? 1 : 0;
    }
    __syncthreads();
    float* dst_f = a.final_obs + (size_t)b0 * n_out;
    float* dst_o = a.obs + (size_t)b0 * n_out;
    for (int j = threadIdx.x; j < nb * n_out; j += kEnvStepBlock) {
        dst_f[j] = s_final[j];
        dst_o[j] = s_obs[j];
    }
}

#ifndef MPK_DEVICE_ONLY
template <int MD>
static void launch_env_step_kind(int kind, dim3 grid, dim3 block, size_t lds, hipStream_t s, const EnvStepArgs& a) {
    if (kind == kEnvStepSimple) hipLaunchKernelGGL((k_reacher_env_step<MD, kEnvStepSimple>), grid, block, lds, s, a);
    else if (kind == MPK_HOLE_REW_VEL_ACC) hipLaunchKernelGGL((k_reacher_env_step<MD, MPK_HOLE_REW_VEL_ACC>), grid, block, lds, s, a);
    else if (kind == MPK_HOLE_REW_UNBOUNDED) hipLaunchKernelGGL((k_reacher_env_step<MD, MPK_HOLE_REW_UNBOUNDED>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_reacher_env_step<MD, MPK_HOLE_REW_SIMPLE>), grid, block, lds, s, a);
}

int launch_reacher_env_step(const EnvStepLaunch& e, int B, int D, void* stream, int* fault) {
    EnvStepArgs a;
    a.r = reset_args(e.reset, B, D, fault);
    a.L = obs_layout(e.obs_layout);
    a.actions = e.actions; a.reward_state = e.reward_state; a.reward = e.reward; a.terminated = e.terminated; a.truncated = e.truncated;
    a.collided = e.collided; a.success = e.success; a.reset_mask = e.reset_mask; a.final_obs = e.final_obs; a.obs = e.obs;
    a.dt = e.dt; a.penalty = e.penalty; a.allow_self = e.allow_self; a.allow_wall = e.allow_wall;
    a.steps_before_reward = e.steps_before_reward; a.max_steps = e.max_steps; a.autoreset = e.autoreset;
    const int kind = e.reset.env == MPK_RESET_HOLE_REACHER ? e.rew_fct : kEnvStepSimple;
    const dim3 grid((unsigned)((B + kEnvStepBlock - 1) / kEnvStepBlock)), block(kEnvStepBlock);
    const size_t lds = (size_t)2 * kEnvStepBlock * e.obs_layout.n_out * sizeof(float);
    const hipStream_t s = (hipStream_t)stream;
    if (D == 2) launch_env_step_kind<2>(kind, grid, block, lds, s, a);
    else if (D == 5) launch_env_step_kind<5>(kind, grid, block, lds, s, a);
    else launch_env_step_kind<kMaxD>(kind, grid, block, lds, s, a);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
