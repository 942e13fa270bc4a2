// The reacher envs' reset and observation as __device__ functions, shared by k_reacher_reset (mpk_reset.hip), k_reacher_obs /
// k_reacher_step_obs (mpk_obs.hip), k_reacher_autoreset (mpk_autoreset.hip) and k_reacher_env_step (mpk_env_step.hip): one text of the draw programs and of the observation
// row, so the kernels give the same bits by construction.
//   reset_episode   the draw program of one episode and everything mpk_reacher_reset writes for its row
//                   HoleReacher   hole_reacher.py:60-71,79-101, base_reacher.py:73-93: [reseed] width, direction + x, depth, first joint
//                   SimpleReacher simple_reacher.py:46-54,85-96, base_reacher.py:73-93: goal (discarded), [reseed] first joint, goal,
//                                 [reseed] first joint
//   obs_row         one row of _get_obs, masked / time-aware as BlackBoxWrapper.observation hands it out
//                   SimpleReacher _get_obs (simple_reacher.py:75-83): [cos q, sin q, qd, ee - goal, steps]
//                   HoleReacher   _get_obs (hole_reacher.py:114-124): [cos q, sin q, qd, width, ee - goal, steps], goal = (x, -depth)
#pragma once
#include "mpk_dev.h"
#include "mpk_nprng.h"

namespace mpk {

constexpr int kGoalDrawCap = 4096;      // rejection rounds of one goal draw (1.27 expected); reaching it raises the fault word

struct ResetArgs {
    const uint64_t* seeds;              // [B] or nullptr
    uint64_t seed_base;
    int seeded_base;                    // seeds == nullptr: 1 = episode b is seeded with seed_base + b, 0 = continue
    NpRng* rng;                         // [B]
    double* q;
    double* qd;
    float* cond_pos;
    float* cond_vel;
    int32_t* traj_steps;
    int32_t* plan_steps;                // or nullptr
    uint8_t* done;                      // or nullptr
    double* task_out;                   // [B, 2] goal or [B, 3] hole
    int* fault;
    double target0, target1, hole_width, hole_x, hole_depth;
    int env, random_start, B, D;
};

// SimpleReacherEnv._generate_goal (simple_reacher.py:85-96): U(-L, L, size=2) until |g| < L, from g = (L, L); L = sum of n_links
// unit lengths.  |g| as np.linalg.norm of a 2-vector: sqrt(x*x + y*y).  false: the cap was reached (g is then NaN)
__device__ __forceinline__ bool draw_goal(NpRng& r, double L, double& gx, double& gy) {
    gx = L; gy = L;
    for (int it = 0; it < kGoalDrawCap; ++it) {
        if (sqrt(gx * gx + gy * gy) < L) return true;
        gx = np_uniform(r, -L, L);
        gy = np_uniform(r, -L, L);
    }
    if (sqrt(gx * gx + gy * gy) < L) return true;
    gx = gy = __builtin_nan("");
    return false;
}

// The reset of episode b: (re)seeds or continues its generator, runs the env's draw program and writes the row of every buffer of
// `a`.  Returns the first joint angle (the other joints start at 0, the arm at rest); t0, t1, t2 = the task row written (goal x, y, -
// or hole x, width, depth).
__device__ __forceinline__ double reset_episode(const ResetArgs& a, int b, double& t0, double& t1, double& t2) {
    const bool seeded = a.seeds != nullptr || a.seeded_base;
    const uint64_t seed = a.seeds ? a.seeds[b] : a.seed_base + (uint64_t)b;
    NpRng r = seeded ? np_seed(seed) : a.rng[b];
    constexpr double kLo = M_PI / 4.0, kHi = 3.0 * M_PI / 4.0;     // np.pi / 4, 3 * np.pi / 4 (base_reacher.py:81)
    double q0;
    bool ok = true;
    if (a.env == MPK_RESET_HOLE_REACHER) {
        // _generate_hole (hole_reacher.py:79-101): a NaN kwarg is None (drawn)
        const double width = isnan(a.hole_width) ? np_uniform(r, 0.15, 0.5) : a.hole_width;
        double x = a.hole_x;
        if (isnan(x)) {
            const double direction = np_choice_pm1(r);
            x = direction * np_uniform(r, width / 2.0, 3.5);
        }
        const double depth = isnan(a.hole_depth) ? np_uniform(r, 1.0, 1.0) : a.hole_depth;   // uniform(1, 1): still one draw
        q0 = a.random_start ? np_uniform(r, kLo, kHi) : M_PI / 2.0;                           // _start_pos (base_reacher.py:33)
        a.task_out[3 * (size_t)b] = x;
        a.task_out[3 * (size_t)b + 1] = width;
        a.task_out[3 * (size_t)b + 2] = depth;
        t0 = x; t1 = width; t2 = depth;
    } else {
        // SimpleReacherEnv.reset (simple_reacher.py:46-54): goal, reset(seed), goal, reset(seed)
        const bool drawn = isnan(a.target0);
        const double L = (double)a.D;
        double gx = a.target0, gy = a.target1;
        if (drawn && !seeded) ok &= draw_goal(r, L, gx, gy);     // the first goal: overwritten below, its draws are consumed
        if (a.random_start) (void)np_uniform(r, kLo, kHi);
        if (drawn) ok &= draw_goal(r, L, gx, gy);
        if (seeded) r = np_seed(seed);
        q0 = a.random_start ? np_uniform(r, kLo, kHi) : 0.0;     // SimpleReacher's _start_pos is zeros (simple_reacher.py:29)
        a.task_out[2 * (size_t)b] = gx;
        a.task_out[2 * (size_t)b + 1] = gy;
        t0 = gx; t1 = gy; t2 = 0.0;
    }
    if (!ok) wave_gave_up(a.fault, 512);
    a.rng[b] = r;
    // what k_episode_reset writes: the arm straight from q0, at rest, counters zero, the fp32 image of the plant state
    const size_t row = (size_t)b * a.D;
    for (int d = 0; d < a.D; ++d) {
        const double v = d == 0 ? q0 : 0.0;
        a.q[row + d] = v;
        a.qd[row + d] = 0.0;
        if (a.cond_pos) { a.cond_pos[row + d] = (float)v; a.cond_vel[row + d] = 0.0f; }
    }
    a.traj_steps[b] = 0;
    if (a.plan_steps) a.plan_steps[b] = 0;       // (k_reacher_env_step has no plans and no done bytes)
    if (a.done) a.done[b] = 0;
    return q0;
}

constexpr int kObsCols = 64;             // >= 3 * kMaxD + 4 full columns + time awareness

struct ObsLayout {
    uint64_t mask;                       // full columns written (bit c = column c), never 0 here
    double time_div;                     // > 0: the time-awareness column
    int env, D, n_full, n_out;
};

// s_pos[c] = output position of full column c (c = n_full: the time-awareness column), -1 = not written
__device__ __forceinline__ void obs_positions(const ObsLayout& L, int* s_pos) {
    for (int c = threadIdx.x; c <= L.n_full; c += blockDim.x) {
        int p = -1;
        if (c < L.n_full) {
            if ((L.mask >> c) & 1ull) p = __popcll(L.mask & ((1ull << c) - 1ull));
        } else if (L.time_div > 0.0) {
            p = L.n_out - 1;
        }
        s_pos[c] = p;
    }
}

// one observation row into r[0 .. n_out) (output order), from the plant state after `steps` env steps
template <int MD>
__device__ __forceinline__ void obs_row(const ObsLayout& L, const int* s_pos, const double* q, const double* qd, double gx, double gy,
                                        double width, int steps, float* r) {
    const int D = MD < kMaxD ? MD : L.D;
    auto put = [&](int c, double v) {
        const int p = s_pos[c];                  // the same for every lane: a broadcast read, a uniform branch
        if (p >= 0) r[p] = (float)v;
    };
    double ex = 0.0, ey = 0.0, ang = 0.0;
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        if (d >= D) continue;
        double s, c;
        sincos(q[d], &s, &c);
        put(d, c);
        put(D + d, s);
        put(2 * D + d, qd[d]);
        ang = d == 0 ? q[0] : ang + q[d];        // np.cumsum(joint angles)
        sincos(ang, &s, &c);
        ex = ex + c;                             // joints[0] + np.cumsum(link vectors): joints[0] = 0
        ey = ey + s;
    }
    int k = 3 * D;
    if (L.env == MPK_RESET_HOLE_REACHER) put(k++, width);
    put(k, ex - gx);
    put(k + 1, ey - gy);
    put(k + 2, (double)steps);
    put(L.n_full, (double)steps / L.time_div);  // TimeAwareObservation: t / max_episode_steps (t = the env's step counter)
}

// goal of episode b: SimpleReacher task [B, 2] = goal; HoleReacher task [B, 3] = (x, width, depth), goal (x, -depth)
__device__ __forceinline__ void obs_task(const ObsLayout& L, const double* task, int b, double& gx, double& gy, double& width) {
    if (L.env == MPK_RESET_HOLE_REACHER) {
        gx = task[3 * (size_t)b];
        width = task[3 * (size_t)b + 1];
        gy = -task[3 * (size_t)b + 2];
    } else {
        gx = task[2 * (size_t)b];
        gy = task[2 * (size_t)b + 1];
        width = 0.0;
    }
}

#ifndef MPK_DEVICE_ONLY
inline ObsLayout obs_layout(const ObsLaunch& l) {
    ObsLayout L;
    L.env = l.env; L.D = l.D; L.n_full = l.n_full; L.n_out = l.n_out; L.mask = l.mask; L.time_div = l.time_div;
    return L;
}

inline ResetArgs reset_args(const ResetLaunch& l, int B, int D, int* fault) {
    static_assert(sizeof(NpRng) == 40, "mpk_nprng_state is 5 x uint64");
    ResetArgs a;
    a.seeds = l.seeds; a.seed_base = l.seed_base; a.seeded_base = l.seeded_base; a.rng = reinterpret_cast<NpRng*>(l.rng);
    a.q = l.q; a.qd = l.qd; a.cond_pos = l.cond_pos; a.cond_vel = l.cond_vel; a.traj_steps = l.traj_steps;
    a.plan_steps = l.plan_steps; a.done = l.done; a.task_out = l.task_out; a.fault = fault;
    a.target0 = l.target[0]; a.target1 = l.target[1]; a.hole_width = l.hole_width; a.hole_x = l.hole_x; a.hole_depth = l.hole_depth;
    a.env = l.env; a.random_start = l.random_start; a.B = B; a.D = D;
    return a;
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
