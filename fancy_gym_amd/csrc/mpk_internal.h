// Internal declarations shared by the host side (mpk_host.cpp) and the gfx950 kernels (mpk_kernels.hip).
// Not part of the public ABI (that is include/mpk.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "mpk.h"

namespace mpk {

constexpr int kMaxKP = 16;     // padded contraction length supported by the MFMA kernel (multiple of 4)
constexpr int kMaxD = 16;      // DoF supported by the MFMA kernel (one 16-column tile per episode group)
constexpr int kMaxDofArgs = 32;  // per-DoF constants carried in kernel arguments

// ---- host-side float64 tables (construction time) ------------------------------------------------------------
struct HostTables {
    // normalised RBFs: centres in phase space and bandwidths (n_total entries incl. zero padding)
    int n_total = 0;
    std::vector<double> centers, bw;
    // ProDMP pre-computed grid
    int n_pc = 0;
    float scaled_dt = 0.f;  // fp32: basis_dt / tau0, used bit-exactly by times_to_indices
    std::vector<double> y1, y2, dy1, dy2, pos_basis, vel_basis, scale;  // pos/vel_basis: [n_pc, nb+1]
};

void build_rbf(const mpk_config& c, HostTables& t);
void build_prodmp(const mpk_config& c, HostTables& t);
// fp32 time grid linspace(0, duration, T+1)[1:] following torch's symmetric scalar recipe
std::vector<float> build_times(double duration, int T);
int steps_for(double duration, double dt);

// ---- kernel-selection overrides (mpk_set_option); -1 = automatic ----------------------------------------------------
struct Tuning {
    int mapping = -1, bulk = -1, quad = -1, pd_quad = -1, write_through = -1, ipw = -1, phase = -1, phase_table = -1,
        phase_chunk = -1, pd_simple = -1, split = -1, lds_pad = -1, pipe = -1, flat = -1, phase_flat = -1,
        ring = -1, ring_np = -1, ring_ns = -1, ring_m = -1, ring_dbg = -1, ring_parts = -1, tiles_wpb = -1, serial_order = -1, ring_nc = -1,
        pd_generic = -1, dmp_response = -1, ablations = -1, ring_tb = -1, pd_helper = -1, phase_waves = -1, phase_split = -1, phase_pipe = -1, pd_pipe = -1,
        hole_sampled = -1, vjp_generic = -1;
};

// ---- device-side configuration (kernel argument, by value) --------------------------------------------------
struct DevCfg {
    int mp_type, phase_type, basis_type;
    int D, nb, n_total, zs;        // n_total: RBF count incl. zero padding; zs: zero-start offset
    int KT, KP;                    // contraction length (learnable + boundary-condition columns), padded to 4
    int P, Kloc, off;              // params per episode, local params per DoF, offset of the local block
    int T;
    int learn_tau, learn_delay, relative_goal, disable_goal, disable_weights;
    int rbf_uniform;               // equally spaced centres, one bandwidth: Gaussians by product recurrence (RbfRecur)
    int relgoal_before_scale;      // MPK_RELGOAL_BEFORE_SCALE
    int dmp_resp;                  // a DMP handle's RESPONSE configuration (round 5): mp_type says PRODMP -- the two-output contraction
                                   // kernels run -- and k_build_shared fills their rows from the explicit Euler map instead (see there)
    int goal_off_on;               // MPK_GOAL_OFFSET_ADD with a non-zero offset: one extra contraction column (x = 1)
    float goal_offset;
    int n_pc, len_factor;
    float tau, delay, alpha_phase, scaled_dt;
    float tau_lo, tau_hi, delay_lo, delay_hi;
    float ws, gs, dmp_alpha, dmp_beta;
    // device tables
    const double* tab;             // ProDMP: [y1|y2|dy1|dy2|pos_basis|vel_basis|weights_goal_scale]; RBF: [centers|bw]
    const float* rows32;           // ProDMP, <= 16 columns: [n_pc][2*KS + 4] = [Psi_0..Psi_nb 0.. y1 y2 | dPsi.. 0.. dy1 dy2 | lo x 4]
    int rows32_stride;             // 2*KS + 4 floats (KS = 8 or 16); DMP handles: the per-episode kernels' interpolation table
                                   // of the forcing rows over the scaled time, [kFastRows = 451][stride = 8] (mpk_traj_phase.hip fast_rows_build)
    const float* base_times;       // [T]
    float t_last;                  // base_times[T - 1] (host side: bounds the scaled time a launch can reach)
};

struct RolloutDev {
    int controller_type, plant_type;
    double dt;
    double pg[kMaxDofArgs], dg[kMaxDofArgs], lo[kMaxDofArgs], hi[kMaxDofArgs];
};

// integer replanning state advanced INSIDE the closed-loop trajectory kernel (mpk_replan_step): all device pointers,
// traj_steps == nullptr switches it off.  Same rule as k_replan_advance, same gather as k_condition_gather.
struct ReplanDev {
    int32_t* traj_steps = nullptr;   // [B] in/out
    int32_t* plan_steps = nullptr;   // [B] in/out
    uint8_t* done = nullptr;         // [B] in/out
    int32_t* seg_len = nullptr;      // [B] out
    uint8_t* done_out = nullptr;     // [B] out, optional: snapshot of `done` after this plan
    float* cond_pos = nullptr;       // [B, D] out, optional: desired state at the last executed step
    float* cond_vel = nullptr;
    int every = 1, max_planning_times = 0, horizon = 0;
};

// fp32 thresholds of a float64 interval: an fp32 position x satisfies !(x > high || x < low) exactly when it satisfies
// !(x > f32_at_most(high) || x < f32_at_least(low)) -- NaN limits stay NaN (never trip), limits beyond the fp32 range become +-FLT_MAX
inline float f32_at_least(double x) {
    float f = (float)x;
    if ((double)f < x) f = __builtin_nextafterf(f, __builtin_inff());
    return f;
}
inline float f32_at_most(double x) {
    float f = (float)x;
    if ((double)f > x) f = __builtin_nextafterf(f, -__builtin_inff());
    return f;
}

// validity gate of the fused closed-loop entry points (mpk_validity_gate of include/mpk.h with the limits copied in)
struct GateDev {
    double lo[kMaxD], hi[kMaxD];     // joint limits
    int check_td = 0;
    double tau_b[2] = {0.0, 0.0}, delay_b[2] = {0.0, 0.0};
    const float* raw_params = nullptr;   // [B, P] the action as passed (NULL: the params of the call)
    uint8_t* valid = nullptr;            // [B] out
    double* penalty = nullptr;           // [B] out, optional
};

// shared-phase table workspace produced by k_build_shared and consumed by k_traj_shared
struct SharedTables {
    float* A = nullptr;    // [n_out][KP][TS]
    float* aux = nullptr;  // [TS]
    int TS = 0, n_out = 0;
};

struct Handle;  // defined in mpk_host.cpp

// ---- a trajectory call as ONE value, from the entry point (mpk_host.cpp) to the route plans -----------------------------------------
// the extras of mpk_episode_return (ret == nullptr: not that call)
struct EpisodeAsk {
    int reward = 0, steps_before_reward = 0, agg = 0;                  // MPK_REWARD_*, MPK_AGG_*
    const double* goal = nullptr;
    const int32_t* step0 = nullptr;
    double* ret = nullptr;                                              // [B]
    int32_t* seg_out = nullptr;                                         // [B], optional
};
// What the caller asks for, and nothing about where it runs.  The planners derive their facts from the pointers: q_state != nullptr is
// the closed loop, actions != nullptr a fused controller (rc is read), pos == nullptr the lean learned-phase launch (mpk_episode_return).
struct TrajRequest {
    const float *params = nullptr, *init_pos = nullptr, *init_vel = nullptr;   // [B, P], [B, D], [B, D]
    const float* init_time = nullptr;                                   // [B] per episode; nullptr: init_time_shared
    float init_time_shared = 0.f;
    float *pos = nullptr, *vel = nullptr, *actions = nullptr;           // [B, T, D] out
    const RolloutDev* rc = nullptr;                                     // controller and plant
    const double *c_pos = nullptr, *c_vel = nullptr;                    // [B, D] the frozen state fused actions track (MPK_PLANT_STATIC)
    double *q_state = nullptr, *qd_state = nullptr;                     // [B, D] in/out: the plant state of the closed loop
    const int32_t* n_steps = nullptr;                                   // [B] steps to execute (nullptr: all, or rp's rule)
    const ReplanDev* rp = nullptr;
    const GateDev* gate = nullptr;
    EpisodeAsk ep;
    int B = 0;
};
// where a launch runs and reports; the route plans get num_cu, tune, ticket and fault of it and never the stream
struct LaunchSite {
    int num_cu = 0;
    Tuning tune;
    void* stream = nullptr;
    const char** kernel_name = nullptr;  // set to the launched kernel's name (static storage)
    unsigned* ticket = nullptr;          // k_traj_ring's batch counter (nullptr: static batch assignment)
    int* fault = nullptr;                // the handle's fault word
    int32_t* range_flag = nullptr;       // ProDMP with a per-episode phase: raised beyond the pre-computed range
};

// ---- launchers implemented in mpk_kernels.hip (all enqueue on the site's `stream`, none synchronise) -------------------
int launch_build_shared(const DevCfg& c, float init_time, const SharedTables& st, int32_t* idx_out,
                        int32_t* range_flag, void* stream);
// (launch_traj_shared / launch_episode_return: the route choice -- plan_traj_shared / plan_episode_return, mpk_traj_route.h -- and ONE
// launch of the family it names)
int launch_traj_shared(const DevCfg& c, const SharedTables& st, const TrajRequest& q, const LaunchSite& at);
int launch_episode_return(const DevCfg& c, const SharedTables& st, const TrajRequest& q, const LaunchSite& at);
int launch_reward_aggregate(const double* rewards, const int32_t* seg_len, int agg, double* out, int B, int T, void* stream);
// shared phase, more than kMaxKP contraction columns: k-chunked GEMM on the matrix cores (trajectory only)
int launch_traj_wide(const DevCfg& c, const SharedTables& st, const TrajRequest& q, const LaunchSite& at);
// mpk_trajectory_vjp (mpk_traj_vjp.hip): the transpose of the shared-phase map, (g_pos, g_vel) [B, T, D] -> g_params [B, P], g_init_pos /
// g_init_vel [B, D]; any input or output may be nullptr (term skipped / not written).  Tile route (matrix cores) for <= kMaxD DoF and
// <= kMaxKP columns, else -- or with tune.vjp_generic == 1 -- one workgroup per episode on the vector ALU.  c: the configuration the
// tables were built for (a DMP handle's response configuration); MPK_ENOTIMPL for plain-DMP forcing tables.
int launch_traj_vjp(const DevCfg& c, const SharedTables& st, const float* g_pos, const float* g_vel, float* g_params, float* g_init_pos,
                    float* g_init_vel, int B, int num_cu, void* stream, const char** kernel_name, const Tuning& tune);
int launch_traj_rows(const DevCfg& c, const TrajRequest& q, const LaunchSite& at);
int launch_pd_rollout(const RolloutDev& rc, int D, const float* des_pos, const float* des_vel, double* q,
                      double* qd, const int32_t* n_steps, float* actions, int B, int T, void* stream,
                      const Tuning& tune, int* fault = nullptr);
// the fused entry points with a per-episode phase (learned tau / delay), promp / prodmp with <= 8 contraction columns and <= 16 DoF
// (mpk_phase_fused.hip): rc->plant_type static = actions for the frozen state (c_pos, c_vel), double integrator = closed loop on (q_state,
// qd_state); pos == nullptr: nothing per step is stored (mpk_episode_return: ep.ret / ep.seg_out).  MPK_ENOTIMPL for other shapes.
bool phase_fused_capable(const DevCfg& c);
int launch_phase_fused(const DevCfg& c, const TrajRequest& q, const LaunchSite& at);
// per-episode-phase DMP: the interpolation table of the forcing rows (mpk_traj_phase.hip fast_rows_build), built once per handle
int fast_rows_floats(const DevCfg& c);      // 0: none for this shape
int fast_rows_stride(const DevCfg& c);      // floats per node = the consuming kernels' KS
int launch_fast_rows_table(const DevCfg& c, float* out, void* stream);
// MPK_DMP_FIRST_IS_STEP: (init_pos, init_vel) advanced by one Euler step from init_time to the first grid time
int launch_dmp_prestep(const DevCfg& c, const TrajRequest& q, float* pos1, float* vel1, void* stream);
int launch_condition_gather(const float* pos, const float* vel, const int32_t* seg_len, float* cond_pos, float* cond_vel,
                            int B, int T, int D, void* stream);
int launch_reacher_rollout(const RolloutDev& rc, int D, const float* des_pos, const float* des_vel, double* q,
                           double* qd, const int32_t* n_steps, const int32_t* step0, const double* goal,
                           int steps_before_reward, float* actions, double* rewards, int B, int T, void* stream,
                           const Tuning& tune, int* fault);
// mpk_reacher_rollout_vjp (mpk_rollout_vjp.hip): the adjoint of launch_reacher_rollout's computation, one launch; any upstream gradient
// and any output may be nullptr (0 / not written).  MPK_ENOTIMPL: more than kMaxD DoF, a plant other than the double integrator, a
// horizon whose tile checkpoints do not fit the LDS.  g_cond_pos / g_cond_vel [B, D]: the upstream of the forward's condition output,
// added to row clamp(n - 1, 0, T - 1) of g_des_pos / g_des_vel whatever the controller reads; nullptr = 0.
// the name of a kernel's variant with the condition upstream (GC): `plain` + " + cond", interned -- the pointer stays valid
const char* cond_variant_name(const char* plain);
int launch_reacher_rollout_vjp(const RolloutDev& rc, int D, const float* des_pos, const float* des_vel, const double* q0,
                               const double* qd0, const int32_t* n_steps, const int32_t* step0, const double* goal,
                               int steps_before_reward, const double* g_rewards, const double* g_q, const double* g_qd,
                               const float* g_cond_pos, const float* g_cond_vel,
                               float* g_des_pos, float* g_des_vel, double* g_q0, double* g_qd0, double* g_goal, int B, int T,
                               void* stream, const char** kernel_name);
// mpk_episode_return_vjp (mpk_episode_vjp.hip): mpk_trajectory, launch_reacher_rollout_vjp and launch_traj_vjp composed in one launch --
// the plan is recomputed from (params, init_pos, init_vel) with the forward's bits, the desired-trajectory gradients never leave the lane.
// Any upstream gradient and any output may be nullptr (0 / not written).  c, st: the configuration and tables of the launch (a DMP
// handle: its response configuration).  MPK_ENOTIMPL: more than kMaxD DoF or kMaxKP columns, a plant other than the double integrator, a
// horizon whose tile checkpoints do not fit the LDS.
struct EpisodeVjpAsk {
    const float *params = nullptr, *init_pos = nullptr, *init_vel = nullptr;   // [B, P], [B, D], [B, D]
    const double *q0 = nullptr, *qd0 = nullptr;                         // [B, D] the state at the start of the plan
    const int32_t *n_steps = nullptr, *step0 = nullptr;                 // [B]
    const double* goal = nullptr;                                       // [B, 2]
    int steps_before_reward = 0, agg = 0;                               // MPK_AGG_*
    const double *g_ret = nullptr, *g_q = nullptr, *g_qd = nullptr;     // [B], [B, D], [B, D] upstream
    const float *g_cond_pos = nullptr, *g_cond_vel = nullptr;           // [B, D] upstream of the forward's condition output
    float *g_params = nullptr, *g_init_pos = nullptr, *g_init_vel = nullptr;
    double *g_q0 = nullptr, *g_qd0 = nullptr, *g_goal = nullptr;
    double *q_end = nullptr, *qd_end = nullptr;                         // [B, D] the state after n_steps, from the replay
};
int launch_episode_return_vjp(const DevCfg& c, const SharedTables& st, const RolloutDev& rc, const EpisodeVjpAsk& q, int B, void* stream,
                              std::string* kernel_name);
int episode_return_vjp_limits(const DevCfg& c);     // MPK_OK, or MPK_ENOTIMPL with the DoF / column / horizon limit in the message
// mpk_hole_reacher_rollout (mpk_hole.hip): the HoleReacher step loop with its break on collision
struct HoleLaunch {
    RolloutDev rc;
    const float* des_pos = nullptr;
    const float* des_vel = nullptr;
    double* q = nullptr;
    double* qd = nullptr;
    const int32_t* n_steps = nullptr;
    const int32_t* step0 = nullptr;
    const double* hole = nullptr;
    float* actions = nullptr;
    double* rewards = nullptr;
    double* ret = nullptr;
    int32_t* n_exec = nullptr;
    uint8_t* collided = nullptr;
    uint8_t* success = nullptr;
    ReplanDev rp;
    double penalty = 0.0;
    int allow_self = 0, allow_wall = 0, steps_before_reward = 0, agg = 0;
    int rew_fct = 0;                        // MPK_HOLE_REW_*
    double* reward_state = nullptr;         // [B, 2] unbounded's stored end effector (MPK_HOLE_REW_UNBOUNDED only)
};
int launch_hole_rollout(const HoleLaunch& h, int B, int T, int D, void* stream, const Tuning& tune);
// mpk_hole_reacher_rollout_vjp (mpk_hole_vjp.hip): the adjoint of launch_hole_rollout's computation with the episode's end and collision
// verdict frozen (n_exec, collided: the forward's outputs), one launch; any upstream gradient and any output may be nullptr (0 / not
// written).  rew_fct: MPK_HOLE_REW_SIMPLE or _VEL_ACC.  MPK_ENOTIMPL: more than kMaxD DoF, a horizon whose tile checkpoints do not fit
// the LDS.
struct HoleVjpLaunch {
    RolloutDev rc;
    const float *des_pos = nullptr, *des_vel = nullptr;                 // [B, T, D]; the one the controller does not read may be nullptr
    const double *q0 = nullptr, *qd0 = nullptr;                         // [B, D] the state at the start of the plan
    const int32_t *n_exec = nullptr, *step0 = nullptr;                  // [B]
    const double* hole = nullptr;                                       // [B, 3]
    const uint8_t* collided = nullptr;                                  // [B]
    int agg = 0;                                                        // MPK_AGG_*
    const double *g_ret = nullptr, *g_rewards = nullptr, *g_q = nullptr, *g_qd = nullptr;   // [B], [B, T], [B, D], [B, D] upstream
    const float *g_cond_pos = nullptr, *g_cond_vel = nullptr;           // [B, D] upstream of the forward's condition output
    float *g_des_pos = nullptr, *g_des_vel = nullptr;
    double *g_q0 = nullptr, *g_qd0 = nullptr, *g_hole = nullptr;
    double penalty = 0.0;
    int steps_before_reward = 0, rew_fct = 0;
};
int launch_hole_rollout_vjp(const HoleVjpLaunch& h, int B, int T, int D, void* stream, const char** kernel_name);
// mpk_trajectory_phase_vjp (mpk_phase_vjp.hip): the transpose of the per-episode-phase trajectory map of promp / prodmp (learned tau /
// delay, per-episode init_time) with prodmp's table indices held and torch.clamp's mask on tau / delay, one launch; either upstream
// gradient and any output may be nullptr (not read / not written).  MPK_ENOTIMPL: dmp, promp with T = 1, shapes beyond the wave
// kernel k_traj_phase's (<= kMaxD DoF here).
struct PhaseVjpLaunch {
    const float *params = nullptr, *init_pos = nullptr, *init_vel = nullptr;    // [B, P], [B, D], [B, D] the forward's inputs
    const float* init_time = nullptr;                                           // [B] per episode; nullptr: init_time_shared
    float init_time_shared = 0.f;
    const float *g_pos = nullptr, *g_vel = nullptr;                             // [B, T, D] upstream
    float *g_params = nullptr, *g_init_pos = nullptr, *g_init_vel = nullptr;    // [B, P], [B, D], [B, D]
    int32_t* range_flag = nullptr;
    int B = 0;
};
int launch_phase_vjp(const DevCfg& c, const PhaseVjpLaunch& q, int num_cu, void* stream, const char** kernel_name);
// mpk_trajectory_fit (mpk_traj_fit.hip): the regularised least-squares fit of the shared-phase map to demonstrated positions, one
// launch of k_traj_fit_tile.  fac: fit_factor_doubles() device doubles from fit_factor_build -- the Cholesky factor of the fitted columns'
// Gram matrix plus reg I and the cross term of the given columns, from the float32 position rows [KP][TS] of the launch's table (host
// copy).  c: the configuration the tables were built for (a DMP handle: its response configuration).  traj_fit_limits: MPK_OK, or
// MPK_ENOTIMPL with the DoF / column / horizon limit in the message (no HIP call; the outputs may be nullptr).
int fit_factor_doubles();
int fit_factor_build(const DevCfg& c, const float* rows, int TS, double reg, double* fac);
int traj_fit_limits(const DevCfg& c, size_t* lds_out, int* sh_out, int* stride_out);
// mpk_trajectory_phase_fit (mpk_traj_fit.hip): the same fit for a per-episode phase of promp / prodmp, one launch of k_phase_fit: one
// wave per episode builds the episode's own Gram matrix, factors it and solves.  phase: the tau / delay columns of params [B, n_phase]
// (nullptr: none learned).  status: set to 1 by an episode whose Gram + reg I is not positive definite (its params row is NaN).
// MPK_ENOTIMPL: dmp, shapes beyond the wave kernel k_traj_phase's (phase_fit_limits: no HIP call).
struct PhaseFitLaunch {
    const float *pos = nullptr, *phase = nullptr, *init_pos = nullptr, *init_vel = nullptr;
    const float* init_time = nullptr;
    float init_time_shared = 0.f;
    double reg = 0.0;
    float* params = nullptr;
    int32_t *range_flag = nullptr, *status = nullptr;
    int B = 0;
};
int phase_fit_limits(const DevCfg& c);
int launch_phase_fit(const DevCfg& c, const PhaseFitLaunch& q, int num_cu, void* stream, const char** kernel_name);
int launch_traj_fit(const DevCfg& c, const SharedTables& st, const double* fac, const float* pos, const float* init_pos,
                    const float* init_vel, float* params, int B, int num_cu, void* stream, const char** kernel_name);
// mpk_trajectory_std (mpk_traj_std.hip): the standard deviation of the shared-phase trajectory under a Gaussian over the non-phase
// parameters given by its lower-triangular factor params_L [B, Pl, Pl], Pl = D Kloc -- the norm of the table row times L, one launch of
// k_traj_std_tile; either output may be nullptr (not computed, not written).  traj_std_limits: MPK_OK, or MPK_ENOTIMPL with the reason in
// the message -- a DMP, more than kMaxD DoF or kMaxKP columns, a horizon whose tables and output images do not fit the LDS (no HIP call;
// the outputs may be nullptr).
int traj_std_limits(const DevCfg& c, size_t* lds_out, int* pitch_out, int* image_out);
int launch_traj_std(const DevCfg& c, const SharedTables& st, const float* params_L, float* pos_std, float* vel_std, int B, int num_cu,
                    void* stream, const char** kernel_name);
// ---- the probabilistic entry points: a launch request is {in, obs, out}, composed from these parts (mpk_gauss_launch.h has the launch
// plumbing the four wave-per-episode units share)
struct GaussIn {                                                        // the Gaussian N(params, L L^T) and the movement's start
    const float *params = nullptr, *params_L = nullptr, *init_pos = nullptr, *init_vel = nullptr;
    float init_time = 0.f;                                              // the tables' (init_time_shared)
    int B = 0;
};
struct PointObs {                                                       // positions / velocities at M shared steps; either pair may be nullptr
    const int32_t* steps = nullptr;                                     // HOST [M], validated by the caller (strictly increasing, in [0, T))
    int M = 0;
    const float *obs_pos = nullptr, *obs_pos_std = nullptr, *obs_vel = nullptr, *obs_vel_std = nullptr;   // [B, M, D]
};
struct DemoObs {                                                        // whole demonstrations
    const float *pos = nullptr, *obs_std = nullptr;                     // [B, T, D]
    bool phase = false;                                                 // the per-episode-phase route (mpk_demonstration_phase_*)
    int32_t* range_flag = nullptr;                                      // phase, ProDMP: raised beyond the pre-computed range
};
struct LikelihoodOut {                                                  // grad = false: log_prob is written; grad = true: g is read and
    bool grad = false;                                                  // g_params / g_params_L (either may be nullptr) are written
    double* log_prob = nullptr;                                         // [B]
    const double* g = nullptr;                                          // [B]
    float *g_params = nullptr, *g_params_L = nullptr;
};
struct PosteriorOut {                                                   // may be the inputs
    float *params_out = nullptr, *params_L_out = nullptr;
};
// mpk_trajectory_condition (mpk_traj_condition.hip): the Gaussian over the non-phase parameters conditioned on point observations -- a
// sequential square-root measurement update of the factor in float64, one launch of k_traj_condition, one wave per episode.
// traj_cond_limits: MPK_OK, or MPK_ENOTIMPL with the reason in the message -- a DMP, more than kMaxD DoF or kMaxKP columns, a Pl whose
// float64 triangle and work vectors exceed the LDS with one wave per workgroup (no HIP call; the outputs may be nullptr).
// mpk_trajectory_phase_* : the point-observation kernels with a PER-EPISODE row source (phase = true) for handles that learn tau /
// delay: every wave evaluates its own episode's rows at the tau / delay in front of its params row (mpk_phase_rows.h, float64; the
// velocity row included) into an image of its own, [2][M][Kloc + 3] float64 more per wave; no shared table is read (st is ignored).
// traj_cond_phase_limits / traj_log_prob_phase_limits: the shared route's refusals in the same words, under the _phase_ entry's name,
// plus rows beyond the 16 slots.  range_flag: raised by a ProDMP timing beyond the pre-computed range.
struct CondLaunch {
    GaussIn in;
    PointObs obs;
    PosteriorOut out;
    bool phase = false;
    int32_t* range_flag = nullptr;
};
int traj_cond_limits(const DevCfg& c, int M, size_t* lds_out, int* waves_out, int* wave_doubles_out);
int traj_cond_phase_limits(const DevCfg& c, int M, size_t* lds_out, int* waves_out, int* wave_doubles_out);
int launch_traj_condition(const DevCfg& c, const SharedTables& st, const CondLaunch& q, int num_cu, void* stream, const char** kernel_name);
// mpk_trajectory_log_prob / _vjp (mpk_traj_log_prob.hip): the log-likelihood of conditioning's scalar observations under N(params, L L^T)
// by a dense float64 Cholesky factorisation of their n x n covariance, and its gradient w.r.t. params and params_L -- one launch of
// k_traj_log_prob each, one wave per episode, the gradient launch recomputing everything from the inputs.  traj_log_prob_limits: MPK_OK,
// or MPK_ENOTIMPL with the reason in the message -- a DMP, more than kMaxD DoF or kMaxKP columns, more than MPK_LOGPROB_MAX_OBS candidate
// observations (M D narr, narr the observation arrays given), float64 images that exceed the LDS with one wave per workgroup (no HIP
// call; the outputs may be nullptr).
struct LogProbLaunch {
    GaussIn in;
    PointObs obs;
    LikelihoodOut out;
    bool phase = false;
    int32_t* range_flag = nullptr;
};
int traj_log_prob_limits(const DevCfg& c, int M, int narr, size_t* lds_out, int* waves_out, int* wave_doubles_out);
int traj_log_prob_phase_limits(const DevCfg& c, int M, int narr, const char* fn, size_t* lds_out, int* waves_out, int* wave_doubles_out);
// mpk_trajectory_phase_std (mpk_traj_phase_std.hip): the trajectory's standard deviation at a per-episode tau / delay, one launch of
// k_traj_phase_std, one wave per episode, the factor form on float64 rows.  traj_phase_std_limits: MPK_OK, or MPK_ENOTIMPL with the
// reason in the message -- a DMP, more than kMaxD DoF or kMaxKP columns, rows beyond the 16 slots, a factor one wave's LDS cannot hold.
int traj_phase_std_limits(const DevCfg& c, size_t* lds_out, int* waves_out, int* wave_floats_out);
int launch_traj_phase_std(const DevCfg& c, const float* params, const float* params_L, float init_time, float* pos_std, float* vel_std,
                          int32_t* range_flag, int B, int num_cu, void* stream, const char** kernel_name);
int launch_traj_log_prob(const DevCfg& c, const SharedTables& st, const LogProbLaunch& q, int num_cu, void* stream,
                         const char** kernel_name);
// mpk_demonstration_log_prob / _vjp (mpk_demo_log_prob.hip): the log-likelihood of whole demonstrations under N(params, L L^T) in the
// information form -- the Gram matrices G_d, M = I + tril(L)^T G tril(L) = C C^T [Pl x Pl] -- and its gradient w.r.t. params and
// params_L: one launch of k_demo_log_prob each, one wave per episode, the gradient launch recomputing everything from the inputs.
// demo_log_prob_limits: MPK_OK and the launch's plan (plan may be nullptr), or MPK_ENOTIMPL with the limit in the message, under the
// entry's name fn -- a DMP, more than kMaxD DoF or kMaxKP columns, Pl > 64 x 4, float64 images that exceed the LDS with one wave per
// workgroup (no HIP call).
// mpk_demonstration_phase_* : the same two kernels with a PER-EPISODE row source (template flag PHASE, obs.phase) for handles that learn
// tau / delay: the tau / delay of episode b are given at the front of params[b], clipped as the forward clips them; the wave evaluates
// its episode's rows a chunk of steps at a time (mpk_phase_rows.h, k_phase_fit's row evaluation) into a chunk image of its own, and no
// shared table is read (st is ignored).  demo_phase_limits: demo_log_prob_limits' refusals in the same words -- with the chunk image
// [tc][(Kloc + 3) | 1] added per wave and [T][KT] replaced by row constants and base times per workgroup -- plus rows beyond
// k_traj_phase's 16 slots.
struct DemoLogProbLaunch {
    GaussIn in;
    DemoObs obs;
    LikelihoodOut out;
};
struct DemoPlan {
    size_t lds = 0;                                                     // bytes per workgroup
    int waves = 0, wave_doubles = 0, tc = 0, scratch = 0;
    int sl = 0, chunk = 0, c_pad = 0;                                   // the phase route's (0 otherwise)
};
int demo_log_prob_limits(const DevCfg& c, DemoPlan* plan, const char* fn = "mpk_demonstration_log_prob");
int demo_phase_limits(const DevCfg& c, DemoPlan* plan, const char* fn);
int launch_demo_log_prob(const DevCfg& c, const SharedTables& st, const DemoLogProbLaunch& q, int num_cu, void* stream,
                         const char** kernel_name);
// mpk_demonstration_condition (mpk_demo_condition.hip): N(params, L L^T) conditioned on the kept entries of whole demonstrations, in the
// same information form -- M = K^T K from the last row (the reverse Cholesky), L' = tril(L) K^-1, mu' = mu + L' K^-T v: one launch of
// k_demo_condition, one wave per episode, k_demo_log_prob's images and workgroups (its limits refuse under this entry's name).
// demo_condition_launch_plan: the workgroups, waves per workgroup and LDS bytes a launch of B episodes takes, on either route (no HIP
// call; any output may be nullptr).
struct DemoCondLaunch {
    GaussIn in;
    DemoObs obs;
    PosteriorOut out;
};
int demo_condition_launch_plan(const DevCfg& c, int B, int num_cu, bool phase, int32_t* blocks_out, int32_t* waves_out,
                               int32_t* lds_bytes_out);
int launch_demo_condition(const DevCfg& c, const SharedTables& st, const DemoCondLaunch& q, int num_cu, void* stream,
                          const char** kernel_name);
int launch_episode_reset(const double* init_q, const double* init_qd, double* q, double* qd, float* cond_pos,
                         float* cond_vel, int32_t* traj_steps, int32_t* plan_steps, uint8_t* done, int B, int D,
                         void* stream);
// mpk_reacher_reset (mpk_reset.hip): seeded / continued reacher resets on numpy's generator
struct ResetLaunch {
    const uint64_t* seeds = nullptr;
    uint64_t seed_base = 0;
    int seeded_base = 0;
    void* rng = nullptr;
    double* q = nullptr;
    double* qd = nullptr;
    float* cond_pos = nullptr;
    float* cond_vel = nullptr;
    int32_t* traj_steps = nullptr;
    int32_t* plan_steps = nullptr;
    uint8_t* done = nullptr;
    double* task_out = nullptr;
    double target[2] = {0.0, 0.0};
    double hole_width = 0.0, hole_x = 0.0, hole_depth = 0.0;
    int env = 0, random_start = 0;
};
int launch_reacher_reset(const ResetLaunch& l, int B, int D, void* stream, int* fault);
// mpk_reacher_observation / mpk_reacher_step_observations (mpk_obs.hip): reacher observation rows, current and replayed per step
struct ObsLaunch {
    uint64_t mask = 0;                  // full columns written, in order (never 0: the host expands "every column")
    double time_div = 0.0;              // > 0: a last column steps / time_div
    int env = 0, D = 0, n_full = 0, n_out = 0;
};
int launch_reacher_obs(const ObsLaunch& l, const double* q, const double* qd, const double* task, const int32_t* steps, float* out,
                       int B, void* stream);
int launch_reacher_step_obs(const ObsLaunch& l, const RolloutDev& rc, const float* des_pos, const float* des_vel, const double* q0,
                            const double* qd0, const double* task, const int32_t* n_exec, const int32_t* step0, float* out,
                            double* q_end, double* qd_end, int B, int T, void* stream);
// mpk_reacher_autoreset (mpk_autoreset.hip): last observation, reset of the selected episodes, next observation in one launch
// (o == nullptr: the masked reset alone)
int launch_reacher_autoreset(const ResetLaunch& l, const ObsLaunch* o, const uint8_t* mask, uint8_t* reset_mask, float* final_obs,
                             float* obs, int B, int D, void* stream, int* fault);
// mpk_reacher_env_step (mpk_env_step.hip): one step of the step-based reacher envs plus the same-step autoreset, one launch
struct EnvStepLaunch {
    ResetLaunch reset;                  // q, qd, traj_steps, rng, task_out; no seeds, no plan_steps / done / cond
    ObsLaunch obs_layout;               // the full row
    const float* actions = nullptr;
    double* reward_state = nullptr;
    double* reward = nullptr;
    uint8_t* terminated = nullptr;
    uint8_t* truncated = nullptr;
    uint8_t* collided = nullptr;
    uint8_t* success = nullptr;
    uint8_t* reset_mask = nullptr;
    float* final_obs = nullptr;
    float* obs = nullptr;
    double dt = 0.0, penalty = 0.0;
    int allow_self = 0, allow_wall = 0, steps_before_reward = 0, max_steps = 0, autoreset = 0, rew_fct = 0;
};
int launch_reacher_env_step(const EnvStepLaunch& e, int B, int D, void* stream, int* fault);
int launch_gate_flags(const uint8_t* valid, const uint8_t* was_done, const uint8_t* done, uint8_t* terminated, uint8_t* truncated, int B,
                      void* stream);
int launch_replan_advance(int32_t* traj_steps, int32_t* plan_steps, int32_t* seg_len, uint8_t* done, int every,
                          int max_planning_times, int horizon, int T, int B, void* stream, const uint8_t* valid = nullptr);
int launch_validity(const float* pos, const float* params, int P, int D, const double* lo, const double* hi,
                    int check_td, const double* tb, const double* db, uint8_t* valid, double* penalty, int B, int T,
                    void* stream);

int launch_scaled_basis(const DevCfg& c, const float* times, int n, float* out, void* stream);
int launch_div_sweep(float d, uint32_t first, uint64_t count, unsigned long long* mismatches, void* stream);

size_t shared_tables_floats(const DevCfg& c, int* TS, int* n_out);
bool shared_tables_lean(const DevCfg& c);     // k_traj_wide-only shapes: position (prodmp: + velocity) rows, no step-major copy
bool traj_wide_fits(const DevCfg& c);         // false: launch_traj_wide would return MPK_ENOTIMPL (ask before building its table)


void set_error(const std::string& msg);

}  // namespace mpk
