// Single-translation-unit build of every gfx950 kernel of libmpk.so: tools/dev/one_kernel.sh (one instantiation in seconds,
// -DMPK_DEVICE_ONLY) and the -DMPK_TRACE development builds (the trace buffer is one device variable).  The library itself is
// built from the files below as separate translation units, in parallel (__graft_entry__.py):
//   mpk_dev.h            scalar device helpers shared by everything
//   mpk_tile.h           the 16 x 16 tile machinery (arguments, lane maps, step chains, epilogue, stores)
//   mpk_traj_{tiles,stream,flat,quad,pipe}.h   one shared-phase trajectory kernel family each
//   mpk_traj_family.hip  the families' template launcher, one unit per MP type (-DMPK_MP_UNIT=0..2)
//   mpk_traj_ring.h / .hip   k_traj_ring / k_traj_burst + their launcher, one unit per MP type
//   mpk_episode.hip      k_episode_return (verbose < 2 step: nothing per step stored), one unit per MP type
//   mpk_reward.h         SimpleReacher reward on float64 LDS images (rollout + episode kernels)
//   mpk_traj_route.h     TrajRoute / EpRoute (what the selection rule hands to the launchers above), their declarations, dispatch helpers
//   mpk_traj_launch.hip  k_build_shared + plan_traj_shared (kernel selection rule, one function per family) + launch_traj_shared
//   mpk_traj_wide.hip    k_traj_wide
//   mpk_traj_vjp.hip     k_traj_vjp_tile / k_traj_vjp_generic: the shared-phase map transposed (mpk_trajectory_vjp)
//   mpk_run_stage.h      an episode's contiguous run HBM -> LDS image, alignment-shifted, shared by mpk_traj_vjp.hip and mpk_traj_fit.hip
//                        (and the way back, LDS image -> HBM: mpk_traj_std.hip)
//   mpk_traj_fit.hip     k_traj_fit_tile: the least-squares fit of the shared-phase map to demonstrations (mpk_trajectory_fit)
//   mpk_traj_std.hip     k_traj_std_tile: the trajectory's standard deviation from the factor of a weight covariance (mpk_trajectory_std)
//   mpk_traj_phase_std.hip   k_traj_phase_std: the same at a per-episode tau / delay, on float64 rows (mpk_trajectory_phase_std)
//   mpk_traj_condition.hip   k_traj_condition: a Gaussian over the parameters conditioned on observed points (mpk_trajectory_condition)
//   mpk_traj_log_prob.hip    k_traj_log_prob: the log-likelihood of observed points under that Gaussian and its gradient (mpk_trajectory_log_prob)
//   mpk_demo_log_prob.hip    k_demo_log_prob: the log-likelihood of whole demonstrations in the Pl x Pl form and its gradient (mpk_demonstration_log_prob)
//   mpk_demo_condition.hip   k_demo_condition: the Gaussian conditioned on whole demonstrations in the same form (mpk_demonstration_condition)
//   mpk_demo_gram.h      the Gram accumulation and the packed M of the information form, shared by the two units above
//   mpk_cond_rows.h      the observed steps' float64 table rows and the wave-level LDS ordering, shared by the five units above
//   mpk_traj_phase.hip   per-episode phase kernels
//   mpk_phase_fused.hip  per-episode phase: the fused entry points (actions, closed loop, replanning step, verbose < 2 step, validity gate)
//   mpk_rollout.hip      rollout kernels
//   mpk_rollout_vjp.hip  k_reacher_rollout_vjp: the reacher rollout transposed (mpk_reacher_rollout_vjp)
//   mpk_episode_vjp.hip  k_episode_return_vjp: plan, rollout adjoint and table transpose in one launch (mpk_episode_return_vjp)
//   mpk_vjp_row.h        the transpose's table rows and transposed input gather, shared by mpk_traj_vjp.hip and mpk_episode_vjp.hip
//   mpk_hole.hip         HoleReacher: direct-velocity plant, collisions, reward, break on collision
//   mpk_hole_vjp.hip     k_hole_rollout_vjp: the HoleReacher rollout transposed, end and verdict frozen (mpk_hole_reacher_rollout_vjp)
//   mpk_phase_vjp.hip    k_phase_vjp: the per-episode-phase trajectory map transposed, tau / delay included (mpk_trajectory_phase_vjp)
//   mpk_reacher_env.h    the reacher envs' draw programs and observation row, shared by the three units below
//   mpk_reset.hip        reacher resets: numpy's generator per episode (mpk_nprng.h), seeded / continued draws
//   mpk_obs.hip          reacher observations: current rows, per-step rows replayed on the stored plan (mpk_plant.h)
//   mpk_autoreset.hip    per-episode autoreset of a vector step: last observation, masked reset, next observation (mpk_reacher_env.h)
//   mpk_hole_geom.h      HoleReacher's link-crossing / wall tests and dtype-bound reward terms, shared by mpk_hole.hip and the unit below
//   mpk_env_step.hip     one step of the step-based reacher envs with the same-step autoreset (plant, collisions, reward, observations)
//   mpk_misc.hip         integer state, reset, gather, validity, self-tests, trace readout
#define MPK_AMALGAMATED 1
#include "mpk_traj_family.hip"
#include "mpk_traj_ring.hip"
#include "mpk_episode.hip"
#include "mpk_traj_launch.hip"
#include "mpk_traj_wide.hip"
#include "mpk_traj_vjp.hip"
#include "mpk_traj_fit.hip"
#include "mpk_traj_std.hip"
#include "mpk_traj_phase_std.hip"
#include "mpk_traj_condition.hip"
#include "mpk_traj_log_prob.hip"
#include "mpk_demo_log_prob.hip"
#include "mpk_demo_condition.hip"
#include "mpk_traj_phase.hip"
#include "mpk_phase_fused.hip"
#include "mpk_rollout.hip"
#include "mpk_rollout_vjp.hip"
#include "mpk_episode_vjp.hip"
#include "mpk_hole.hip"
#include "mpk_hole_vjp.hip"
#include "mpk_phase_vjp.hip"
#include "mpk_reset.hip"
#include "mpk_obs.hip"
#include "mpk_autoreset.hip"
#include "mpk_env_step.hip"
#include "mpk_misc.hip"
