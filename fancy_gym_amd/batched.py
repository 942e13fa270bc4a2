"""
BatchedBlackBox -- the batched sibling of BlackBoxWrapper: B independent episodes of ONE movement-primitive
configuration evaluated at once on one GPU (the reference always runs B = 1: black_box_wrapper.py:96-120,175-203).

One ``step(params[B, P])`` does what ``BlackBoxWrapper.step`` does for every episode:
    plan      get_trajectory: clip -> (frozen tau/delay) -> boundary conditions -> (pos, vel)[B, T, D]     [HIP]
    validity  optional joint-limit / bound check (raw_interface_wrapper.py:55-72)                         [HIP]
    schedule  integer replanning bookkeeping for the schedule ``t % every == 0``                            [HIP]
    execute   tracking controller + plant loop for the executed steps (plants that live on the GPU)        [HIP]
and returns everything as CUDA tensors.  Environments that cannot live on the GPU (MuJoCo) consume ``des_pos`` /
``des_vel`` on the host instead (``plant=None``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .black_box.controller.base_controller import BaseController
from .engine import RolloutSpec, TrajectoryEngine
from .mp.traj import MPInterface


def reacher_observation_layout(reward: str, n_links: int, random_start: bool = True, hole_width=None, context: bool = True,
                               time_aware: bool = False):
    """
    The observation a BlackBoxWrapper over a reacher env hands out, as (col_mask, space): ``col_mask`` bit c = column c of the env's
    full _get_obs() row is part of it (mpk.h: mpk_obs_cfg), ``space`` the wrapper's observation_space.  Full row and bounds as the
    envs build them (base_reacher.py:40-48, simple_reacher.py:32-39; HoleReacher adds the hole width before the goal offset);
    ``context`` masks it with the MP wrapper's context_mask (simple_reacher/mp_wrapper.py, hole_reacher/mp_wrapper.py;
    black_box_wrapper.py:141-148), ``time_aware`` appends TimeAwareObservation's [0, 1] column (utils/wrappers.py:33-38).
    """
    from . import _gym
    n = int(n_links)
    hole = reward == "hole_reacher"
    if reward not in ("simple_reacher", "hole_reacher"):
        raise ValueError(f"no env observation for reward {reward!r}")
    bound = np.hstack([[np.pi] * n, [np.pi] * n, [np.inf] * n] + ([[np.inf]] if hole else []) + [[np.inf] * 2, [np.inf]])
    mask = np.hstack([[bool(random_start)] * (3 * n)] + ([[hole_width is None]] if hole else []) + [[True, True], [False]])
    keep = mask.astype(bool) if context else np.ones(bound.shape, bool)
    col_mask = sum(1 << int(c) for c in np.flatnonzero(keep))
    low, high = -bound[keep], bound[keep]
    if time_aware:
        low, high = np.append(low, 0.0), np.append(high, 1.0)
    return col_mask, _gym.spaces.Box(low=low, high=high, dtype=np.float32)


class BatchedBlackBox:

    def __init__(self, trajectory_generator: MPInterface, tracking_controller: BaseController, num_envs: int,
                 dt: float, duration: float, act_low=-math.inf, act_high=math.inf,
                 plant: Optional[str] = "double_integrator", replanning_every: Optional[int] = None,
                 max_planning_times: Union[int, float] = math.inf, condition_on_desired: bool = False,
                 max_episode_steps: Optional[int] = None, pos_limits: Optional[Sequence] = None,
                 check_tau_delay: bool = False, reward: Optional[str] = None, steps_before_reward: int = 199,
                 device=None, learn_sub_trajectories: bool = False, reward_aggregation="sum", verbose: int = 2,
                 collision_penalty: float = 100.0, allow_self_collision: bool = False, allow_wall_collision: bool = False,
                 env_kwargs: Optional[dict] = None, observations: bool = False, rew_fct: str = "simple",
                 collision_gradient: Optional[str] = None, phase_gradient: Optional[str] = None,
                 replan_gradient: Optional[str] = None):
        """
        trajectory_generator / tracking_controller: the objects the factories return (``get_trajectory_generator``,
        ``get_controller``).  ``replanning_every = n`` is the schedule ``lambda pos, vel, obs, action, t: t % n == 0``
        (e.g. envs/mujoco/box_pushing/mp_wrapper.py:89).  ``pos_limits = (low[D], high[D])`` enables the batched
        validity check (envs/mujoco/table_tennis/table_tennis_env.py:303-309).  ``reward = "simple_reacher"`` adds the
        per-step reward of the reference's SimpleReacher (envs/classic_control/simple_reacher/simple_reacher.py:56-72)
        to the device rollout: ``step`` then also returns ``step_rewards [B, T]`` and their sum ``rewards [B]``
        (``reward_aggregation``: "sum" / "mean" / "last" or np.sum / np.mean -- black_box_wrapper.py:24,216 -- over the EXECUTED
        steps of each episode, on the device); goals are given to ``reset``.

        ``reward = "hole_reacher"`` with ``plant = "velocity_direct"`` runs the reference's HoleReacher (envs/classic_control/
        hole_reacher, rew_fct "simple"; ``collision_penalty`` / ``allow_self_collision`` / ``allow_wall_collision`` as its kwargs) on
        the device: a collision ends the episode in the middle of a plan (terminated, black_box_wrapper.py:197-203), so
        ``trajectory_length`` is the executed steps and ``rewards`` aggregates only those.  Holes [B, 3] = (x, width, depth) are given
        to ``reset`` (``sample_hole_reacher_starts`` draws starts and holes as the reference does).  ``step`` also returns
        ``is_collided`` / ``is_success``.  Collided episodes are done, so the live ones keep lockstep under replanning.  ``rew_fct``
        is the env's reward function (hole_reacher.py:48-58): "simple" (the default), "vel_acc" or "unbounded" -- the last two with
        steps_before_reward = 199; "unbounded" keeps its end effector of step 180 in a device buffer of the object, across plans.

        ``reset(seed=...)`` draws the episodes on the device the way the registered env's ``reset(seed=...)`` does (one launch,
        mpk_reacher_reset): ``env_kwargs`` holds the env's reset constants -- SimpleReacher ``random_start``, ``target``; HoleReacher
        ``random_start``, ``hole_width``, ``hole_x``, ``hole_depth`` (None = drawn) -- and defaults to the registered ids' kwargs
        (fancy/(Long)SimpleReacher-v0: random start, goal drawn; fancy/HoleReacher-v0: random start, width and x drawn, depth 1).

        ``observations=True`` (a reacher reward, no ``pos_limits``) returns what BlackBoxWrapper returns as its observation, computed on
        the device (mpk_reacher_observation): ``observe()`` gives the current one [B, n_obs] float32 -- the context rows of the MP
        wrapper's context_mask, or with replanning / sub-trajectories the full rows plus TimeAwareObservation's t / max_episode_steps
        --, ``step`` adds it as ``obs`` and at verbose >= 2 ``step_observations`` [B, T, n_full] (the full rows the env returned
        per step, 0 behind ``trajectory_length``; one launch that replays the executed steps, mpk_reacher_step_observations).
        ``observation_space`` is the host wrapper's.  Off (the default), nothing is launched for it.

        ``learn_sub_trajectories`` (black_box_wrapper.py:98-102, utils/make_env_helpers.py:89-117): every ``step`` plans a new
        sub-trajectory of ``round(tau / dt)`` steps from the current state -- tau is the first parameter (``learn_tau``), read
        anew by every plan (nothing is frozen), clipped to its bounds; an episode ends when ``max_episode_steps`` are done.  On
        the device a plan is a row mask over the max-length plan: episode b executes the first ``round(tau_b / dt)`` rows
        (``trajectory_length``), the rows behind them are not part of its plan.  (A single-episode wrapper evaluates the plan on
        the grid ``linspace(0, T_b dt, T_b + 1)[1:]``, the batch on the first T_b points of the grid of the longest plan: the
        same times up to one fp32 rounding of the grid, exactly the same whenever the grid values are exact in fp32.)
        Not with replanning (make_env_helpers.py:91-92).

        Arbitrary ``replanning_schedule`` callables see host state per step and stay with the single-episode wrapper; the
        device schedule is ``t % replanning_every == 0``.

        ``verbose`` (black_box_wrapper.py:21,160,184,208-213): 2 (the default HERE: this class has always returned everything)
        ``step`` returns the plans, step actions and step rewards [B, T, .] like ``infos`` of a verbose = 2 wrapper; < 2 (the
        reference's default is 1) it returns what ``BlackBoxWrapper.step`` returns then -- the aggregated reward, the flags,
        ``trajectory_length`` and the plant state -- and with a device plant the whole step is ONE launch that stores nothing per
        step (mpk_episode_return): plan, controller, plant, reward and aggregation on the CU.  Same state bit for bit; the same
        aggregated rewards bit for bit wherever the verbose = 2 path writes its step rewards with the tile kernel (every shape this
        path accepts; the per-episode fallback kernel behind "pd_generic" 1 / D = 1 sums a step's squared actions as a tree: 1e-13
        relative -- mpk.h, mpk_episode_return).  Falls back to the verbose = 2 launches (and drops their arrays)
        where the fused kernel does not apply: sub-trajectories, a device reward together with a learned phase, drifted episodes.

        ``collision_gradient`` (None, the default, or "frozen"): HoleReacher's return is discontinuous where a collision starts or the
        episode's end moves, so ``step(differentiable=True)`` refuses reward "hole_reacher" unless this says what the gradient should
        be.  "frozen": the pathwise gradient with each episode's end and collision verdict held at what the forward found -- the
        collision penalty is a constant, the distance paid on the colliding step still pulls the arm (mpk_hole_reacher_rollout_vjp;
        rew_fct "simple" and "vel_acc").  Ignored by the other rewards.

        ``phase_gradient`` (None, the default, or "pathwise"): passed to ``TrajectoryEngine.trajectory`` by ``get_trajectory`` -- with
        "pathwise" a box with a learned tau / delay (the TableTennis / BeerPong families), or one whose episodes have their own plan
        clocks after partial resets, keeps the graph from ``des_pos`` / ``des_vel`` to ``params`` (one mpk_trajectory_phase_vjp launch
        backward; a ProDMP's table indices held, torch.clamp's mask on tau / delay).  NotImplementedError with
        ``learn_sub_trajectories``.  ``step(differentiable=True)`` is unchanged: its refusals stay.

        ``replan_gradient`` (None, the default, or "episode"): what ``step(differentiable=True)`` differentiates on a replanning box.
        None: every plan on its own -- this step's reward w.r.t. this step's parameters, the state and the condition the plan starts
        from are constants.  "episode": the gradient crosses plan boundaries.  The box keeps graph-carrying twins of the plant state
        (and, with ``condition_on_desired``, of the stored condition), bit for bit equal to ``q``, ``qd``, ``condition_pos``,
        ``condition_vel``; plan k starts from the twins plan k - 1 left (without ``condition_on_desired`` its init_pos / init_vel are
        ``twin.float()``, the cast being the identity for the derivative), so ``rewards`` of plan k reaches the ``params`` of every
        plan j <= k and the goal / hole, and ``step`` also returns ``end_pos`` / ``end_vel``, float64 [B, D]: the twins after the plan,
        for a cost on the state (``current_pos`` / ``current_vel`` stay the graph-free state).  Forward values, the in-place state and
        every integer output are the plain step's, from the same launches; each plan's backward is still the launch(es) of that plan
        (mpk_episode_return_vjp_cond, or mpk_reacher_rollout_vjp_cond / mpk_hole_reacher_rollout_vjp_cond + mpk_trajectory_vjp).  The
        chain is cut -- the next plan starts from constants -- by ``reset`` / ``reset_done`` / ``autoreset``, by any step that is not
        ``differentiable=True``, and by ``get_trajectory`` called on its own.  NOT differentiated: the state given to ``reset``, the
        observations, the integer schedule (which steps a plan executes, where an episode ends or collides).  Without replanning the
        option is accepted and changes nothing; every refusal of ``step(differentiable=True)`` stays.
        """
        if replan_gradient not in (None, "episode"):
            raise ValueError(f"replan_gradient must be None or 'episode', got {replan_gradient!r}")
        self.replan_gradient = replan_gradient
        self._twin = None           # replan_gradient="episode": the graph-carrying twins dict(q, qd[, cond_pos, cond_vel]) of the last plan
        if collision_gradient not in (None, "frozen"):
            raise ValueError(f"collision_gradient must be None or 'frozen', got {collision_gradient!r}")
        self.collision_gradient = collision_gradient
        if phase_gradient not in (None, "pathwise"):
            raise ValueError(f"phase_gradient must be None or 'pathwise', got {phase_gradient!r}")
        if phase_gradient is not None and learn_sub_trajectories:
            raise NotImplementedError("phase_gradient='pathwise' with learn_sub_trajectories is not built: tau also sets the number of "
                                      "steps a sub-trajectory executes, an integer the pathwise gradient cannot see")
        self.phase_gradient = phase_gradient
        if rew_fct != "simple" and reward != "hole_reacher":
            raise ValueError(f"rew_fct={rew_fct!r} is HoleReacher's reward function: it needs reward='hole_reacher'")
        _lib.hole_rew_fct(rew_fct, steps_before_reward)        # (refused before anything is built)
        self.rew_fct = rew_fct
        self.verbose = int(verbose)
        self._lean_ok = True
        self.traj_gen = trajectory_generator
        self.tracking_controller = tracking_controller
        self.B, self.dt, self.duration = int(num_envs), float(dt), float(duration)
        if device is not None:
            self.traj_gen._device = device
        self.traj_gen.set_duration(self.duration, self.dt)
        self.engine: TrajectoryEngine = self.traj_gen.engine()
        self.device = self.engine.device
        self.D, self.T = self.engine.num_dof, self.engine.num_steps
        self.horizon = int(max_episode_steps) if max_episode_steps is not None else self.T
        self.learn_sub_trajectories = bool(learn_sub_trajectories)
        if self.learn_sub_trajectories and replanning_every is not None:
            raise ValueError("Cannot used sub-trajectory learning and replanning together.")      # make_env_helpers.py:91-92
        if self.learn_sub_trajectories and not self.traj_gen.phase_gn.learn_tau:
            raise ValueError("learn_sub_trajectories needs a learned tau (make_bb sets learn_tau: make_env_helpers.py:110-112)")
        agg = {np.sum: "sum", np.mean: "mean"}.get(reward_aggregation, reward_aggregation)
        if agg not in ("sum", "mean", "last"):
            raise ValueError(f"reward_aggregation must be 'sum', 'mean', 'last', np.sum or np.mean on the device, got {reward_aggregation!r}")
        self.reward_aggregation = agg
        self.do_replanning = replanning_every is not None
        self.every = int(replanning_every) if self.do_replanning else self.horizon + 1
        self.max_planning_times = max_planning_times
        self.condition_on_desired = bool(condition_on_desired)
        self.plant = plant
        self.pos_limits = pos_limits
        self.check_tau_delay = bool(check_tau_delay)
        if reward not in (None, "simple_reacher", "hole_reacher"):
            raise ValueError(f"unknown device reward {reward!r}")
        if reward == "simple_reacher" and plant != "double_integrator":
            raise ValueError("the simple_reacher reward needs plant='double_integrator'")
        if (reward == "hole_reacher") != (plant == "velocity_direct"):
            raise ValueError("the hole_reacher reward and plant='velocity_direct' go together")
        self.hole_task = dict(collision_penalty=float(collision_penalty), allow_self_collision=bool(allow_self_collision),
                              allow_wall_collision=bool(allow_wall_collision))
        self.hole = None
        # unbounded's stored end effector [B, 2], allocated once: captured episodes keep pointing at it
        self._reward_state = (torch.zeros((self.B, 2), dtype=torch.float64, device=self.device) if rew_fct == "unbounded"
                              else None)
        self.reward = reward
        defaults = {"simple_reacher": dict(random_start=True, target=None),
                    "hole_reacher": dict(random_start=True, hole_width=None, hole_x=None, hole_depth=1.0)}.get(reward)
        if env_kwargs is not None:
            if defaults is None:
                raise ValueError("env_kwargs are the reset constants of a reacher reward (reward='simple_reacher' / 'hole_reacher')")
            unknown = set(env_kwargs) - set(defaults)
            if unknown:
                raise ValueError(f"env_kwargs of {reward!r} take {sorted(defaults)}, got {sorted(unknown)}")
            defaults = {**defaults, **env_kwargs}
        self.env_kwargs = defaults
        self.observations = bool(observations)
        self.observation_space = None
        if self.observations:
            if reward not in ("simple_reacher", "hole_reacher"):
                raise ValueError("observations=True needs reward='simple_reacher' or 'hole_reacher': the other device plants have no env "
                                 "observation")
            if pos_limits is not None:
                raise ValueError("observations=True does not take pos_limits: the observation of the invalid-plan callback is not built")
            context = not (self.learn_sub_trajectories or self.do_replanning)
            self._obs_time_div = 0.0 if context else float(self.horizon)     # t / max_episode_steps (the TimeLimit's steps)
            self._obs_mask, self.observation_space = reacher_observation_layout(
                reward, self.D, self.env_kwargs["random_start"], self.env_kwargs.get("hole_width"), context, not context)
        self._rng = None                    # int64 [B, 5]: every episode's numpy generator (mpk_nprng_state), after a seeded reset
        self._task_buf = None               # the goal / hole buffer the device resets write
        self.steps_before_reward = int(steps_before_reward)
        self.goal = None
        ctype = getattr(tracking_controller, "device_type", None)
        self.spec = None
        if plant is not None:
            if ctype is None:
                raise ValueError(f"{type(tracking_controller).__name__} has no device implementation; use plant=None "
                                 f"and step the environments on the host")
            self.spec = RolloutSpec(ctype, self.D, getattr(tracking_controller, "p_gains", 0.0),
                                    getattr(tracking_controller, "d_gains", 0.0), act_low, act_high, plant=plant,
                                    dt=self.dt)
        phase = self.traj_gen.phase_gn
        self.tau_bound = getattr(phase, "tau_bound", [-np.inf, np.inf])
        self.delay_bound = getattr(phase, "delay_bound", [-np.inf, np.inf])
        self._n_phase = int(phase.learn_tau) + int(phase.learn_delay)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.traj_steps = torch.zeros(self.B, **i32)
        self.plan_steps = torch.zeros(self.B, **i32)
        self.done = torch.zeros(self.B, dtype=torch.uint8, device=self.device)
        self._prev_done, self._prev_done_known = None, True
        self.q = torch.zeros((self.B, self.D), dtype=torch.float64, device=self.device)
        self.qd = torch.zeros_like(self.q)
        self.condition_pos = None
        self.condition_vel = None
        self._frozen_phase = None
        # traj_steps of every live episode while the schedule keeps them in lockstep; None = per-episode init_time from the
        # device counters.  With the validity gate an invalid plan takes its episode out of lockstep, which the host can only
        # learn by reading the device back; `device_time` (set by capture_episode for a gated episode) runs the gate on
        # per-episode times from the first plan on instead: nothing synchronises, the step is a fixed sequence of launches
        self.device_time = False
        self._lockstep = 0
        self._host_plans = 0
        self._const_flags = None    # (all-True, all-False) [B], shared by every fused step's result
        self._phase_bounds = None   # [2, n_phase] bounds of the learned tau / delay, on the device
        self._plans_since_reset = 0
        self._start32 = None        # fp32 image of the plant state at reset (boundary condition of the first plan)
        # partial resets (reset(mask=...), reset_done(), autoreset()): episodes no longer share a clock or a first plan.  `_partial`
        # holds from the first such reset to the next reset of everybody, `partial_resets` (enable_partial_resets) from the start
        self.partial_resets = False
        self._partial = False
        self._cond_buf = None       # partial_resets + condition_on_desired: the condition lives in ONE pair of buffers (capturable)

    @classmethod
    def from_id(cls, id: str, num_envs: int, **kwargs) -> "BatchedBlackBox":
        """the BatchedBlackBox of a registered MP id (``fancy_ProMP/HoleReacher-v0`` ...), every constant taken from the registry and
        the env: ``fancy_gym_amd.make_batched`` (batched_make.py), same arguments"""
        from .batched_make import make_batched
        return make_batched(id, num_envs, **kwargs)

    # ---- episode control ---------------------------------------------------------------------------------------------
    def check_range(self):
        """
        ProDMP with a per-episode phase (learned tau / delay, drifted init_time): a plan whose scaled time leaves the
        pre-computed table range raises RuntimeError in mp_pytorch and in the single-episode BlackBoxWrapper; the batched
        kernels can only raise a device flag (and clamp the index).  This synchronises and raises that RuntimeError if any
        plan since the last check left the range.  ``reset`` calls it for the episodes just finished (skipped while a
        hipGraph is being captured -- call it yourself after a replay).
        """
        self.engine.check_range()

    def _range_can_overflow(self) -> bool:
        cfg = self.engine.config
        return self.engine.mp_type == "prodmp" and bool(cfg.learn_tau or cfg.learn_delay or self._lockstep is None)

    def _seed_args(self, seed, sample: bool, explicit: bool) -> dict:
        """the seeding of a device-drawn reset: dict(seed_base=...) / dict(seeds=...) / {} (continue), validated"""
        if explicit:
            raise ValueError("reset(seed=...) / reset(sample=True) draw init_pos / goal / hole on the device: do not pass them")
        if self.reward not in ("simple_reacher", "hole_reacher"):
            raise ValueError("reset(seed=...) / reset(sample=True) draw a reacher's episodes: they need reward='simple_reacher' or "
                             "'hole_reacher'")
        if sample:
            if seed is not None:
                raise ValueError("reset: seed=... reseeds, sample=True continues the streams -- not both")
            if self._rng is None:
                raise ValueError("reset(sample=True) continues the streams of a seeded reset: call reset(seed=...) first")
            return {}
        if isinstance(seed, (bool, np.bool_)):
            raise ValueError(f"seed must be an int or a sequence of {self.B} ints, got {seed!r}")
        if isinstance(seed, (int, np.integer)):
            seed = int(seed)
            if seed < 0 or seed + self.B - 1 >= 2 ** 64:
                raise ValueError(f"seeds seed + b must lie in [0, 2^64), got seed={seed} for {self.B} episodes")
            return dict(seed_base=seed)
        seeds = [int(s) for s in seed]
        if len(seeds) != self.B:
            raise ValueError(f"reset(seed=...) takes an int or {self.B} seeds, got {len(seeds)}")
        if any(s < 0 or s >= 2 ** 64 for s in seeds):
            raise ValueError("seeds must lie in [0, 2^64)")
        host = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64))
        return dict(seeds=host.to(self.device, non_blocking=False))

    def reset(self, init_pos=None, init_vel=None, goal=None, hole=None, *, seed=None, sample: bool = False, mask=None):
        """start B new episodes from plant state (init_pos, init_vel) [B, D] (default zeros); goal [B, 2] for the
        simple_reacher reward, hole [B, 3] = (x, width, depth) for the hole_reacher reward.

        With a reacher reward the episodes can be drawn on the device instead (one launch, mpk_reacher_reset): ``seed`` = an int
        starts episode b as ``env.reset(seed=seed + b)`` starts the registered env (gymnasium's vector-env rule), a sequence of B
        ints seeds each episode; ``sample=True`` continues every episode's stream as ``env.reset()`` would.  The start pose, goal /
        hole and generators stay on the device (``goal`` / ``hole`` attributes, ``rng_state()``).

        ``mask`` (bool or uint8 [B], device or host; with ``seed`` or ``sample=True``) restricts the drawn reset to the rows it selects
        (one launch, mpk_reacher_autoreset): the others keep plant state, counters, goal / hole, generator, condition and reward state
        bit for bit, and a ``seed`` seeds the selected rows only.  ``reset_done()`` is the form ``mask = done`` that reads nothing back.
        From then on the episodes do not share a clock: every plan takes its episode's ``init_time = traj_steps * dt`` from the device
        counters (ProMP: per-episode-phase kernels; DMP / ProDMP: one shared-phase launch per clock value, ``_trajectory``), and the one-launch steps (mpk_replan_step, mpk_episode_return), which need lockstep under replanning, give way to the
        separate launches -- the same results.  A partial reset synchronises nothing, so it does not run ``check_range()`` for the
        episodes it ends: call it yourself where a ProDMP plan can leave the table range.  Not with a learned tau / delay (the phase an
        episode freezes at its first plan would have to be re-frozen row by row: not built)."""
        self._twin = None           # (replan_gradient: any reset cuts the chain)
        drawn = seed is not None or bool(sample)
        explicit = any(x is not None for x in (init_pos, init_vel, goal, hole))
        if mask is not None and not drawn:
            raise ValueError("reset(mask=...) restricts a reset drawn on the device: pass seed=... or sample=True with it"
                             + (", not init_pos / init_vel / goal / hole" if explicit else ""))
        seeding = self._seed_args(seed, bool(sample), explicit) if drawn else None
        if mask is not None:
            self._masked_reset(seeding, self._mask_arg(mask))
            return self.q, self.qd
        if self._plans_since_reset and self._range_can_overflow() and not torch.cuda.is_current_stream_capturing():
            self.check_range()
        elif self._plans_since_reset:
            # the episodes just finished: whoever read their results has synchronised; a ring kernel that gave up waiting in their LAST
            # plan would otherwise be reported by the next launch only (costs nothing: the fault word lives in host memory)
            self.engine.poll_fault()
        if drawn:
            self._device_draw(seeding)
        elif self.reward == "hole_reacher":
            if hole is None:
                raise ValueError("reward='hole_reacher' needs hole [B, 3] at reset")
            self.hole = torch.as_tensor(hole, dtype=torch.float64, device=self.device).expand(self.B, 3).contiguous()
        elif self.reward is not None:
            if goal is None:
                raise ValueError("reward='simple_reacher' needs goal [B, 2] at reset")
            self.goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).expand(self.B, 2).contiguous()
        # one launch (mpk_episode_reset): integer state, plant state and its fp32 image (the first plan's boundary state)
        def state(x):
            if x is None:
                return None
            x = torch.as_tensor(x, dtype=torch.float64, device=self.device)
            return x.contiguous() if tuple(x.shape) == (self.B, self.D) else x.expand(self.B, self.D).contiguous()
        if self._start32 is None:
            self._start32 = tuple(torch.empty((self.B, self.D), dtype=torch.float32, device=self.device)
                                  for _ in range(2))
        if not drawn:
            self.engine.episode_reset(self.q, self.qd, self.traj_steps, self.plan_steps, self.done, state(init_pos),
                                      state(init_vel), cond=self._start32)
        self.condition_pos = self.condition_vel = None
        self._partial = self.partial_resets
        if self._cond_buf is not None:
            # the first plan's boundary state is the start state: its fp32 image, in the buffers every later step rewrites
            for dst, src in zip(self._cond_buf, self._start32):
                dst.copy_(src)
            self.condition_pos, self.condition_vel = self._cond_buf
        self._frozen_phase = None
        self._lockstep = None if ((self.device_time or self.partial_resets) and self.do_replanning) else 0
        self._host_plans = 0
        self._plans_since_reset = 0
        self._prev_done = None              # the done bytes before the next plan: none is done (mpk_gate_flags takes NULL)
        self._prev_done_known = True
        self.traj_gen.reset()
        return self.q, self.qd

    def _device_draw(self, seeding: dict):
        """the one launch of a device-drawn reset (mpk_reacher_reset): state, start pose and its fp32 image, goal / hole, generators"""
        if self._start32 is None:
            self._start32 = tuple(torch.empty((self.B, self.D), dtype=torch.float32, device=self.device)
                                  for _ in range(2))
        if self._rng is None:
            self._rng = torch.zeros((self.B, 5), dtype=torch.int64, device=self.device)
        if self._task_buf is None:
            self._task_buf = torch.empty((self.B, 2 if self.reward == "simple_reacher" else 3), dtype=torch.float64,
                                         device=self.device)
        self.engine.reacher_reset(self.reward, self.q, self.qd, self.traj_steps, self.plan_steps, self.done, self._rng,
                                  self._task_buf, cond=self._start32, **seeding, **self.env_kwargs)
        if self.reward == "hole_reacher":
            self.hole = self._task_buf
        else:
            self.goal = self._task_buf

    # ---- partial resets ----------------------------------------------------------------------------------------------------
    def enable_partial_resets(self):
        """episodes will be reset row by row (BatchedVectorEnv(partial_resets=True)): from the next ``reset`` on every step is the
        same sequence of launches whatever the episodes do -- per-episode plan times from the device counters, the boundary state of
        a plan read from the plant state (or, with ``condition_on_desired``, from one pair of buffers that steps and resets rewrite
        in place) -- so that a step can be captured with replanning"""
        self._refuse_partial()
        self.partial_resets = True
        if self.condition_on_desired and self._cond_buf is None:
            self._cond_buf = tuple(torch.zeros((self.B, self.D), dtype=torch.float32, device=self.device) for _ in range(2))

    def _refuse_partial(self):
        if self.reward not in ("simple_reacher", "hole_reacher"):
            raise ValueError("partial resets draw a reacher's episodes: they need reward='simple_reacher' or 'hole_reacher'")
        if self._n_phase and not self.learn_sub_trajectories:
            raise ValueError("partial resets with a learned tau / delay are not built: the phase an episode freezes at its first plan "
                             "would have to be re-frozen row by row")
        if self.learn_sub_trajectories:
            raise ValueError("partial resets with learn_sub_trajectories are not built")

    def _mask_arg(self, mask) -> torch.Tensor:
        mask = torch.as_tensor(mask)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool or uint8, got {mask.dtype}")
        if tuple(mask.shape) != (self.B,):
            raise ValueError(f"mask must be [{self.B}], got {tuple(mask.shape)}")
        return mask.to(self.device).contiguous()

    def _autoreset_launch(self, seeding: dict, mask, observe: bool):
        """the one launch of every partial reset (mpk_reacher_autoreset) and the host bookkeeping that goes with it"""
        self._refuse_partial()
        self._twin = None
        if self._rng is None and not seeding:
            raise ValueError("a partial reset continues the streams of a seeded reset: call reset(seed=...) first")
        if self._rng is None:
            self._rng = torch.zeros((self.B, 5), dtype=torch.int64, device=self.device)
        if self._task_buf is None:
            raise ValueError("a partial reset needs episodes drawn on the device: call reset(seed=...) first")
        if self._plans_since_reset:
            self.engine.poll_fault()
        # a reset row's next plan starts from its start state: the kernel writes the fp32 image where that plan reads its condition
        cond = (self.condition_pos, self.condition_vel) if self.condition_pos is not None else self._start32
        obs_kw = dict(col_mask=self._obs_mask, time_div=self._obs_time_div) if observe else {}
        res = self.engine.reacher_autoreset(self.reward, self.q, self.qd, self.traj_steps, self.plan_steps, self.done, self._rng,
                                            self._task_buf, mask=mask, observe=observe, cond=cond, **obs_kw, **seeding,
                                            **self.env_kwargs)
        self._partial = True
        self._lockstep = None
        self._prev_done_known = False       # the snapshot of the last step no longer shows the reset rows
        return res

    def _masked_reset(self, seeding: dict, mask):
        if (self.hole if self.reward == "hole_reacher" else self.goal) is not self._task_buf or self._task_buf is None:
            raise ValueError("reset(mask=...) / reset_done() continue episodes that were drawn on the device: call reset(seed=...) first")
        self._autoreset_launch(seeding, mask, observe=False)

    def reset_done(self):
        """``reset(sample=True, mask=done)`` without reading ``done`` back: every finished episode starts anew from its own stream,
        the others run on (one launch)"""
        self._seed_args(None, True, False)
        self._masked_reset({}, None)
        return self.q, self.qd

    def autoreset(self):
        """what a vector step does after ``step``, in one launch (``observations=True``): (final_obs, obs, reset_mask) -- the
        observation of the state the step left, ``reset_done()``, and the observation after it (the new episode's first one for the
        rows that were reset, ``final_obs`` for the others); reset_mask bool [B]"""
        if not self.observations:
            raise ValueError("autoreset() needs BatchedBlackBox(..., observations=True)")
        self._seed_args(None, True, False)
        if (self.hole if self.reward == "hole_reacher" else self.goal) is not self._task_buf or self._task_buf is None:
            raise ValueError("autoreset() continues episodes that were drawn on the device: call reset(seed=...) first")
        final, obs, reset_mask = self._autoreset_launch({}, None, observe=True)
        return final, obs, reset_mask.view(torch.bool)

    def _plan_condition(self):
        """(cond_pos, cond_vel) float32 [B, D] of the next plan: the stored desired state, else the plant state -- right after a reset
        of everybody its fp32 image, which the reset launch wrote (no cast launches)"""
        if self.condition_pos is not None:
            return self.condition_pos, self.condition_vel
        if self._start32 is not None and self._plans_since_reset == 1 and not self._partial:
            return self._start32
        return self.q.float(), self.qd.float()

    def _store_condition(self, cond_pos, cond_vel):
        if self._cond_buf is None:
            self.condition_pos, self.condition_vel = cond_pos, cond_vel
            return
        self._cond_buf[0].copy_(cond_pos)
        self._cond_buf[1].copy_(cond_vel)
        self.condition_pos, self.condition_vel = self._cond_buf

    def _plan_time(self):
        """init_time of the next plan: 0 without replanning, the shared clock while the episodes move in lockstep, else per episode"""
        if not self.do_replanning:
            return 0.0
        if self._lockstep is None:
            return (self.traj_steps.double() * self.dt).float()
        return float(self._lockstep * self.dt)

    def _on_clock_grid(self) -> bool:
        """every live episode's step counter is a multiple of ``every``: a plan ends at the next multiple, at the step limit or at a
        collision, and the last two end the episode (whose reset starts it at 0).  Not with a plan cap, the validity gate or plans
        shorter than the schedule's period -- their segments can end anywhere"""
        return (self.do_replanning and not math.isfinite(self.max_planning_times) and self.pos_limits is None
                and self.every <= self.T and not self.learn_sub_trajectories)

    def _trajectory(self, params, cond_pos, cond_vel):
        """the plan (pos, vel) [B, T, D].  In lockstep one launch on the shared clock.  Out of lockstep ProMP takes the per-episode
        init_time directly: its per-episode-phase kernels give the bits of the shared-phase ones.  DMP's and ProDMP's do not (serial
        recurrence instead of the response rows; regrouped boundary terms: ~1e-6 of the scale apart), and a single-episode wrapper's
        plans are shared-phase plans, so where the live counters lie on the clock grid {0, every, 2 every, ...} the batch is planned
        once per clock value with the shared-phase kernels and every episode keeps the rows of its own clock -- horizon / every
        launches and in-place selects, nothing read back, the same bits as B single-episode wrappers.  (Rows that are done and were
        not reset execute nothing; off the grid they keep the plan of clock 0.)"""
        t = self._plan_time()
        pg = getattr(self, "phase_gradient", None)
        if not isinstance(t, torch.Tensor) or self.engine.mp_type == "promp" or not self._on_clock_grid():
            return self.engine.trajectory(params, cond_pos, cond_vel, t, phase_gradient=pg)
        pos, vel = self.engine.trajectory(params, cond_pos, cond_vel, 0.0, phase_gradient=pg)
        for clock in range(self.every, self.horizon, self.every):
            p, v = self.engine.trajectory(params, cond_pos, cond_vel, float(clock * self.dt), phase_gradient=pg)
            own = (self.traj_steps == clock).view(self.B, 1, 1)
            if pos.requires_grad:                     # a differentiable plan: autograd takes no out=
                pos, vel = torch.where(own, p, pos), torch.where(own, v, vel)
                continue
            torch.where(own, p, pos, out=pos)
            torch.where(own, v, vel, out=vel)
        return pos, vel

    def rng_state(self, episodes=None) -> list:
        """numpy's ``bit_generator.state`` of the chosen episodes' generators after the last device-drawn reset (synchronises)"""
        if self._rng is None:
            raise ValueError("no device-drawn reset yet: call reset(seed=...)")
        from .engine import nprng_state
        return nprng_state(self._rng, episodes)

    def observe(self) -> torch.Tensor:
        """the current observation [B, n_obs] float32 on the device (``observations=True``), one launch: after ``reset`` the reset
        observation, after a step that step's ``obs`` (BlackBoxWrapper.observation of the env's _get_obs(), black_box_wrapper.py:89-94)"""
        if not self.observations:
            raise ValueError("observe() needs BatchedBlackBox(..., observations=True)")
        task = self.hole if self.reward == "hole_reacher" else self.goal
        if task is None:
            raise ValueError("observe(): no episode yet -- call reset first")
        return self.engine.reacher_observation(self.reward, self.q, self.qd, task, self.traj_steps, col_mask=self._obs_mask,
                                               time_div=self._obs_time_div)

    def _add_observations(self, out: Dict[str, torch.Tensor], start) -> Dict[str, torch.Tensor]:
        """``obs`` and, given the plan-start state, ``step_observations`` (the replay of the executed steps) of a finished step"""
        if start is not None and "des_pos" in out:
            out["step_observations"] = self._add_step_observations(out, start)
        out["obs"] = self.observe()
        return out

    def _add_step_observations(self, out, start) -> torch.Tensor:
        seg = out["trajectory_length"]
        task = self.hole if self.reward == "hole_reacher" else self.goal
        return self.engine.reacher_step_observations(
            self.reward, self.spec, out["des_pos"], out["des_vel"], start[0], start[1], task, seg, self.traj_steps - seg,
            time_div=self._obs_time_div)

    @property
    def current_pos(self) -> torch.Tensor:
        return self.q

    @property
    def current_vel(self) -> torch.Tensor:
        return self.qd

    def params_bounds(self) -> np.ndarray:
        return self.engine.params_bounds()

    # ---- plan ----------------------------------------------------------------------------------------------------------
    def _plan_params(self, params) -> torch.Tensor:
        """[B, P] float32 on the device, with the phase parameters the episode froze at its first plan"""
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.shape != (self.B, self.engine.num_params):
            raise ValueError(f"params must be [{self.B}, {self.engine.num_params}], got {tuple(params.shape)}")
        if self._n_phase and self.learn_sub_trajectories:
            # every sub-trajectory sets tau / delay anew (the reference resets the generator: black_box_wrapper.py:99-102);
            # the kernels clip them to their bounds
            return params.contiguous()
        if self._n_phase:
            # tau / delay are frozen by the first plan of an episode (mp_pytorch 'finalize'; pinned by
            # test/test_replanning_sequencing.py:231-335): later plans reuse them
            if self._frozen_phase is None:
                if self._phase_bounds is None:
                    self._phase_bounds = torch.as_tensor(self.engine.params_bounds()[:, :self._n_phase],
                                                         device=self.device)
                lo = self._phase_bounds
                self._frozen_phase = torch.minimum(torch.maximum(params[:, :self._n_phase], lo[0]), lo[1]).to(torch.float32)
            # (one launch -- a clone and a slice assignment were two; the plan's own columns follow the frozen ones)
            params = torch.cat((self._frozen_phase, params[:, self._n_phase:]), dim=1)
        return params

    def get_trajectory(self, params) -> Dict[str, torch.Tensor]:
        self._twin = None           # (replan_gradient: a plan asked for on its own cuts the chain)
        return self._get_trajectory(params)

    def fit_trajectory(self, pos, phase_params=None, reg: float = 1e-9) -> torch.Tensor:
        """params [B, P] whose plan reproduces the demonstrated positions ``pos`` [B, T, D] best (``TrajectoryEngine.fit_trajectory``:
        regularised least squares, one launch) from the init_time / init_pos / init_vel ``get_trajectory`` would use now -- so the
        result can be handed straight to ``step`` / ``get_trajectory``"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.fit_trajectory(pos, cond_pos, cond_vel, self._plan_time(), reg=reg, phase_params=phase_params)

    def condition(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, *, obs_vel=None, obs_vel_std=None, out=None):
        """``(params, params_L)`` of the Gaussian ``N(params, L L^T)`` conditioned on observed points of the plan
        (``TrajectoryEngine.condition``: the ProMP operation, one launch) from the init_time / init_pos / init_vel ``get_trajectory``
        would use now -- so the posterior mean can be handed straight to ``step`` / ``get_trajectory`` and the pair to
        ``TrajectoryEngine.sample_trajectories``"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.condition(params, params_L, obs_steps, obs_pos, obs_std, cond_pos, cond_vel, self._plan_time(),
                                     obs_vel=obs_vel, obs_vel_std=obs_vel_std, out=out)

    def trajectory_log_prob(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, *, obs_vel=None, obs_vel_std=None):
        """the log-likelihood [B] float64 of observed points of the plan under the Gaussian ``N(params, L L^T)``
        (``TrajectoryEngine.trajectory_log_prob``, one launch; differentiable w.r.t. ``params`` and ``params_L``) from the init_time /
        init_pos / init_vel ``get_trajectory`` would use now, as ``condition`` takes them"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.trajectory_log_prob(params, params_L, obs_steps, obs_pos, obs_std, cond_pos.detach(), cond_vel.detach(),
                                               self._plan_time(), obs_vel=obs_vel, obs_vel_std=obs_vel_std)

    def condition_given_timing(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, *, obs_vel=None, obs_vel_std=None, out=None):
        """``condition`` for a learned tau / delay (``TrajectoryEngine.condition_given_timing``, one launch): every episode at the tau /
        delay in front of its ``params`` row, which come back as given; the Gaussian over the non-phase parameters"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.condition_given_timing(params, params_L, obs_steps, obs_pos, obs_std, cond_pos.detach(), cond_vel.detach(),
                                                  self._plan_time(), obs_vel=obs_vel, obs_vel_std=obs_vel_std, out=out)

    def trajectory_log_prob_given_timing(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, *, obs_vel=None,
                                         obs_vel_std=None):
        """``trajectory_log_prob`` for a learned tau / delay (``TrajectoryEngine.trajectory_log_prob_given_timing``, one launch;
        differentiable w.r.t. ``params`` and ``params_L``, exact zeros in the phase columns): every episode at the tau / delay in
        front of its ``params`` row"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.trajectory_log_prob_given_timing(params, params_L, obs_steps, obs_pos, obs_std, cond_pos.detach(),
                                                            cond_vel.detach(), self._plan_time(), obs_vel=obs_vel,
                                                            obs_vel_std=obs_vel_std)

    def demonstration_log_prob(self, params, params_L, pos, obs_std):
        """the log-likelihood [B] float64 of whole demonstrations ``pos`` [B, T, D] of the plan under the Gaussian ``N(params, L L^T)``
        (``TrajectoryEngine.demonstration_log_prob``, one launch; differentiable w.r.t. ``params`` and ``params_L``) from the
        init_time / init_pos / init_vel ``get_trajectory`` would use now, as ``trajectory_log_prob`` takes them"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.demonstration_log_prob(params, params_L, pos, obs_std, cond_pos.detach(), cond_vel.detach(), self._plan_time())

    def demonstration_log_prob_given_timing(self, params, params_L, pos, obs_std):
        """``demonstration_log_prob`` for a learned tau / delay (``TrajectoryEngine.demonstration_log_prob_given_timing``, one launch):
        every episode at the tau / delay in front of its ``params`` row, the Gaussian over the non-phase parameters"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.demonstration_log_prob_given_timing(params, params_L, pos, obs_std, cond_pos.detach(), cond_vel.detach(),
                                                               self._plan_time())

    def condition_on_demonstration(self, params, params_L, pos, obs_std, *, out=None):
        """``(params, params_L)`` of the Gaussian ``N(params, L L^T)`` conditioned on whole demonstrations ``pos`` [B, T, D] of the plan
        (``TrajectoryEngine.condition_on_demonstration``, one launch; ``obs_std = inf`` removes an entry, so a prefix is the rest at
        ``inf``) from the init_time / init_pos / init_vel ``get_trajectory`` would use now, as ``condition`` takes them"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.condition_on_demonstration(params, params_L, pos, obs_std, cond_pos.detach(), cond_vel.detach(),
                                                      self._plan_time(), out=out)

    def condition_on_demonstration_given_timing(self, params, params_L, pos, obs_std, *, out=None):
        """``condition_on_demonstration`` for a learned tau / delay (``TrajectoryEngine.condition_on_demonstration_given_timing``, one
        launch): every episode at the tau / delay in front of its ``params`` row, which come back as given"""
        cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
        cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        return self.engine.condition_on_demonstration_given_timing(params, params_L, pos, obs_std, cond_pos.detach(), cond_vel.detach(),
                                                                   self._plan_time(), out=out)

    def _carry_start(self):
        """replan_gradient="episode": (init_pos, init_vel, q_in, qd_in) of the next plan -- what the twins of the plan before give (the
        same bits as ``_plan_condition`` and ``q``, ``qd``), or right after a cut the constants themselves"""
        tw = self._twin
        if tw is None:
            return (*self._plan_condition(), self.q, self.qd)
        if self.condition_on_desired and tw.get("cond_pos") is not None:
            return tw["cond_pos"], tw["cond_vel"], tw["q"], tw["qd"]
        if self.condition_pos is not None:
            return self.condition_pos, self.condition_vel, tw["q"], tw["qd"]
        return tw["q"].float(), tw["qd"].float(), tw["q"], tw["qd"]

    def _carry_end(self, out, twins):
        self._twin = twins
        out.update(end_pos=twins["q"], end_vel=twins["qd"])
        return out

    def _get_trajectory(self, params, cond=None) -> Dict[str, torch.Tensor]:
        params = self._plan_params(params)
        if cond is not None:
            cond_pos, cond_vel = cond
        else:
            cond_pos = self.condition_pos if self.condition_pos is not None else self.q.float()
            cond_vel = self.condition_vel if self.condition_vel is not None else self.qd.float()
        pos, vel = self._trajectory(params, cond_pos, cond_vel)
        if self.learn_sub_trajectories and self.engine.mp_type == "promp":
            # ProMP's velocity is the forward difference of its positions with the LAST row repeating the one before
            # (mp_pytorch; make_env_helpers.py:119-122): the last row of a sub-trajectory of T_b steps is row T_b - 2, not the
            # difference towards a step T_b the sub-trajectory does not have
            n = self._plan_length(params).to(torch.int64)
            rows = torch.arange(self.B, device=self.device)
            vel[rows, n - 1] = vel[rows, (n - 2).clamp(min=0)]
        return {"params": params, "des_pos": pos, "des_vel": vel}

    def _plan_length(self, params: torch.Tensor) -> torch.Tensor:
        """learn_sub_trajectories: round(clip(tau_b) / dt) steps (np.round and torch.round: half to even), int32 [B]"""
        tau = params[:, 0].clamp(float(self.tau_bound[0]), float(self.tau_bound[1]))     # what the kernels use (fp32 clip)
        return torch.round(tau.double() / self.dt).to(torch.int32).clamp(1, self.T)

    # ---- plan + execute ----------------------------------------------------------------------------------------------
    def _host_segment(self) -> int:
        """host mirror of the integer rule for episodes that move in lockstep (no device read-back)"""
        cur = self._lockstep
        if cur >= self.horizon:
            return 0
        self._host_plans += 1
        g_break = self.horizon
        if self._host_plans < self.max_planning_times:
            g_break = min((cur // self.every + 1) * self.every, self.horizon)
        return max(1, min(g_break - cur, self.T))

    def _can_fuse(self) -> bool:
        """plan + execute through mpk_replan_step(_gated) (one launch for promp / prodmp with a shared OR a learned phase and for
        dmp on its response route, the separate kernels otherwise): needs the device plant, no device reward, and episodes that
        still move in lockstep (one init_time for all).  Round 6: the validity gate runs inside the same launch."""
        return (self.spec is not None and self.plant == "double_integrator"
                and self.reward is None and not self.learn_sub_trajectories
                and (not self.do_replanning or self._lockstep is not None))

    def _gate(self, raw_params):
        """the validity gate of this wrapper as the engine takes it (mpk.h: mpk_validity_gate); None without pos_limits"""
        if self.pos_limits is None:
            return None
        return dict(pos_low=self.pos_limits[0], pos_high=self.pos_limits[1], check_tau_delay=self.check_tau_delay,
                    tau_bound=self.tau_bound, delay_bound=self.delay_bound,
                    raw_params=torch.as_tensor(raw_params, dtype=torch.float32, device=self.device) if self.check_tau_delay else None)

    def _was_done(self) -> Optional[torch.Tensor]:
        """the done bytes before this plan WITHOUT a launch: the snapshot the step before returned (the one-launch steps write it), None
        right after a reset (none is done); a copy only after a step of the separate-launch path"""
        if getattr(self, "_prev_done_known", False):
            return self._prev_done
        return self.done.clone()

    def _step_fused(self, params) -> Dict[str, torch.Tensor]:
        """plan + execute as ONE device operation (mpk_replan_step: integer state, trajectory + rollout, condition gather
        in a single launch where the fused closed-loop kernel applies)"""
        gate = self._gate(params)           # (the RAW action: the reference checks tau / delay before clipping, table_tennis_env.py:305-306)
        was_done = self._was_done() if gate is not None else None
        params = self._plan_params(params)
        cond_pos, cond_vel = self._plan_condition()
        init_time = float(self._lockstep * self.dt) if self.do_replanning else 0.0
        mpt = self.max_planning_times if math.isfinite(self.max_planning_times) else 2 ** 31 - 1
        r = self.engine.replan_step(params, cond_pos, cond_vel, self.spec, self.q, self.qd, self.traj_steps,
                                    self.plan_steps, self.done, self.every, int(mpt), self.horizon,
                                    init_time=init_time, condition=self.condition_on_desired, gate=gate)
        seg = r["seg_len"]
        if self.condition_on_desired:
            self._store_condition(r["cond_pos"], r["cond_vel"])
        if self.do_replanning:
            # the host mirrors the integer rule -- with the gate too: an invalid plan FINISHES its episode, so every episode
            # that is still live has executed exactly the segments the rule gives (nothing is read back from the device)
            self._lockstep += self._host_segment()
        done = r["done"].view(torch.bool)               # 0 / 1 bytes: a view, not a launch
        self._prev_done, self._prev_done_known = r["done"], True
        if gate is not None:
            valid = r["valid"].view(torch.bool)
            # invalid plans terminate their episode without executing a step (black_box_wrapper.py:169-172); both flags in one launch
            terminated, truncated = self.engine.gate_flags(r["valid"], was_done, r["done"])
            return dict(params=params, des_pos=r["pos"], des_vel=r["vel"], step_actions=r["actions"], valid=valid,
                        invalid_penalty=r["penalty"], trajectory_length=seg, done=done, terminated=terminated,
                        truncated=truncated, current_pos=self.q, current_vel=self.qd)
        if self._const_flags is None:
            self._const_flags = (torch.ones(self.B, dtype=torch.bool, device=self.device),
                                 torch.zeros(self.B, dtype=torch.bool, device=self.device))
        valid, never = self._const_flags
        # nothing can invalidate a plan on this path: terminated stays False, truncated is `done`
        return dict(params=params, des_pos=r["pos"], des_vel=r["vel"], step_actions=r["actions"], valid=valid,
                    trajectory_length=seg, done=done, terminated=never, truncated=done, current_pos=self.q,
                    current_vel=self.qd)

    def _can_episode_return(self) -> bool:
        return (self.verbose < 2 and self._lean_ok and self.spec is not None and self.plant == "double_integrator"
                and not self.learn_sub_trajectories and (self._n_phase == 0 or self.reward is None)
                and (not self.do_replanning or self._lockstep is not None))

    def _step_lean(self, params, differentiable: bool = False, carry: bool = False) -> Optional[Dict[str, torch.Tensor]]:
        """the verbose < 2 step as ONE launch without per-step outputs (mpk_episode_return); None = not available here.
        ``differentiable``: ``rewards`` carries the graph of ONE mpk_episode_return_vjp launch back to ``params``"""
        gate = self._gate(params)
        was_done = self._was_done() if gate is not None else None
        params = self._plan_params(params)
        if carry:
            cond_pos, cond_vel, q_in, qd_in = self._carry_start()
        else:
            cond_pos, cond_vel = self._plan_condition()
        kw = dict(carry=(q_in, qd_in)) if carry else {}
        init_time = float(self._lockstep * self.dt) if self.do_replanning else 0.0
        mpt = self.max_planning_times if math.isfinite(self.max_planning_times) else 2 ** 31 - 1
        try:
            r = self.engine.episode_return(params, cond_pos, cond_vel, self.spec, self.q, self.qd,
                                           replan=(self.traj_steps, self.plan_steps, self.done, self.every, int(mpt), self.horizon),
                                           reward=self.reward, goal=self.goal, steps_before_reward=self.steps_before_reward,
                                           aggregation=self.reward_aggregation, init_time=init_time,
                                           condition=self.condition_on_desired, gate=gate, differentiable=differentiable, **kw)
        except NotImplementedError:
            # (refused before anything ran.  The plain step never gets another try; a refusal of the gradient says nothing about it.)
            if not differentiable:
                self._lean_ok = False
            return None
        if self.condition_on_desired:
            self._store_condition(r["cond_pos"], r["cond_vel"])
        if self.do_replanning:
            self._lockstep += self._host_segment()
        done = r["done"].view(torch.bool)
        self._prev_done, self._prev_done_known = r["done"], True
        if self._const_flags is None:
            self._const_flags = (torch.ones(self.B, dtype=torch.bool, device=self.device),
                                 torch.zeros(self.B, dtype=torch.bool, device=self.device))
        valid, never = self._const_flags
        out = dict(params=params, valid=valid, trajectory_length=r["seg_len"], done=done, terminated=never, truncated=done,
                   current_pos=self.q, current_vel=self.qd)
        if gate is not None:
            valid = r["valid"].view(torch.bool)
            terminated, truncated = self.engine.gate_flags(r["valid"], was_done, r["done"])
            out.update(valid=valid, invalid_penalty=r["penalty"], terminated=terminated, truncated=truncated)
        if self.reward is not None:
            out["rewards"] = r["ret"]
        return self._carry_end(out, r["carry"]) if carry else out

    def _finish(self, out, seg, valid, was_done, cond=None) -> Dict[str, torch.Tensor]:
        pos, vel = out["des_pos"], out["des_vel"]
        out.update(valid=valid, trajectory_length=seg, done=self.done.bool(), terminated=~valid & ~was_done,
                   truncated=self.done.bool() & valid)
        if self.condition_on_desired and not self.learn_sub_trajectories:
            # (black_box_wrapper.py:197-203 stores the desired state only inside the break branch -- terminated, truncated, or the
            # replanning schedule.  With sub-trajectories the schedule is never true: a plan that ends before the episode does leaves
            # condition_pos None, and the next one starts from env.current_pos / current_vel -- self.q / self.qd here.)
            # (``cond``: the carrying rollout of replan_gradient="episode" has gathered it already -- the same launch on the same plan)
            self._store_condition(*(cond if cond is not None else self.engine.condition_gather(pos, vel, seg)))
        if self.do_replanning and self._lockstep is not None:
            if self.pos_limits is None:
                # no validity gate: every episode follows the same integer sequence, which the host can mirror without
                # reading the device state back (k_replan_advance's rule, black_box_wrapper.py:174,197,206)
                self._lockstep += self._host_segment()
            else:
                live = ~self.done.bool() | ~was_done
                s = seg[live]
                if s.numel() and bool((s == s[0]).all()) and bool(valid.all()):
                    self._lockstep += int(s[0])
                else:
                    self._lockstep = None      # episodes drifted apart: per-episode init_time from now on
        out.update(current_pos=self.q, current_vel=self.qd)
        return out

    _PER_STEP = ("des_pos", "des_vel", "step_actions", "step_rewards")

    def step(self, params, fuse: bool = True, differentiable: bool = False) -> Dict[str, torch.Tensor]:
        """one plan of every episode.  ``differentiable=True`` (reward "simple_reacher"; off by default, and then nothing changes on any
        path): ``out["rewards"]`` carries the graph back to ``params``.  At ``verbose < 2`` with ``fuse=True`` the step is the one
        mpk_episode_return launch of the plain step -- the same values, state and integer outputs -- and its backward ONE
        mpk_episode_return_vjp launch.  With ``verbose >= 2`` or ``fuse=False`` (and where the one-launch gradient does not apply) the step
        takes the separate launches under autograd -- differentiable ``get_trajectory`` -> differentiable ``reacher_rollout`` ->
        ``reward_aggregate`` -- so that ``step_rewards`` carry the graph too: the same values, state and integer outputs as
        ``step(params, fuse=False)``, and a backward of two launches, mpk_reacher_rollout_vjp and mpk_trajectory_vjp.  With replanning the gradient is that of THIS step's reward w.r.t. THIS
        step's parameters: the plant state and the condition the plan starts from are constants of the graph, nothing flows into
        earlier steps -- unless the box was built with ``replan_gradient="episode"`` (the constructor's argument), which carries the
        graph across plan boundaries and adds ``end_pos`` / ``end_vel`` to the result.
        Reward "hole_reacher" takes part only with ``collision_gradient="frozen"`` (the constructor's argument): the
        plain step's two launches under autograd, the same values, state and integer outputs, and a backward of two launches,
        mpk_hole_reacher_rollout_vjp at the forward's own ``trajectory_length`` / ``is_collided`` and mpk_trajectory_vjp; at
        ``verbose < 2`` nothing per step is stored.  NotImplementedError: another reward, HoleReacher without that option or with rew_fct
        "unbounded", ``pos_limits``, and what ``trajectory`` refuses under autograd (a learned tau / delay, per-episode plan times after
        partial resets)."""
        if differentiable:
            self._refuse_differentiable()
        out = self._step(params, fuse, differentiable)
        # (the plan-start state for the replay of step_observations: a copy taken by _step before the plan)
        return self._add_observations(out, self._obs_start) if self.observations else out

    def _refuse_differentiable(self):
        """what neither gradient path takes -- the one-launch backward of the ``verbose < 2`` step (mpk_episode_return_vjp) nor the two
        launches of the separate path: both differentiate SimpleReacher's reward through a plan that is linear in its parameters --
        nor HoleReacher's two launches, which differentiate only where ``collision_gradient`` says how"""
        frozen = self.reward == "hole_reacher" and getattr(self, "collision_gradient", None) == "frozen"
        if self.reward != "simple_reacher" and not frozen:
            raise NotImplementedError(f"step(differentiable=True) is built for reward='simple_reacher' (the torque double integrator), "
                                      f"not for reward={self.reward!r}: HoleReacher's return is discontinuous at collisions "
                                      f"(collision_gradient='frozen' gives its gradient with the episode's end and verdict held)")
        if frozen and getattr(self, "rew_fct", "simple") == "unbounded":
            raise NotImplementedError("step(differentiable=True) with collision_gradient='frozen' takes rew_fct 'simple' and 'vel_acc': "
                                      "'unbounded' pays on the end effector stored at step 180, which may belong to an earlier plan")
        if self.pos_limits is not None:
            raise NotImplementedError("step(differentiable=True) does not take pos_limits: the validity gate ends episodes on a "
                                      "threshold of the plan, which has no derivative")
        if self._n_phase:
            raise NotImplementedError("step(differentiable=True) needs a shared phase: with a learned tau / delay the trajectory is "
                                      "not linear in those two parameters, and they are clipped to their bounds")
        if self.do_replanning and self._lockstep is None:
            raise NotImplementedError("step(differentiable=True) needs one plan time for the batch: after partial resets (or with "
                                      "device_time) every episode has its own init_time, which trajectory() refuses under autograd")

    def _step(self, params, fuse: bool, differentiable: bool = False) -> Dict[str, torch.Tensor]:
        self._plans_since_reset += 1
        self._obs_start = (self.q.clone(), self.qd.clone()) if self.observations and self.verbose >= 2 else None
        # replan_gradient="episode": this plan starts from the twins of the one before and leaves its own; any other step cuts the chain
        carry = differentiable and self.replan_gradient == "episode" and self.do_replanning
        if not carry:
            self._twin = None
        if differentiable and self.reward == "hole_reacher":
            # collision_gradient="frozen": the plan and the rollout under autograd, two launches backward (mpk_hole_reacher_rollout_vjp,
            # mpk_trajectory_vjp); at verbose < 2 nothing per step is stored, the return's gradient enters the kernel through agg
            with torch.enable_grad():
                return self._step_hole(params, differentiable=True, carry=carry)
        if differentiable:
            with torch.enable_grad():
                # the default verbosity: mpk_episode_return forward, one mpk_episode_return_vjp launch backward; what that refuses,
                # verbose >= 2 and fuse=False take the separate launches (two backward)
                out = self._step_lean(params, differentiable=True, carry=carry) if fuse and self._can_episode_return() else None
                if out is not None:
                    return out
                out = self._step_full(params, fuse=False, differentiable=True, carry=carry)
            if self.verbose < 2:
                for k in self._PER_STEP:
                    out.pop(k, None)
            return out
        if self.reward == "hole_reacher":
            return self._step_hole(params)
        if fuse and self._can_episode_return():
            out = self._step_lean(params)
            if out is not None:
                return out
        out = self._step_full(params, fuse)
        if self.verbose < 2:        # (the launches of the verbose = 2 path ran: what it keeps per step is simply not returned)
            for k in self._PER_STEP:
                out.pop(k, None)
        return out

    def _step_full(self, params, fuse: bool = True, differentiable: bool = False, carry: bool = False) -> Dict[str, torch.Tensor]:
        if fuse and self._can_fuse():
            return self._step_fused(params)
        start = self._carry_start() if carry else None
        # (right after a cut the plan's condition is chosen as without the option)
        out = self._get_trajectory(params, cond=start[:2] if carry and self._twin is not None else None)
        pos, vel = out["des_pos"], out["des_vel"]
        was_done = self.done.bool()
        self._prev_done_known = False       # (this path changes the done bytes with launches of its own: _was_done copies them next time)
        valid = torch.ones(self.B, dtype=torch.bool, device=self.device)
        if self.pos_limits is not None:
            # `params` as the caller passed them: the reference checks the raw action, not the clipped one
            raw = torch.as_tensor(params, dtype=torch.float32, device=self.device)
            valid, out["invalid_penalty"] = self.engine.traj_validity(
                pos, self.pos_limits[0], self.pos_limits[1], raw if self.check_tau_delay else None,
                self.tau_bound if self.check_tau_delay else None,
                self.delay_bound if self.check_tau_delay else None, with_penalty=True)
            # invalid plans terminate their episode without executing a step (black_box_wrapper.py:169-172)
            self.done |= (~valid).to(torch.uint8)
        mpt = self.max_planning_times if math.isfinite(self.max_planning_times) else 2 ** 31 - 1
        if self.learn_sub_trajectories:
            seg = self._sub_trajectory_advance(out["params"])
        else:
            seg = self.engine.replan_advance(self.traj_steps, self.plan_steps, self.done, self.every, int(mpt),
                                             self.horizon)
        if self.reward is not None:
            if not differentiable:
                # (a plan that kept its graph -- params.requires_grad_() -- is rolled out as a constant, as before step(differentiable=True)
                # existed: no clone of the state, no grad_fn on the rewards)
                pos, vel = pos.detach(), vel.detach()
            if carry:
                # (the carrying rollout gathers the condition itself, so that it is an output of the plan's one backward launch)
                act, rew, twins = self.engine.reacher_rollout(
                    self.spec, pos, vel, self.q, self.qd, self.goal, n_steps=seg, step0=self.traj_steps - seg,
                    steps_before_reward=self.steps_before_reward, carry=start[2:],
                    condition=self.condition_on_desired and not self.learn_sub_trajectories)
                out.update(step_actions=act, step_rewards=rew, rewards=self._aggregate(rew, seg))
                return self._carry_end(self._finish(out, seg, valid, was_done, cond=twins.pop("cond", None)), twins)
            act, rew = self.engine.reacher_rollout(self.spec, pos, vel, self.q, self.qd, self.goal, n_steps=seg,
                                                   step0=self.traj_steps - seg,
                                                   steps_before_reward=self.steps_before_reward)
            out.update(step_actions=act, step_rewards=rew, rewards=self._aggregate(rew, seg))
        elif self.spec is not None:
            out["step_actions"] = self.engine.pd_rollout(self.spec, pos, vel, self.q, self.qd, n_steps=seg)
        return self._finish(out, seg, valid, was_done)


    def _step_hole(self, params, differentiable: bool = False, carry: bool = False) -> Dict[str, torch.Tensor]:
        """HoleReacher: the plan, then ONE rollout launch that advances the integer state, executes until the plan ends or the
        arm collides, and commits the break (mpk_hole_reacher_rollout); at verbose < 2 it stores nothing per step.  The plan's
        init_time is the shared clock while the episodes move in lockstep, per episode from the device counters after a partial reset"""
        params = self._plan_params(params)
        if carry:
            cond_pos, cond_vel, q_in, qd_in = self._carry_start()
        else:
            cond_pos, cond_vel = self._plan_condition()
        kw = dict(carry=(q_in, qd_in)) if carry else {}
        pos, vel = self._trajectory(params, cond_pos, cond_vel)
        mpt = self.max_planning_times if math.isfinite(self.max_planning_times) else 2 ** 31 - 1
        full = self.verbose >= 2
        r = self.engine.hole_reacher_rollout(
            self.spec, pos, vel, self.q, self.qd, self.hole, steps_before_reward=self.steps_before_reward,
            replan=(self.traj_steps, self.plan_steps, self.done, self.every, int(mpt), self.horizon),
            condition=self.condition_on_desired, want_actions=full, want_rewards=full, aggregation=self.reward_aggregation,
            rew_fct=self.rew_fct, reward_state=self._reward_state, differentiable=differentiable, **kw, **self.hole_task)
        if self.condition_on_desired:
            self._store_condition(r["cond_pos"], r["cond_vel"])
        if self.do_replanning and self._lockstep is not None:
            # a collision finishes its episode: every live episode executed the segment of the integer rule
            self._lockstep += self._host_segment()
        self._prev_done, self._prev_done_known = r["done"], True
        collided = r["collided"].view(torch.bool)
        out = dict(params=params, trajectory_length=r["n_exec"], done=r["done"].view(torch.bool), terminated=collided,
                   truncated=self.traj_steps >= self.horizon, rewards=r["ret"], is_collided=collided,
                   is_success=r["success"].view(torch.bool), current_pos=self.q, current_vel=self.qd)
        if full:
            out.update(des_pos=pos, des_vel=vel, step_actions=r["actions"], step_rewards=r["rewards"])
        return self._carry_end(out, r["carry"]) if carry else out

    def _sub_trajectory_advance(self, params: torch.Tensor) -> torch.Tensor:
        """
        learn_sub_trajectories: the integer part of one step, on the device (a handful of elementwise launches, nothing read
        back).  Episode b plans round(clip(tau_b) / dt) steps (np.round: half to even, as torch.round) and executes them unless
        its step budget ends first (the TimeLimit of the reference's step-based env truncates: test/test_replanning_sequencing.
        py:100-109); finished episodes are left alone.  Returns the executed steps int32 [B].
        """
        plan_len = self._plan_length(params)
        live = self.done == 0
        left = (self.horizon - self.traj_steps).clamp(min=0)
        seg = torch.where(live, torch.minimum(plan_len, left), torch.zeros_like(plan_len))
        self.traj_steps += seg
        self.plan_steps += live.to(torch.int32)
        self.done |= (self.traj_steps >= self.horizon).to(torch.uint8)
        return seg

    def _aggregate(self, rew: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
        """reward_aggregation(rewards[:t + 1]) of black_box_wrapper.py:216 for every episode: sum / mean / last over its
        executed steps (step_rewards are zero behind them); an episode that executed nothing gets 0"""
        # one launch, in the order of additions of the verbose < 2 kernel (mpk_reward_aggregate): the two paths agree bit for bit
        return self.engine.reward_aggregate(rew, seg, self.reward_aggregation)

    # ---- whole episodes as one hipGraph ----------------------------------------------------------------------------------
    def capture_episode(self, n_plans: int, with_goal: bool = False, sample: bool = False) -> "EpisodeGraph":
        """
        Capture ``reset`` + ``n_plans`` calls of ``step`` into one hipGraph.  At B of a few thousand a plan costs ~100 us of
        Python / ctypes / allocator work around ~20 us of kernels; a replay pays one graph launch for the whole
        episode.  Requirement: a device-resident plant (``plant != None``).  With the validity gate the episodes run on
        per-episode times from the device counters (``device_time``: an invalid plan takes its episode out of lockstep, which
        only the device knows), so that nothing synchronises during capture either.

        Write the inputs into the returned object's static buffers (``init_pos``, ``init_vel``, ``params[k]``, ``goal``),
        call ``replay()``, read ``outs[k]`` (the dicts ``step`` returned during capture; their tensors are rewritten by
        every replay).

        ``sample=True`` (a reacher reward, after a seeded ``reset``): the captured reset is ``reset(sample=True)``, so every replay
        draws a new generation of episodes from the streams -- replay k draws what the k-th eager ``reset(sample=True)`` would have
        (the eager warm-up pass restores the generators it advanced).  ``init_pos`` / ``goal`` / ``hole`` are then not inputs.
        """
        if sample:
            self._seed_args(None, True, False)
        if self.spec is None:
            raise ValueError("capture_episode needs a device plant (host environments cannot be captured)")
        if self.pos_limits is not None and not (self.plant == "double_integrator" and self.reward is None
                                                and not self.learn_sub_trajectories):
            self.device_time = True         # (the fused, gated step keeps the host's lockstep mirror: nothing to read back)
        return EpisodeGraph(self, int(n_plans), with_goal, sample)


class EpisodeGraph:
    def __init__(self, bb: BatchedBlackBox, n_plans: int, with_goal: bool, sample: bool = False):
        self.bb = bb
        dev = bb.device
        self.init_pos = torch.zeros((bb.B, bb.D), dtype=torch.float64, device=dev)
        self.init_vel = torch.zeros((bb.B, bb.D), dtype=torch.float64, device=dev)
        self.goal = torch.zeros((bb.B, 2), dtype=torch.float64, device=dev) if (with_goal or bb.reward == "simple_reacher") else None
        self.hole = torch.zeros((bb.B, 3), dtype=torch.float64, device=dev) if bb.reward == "hole_reacher" else None
        self.params = [torch.zeros((bb.B, bb.engine.num_params), dtype=torch.float32, device=dev)
                       for _ in range(n_plans)]
        self.outs = []
        self.reset_obs = None           # observations=True: the captured reset observation [B, n_obs], rewritten by every replay

        if sample:
            self.init_pos = self.init_vel = self.goal = self.hole = None

        def episode():
            if sample:
                bb.reset(sample=True)
            else:
                kw = {"goal": self.goal} if self.goal is not None else {}
                if self.hole is not None:
                    kw["hole"] = self.hole
                bb.reset(self.init_pos, self.init_vel, **kw)
            reset_obs = bb.observe() if bb.observations else None
            return reset_obs, [bb.step(p) for p in self.params]

        # one eager pass on a side stream first (allocator warm-up, lazy initialisation), then the capture; the warm-up's draws are
        # undone, so that the first replay continues the streams where the eager resets left them
        snapshot = bb._rng.clone() if sample else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            episode()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if sample:
            bb._rng.copy_(snapshot)
            torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.reset_obs, self.outs = episode()
        torch.cuda.synchronize(dev)

    def replay(self):
        self.graph.replay()
        return self.outs
