"""
The front door of the device path: ``make_batched(id, num_envs)`` builds the ``BatchedBlackBox`` of a registered movement-primitive id
the way ``_gym.make(id)`` builds its single-episode ``BlackBoxWrapper`` -- every constant comes from the registry, the MP wrapper's
``mp_config`` and the step-based env, none is typed by the caller.

``resolve_batched_config`` is the pure-Python half (no GPU): the merged MP configuration through the path ``bb_env_constructor`` takes
(``resolve_mp_config``, then ``make_bb``'s derived defaults: ``complete_mp_kwargs``), and the plant / reward / reset constants read from a
throw-away instance of the registered env, so that a change of the host env or of the registry shows on the batched side as well.
Only the two reacher families have a device plant (SimpleReacherEnv: torque double integrator; HoleReacherEnv: direct velocity).
"""
from __future__ import annotations

import copy
import inspect
import math
from typing import Any, Dict, Optional

import numpy as np

from . import _gym
from .black_box.factory import get_basis_generator, get_controller, get_phase_generator, get_trajectory_generator
from .envs.classic_control.hole_reacher import HoleReacherEnv
from .envs.classic_control.simple_reacher import SimpleReacherEnv
from .envs.registry import bb_env_constructor, resolve_mp_config
from .utils.make_env_helpers import _verify_time_limit, complete_mp_kwargs, get_env_duration

# the four kwarg groups of the factories, under the names the merged configuration gives them
FACTORY_GROUPS = ("phase_generator_kwargs", "basis_generator_kwargs", "trajectory_generator_kwargs", "controller_kwargs")
# black_box_kwargs BatchedBlackBox takes under the same name (BlackBoxWrapper's constructor, black_box_wrapper.py:56-66) ...
_BLACK_BOX_KEYS = ("verbose", "learn_sub_trajectories", "reward_aggregation", "max_planning_times", "condition_on_desired")
# ... and the schedule: a callable cannot run on the device, ``replanning_every=n`` stands for ``t % n == 0``
_SCHEDULE_KEYS = ("replanning_schedule", "replanning_every")


def _registered(id: str):
    if id not in _gym.registry:
        raise ValueError(f"No registered env with id: {id}")
    return _gym.registry[id]


def _entry_point(spec):
    ep = spec.entry_point
    if isinstance(ep, str):
        import importlib
        mod, attr = ep.split(":")
        ep = getattr(importlib.import_module(mod), attr)
    return ep


def _reacher_task(env) -> Dict[str, Any]:
    """plant, reward and reset constants of a step-based reacher env, read from the instance"""
    if isinstance(env, SimpleReacherEnv):
        target = None if env.fixed_target is None else tuple(float(t) for t in env.fixed_target)
        return dict(plant="double_integrator", reward="simple_reacher", steps_before_reward=int(env.steps_before_reward),
                    env_kwargs=dict(random_start=env.random_start, target=target))
    if isinstance(env, HoleReacherEnv):
        return dict(plant="velocity_direct", reward="hole_reacher", steps_before_reward=int(env.steps_before_reward),
                    rew_fct=env.rew_fct, collision_penalty=float(env.collision_penalty),
                    allow_self_collision=env.allow_self_collision, allow_wall_collision=env.allow_wall_collision,
                    env_kwargs=dict(random_start=env.random_start, hole_width=env.initial_width, hole_x=env.initial_x,
                                    hole_depth=env.initial_depth))
    raise ValueError(f"the base env of this id is a {type(env).__module__}.{type(env).__qualname__}: only the two reacher families "
                     f"(SimpleReacherEnv, HoleReacherEnv) run on the device -- step other envs on the host (_gym.make, VectorBlackBox)")


def resolve_batched_config(id: str, mp_config_override: Optional[dict] = None, **env_kwargs) -> Dict[str, Any]:
    """
    Everything ``BatchedBlackBox`` needs for the registered MP id ``id`` (``fancy_{ProMP,DMP,ProDMP}/...-v0``), derived:

      * ``phase_generator_kwargs`` / ``basis_generator_kwargs`` / ``trajectory_generator_kwargs`` / ``controller_kwargs``: what
        ``make_bb`` hands to the factories -- defaults <- the MP wrapper's ``mp_config`` <- the register-time override <-
        ``mp_config_override`` (registry.py:284-292), completed by ``make_bb``'s rules (action_dim, tau = duration, bounds of a learned
        tau / delay);
      * every other key is a ``BatchedBlackBox`` argument of that name: ``dt``, ``duration`` (``get_env_duration``: the TimeLimit's steps
        times dt, unless ``black_box_kwargs`` gives one), ``max_episode_steps``, ``act_low`` / ``act_high`` (the env's action space),
        ``plant``, ``reward``, ``steps_before_reward``, for HoleReacher ``rew_fct`` / ``collision_penalty`` / ``allow_self_collision`` /
        ``allow_wall_collision``, the reset constants ``env_kwargs``, and the ``black_box_kwargs``;
      * ``n_links``, ``id``, ``base_id``, ``mp_type`` for the record.

    ``**env_kwargs`` go to the step-based env as ``_gym.make(id, **env_kwargs)`` passes them on (``random_start=False``, ``hole_width=0.3``,
    ``rew_fct="vel_acc"`` ...).  A ``replanning_schedule`` callable sees host state and cannot run on the device: give
    ``black_box_kwargs={"replanning_every": n}`` for the schedule ``t % n == 0`` instead.  ValueError for an id without device plant, an
    env kwarg the env does not take, and black-box settings that have no device form -- each names the offender.
    """
    spec = _registered(id)
    reg = dict(spec.kwargs or {})
    if _entry_point(spec) is not bb_env_constructor or "underlying_id" not in reg:
        raise ValueError(f"{id!r} is not a movement-primitive id (register / upgrade make them: fancy_ProMP/..., fancy_DMP/..., "
                         f"fancy_ProDMP/...)")
    base_id, mp_wrapper, mp_type = reg["underlying_id"], reg["mp_wrapper"], reg["mp_type"]
    base = _registered(base_id)
    env_cls = _entry_point(base)
    if inspect.isclass(env_cls):
        taken = inspect.signature(env_cls.__init__).parameters
        if not any(p.kind is p.VAR_KEYWORD for p in taken.values()):
            unknown = sorted(set(env_kwargs) - set(taken))
            if unknown:
                raise ValueError(f"{env_cls.__name__} ({base_id}) takes no {', '.join(repr(k) for k in unknown)}")

    # the throw-away host instance: what bb_env_constructor wraps (registry.py:279-281)
    raw = _gym.make(base_id, **env_kwargs)
    env = mp_wrapper(raw)
    task = _reacher_task(raw.unwrapped)

    config = resolve_mp_config(mp_type, getattr(env, "mp_config", {}), reg.get("_mp_config_override_register", {}),
                               copy.deepcopy(mp_config_override) if mp_config_override else {})
    if config.pop("wrappers", []):
        raise ValueError("'wrappers': additional env wrappers have no device form")
    black_box = config.pop("black_box_kwargs", {})
    groups = {g: config.pop(g, {}) for g in FACTORY_GROUPS}
    _verify_time_limit(groups["trajectory_generator_kwargs"].get("duration"), config.pop("time_limit", None))
    config.pop("fallback_max_steps", None)          # (the registered reachers carry their TimeLimit)
    if config:
        raise ValueError(f"mp config keys without a device form: {sorted(config)}")

    unknown = sorted(set(black_box) - set(_BLACK_BOX_KEYS) - set(_SCHEDULE_KEYS) - {"duration"})
    if unknown:
        raise ValueError(f"black_box_kwargs {unknown} are not BlackBoxWrapper arguments")
    if black_box.get("replanning_schedule") is not None:
        raise ValueError("black_box_kwargs 'replanning_schedule': a schedule callable sees host state per step and cannot run on the "
                         "device; give 'replanning_every': n for the schedule t % n == 0")
    every = black_box.get("replanning_every")
    if every is not None and (isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1):
        raise ValueError(f"black_box_kwargs 'replanning_every' must be a positive int, got {every!r}")
    if black_box.get("learn_sub_trajectories") and every is not None:
        raise ValueError("Cannot used sub-trajectory learning and replanning together.")      # make_env_helpers.py:91-92

    action_space = env.action_space
    complete_mp_kwargs(black_box, groups["trajectory_generator_kwargs"], groups["phase_generator_kwargs"],
                       action_dim=int(np.prod(action_space.shape)), dt=env.dt, env_duration=lambda: get_env_duration(env))

    out: Dict[str, Any] = dict(id=id, base_id=base_id, mp_type=mp_type, n_links=int(raw.unwrapped.n_links), **groups)
    out.update(dt=float(env.dt), duration=float(black_box["duration"]), max_episode_steps=int(env.spec.max_episode_steps),
               act_low=np.asarray(action_space.low, np.float64), act_high=np.asarray(action_space.high, np.float64),
               replanning_every=None if every is None else int(every),
               verbose=black_box.get("verbose", 1), learn_sub_trajectories=bool(black_box.get("learn_sub_trajectories", False)),
               reward_aggregation=black_box.get("reward_aggregation", np.sum),
               max_planning_times=black_box.get("max_planning_times", math.inf),
               condition_on_desired=bool(black_box.get("condition_on_desired", False)), **task)
    return out


def make_batched(id: str, num_envs: int, *, device=None, verbose: Optional[int] = None, observations: bool = True,
                 mp_config_override: Optional[dict] = None, collision_gradient: Optional[str] = None,
                 phase_gradient: Optional[str] = None, replan_gradient: Optional[str] = None, **env_kwargs):
    """
    The ``BatchedBlackBox`` of ``num_envs`` episodes of the registered MP id ``id`` -- the batched ``_gym.make(id, mp_config_override=...,
    **env_kwargs)``: generator and controller from the factories, everything else from ``resolve_batched_config``.  ``verbose`` as
    BlackBoxWrapper's (None: ``black_box_kwargs``' value, else the reference's default 1: ``step`` returns what the wrapper returns and
    stores nothing per step); ``observations`` as ``BatchedBlackBox``'s (on here: an id has an observation); ``collision_gradient`` as
    ``BatchedBlackBox``'s (None or "frozen": what ``step(differentiable=True)`` differentiates on a HoleReacher id; a SimpleReacher id
    accepts and ignores it); ``phase_gradient`` as ``BatchedBlackBox``'s (None or "pathwise": whether ``get_trajectory`` keeps the autograd
    graph through a learned tau / delay or per-episode plan clocks); ``replan_gradient`` as ``BatchedBlackBox``'s (None or "episode":
    whether the gradient of ``step(differentiable=True)`` crosses plan boundaries on a replanning id; an id without replanning accepts
    and ignores it).
    """
    from .batched import BatchedBlackBox
    if collision_gradient not in (None, "frozen"):
        raise ValueError(f"collision_gradient must be None or 'frozen', got {collision_gradient!r}")
    if phase_gradient not in (None, "pathwise"):
        raise ValueError(f"phase_gradient must be None or 'pathwise', got {phase_gradient!r}")
    if replan_gradient not in (None, "episode"):
        raise ValueError(f"replan_gradient must be None or 'episode', got {replan_gradient!r}")
    cfg = resolve_batched_config(id, mp_config_override, **env_kwargs)
    for key in ("id", "base_id", "mp_type", "n_links"):
        cfg.pop(key)
    phase_gen = get_phase_generator(**cfg.pop("phase_generator_kwargs"))
    basis_gen = get_basis_generator(phase_generator=phase_gen, **cfg.pop("basis_generator_kwargs"))
    controller = get_controller(**cfg.pop("controller_kwargs"))
    traj_gen = get_trajectory_generator(basis_generator=basis_gen, **cfg.pop("trajectory_generator_kwargs"))
    if verbose is not None:
        cfg["verbose"] = verbose
    return BatchedBlackBox(traj_gen, controller, int(num_envs), device=device, observations=observations,
                           collision_gradient=collision_gradient, phase_gradient=phase_gradient, replan_gradient=replan_gradient,
                           **cfg)


def make_batched_vec(id: str, num_envs: int, *, partial_resets: bool = False, **kwargs):
    """``make_batched`` behind the gymnasium vector-env contract: a ``BatchedVectorEnv`` (same arguments).  ``partial_resets=True``:
    every episode is reset on its own in the step that ends it (one launch, mpk_reacher_autoreset) instead of all together when the
    last one ends -- what replanning ids (``black_box_kwargs={"replanning_every": n}``) need, and what lets their steps be captured"""
    from .batched_vector import BatchedVectorEnv
    return BatchedVectorEnv(make_batched(id, num_envs, **kwargs), partial_resets=partial_resets)


def resolve_batched_step_config(id: str, **env_kwargs) -> Dict[str, Any]:
    """
    Everything ``BatchedStepEnv`` needs for the registered STEP-BASED reacher id ``id`` (``fancy/SimpleReacher-v0``,
    ``fancy/LongSimpleReacher-v0``, ``fancy/HoleReacher-v0``), derived: ``env`` ("simple_reacher" / "hole_reacher"), ``n_links``, ``dt``,
    ``max_episode_steps`` (the registered TimeLimit), ``act_bound`` (the env's max_torque / max_vel, from its action space),
    ``steps_before_reward``, for HoleReacher ``rew_fct`` / ``collision_penalty`` / ``allow_self_collision`` / ``allow_wall_collision``,
    and the reset constants ``env_kwargs`` -- all read from a throw-away ``_gym.make(id, **env_kwargs)`` instance and the registry.
    ValueError, naming the offender, for a movement-primitive id (``make_batched_vec`` steps those), an id whose env is not one of the
    two reacher families, and an env kwarg the env does not take.
    """
    spec = _registered(id)
    reg = dict(spec.kwargs or {})
    env_cls = _entry_point(spec)
    if env_cls is bb_env_constructor or "underlying_id" in reg:
        raise ValueError(f"{id!r} is a movement-primitive id: a step of it is a whole plan -- use make_batched_vec({id!r}, ...); "
                         f"make_batched_step_vec takes the step-based id ({reg.get('underlying_id', 'fancy/...')!r})")
    if inspect.isclass(env_cls):
        taken = inspect.signature(env_cls.__init__).parameters
        if not any(p.kind is p.VAR_KEYWORD for p in taken.values()):
            unknown = sorted(set(env_kwargs) - set(taken))
            if unknown:
                raise ValueError(f"{env_cls.__name__} ({id}) takes no {', '.join(repr(k) for k in unknown)}")
    raw = _gym.make(id, **env_kwargs)
    env = raw.unwrapped
    try:
        task = _reacher_task(env)
    except ValueError as e:
        raise ValueError(f"{id!r}: {e}") from None
    if raw.spec.max_episode_steps is None:
        raise ValueError(f"{id!r} is registered without max_episode_steps: the device step needs the TimeLimit")
    high = np.asarray(env.action_space.high, np.float64)
    out: Dict[str, Any] = dict(id=id, env=task.pop("reward"), n_links=int(env.n_links), dt=float(env.dt),
                               max_episode_steps=int(raw.spec.max_episode_steps), act_bound=float(high[0]))
    task.pop("plant")
    out.update(task)
    return out


def make_batched_step_vec(id: str, num_envs: int, *, device=None, autoreset: bool = True, **env_kwargs):
    """The ``BatchedStepEnv`` of ``num_envs`` episodes of the registered step-based reacher id ``id`` -- the batched, device-resident
    ``_gym.make(id, **env_kwargs)`` behind the vector-env contract: one launch per environment step (mpk_reacher_env_step), same-step
    autoreset (``autoreset=False``: ended rows stay where they are).  Every constant comes from ``resolve_batched_step_config``."""
    from .batched_step import BatchedStepEnv
    cfg = resolve_batched_step_config(id, **env_kwargs)
    cfg.pop("id")
    return BatchedStepEnv(int(num_envs), device=device, autoreset=autoreset, **cfg)
