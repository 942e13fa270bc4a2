"""
BatchedStepEnv -- the gymnasium vector-env contract over the STEP-BASED reacher ids (``fancy/SimpleReacher-v0``,
``fancy/LongSimpleReacher-v0``, ``fancy/HoleReacher-v0``) with every episode on the device: ``step(actions)`` is one environment step
of every episode and ONE launch (mpk_reacher_env_step: plant in numpy's dtypes for the float32 action, collisions, reward, TimeLimit,
last observation, same-step autoreset from the episode's own numpy-identical generator, next observation).  ``BatchedVectorEnv``
(batched_vector.py) has this role for the movement-primitive ids, where a step is a whole plan; this is the step-based twin PPO / SAC
baselines train on.  Nothing leaves the GPU and nothing is decided on the host, so ``capture()`` turns the step into one graph node.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _gym, _lib
from .batched_vector import _batched_box
from .engine import TrajectoryEngine

_ENVS = {"simple_reacher": dict(random_start=True, target=None),
         "hole_reacher": dict(random_start=True, hole_width=None, hole_x=None, hole_depth=1.0)}


class BatchedStepEnv:
    """
    ``num_envs`` episodes of one step-based reacher env.  ``env`` is "simple_reacher" (torque double integrator, never terminates) or
    "hole_reacher" (direct velocity, terminated = collided); ``env_kwargs`` are the env's reset constants (None = drawn) as
    ``BatchedBlackBox`` takes them.  Actions are float32 [num_envs, n_links] and are NOT clipped -- the reference's step-based envs do
    not clip, only the black-box wrapper does.

    Autoreset mode: **same-step**.  Where ``terminated | truncated`` the episode starts anew in the same launch: ``obs`` holds the new
    episode's first observation, ``info["final_obs"]`` the finished episode's last one, ``info["_final_obs"]`` the rows that were
    reset; both are present in every step.  ``autoreset=False`` leaves ended rows where they are (they keep stepping).
    """

    def __init__(self, num_envs: int, *, env: str, n_links: int, dt: float = 0.01, max_episode_steps: int = 200,
                 steps_before_reward: int = 199, rew_fct: str = "simple", collision_penalty: float = 100.0,
                 allow_self_collision: bool = False, allow_wall_collision: bool = False, env_kwargs: Optional[dict] = None,
                 act_bound: Optional[float] = None, autoreset: bool = True, device=None):
        if env not in _ENVS:
            raise ValueError(f"no device step for env {env!r}: choose one of {sorted(_ENVS)}")
        hole = env == "hole_reacher"
        if rew_fct != "simple" and not hole:
            raise ValueError(f"rew_fct={rew_fct!r} is HoleReacher's reward function: it needs env='hole_reacher'")
        _lib.hole_rew_fct(rew_fct, steps_before_reward)
        defaults = dict(_ENVS[env])
        unknown = set(env_kwargs or {}) - set(defaults)
        if unknown:
            raise ValueError(f"env_kwargs of {env!r} take {sorted(defaults)}, got {sorted(unknown)}")
        defaults.update(env_kwargs or {})
        self.env, self.env_kwargs = env, defaults
        self.num_envs, self.n_links = int(num_envs), int(n_links)
        if not 1 <= self.n_links <= 16:
            raise ValueError(f"n_links must be 1 .. 16 on the device, got {n_links}")
        self.dt, self.max_episode_steps = float(dt), int(max_episode_steps)
        self.autoreset = bool(autoreset)
        self._step_kw = dict(dt=self.dt, max_episode_steps=self.max_episode_steps, steps_before_reward=int(steps_before_reward),
                             rew_fct=rew_fct, collision_penalty=float(collision_penalty),
                             allow_self_collision=bool(allow_self_collision), allow_wall_collision=bool(allow_wall_collision))
        # the handle carries the device, the link count and the fault word; its movement primitive is never evaluated
        self.engine = TrajectoryEngine("promp", "linear", "zero_rbf", self.n_links, 5, dt=self.dt,
                                       duration=self.max_episode_steps * self.dt, tau=self.max_episode_steps * self.dt,
                                       num_basis_zero_start=1, device=device)
        self.device = dev = self.engine.device
        B, D = self.num_envs, self.n_links
        n = 3 * D + (4 if hole else 3)
        bound = np.concatenate([np.full(2 * D, np.pi), np.full(n - 2 * D, np.inf)])
        self.single_observation_space = _gym.spaces.Box(low=-bound, high=bound, shape=bound.shape)
        if act_bound is None:
            act_bound = 2 * np.pi if hole else 1000.0        # max_vel (base_reacher_direct.py:17) / max_torque (base_reacher_torque.py:16)
        act = np.full(D, float(act_bound))
        self.single_action_space = _gym.spaces.Box(low=-act, high=act, shape=act.shape)
        self.observation_space = _batched_box(self.single_observation_space, B)
        self.action_space = _batched_box(self.single_action_space, B)
        self.q = torch.zeros((B, D), dtype=torch.float64, device=dev)
        self.qd = torch.zeros_like(self.q)
        self.traj_steps = torch.zeros(B, dtype=torch.int32, device=dev)
        self.task = torch.zeros((B, 3 if hole else 2), dtype=torch.float64, device=dev)        # hole (x, width, depth) / goal
        self.rng = torch.zeros((B, 5), dtype=torch.int64, device=dev)
        self.reward_state = torch.zeros((B, 2), dtype=torch.float64, device=dev) if rew_fct == "unbounded" else None
        self._plan_steps = torch.zeros(B, dtype=torch.int32, device=dev)        # what mpk_reacher_reset also clears: not used here
        self._done = torch.zeros(B, dtype=torch.uint8, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self._out = dict(reward=torch.zeros(B, dtype=torch.float64, device=dev), terminated=torch.zeros(B, **u8),
                         truncated=torch.zeros(B, **u8), reset_mask=torch.zeros(B, **u8),
                         final_obs=torch.zeros((B, n), dtype=torch.float32, device=dev),
                         obs=torch.zeros((B, n), dtype=torch.float32, device=dev))
        if hole:
            self._out.update(is_collided=torch.zeros(B, **u8), is_success=torch.zeros(B, **u8))
        self._seeded = False

    def state_tensors(self):
        """everything a step changes on the device besides its outputs"""
        return [self.q, self.qd, self.traj_steps, self.task, self.rng] + ([self.reward_state] if self.reward_state is not None else [])

    def reset(self, *, seed: Optional[int] = None, options=None) -> Tuple[torch.Tensor, dict]:
        """(obs [num_envs, n] float32 on the device, {}): ``seed`` = int seeds episode b with ``seed + b`` (gymnasium's vector rule),
        None continues the streams -- the first reset needs a seed, the device generators have no OS entropy to start from"""
        if options:
            raise ValueError(f"reset options are not supported on the device, got {sorted(options)}")
        if seed is None:
            if not self._seeded:
                raise ValueError("the first reset needs a seed: reset(seed=int) -- the device streams have no OS entropy source")
            seeding = {}
        else:
            if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
                raise ValueError(f"seed must be an int, got {seed!r}")
            if seed < 0 or int(seed) + self.num_envs - 1 >= 2 ** 64:
                raise ValueError(f"seeds seed + b must lie in [0, 2^64), got seed={seed} for {self.num_envs} episodes")
            seeding = dict(seed_base=int(seed))
        self.engine.reacher_reset(self.env, self.q, self.qd, self.traj_steps, self._plan_steps, self._done, self.rng, self.task,
                                  **seeding, **self.env_kwargs)
        self._seeded = True
        return self.engine.reacher_observation(self.env, self.q, self.qd, self.task, self.traj_steps), {}

    def step(self, actions) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """actions float32 [num_envs, n_links] -> (obs [num_envs, n] float32, rewards [num_envs] float64, terminated, truncated
        [num_envs] bool, info), all on the device; the same tensors every step (copy what must outlive the next one)"""
        if not self._seeded:
            raise ValueError("step before reset: call reset(seed=int) first")
        actions = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
        if tuple(actions.shape) != (self.num_envs, self.n_links):
            raise ValueError(f"actions must be [{self.num_envs}, {self.n_links}], got {tuple(actions.shape)}")
        o = self.engine.reacher_env_step(self.env, actions.contiguous(), self.q, self.qd, self.traj_steps, self.rng, self.task, self._out,
                                         autoreset=self.autoreset, reward_state=self.reward_state, **self._step_kw, **self.env_kwargs)
        info = {"final_obs": o["final_obs"], "_final_obs": o["reset_mask"].view(torch.bool)}
        if self.env == "hole_reacher":
            info["is_collided"] = o["is_collided"].view(torch.bool)
            info["is_success"] = o["is_success"].view(torch.bool)
        return o["obs"], o["reward"], o["terminated"].view(torch.bool), o["truncated"].view(torch.bool), info

    def rng_state(self, episodes=None) -> list:
        """numpy's ``bit_generator.state`` of the chosen episodes' generators (synchronises)"""
        from .engine import nprng_state
        return nprng_state(self.rng, episodes)

    def capture(self) -> "EnvStepGraph":
        """one environment step as one hipGraph with ONE kernel node: write the actions into the returned object's ``actions``
        buffer, ``replay()``, read the tuple ``step`` would have returned.  After ``reset(seed=...)``."""
        return EnvStepGraph(self)

    def close(self):
        self.engine.close()


class EnvStepGraph:
    """``BatchedStepEnv.step`` captured the way ``VectorStepGraph`` captures a vector step: one eager pass on a side stream whose
    effects on the episodes are undone, then the capture"""

    def __init__(self, env: BatchedStepEnv):
        if not env._seeded:
            raise ValueError("capture() continues the streams of a seeded reset: call reset(seed=...) first")
        self.env = env
        dev = env.device
        self.actions = torch.zeros((env.num_envs, env.n_links), dtype=torch.float32, device=dev)
        state = env.state_tensors()
        snapshot = [t.clone() for t in state]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            env.step(self.actions)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for t, s in zip(state, snapshot):
            t.copy_(s)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outs = env.step(self.actions)
        torch.cuda.synchronize(dev)
        # the captured pass only recorded: the episodes are where the snapshot left them

    def replay(self):
        self.graph.replay()
        return self.outs
