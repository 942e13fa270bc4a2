"""
BatchedVectorEnv -- the gymnasium vector-env contract (``reset -> obs, info``; ``step(actions) -> obs, rewards, terminated, truncated,
info``; autoreset) over a ``BatchedBlackBox``, for the ids whose episodes live on the device (``make_batched_vec``).  ``VectorBlackBox``
(vector.py) has this role for host envs; here nothing leaves the GPU: observations, rewards and flags are torch tensors on the device,
and a step issues exactly the launches of ``BatchedBlackBox.step`` / ``reset(sample=True)`` / ``observe()``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _gym
from .batched import BatchedBlackBox

# what BatchedBlackBox.step returns that is neither a return value of the vector step nor a view of state the autoreset overwrites
_NOT_INFO = ("params", "obs", "rewards", "terminated", "truncated", "done", "current_pos", "current_vel")


def _batched_box(space, n: int):
    return _gym.spaces.Box(low=np.repeat(space.low[None], n, axis=0), high=np.repeat(space.high[None], n, axis=0), dtype=space.dtype)


class BatchedVectorEnv:
    """
    ``num_envs`` episodes of one movement-primitive id as a vector env.  One ``step`` is one whole episode of every env (black-box RL:
    the action is the MP parameter vector), so every step ends every episode.

    Autoreset mode: **same-step** (gymnasium's ``AutoresetMode.SAME_STEP``).  The step that ends the episodes also resets them
    (``BatchedBlackBox.reset(sample=True)``: every episode's stream continues as the host env's ``reset()`` would): the returned ``obs`` is
    the first observation of the NEXT episodes, the last observation of the finished ones is ``info["final_obs"]``; rewards and flags
    belong to the finished episodes.  ``info`` also carries ``trajectory_length`` and, for HoleReacher, ``is_collided`` / ``is_success``
    (at verbose >= 2 the per-step arrays of ``BatchedBlackBox.step`` as well), all [num_envs, ...] tensors.

    With replanning (``black_box_kwargs={"replanning_every": n}``) a step does not end the episode: ``step`` returns the time-aware
    observation of the running episodes and no ``final_obs``, and the autoreset happens in the step in which the LAST episodes reach
    their step limit -- all episodes are reset together: in this default mode an episode that collided early stays done, executes
    nothing (``trajectory_length`` 0, reward 0) and is reset with the rest.

    ``partial_resets=True`` is the vector-env contract per sub-env: an episode that ended in this step starts anew in this step, from
    its own stream, while the others run on.  ``step`` is then ``BatchedBlackBox.step`` plus ONE launch (mpk_reacher_autoreset: last
    observation, reset of the finished rows, next observation).  ``obs`` holds the first observation of the new episode for the rows
    that were reset and the step's observation for the others; ``info["final_obs"]`` [num_envs, n] (the step's observation of every
    row) and ``info["_final_obs"]`` (bool [num_envs]: the rows that were reset, for which ``final_obs`` is the finished episode's last
    observation) are present in every step.  Nothing in the step is decided on the host, so ``capture()`` works with replanning too.
    The episodes leave lockstep: every plan takes its ``init_time`` from its episode's device counter, and the SimpleReacher ids step
    through the separate plan / rollout launches instead of their one-launch step (same results).  Without replanning every step ends
    every episode and the mode returns exactly what the default mode returns, plus the all-true ``_final_obs``.  A partial reset
    synchronises nothing: ``bb.check_range()`` (ProDMP) is the caller's to call.

    Sub-trajectory learning is refused in both modes (its episodes end at different steps, and a partial reset of them is not built).

    No host synchronisation beyond what ``BatchedBlackBox.step`` / ``reset`` do themselves.
    """

    def __init__(self, bb: BatchedBlackBox, partial_resets: bool = False):
        if not bb.observations:
            raise ValueError("BatchedVectorEnv needs a BatchedBlackBox with observations=True")
        if bb.learn_sub_trajectories:
            raise ValueError("learn_sub_trajectories ends episodes at different steps: partial resets are not built")
        self.partial_resets = bool(partial_resets)
        if self.partial_resets:
            bb.enable_partial_resets()
        self.bb = bb
        self.num_envs = bb.B
        self.single_observation_space = bb.observation_space
        low, high = bb.params_bounds()
        self.single_action_space = _gym.spaces.Box(low=low, high=high, dtype=np.float32)      # BlackBoxWrapper.action_space
        self.observation_space = _batched_box(self.single_observation_space, self.num_envs)
        self.action_space = _batched_box(self.single_action_space, self.num_envs)
        self._seeded = False

    def reset(self, *, seed: Optional[int] = None, options=None) -> Tuple[torch.Tensor, dict]:
        """(obs [num_envs, n] float32 on the device, {}): ``seed`` = int seeds episode b with ``seed + b`` (gymnasium's vector rule; a
        sequence of num_envs ints seeds each), None continues the streams -- the first reset needs a seed, the device generators have
        no OS entropy to start from"""
        if options:
            raise ValueError(f"reset options are not supported on the device, got {sorted(options)}")
        if seed is None:
            if not self._seeded:
                raise ValueError("the first reset needs a seed: reset(seed=int) -- the device streams have no OS entropy source")
            self.bb.reset(sample=True)
        else:
            self.bb.reset(seed=seed)
            self._seeded = True
        return self.bb.observe(), {}

    def _episodes_over(self) -> bool:
        """the host's mirror of the integer rule (no read-back): the episodes that still run have reached the step limit"""
        bb = self.bb
        return not bb.do_replanning or (bb._lockstep is not None and bb._lockstep >= bb.horizon)

    def step(self, actions) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """actions [num_envs, P] -> (obs [num_envs, n] float32, rewards [num_envs] float64, terminated, truncated [num_envs] bool, info)"""
        if not self._seeded:
            raise ValueError("step before reset: call reset(seed=int) first")
        bb = self.bb
        if self.partial_resets:
            # (the step's own observation launch is the autoreset's final_obs: not launched twice)
            out = bb._step(actions, True)
            info = {k: v for k, v in out.items() if k not in _NOT_INFO}
            if bb._obs_start is not None and "des_pos" in out:
                info["step_observations"] = bb._add_step_observations(out, bb._obs_start)
            info["final_obs"], obs, info["_final_obs"] = bb.autoreset()
            return obs, out["rewards"], out["terminated"], out["truncated"], info
        out = bb.step(actions)
        info = {k: v for k, v in out.items() if k not in _NOT_INFO}
        obs = out["obs"]
        if self._episodes_over():
            info["final_obs"] = obs
            bb.reset(sample=True)
            obs = bb.observe()
        return obs, out["rewards"], out["terminated"], out["truncated"], info

    def capture(self) -> "VectorStepGraph":
        """one whole vector step (plan, rollout, last observation, reset draw, first observation) as one hipGraph: write the actions
        into the returned object's ``actions`` buffer, ``replay()``, read the tuple ``step`` would have returned (the same tensors every
        replay).  After ``reset(seed=...)``; in the default mode not with replanning, where the host decides per step whether the
        episodes are over -- ``partial_resets=True`` has no such decision and captures a replanning step as well."""
        return VectorStepGraph(self)

    def close(self):
        return None


class VectorStepGraph:
    """``BatchedVectorEnv.step`` captured the way ``BatchedBlackBox.capture_episode`` captures an episode: one eager pass on a side
    stream (allocator warm-up, lazy initialisation) whose effects on the episodes are undone, then the capture"""

    def __init__(self, env: BatchedVectorEnv):
        bb = env.bb
        if not env._seeded:
            raise ValueError("capture() continues the streams of a seeded reset: call reset(seed=...) first")
        if bb.do_replanning and not env.partial_resets:
            raise ValueError("capture() holds a fixed sequence of launches: with replanning the host decides whether a step resets")
        if bb.spec is None:
            raise ValueError("capture() needs a device plant")
        self.env = env
        dev = bb.device
        self.actions = torch.zeros((bb.B, bb.engine.num_params), dtype=torch.float32, device=dev)
        # everything a vector step changes on the device: the warm-up pass runs one, the first replay must start where step() would
        state = [bb.q, bb.qd, bb.traj_steps, bb.plan_steps, bb.done, bb._rng, bb._task_buf, *bb._start32]
        if bb._reward_state is not None:
            state.append(bb._reward_state)
        if bb._cond_buf is not None:
            state.extend(bb._cond_buf)
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
