"""
TrajectoryEngine -- thin, typed wrapper over one ``mpk_handle`` (include/mpk.h).

It owns no arithmetic: every number it returns was produced by the HIP kernels in ``csrc/``.  PyTorch is used only for
device memory and streams (tensors are passed to the C-ABI as raw device pointers).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import (BASIS_TYPES, CTRL_TYPES, MP_TYPES, PHASE_TYPES, PLANT_TYPES, MPKLibraryError, mpk_config,
                   mpk_rollout_cfg)

_INF = float("inf")


def _dptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dvec(x, n: int):
    """scalar or sequence -> (ctypes double[n], keep-alive)"""
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)))
    return a.ctypes.data_as(C.POINTER(C.c_double)), a


def nprng_state(rng: torch.Tensor, episodes=None) -> list:
    """numpy's ``bit_generator.state`` dicts of the chosen episodes of a reacher reset's generator (int64 [B, 5], mpk_nprng_state):
    ``np.random.default_rng(); rng.bit_generator.state = d`` continues that episode's stream on the host.  Synchronises."""
    words = rng.detach().cpu().numpy().view(np.uint64)
    idx = range(words.shape[0]) if episodes is None else np.atleast_1d(np.asarray(episodes)).tolist()
    out = []
    for b in idx:
        w = [int(v) for v in words[b]]
        out.append({"bit_generator": "PCG64", "state": {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]},
                    "has_uint32": w[4] & 0xFFFFFFFF, "uinteger": w[4] >> 32})
    return out


class RolloutSpec:
    """Controller + plant description for the device rollout (mpk_rollout_cfg)."""

    def __init__(self, controller_type: str, num_dof: int, p_gains=1.0, d_gains=0.5, act_low=-_INF, act_high=_INF,
                 plant: str = "static", dt: float = 0.0):
        controller_type = controller_type.lower()
        # 'metaworld' (controller/meta_world_controller.py:15-25: xyz as a position delta, last entry = the raw gripper
        # opening) is the motor controller with unit position gains, no velocity gains and a zero in the last entry of the
        # current position -- 1.0 * (des - cur) + 0.0 * (..) is exact in float64 -- so it runs on the motor kernels; there is
        # no batchable metaworld plant, hence open loop (frozen state) only: TrajectoryEngine.trajectory_actions / pd_rollout
        self.metaworld = controller_type == "metaworld"
        if self.metaworld:
            if plant != "static":
                raise ValueError("the metaworld controller has no device plant: use plant='static' (actions for a frozen "
                                 "state) or step the environments on the host (VectorBlackBox)")
            controller_type, p_gains, d_gains = "motor", 1.0, 0.0
        if controller_type not in CTRL_TYPES:
            raise ValueError(f"controller type {controller_type!r} has no device implementation; "
                             f"choose one of {list(CTRL_TYPES)}")
        if plant not in PLANT_TYPES:
            raise ValueError(f"unknown plant {plant!r}; choose one of {list(PLANT_TYPES)}")
        self.controller_type, self.plant, self.num_dof, self.dt = controller_type, plant, num_dof, float(dt)
        self._keep = []
        self.c = mpk_rollout_cfg()
        self.c.controller_type = CTRL_TYPES[controller_type]
        self.c.plant_type = PLANT_TYPES[plant]
        self.c.dt = float(dt)
        for name, val in (("p_gains", p_gains), ("d_gains", d_gains), ("act_low", act_low), ("act_high", act_high)):
            v = np.asarray(val, dtype=np.float64)
            if v.ndim > 0 and v.shape != (num_dof,):
                raise ValueError(f"Mismatch in dimension between {name} {v.shape} and the action dimension ({num_dof},)")
            ptr, keep = _dvec(val, num_dof)
            setattr(self.c, name, ptr)
            self._keep.append(keep)


class _TrajectoryFn(torch.autograd.Function):
    """``TrajectoryEngine.trajectory`` with a backward: forward = the mpk_trajectory launch as without autograd, backward = one
    mpk_trajectory_vjp launch on the current stream; ``needs_input_grad`` decides which of its outputs are computed at all"""

    @staticmethod
    def forward(ctx, engine, init_time, out, params, init_pos, init_vel):
        ctx.engine, ctx.init_time = engine, init_time
        ctx.set_materialize_grads(False)          # an output the loss never saw arrives as None: its term is skipped, not read
        return engine._trajectory_launch(params, init_pos, init_vel, None, init_time, out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pos, g_vel):
        need = ctx.needs_input_grad[3:6]
        if g_pos is None and g_vel is None:
            return (None,) * 6
        g_params, g_init_pos, g_init_vel = ctx.engine.trajectory_vjp(g_pos, g_vel, ctx.init_time, need=need)
        return None, None, None, g_params, g_init_pos, g_init_vel


class _TrajectoryPhaseFn(torch.autograd.Function):
    """``TrajectoryEngine.trajectory(..., phase_gradient="pathwise")`` for a per-episode phase (learned tau / delay, per-episode
    init_time): forward = the plain mpk_trajectory launch, backward = one mpk_trajectory_phase_vjp launch, which recomputes the episode's
    phase and rows from the forward's inputs (nothing of the forward launch is kept but those); ``init_time`` gets no gradient"""

    @staticmethod
    def forward(ctx, engine, it_t, it_s, out, params, init_pos, init_vel):
        ctx.engine, ctx.it_t, ctx.it_s = engine, it_t, it_s
        ctx.save_for_backward(params, init_pos, init_vel)
        ctx.set_materialize_grads(False)
        return engine._trajectory_launch(params, init_pos, init_vel, it_t, it_s, out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pos, g_vel):
        need = ctx.needs_input_grad[4:7]
        if g_pos is None and g_vel is None:
            return (None,) * 7
        params, init_pos, init_vel = ctx.saved_tensors
        g = ctx.engine.trajectory_phase_vjp(params, init_pos, init_vel, g_pos, g_vel, ctx.it_t if ctx.it_t is not None else ctx.it_s,
                                            need=need)
        return (None, None, None, None) + tuple(g)


class _TrajectoryLogProbFn(torch.autograd.Function):
    """``TrajectoryEngine.trajectory_log_prob`` with a backward: forward = the mpk_trajectory_log_prob launch as without autograd,
    backward = one mpk_trajectory_log_prob_vjp launch, which recomputes the factorisation from the forward's inputs (nothing of the
    forward launch is kept but those); the observations and the initial conditions get no gradient.  ``phase``: the per-episode-phase
    route (``trajectory_log_prob_given_timing``: mpk_trajectory_phase_log_prob / _vjp), whose backward leaves exact zeros in the phase
    columns"""

    @staticmethod
    def forward(ctx, engine, steps, inputs, init_time, params, params_L, phase=False):
        ctx.engine, ctx.steps, ctx.inputs, ctx.init_time, ctx.phase = engine, steps, inputs, init_time, phase
        ctx.save_for_backward(params, params_L)
        return engine._log_prob_launch(params, params_L, steps, inputs, init_time, phase)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        params, params_L = ctx.saved_tensors
        g_params, g_L = ctx.engine._log_prob_vjp_launch(g, params, params_L, ctx.steps, ctx.inputs, ctx.init_time,
                                                        ctx.needs_input_grad[4:6], ctx.phase)
        return None, None, None, None, g_params, g_L, None


class _DemonstrationLogProbFn(torch.autograd.Function):
    """``TrajectoryEngine.demonstration_log_prob`` with a backward: forward = the mpk_demonstration_log_prob launch as without autograd,
    backward = one mpk_demonstration_log_prob_vjp launch, which recomputes the Gram matrices and the factorisation from the forward's
    inputs; the demonstrations, their standard deviations and the initial conditions get no gradient.  ``phase``: the per-episode-phase
    route (``timing="given"``: mpk_demonstration_phase_log_prob / _vjp), whose backward leaves exact zeros in the phase columns"""

    @staticmethod
    def forward(ctx, engine, inputs, init_time, params, params_L, phase=False):
        ctx.engine, ctx.inputs, ctx.init_time, ctx.phase = engine, inputs, init_time, phase
        ctx.save_for_backward(params, params_L)
        return engine._demo_log_prob_launch(params, params_L, inputs, init_time, phase)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        params, params_L = ctx.saved_tensors
        g_params, g_L = ctx.engine._demo_log_prob_vjp_launch(g, params, params_L, ctx.inputs, ctx.init_time, ctx.needs_input_grad[3:5],
                                                             ctx.phase)
        return None, None, None, g_params, g_L, None


class _ReacherRolloutFn(torch.autograd.Function):
    """``TrajectoryEngine.reacher_rollout`` with a backward: forward = a copy of the plan-start (q, qd) and the mpk_reacher_rollout launch
    as without autograd, backward = one mpk_reacher_rollout_vjp launch; the actions and the in-place q, qd carry no graph"""

    @staticmethod
    def forward(ctx, engine, spec, q, qd, n_steps, step0, steps_before_reward, want_actions, out, des_pos, des_vel, goal):
        ctx.engine, ctx.spec, ctx.n_steps, ctx.step0, ctx.sbr = engine, spec, n_steps, step0, int(steps_before_reward)
        ctx.start = (q.clone(), qd.clone())
        ctx.save_for_backward(des_pos, des_vel, goal)
        act, rew = engine._reacher_rollout_launch(spec, des_pos, des_vel, q, qd, goal, n_steps, step0, steps_before_reward,
                                                  want_actions, out)
        if act is None:
            return rew
        ctx.mark_non_differentiable(act)
        return act, rew

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        g_rew = grads[-1]
        des_pos, des_vel, goal = ctx.saved_tensors
        need = ctx.needs_input_grad[9:12]
        g_pos, g_vel, _, _, g_goal = ctx.engine.reacher_rollout_vjp(
            ctx.spec, des_pos, des_vel, ctx.start[0], ctx.start[1], goal, g_rew, n_steps=ctx.n_steps, step0=ctx.step0,
            steps_before_reward=ctx.sbr, need=(need[0], need[1], False, False, need[2]))
        return (None,) * 9 + (g_pos, g_vel, g_goal)


class _HoleRolloutFn(torch.autograd.Function):
    """``TrajectoryEngine.hole_reacher_rollout(differentiable=True)``: forward = a copy of the plan-start (q, qd) and of the step counters
    and the mpk_hole_reacher_rollout2 launch as without autograd, backward = ONE mpk_hole_reacher_rollout_vjp launch at the forward's own
    (n_exec, collided) -- the episode's end and verdict are frozen; the actions, the in-place state and the integer outputs carry no
    graph.  Returns (ret, rewards) -- either may be None --, the launch's dict is left in ``box``"""

    @staticmethod
    def forward(ctx, engine, launch, box, spec, q, qd, step0, task_kw, aggregation, des_pos, des_vel, hole):
        ctx.engine, ctx.spec, ctx.task_kw, ctx.agg = engine, spec, task_kw, aggregation
        ctx.start = (q.clone(), qd.clone())
        ctx.step0 = None if step0 is None else step0.clone()      # (a replanning state's traj_steps is advanced by the launch)
        r = launch()
        box.update(r)
        ctx.n_exec, ctx.collided = r["n_exec"], r["collided"]
        ctx.has_pos = des_pos is not None
        ctx.save_for_backward(*([des_pos] if ctx.has_pos else []), des_vel, hole)
        ctx.set_materialize_grads(False)
        outs = tuple(t for t in (r["ret"], r["rewards"]) if t is not None)
        ctx.which = tuple(k for k in ("ret", "rewards") if r[k] is not None)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        des_pos = saved[0] if ctx.has_pos else None
        des_vel, hole = saved[-2], saved[-1]
        g = dict(zip(ctx.which, grads))
        need = ctx.needs_input_grad[9:12]
        if g.get("ret") is None and g.get("rewards") is None:
            return (None,) * 12
        g_pos, g_vel, _, _, g_hole = ctx.engine.hole_reacher_rollout_vjp(
            ctx.spec, des_pos, des_vel, ctx.start[0], ctx.start[1], hole, n_exec=ctx.n_exec, collided=ctx.collided, step0=ctx.step0,
            g_rewards=g.get("rewards"), g_ret=g.get("ret"), aggregation=ctx.agg or "sum",
            need=(bool(need[0]) and ctx.has_pos, need[1], False, False, need[2]), **ctx.task_kw)
        return (None,) * 9 + (g_pos, g_vel, g_hole)


class _EpisodeReturnFn(torch.autograd.Function):
    """``TrajectoryEngine.episode_return(differentiable=True)``: forward = a copy of the plan-start (q, qd) and of the step counters and
    the mpk_episode_return launch as without autograd, backward = ONE mpk_episode_return_vjp launch (plan, rollout adjoint and table
    transpose fused); the in-place state and the integer outputs carry no graph"""

    @staticmethod
    def forward(ctx, engine, launch, spec, q, qd, step0, steps_before_reward, aggregation, init_time, params, init_pos, init_vel, goal):
        ctx.engine, ctx.spec, ctx.sbr, ctx.agg, ctx.init_time = engine, spec, int(steps_before_reward), aggregation, float(init_time)
        ctx.start = (q.clone(), qd.clone())
        ctx.step0 = None if step0 is None else step0.clone()      # (a replanning state's traj_steps is advanced by the launch)
        r = launch()
        ctx.seg = r["seg_len"]
        ctx.save_for_backward(params, init_pos, init_vel, goal)
        return r["ret"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ret):
        params, init_pos, init_vel, goal = ctx.saved_tensors
        need = ctx.needs_input_grad[9:13]
        g_params, g_ip, g_iv, _, _, g_goal, _, _ = ctx.engine.episode_return_vjp(
            params, init_pos, init_vel, ctx.spec, ctx.start[0], ctx.start[1], goal, g_ret, n_steps=ctx.seg, step0=ctx.step0,
            steps_before_reward=ctx.sbr, aggregation=ctx.agg, init_time=ctx.init_time,
            need=(need[0], need[1], need[2], False, False, need[3], False, False))
        return (None,) * 9 + (g_params, g_ip, g_iv, g_goal)


def _carry_outputs(q, qd, cond_pos, cond_vel):
    """the differentiable outputs a carrying function adds: clones of what the launch left in q, qd and, where it wrote them, of the
    condition -- the same bits; the caller's in-place q, qd and the launch's own cond tensors stay graph-free"""
    outs = [q.clone(), qd.clone()]
    if cond_pos is not None:
        outs += [cond_pos.clone(), cond_vel.clone()]
    return outs


class _ReacherRolloutCarryFn(torch.autograd.Function):
    """``_ReacherRolloutFn`` in its carrying form (``reacher_rollout(carry=...)``): the plan-start state ``q_in``, ``qd_in`` -- float64
    [B, D] tensors with the bits of q, qd that may carry the graph of earlier plans -- are inputs, and the state after the plan
    (``q_end``, ``qd_end``) and, with ``condition``, the gathered condition (``cond_pos``, ``cond_vel``: mpk_condition_gather on this plan
    at ``n_steps``) are differentiable outputs.  The backward is still ONE launch, mpk_reacher_rollout_vjp[_cond], fed with the incoming
    gradients of the rewards, the end state and the condition (a missing one is passed as NULL); it returns g_q0, g_qd0 for ``q_in``,
    ``qd_in``.  Returns (rewards, q_end, qd_end[, cond_pos, cond_vel]); the actions are left in ``box``"""

    @staticmethod
    def forward(ctx, engine, spec, q, qd, n_steps, step0, steps_before_reward, want_actions, out, condition, box, des_pos, des_vel, goal,
                q_in, qd_in):
        ctx.engine, ctx.spec, ctx.n_steps, ctx.step0, ctx.sbr = engine, spec, n_steps, step0, int(steps_before_reward)
        ctx.start = (q.clone(), qd.clone())
        ctx.save_for_backward(des_pos, des_vel, goal)
        ctx.set_materialize_grads(False)
        act, rew = engine._reacher_rollout_launch(spec, des_pos, des_vel, q, qd, goal, n_steps, step0, steps_before_reward,
                                                  want_actions, out)
        box["actions"] = act
        cp = cv = None
        if condition:
            T = des_pos.shape[1]
            seg = n_steps if n_steps is not None else torch.full((des_pos.shape[0],), T, dtype=torch.int32, device=des_pos.device)
            cp, cv = engine.condition_gather(des_pos, des_vel, seg)
        box["cond_pos"], box["cond_vel"] = cp, cv
        ctx.has_cond = condition
        return (rew, *_carry_outputs(q, qd, cp, cv))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rew, g_qe, g_qde, g_cp=None, g_cv=None):
        if all(g is None for g in (g_rew, g_qe, g_qde, g_cp, g_cv)):
            return (None,) * 16
        des_pos, des_vel, goal = ctx.saved_tensors
        need = ctx.needs_input_grad[11:16]
        g_pos, g_vel, g_q0, g_qd0, g_goal = ctx.engine.reacher_rollout_vjp(
            ctx.spec, des_pos, des_vel, ctx.start[0], ctx.start[1], goal, g_rew, g_q=g_qe, g_qd=g_qde, n_steps=ctx.n_steps,
            step0=ctx.step0, steps_before_reward=ctx.sbr, need=(need[0], need[1], need[3], need[4], need[2]),
            g_cond_pos=g_cp, g_cond_vel=g_cv)
        return (None,) * 11 + (g_pos, g_vel, g_goal, g_q0, g_qd0)


class _HoleRolloutCarryFn(torch.autograd.Function):
    """``_HoleRolloutFn`` in its carrying form (``hole_reacher_rollout(differentiable=True, carry=...)``): ``q_in``, ``qd_in`` -- float64
    [B, D] tensors with the bits of q, qd that may carry the graph of earlier plans -- are inputs; the state after the plan and, where
    the launch wrote it, the condition are differentiable outputs.  ONE mpk_hole_reacher_rollout_vjp[_cond] launch backward, at the
    forward's own (n_exec, collided): an episode that executed nothing hands the gradient of its end state on unchanged.  Returns
    ([ret][, rewards], q_end, qd_end[, cond_pos, cond_vel]), the launch's dict is left in ``box``"""

    @staticmethod
    def forward(ctx, engine, launch, box, spec, q, qd, step0, task_kw, aggregation, des_pos, des_vel, hole, q_in, qd_in):
        ctx.engine, ctx.spec, ctx.task_kw, ctx.agg = engine, spec, task_kw, aggregation
        ctx.start = (q.clone(), qd.clone())
        ctx.step0 = None if step0 is None else step0.clone()      # (a replanning state's traj_steps is advanced by the launch)
        r = launch()
        box.update(r)
        ctx.n_exec, ctx.collided = r["n_exec"], r["collided"]
        ctx.has_pos = des_pos is not None
        ctx.save_for_backward(*([des_pos] if ctx.has_pos else []), des_vel, hole)
        ctx.set_materialize_grads(False)
        ctx.which = tuple(k for k in ("ret", "rewards") if r[k] is not None) + ("q", "qd") + \
            (("cond_pos", "cond_vel") if r.get("cond_pos") is not None else ())
        return (*(r[k] for k in ("ret", "rewards") if r[k] is not None), *_carry_outputs(q, qd, r.get("cond_pos"), r.get("cond_vel")))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        des_pos = saved[0] if ctx.has_pos else None
        des_vel, hole = saved[-2], saved[-1]
        g = dict(zip(ctx.which, grads))
        if all(v is None for v in g.values()):
            return (None,) * 14
        need = ctx.needs_input_grad[9:14]
        g_pos, g_vel, g_q0, g_qd0, g_hole = ctx.engine.hole_reacher_rollout_vjp(
            ctx.spec, des_pos, des_vel, ctx.start[0], ctx.start[1], hole, n_exec=ctx.n_exec, collided=ctx.collided, step0=ctx.step0,
            g_rewards=g.get("rewards"), g_ret=g.get("ret"), aggregation=ctx.agg or "sum", g_q=g.get("q"), g_qd=g.get("qd"),
            need=(bool(need[0]) and ctx.has_pos, need[1], need[3], need[4], need[2]),
            g_cond_pos=g.get("cond_pos"), g_cond_vel=g.get("cond_vel"), **ctx.task_kw)
        return (None,) * 9 + (g_pos, g_vel, g_hole, g_q0, g_qd0)


class _EpisodeReturnCarryFn(torch.autograd.Function):
    """``_EpisodeReturnFn`` in its carrying form (``episode_return(differentiable=True, carry=...)``): ``q_in``, ``qd_in`` -- float64
    [B, D] tensors with the bits of q, qd that may carry the graph of earlier plans -- are inputs; the state after the plan and, where
    the launch wrote it, the condition are differentiable outputs.  ONE mpk_episode_return_vjp[_cond] launch backward: the incoming
    gradients of the return, the end state and the condition (a missing one as NULL) -> params, init_pos, init_vel, goal and g_q0,
    g_qd0 for ``q_in``, ``qd_in``.  Returns (ret, q_end, qd_end[, cond_pos, cond_vel])"""

    @staticmethod
    def forward(ctx, engine, launch, spec, q, qd, step0, steps_before_reward, aggregation, init_time, params, init_pos, init_vel, goal,
                q_in, qd_in):
        ctx.engine, ctx.spec, ctx.sbr, ctx.agg, ctx.init_time = engine, spec, int(steps_before_reward), aggregation, float(init_time)
        ctx.start = (q.clone(), qd.clone())
        ctx.step0 = None if step0 is None else step0.clone()      # (a replanning state's traj_steps is advanced by the launch)
        r = launch()
        ctx.seg = r["seg_len"]
        ctx.save_for_backward(params, init_pos, init_vel, goal)
        ctx.set_materialize_grads(False)
        return (r["ret"], *_carry_outputs(q, qd, r.get("cond_pos"), r.get("cond_vel")))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ret, g_qe, g_qde, g_cp=None, g_cv=None):
        if all(g is None for g in (g_ret, g_qe, g_qde, g_cp, g_cv)):
            return (None,) * 15
        params, init_pos, init_vel, goal = ctx.saved_tensors
        need = ctx.needs_input_grad[9:15]
        g_params, g_ip, g_iv, g_q0, g_qd0, g_goal, _, _ = ctx.engine.episode_return_vjp(
            params, init_pos, init_vel, ctx.spec, ctx.start[0], ctx.start[1], goal, g_ret, g_q=g_qe, g_qd=g_qde, n_steps=ctx.seg,
            step0=ctx.step0, steps_before_reward=ctx.sbr, aggregation=ctx.agg, init_time=ctx.init_time,
            need=(need[0], need[1], need[2], need[4], need[5], need[3], False, False), g_cond_pos=g_cp, g_cond_vel=g_cv)
        return (None,) * 9 + (g_params, g_ip, g_iv, g_goal, g_q0, g_qd0)


class _RewardAggregateFn(torch.autograd.Function):
    """``reward_aggregate`` with a backward: the value is the mpk_reward_aggregate launch's, bit for bit; the aggregation is linear, so
    the gradient of the step rewards is g_ret[b] times 1 (sum), 1 / seg (mean) or the last-step indicator (last) for t < seg[b]"""

    @staticmethod
    def forward(ctx, engine, seg_len, aggregation, rewards):
        ctx.seg, ctx.agg, ctx.T = seg_len, aggregation, rewards.shape[1]
        return engine._reward_aggregate_launch(rewards, seg_len, aggregation)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ret):
        seg = ctx.seg.view(-1, 1)
        t = torch.arange(ctx.T, device=g_ret.device, dtype=seg.dtype).view(1, -1)
        g = g_ret.view(-1, 1)
        if ctx.agg == "mean":
            g = g / seg.clamp(min=1).to(g.dtype)
        live = (t == seg - 1) if ctx.agg == "last" else (t < seg)
        return None, None, None, torch.where(live, g, torch.zeros((), dtype=g.dtype, device=g.device))


class TrajectoryEngine:
    """
    One configured movement primitive on one GPU.  Constructor arguments mirror the kwarg groups the reference hands
    to mp_pytorch (fancy_gym/utils/make_env_helpers.py:128-131; fancy_gym/envs/registry.py:62-129).
    """

    def __init__(self, mp_type: str, phase_type: str, basis_type: str, num_dof: int, num_basis: int, *, dt: float,
                 duration: float, tau: float, delay: float = 0.0, alpha_phase: float = 3.0, learn_tau: bool = False,
                 learn_delay: bool = False, tau_bound: Sequence[float] = (1e-5, _INF),
                 delay_bound: Sequence[float] = (0.0, _INF), basis_bandwidth_factor: float = 3.0,
                 num_basis_outside: int = 0, num_basis_zero_start: int = 0, num_basis_zero_goal: int = 0,
                 basis_alpha: float = 25.0, basis_dt: float = 0.01, pre_compute_length_factor: int = 6,
                 weights_scale: float = 1.0, goal_scale: float = 1.0, dmp_alpha: float = 25.0,
                 auto_scale_basis: bool = False, relative_goal: bool = False, disable_goal: bool = False,
                 disable_weights: bool = False, relative_goal_mode: str = "before_scale",
                 goal_offset_mode: str = "ignore", goal_offset: float = 0.0, single_rbf_mode: str = "unit_gap",
                 dmp_first_sample: str = "init", device: Union[int, torch.device, None] = None):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        for name, table, val in (("movement primitive", MP_TYPES, mp_type), ("phase generator", PHASE_TYPES, phase_type),
                                 ("basis generator", BASIS_TYPES, basis_type)):
            if val not in table:
                raise ValueError(f"Specified {name} type {val} not supported, please choose one of {list(table)}.")
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        if isinstance(device, torch.device):
            device = device.index or 0
        c = mpk_config()
        c.abi_version = _lib.MPK_ABI_VERSION
        c.device = int(device)
        c.mp_type, c.phase_type, c.basis_type = MP_TYPES[mp_type], PHASE_TYPES[phase_type], BASIS_TYPES[basis_type]
        c.num_dof, c.num_basis = int(num_dof), int(num_basis)
        c.num_basis_outside = int(num_basis_outside)
        c.num_basis_zero_start, c.num_basis_zero_goal = int(num_basis_zero_start), int(num_basis_zero_goal)
        c.learn_tau, c.learn_delay = int(bool(learn_tau)), int(bool(learn_delay))
        c.auto_scale_basis, c.relative_goal = int(bool(auto_scale_basis)), int(bool(relative_goal))
        c.disable_goal, c.disable_weights = int(bool(disable_goal)), int(bool(disable_weights))
        c.pre_compute_length_factor = int(pre_compute_length_factor)
        # the "(?)" items of SURVEY Appendix A as named options (include/mpk.h MPK_RELGOAL_* ...); first = default
        for field, table, val in (("relative_goal_mode", _lib.RELATIVE_GOAL_MODES, relative_goal_mode),
                                  ("goal_offset_mode", _lib.GOAL_OFFSET_MODES, goal_offset_mode),
                                  ("single_rbf_mode", _lib.SINGLE_RBF_MODES, single_rbf_mode),
                                  ("dmp_first_sample", _lib.DMP_FIRST_SAMPLE_MODES, dmp_first_sample)):
            if val not in table:
                raise ValueError(f"{field} {val!r} not supported, please choose one of {list(table)}.")
            setattr(c, field, table[val])
        c.goal_offset = float(goal_offset or 0.0)
        c.tau, c.delay, c.alpha_phase = float(tau), float(delay), float(alpha_phase)
        c.tau_bound[0], c.tau_bound[1] = float(tau_bound[0]), float(tau_bound[1])
        c.delay_bound[0], c.delay_bound[1] = float(delay_bound[0]), float(delay_bound[1])
        c.basis_bandwidth_factor, c.basis_alpha, c.basis_dt = float(basis_bandwidth_factor), float(basis_alpha), float(basis_dt)
        c.weights_scale, c.goal_scale, c.dmp_alpha = float(weights_scale), float(goal_scale), float(dmp_alpha)
        c.dt, c.duration = float(dt), float(duration)
        self.config = c
        self.mp_type, self.phase_type, self.basis_type = mp_type, phase_type, basis_type
        self.device = torch.device("cuda", int(device))
        _lib.check(self._lib.mpk_create(C.byref(c), C.byref(self._h)))
        self.num_dof = self._lib.mpk_num_dof(self._h)
        self.num_params = self._lib.mpk_num_params(self._h)
        self._host_stage = None     # pinned / device staging of trajectory_host, allocated on first use
        # B = 1 host path: the kernel reads / writes the pinned host buffers directly (False: staged device copies)
        self.b1_zero_copy = os.environ.get("MPK_B1_ZEROCOPY", "1") != "0"

    # ---- lifecycle ---------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mpk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- shape / bounds ----------------------------------------------------------------------------------------
    @property
    def num_steps(self) -> int:
        return self._lib.mpk_num_steps(self._h)

    def params_bounds(self) -> np.ndarray:
        """[2, P] float32 (traj_gen.get_params_bounds(), black_box_wrapper.py:122-127)."""
        out = np.empty((2, self.num_params), np.float32)
        _lib.check(self._lib.mpk_params_bounds(self._h, out[0].ctypes.data, out[1].ctypes.data))
        return out

    def set_duration(self, duration: float, dt: float):
        _lib.check(self._lib.mpk_set_duration(self._h, float(duration), float(dt)))

    def times(self) -> np.ndarray:
        t = np.empty(self.num_steps, np.float32)
        _lib.check(self._lib.mpk_times(self._h, t.ctypes.data))
        return t

    # ---- helpers -----------------------------------------------------------------------------------------------
    def _f32(self, x, shape) -> torch.Tensor:
        t = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        if t.shape != shape:
            t = t.expand(shape)
        return t.contiguous()

    def _f64(self, x, shape) -> torch.Tensor:
        t = torch.as_tensor(x, dtype=torch.float64, device=self.device)
        if t.shape != shape:
            t = t.expand(shape)
        return t.contiguous()

    def _stream(self) -> int:
        """the current stream of THIS engine's device (not of whatever device is current)"""
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_option(self, key: str, value: int = _lib.MPK_OPT_AUTO):
        """kernel-selection override for this engine only (mpk_set_option; A/B runs and variant-pinning tests)"""
        _lib.set_option(key, value, self._h)

    def get_option(self, key: str) -> int:
        return _lib.get_option(key, self._h)

    # ---- hot path ----------------------------------------------------------------------------------------------
    def trajectory(self, params, init_pos, init_vel, init_time=0.0, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   phase_gradient: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        params [B, P] -> (pos [B, T, D], vel [B, T, D]) float32 CUDA tensors.  ``init_time`` is a python float shared by
        all episodes, or a tensor [B] of per-episode values.

        ``phase_gradient`` (None, the default, or "pathwise") says what autograd does with a per-episode phase -- a handle with a
        learned tau / delay, or a per-episode ``init_time`` tensor.  None: such a call refuses under autograd.  "pathwise": it keeps
        the graph; the forward is the plain launch (same bits, same ``last_kernel``), the backward ONE mpk_trajectory_phase_vjp launch
        with the convention of mpk.h: a ProDMP's integer table indices are held (so its delay gets exactly 0), tau / delay outside
        their bounds get exactly 0 (torch.clamp), ``init_time`` gets no gradient.  A shared-phase call with a float ``init_time`` keeps
        using mpk_trajectory_vjp.  NotImplementedError: a DMP.
        """
        if phase_gradient not in (None, "pathwise"):
            raise ValueError(f"phase_gradient must be None or 'pathwise', got {phase_gradient!r}")
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B = params.shape[0]
        if params.shape[1] != self.num_params:
            raise ValueError(f"params has {params.shape[1]} entries per episode, expected {self.num_params}")
        D = self.num_dof
        init_pos, init_vel = self._f32(init_pos, (B, D)), self._f32(init_vel, (B, D))
        it_t = None
        it_s = 0.0
        if isinstance(init_time, torch.Tensor) and init_time.dim() > 0:
            it_t = self._f32(init_time, (B,))
        else:
            it_s = float(init_time)
        if torch.is_grad_enabled() and (params.requires_grad or init_pos.requires_grad or init_vel.requires_grad):
            # differentiable: the same forward launch, and one mpk_trajectory_vjp launch as its backward (shared phase only)
            learned = bool(self.config.learn_tau or self.config.learn_delay)
            if phase_gradient == "pathwise" and (learned or it_t is not None):
                if self.mp_type == "dmp":
                    raise NotImplementedError("trajectory(phase_gradient='pathwise') is built for promp and prodmp: a DMP with a "
                                              "per-episode phase is an Euler recurrence in the scaled time, which has no adjoint kernel")
                return _TrajectoryPhaseFn.apply(self, it_t, it_s, out, params, init_pos, init_vel)
            if self.config.learn_tau or self.config.learn_delay:
                raise NotImplementedError("trajectory() is differentiable for a shared phase only: with a learned tau / delay the "
                                          "trajectory is not linear in those two parameters, and they are clipped to their bounds")
            if it_t is not None:
                raise NotImplementedError("trajectory() is differentiable for one init_time shared by the batch only: pass a float, "
                                          "not a per-episode tensor")
            return _TrajectoryFn.apply(self, it_s, out, params, init_pos, init_vel)
        return self._trajectory_launch(params, init_pos, init_vel, it_t, it_s, out)

    def _trajectory_launch(self, params, init_pos, init_vel, it_t, it_s, out):
        B, D, T = params.shape[0], self.num_dof, self.num_steps
        if out is None:
            pos = torch.empty((B, T, D), dtype=torch.float32, device=self.device)
            vel = torch.empty((B, T, D), dtype=torch.float32, device=self.device)
        else:
            pos, vel = out
        _lib.check(self._lib.mpk_trajectory(self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(),
                                            _dptr(it_t), it_s, pos.data_ptr(), vel.data_ptr(), B, self._stream()))
        return pos, vel

    def trajectory_vjp(self, g_pos: Optional[torch.Tensor], g_vel: Optional[torch.Tensor], init_time: float = 0.0, *,
                       need: Sequence[bool] = (True, True, True), out: Optional[Sequence[Optional[torch.Tensor]]] = None
                       ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``trajectory`` for a shared phase (mpk.h: mpk_trajectory_vjp), one launch: gradients of a loss
        w.r.t. pos / vel [B, T, D] (either may be None: that output did not reach the loss) -> (g_params [B, P], g_init_pos [B, D],
        g_init_vel [B, D]) float32 on the device.  ``need[i]`` False: that output is not computed (None is returned in its place);
        ``out``: buffers to write the needed ones into.  NotImplementedError for a learned tau / delay and for a DMP outside its
        response route.
        """
        ref = g_pos if g_pos is not None else g_vel
        if ref is None:
            raise ValueError("trajectory_vjp needs g_pos or g_vel")
        D, T = self.num_dof, self.num_steps
        B = ref.shape[0]
        gs = []
        for name, g in (("g_pos", g_pos), ("g_vel", g_vel)):
            if g is not None:
                g = torch.as_tensor(g, dtype=torch.float32, device=self.device)
                if g.shape != (B, T, D):
                    raise ValueError(f"{name} must be [{B}, {T}, {D}], got {tuple(g.shape)}")
                g = g.contiguous()
            gs.append(g)
        res = []
        for i, shape in enumerate(((B, self.num_params), (B, D), (B, D))):
            if not need[i]:
                res.append(None)
            elif out is not None and out[i] is not None:
                if out[i].shape != shape or out[i].dtype != torch.float32 or not out[i].is_contiguous() or out[i].device != self.device:
                    raise ValueError(f"out[{i}] must be a contiguous float32 tensor of shape {shape} on {self.device}")
                res.append(out[i])
            else:
                res.append(torch.empty(shape, dtype=torch.float32, device=self.device))
        _lib.check(self._lib.mpk_trajectory_vjp(self._h, _dptr(gs[0]), _dptr(gs[1]), float(init_time), _dptr(res[0]), _dptr(res[1]),
                                                _dptr(res[2]), B, self._stream()))
        return res[0], res[1], res[2]

    def trajectory_phase_vjp(self, params, init_pos, init_vel, g_pos: Optional[torch.Tensor], g_vel: Optional[torch.Tensor],
                             init_time=0.0, *, need: Sequence[bool] = (True, True, True),
                             out: Optional[Sequence[Optional[torch.Tensor]]] = None
                             ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``trajectory`` for a per-episode phase (mpk.h: mpk_trajectory_phase_vjp), one launch: the
        forward's own inputs (``init_time`` a float or a tensor [B]) and the gradients of a loss w.r.t. pos / vel [B, T, D] (either may
        be None) -> (g_params [B, P], g_init_pos [B, D], g_init_vel [B, D]) float32 on the device; ``need`` / ``out`` as
        ``trajectory_vjp``.  The convention is mpk.h's: a ProDMP's table indices held (g_delay = 0), torch.clamp's mask on tau /
        delay.  NotImplementedError: a DMP, a ProMP with one step, shapes beyond the forward's wave kernel.
        """
        ref = g_pos if g_pos is not None else g_vel
        if ref is None:
            raise ValueError("trajectory_phase_vjp needs g_pos or g_vel")
        D, T = self.num_dof, self.num_steps
        B = ref.shape[0]
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.detach().contiguous()
        if params.shape != (B, self.num_params):
            raise ValueError(f"params must be [{B}, {self.num_params}], got {tuple(params.shape)}")
        init_pos, init_vel = self._f32(init_pos, (B, D)).detach(), self._f32(init_vel, (B, D)).detach()
        it_t, it_s = None, 0.0
        if isinstance(init_time, torch.Tensor) and init_time.dim() > 0:
            it_t = self._f32(init_time, (B,))
        else:
            it_s = float(init_time)
        gs = []
        for name, g in (("g_pos", g_pos), ("g_vel", g_vel)):
            if g is not None:
                g = torch.as_tensor(g, dtype=torch.float32, device=self.device)
                if g.shape != (B, T, D):
                    raise ValueError(f"{name} must be [{B}, {T}, {D}], got {tuple(g.shape)}")
                g = g.contiguous()
            gs.append(g)
        res = []
        for i, shape in enumerate(((B, self.num_params), (B, D), (B, D))):
            if not need[i]:
                res.append(None)
            elif out is not None and out[i] is not None:
                if out[i].shape != shape or out[i].dtype != torch.float32 or not out[i].is_contiguous() or out[i].device != self.device:
                    raise ValueError(f"out[{i}] must be a contiguous float32 tensor of shape {shape} on {self.device}")
                res.append(out[i])
            else:
                res.append(torch.empty(shape, dtype=torch.float32, device=self.device))
        _lib.check(self._lib.mpk_trajectory_phase_vjp(self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), _dptr(it_t),
                                                      it_s, _dptr(gs[0]), _dptr(gs[1]), _dptr(res[0]), _dptr(res[1]), _dptr(res[2]), B,
                                                      self._stream()))
        return res[0], res[1], res[2]

    def fit_trajectory(self, pos, init_pos=None, init_vel=None, init_time=0.0, *, reg: float = 1e-9, phase_params=None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """
        The closed-form fit of the parameters to demonstrated positions (mpk.h: mpk_trajectory_fit), one launch: ``pos`` [B, T, D] ->
        ``params`` [B, P] float32 on the device, without an autograd graph.  For episode b the handle defines the affine map
        ``pos_b(p) = Psi p + c_b`` -- ``p`` the non-phase part of ``params`` in the user's units (scales, relative goal, zero padding,
        disable_* folded in as ``trajectory`` folds them), ``c_b`` what ``init_pos`` / ``init_vel`` / the goal offset contribute -- and
        the result is ``argmin_p |Psi p + c_b - pos_b|^2 + reg |p|^2``, solved per DoF in float64.  Positions only; ``reg`` is absolute
        and must be > 0.  This stands in for mp_pytorch's ``learn_mp_params_from_trajs`` on a batch: ``trajectory(fit_trajectory(y), ...)``
        is the best reproduction of ``y`` the handle has.

        ``init_pos`` / ``init_vel`` [B, D] are given, not fitted; None only for a ProMP (zeros).  ``init_time`` is one float for the
        batch.  A handle with a learned tau / delay, or an ``init_time`` tensor [B], gives every episode its own phase
        (mpk_trajectory_phase_fit, ProMP / ProDMP): each episode's tau / delay are inputs, ``phase_params`` [B, n_phase] in the order
        they have at the front of ``params``; they are clipped to the handle's bounds as ``trajectory`` clips them and come back
        unclipped at the front of the result.  There an episode whose Gram matrix plus ``reg`` I is not positive definite in float64
        gets a NaN row, and ``fit_status()`` says so.  ``phase_params`` on a shared-phase handle is a ValueError.  Every refusal is
        raised before any launch: ValueError for ``reg <= 0``, wrong shapes, a learned-phase handle without ``phase_params``,
        ``init_pos=None`` on a ProDMP / DMP; NotImplementedError for more than 16 DoF or 16 table columns, a DMP off its response
        route and a DMP with a per-episode phase.
        """
        reg = float(reg)
        if not (reg > 0.0) or not np.isfinite(reg):
            raise ValueError(f"fit_trajectory: reg must be a positive finite number, got {reg!r}")
        D, T, P = self.num_dof, self.num_steps, self.num_params
        shape = tuple(pos.shape) if hasattr(pos, "shape") else np.shape(pos)
        if len(shape) != 3 or shape[1:] != (T, D):
            raise ValueError(f"fit_trajectory: pos must be [B, {T}, {D}], got {shape}")
        B = shape[0]
        n_phase = int(bool(self.config.learn_tau)) + int(bool(self.config.learn_delay))
        per_episode_time = isinstance(init_time, torch.Tensor) and init_time.dim() > 0
        if n_phase and phase_params is None:
            raise ValueError("fit_trajectory: this handle learns " + " and ".join(
                n for n, on in (("tau", self.config.learn_tau), ("delay", self.config.learn_delay)) if on) +
                f": pass each episode's values as phase_params [{B}, {n_phase}] (they are inputs of the fit, not fitted)")
        if not n_phase and phase_params is not None:
            raise ValueError("fit_trajectory: phase_params given, but this handle has a shared phase (no learned tau / delay)")
        if (init_pos is None or init_vel is None) and self.mp_type != "promp":
            raise ValueError(f"fit_trajectory: init_pos / init_vel may be None only for a ProMP, which ignores them; a {self.mp_type} "
                             "starts from them")
        for name, x in (("init_pos", init_pos), ("init_vel", init_vel)):
            xs = None if x is None else (tuple(x.shape) if hasattr(x, "shape") else np.shape(x))
            if xs is not None and xs not in ((B, D), (D,)):
                raise ValueError(f"fit_trajectory: {name} must be [{B}, {D}], got {xs}")
        if out is not None and (tuple(out.shape) != (B, P) or out.dtype != torch.float32 or not out.is_contiguous()
                                or out.device != self.device):
            raise ValueError(f"fit_trajectory: out must be a contiguous float32 tensor of shape {(B, P)} on {self.device}")
        if phase_params is not None:
            ps = tuple(phase_params.shape) if hasattr(phase_params, "shape") else np.shape(phase_params)
            if ps != (B, n_phase):
                raise ValueError(f"fit_trajectory: phase_params must be [{B}, {n_phase}], got {ps}")
        if per_episode_time and tuple(init_time.shape) != (B,):
            raise ValueError(f"fit_trajectory: an init_time tensor must be [{B}], got {tuple(init_time.shape)}")
        if n_phase or per_episode_time:
            if self.mp_type == "dmp":
                raise NotImplementedError("fit_trajectory: a DMP with a per-episode phase is an Euler recurrence in the scaled time, "
                                          "which is not a table the fit could invert (promp / prodmp only)")
            with torch.no_grad():
                pos = torch.as_tensor(pos, dtype=torch.float32, device=self.device).detach().contiguous()
                ip = None if init_pos is None else self._f32(init_pos, (B, D)).detach()
                iv = None if init_vel is None else self._f32(init_vel, (B, D)).detach()
                ph = None if not n_phase else self._f32(phase_params, (B, n_phase)).detach()
                it_t = self._f32(init_time, (B,)) if per_episode_time else None
                params = out if out is not None else torch.empty((B, P), dtype=torch.float32, device=self.device)
                _lib.check(self._lib.mpk_trajectory_phase_fit(self._h, pos.data_ptr(), _dptr(ph), _dptr(ip), _dptr(iv), _dptr(it_t),
                                                              0.0 if per_episode_time else float(init_time), reg, params.data_ptr(),
                                                              B, self._stream()))
            return params
        with torch.no_grad():
            pos = torch.as_tensor(pos, dtype=torch.float32, device=self.device).detach().contiguous()
            ip = None if init_pos is None else self._f32(init_pos, (B, D)).detach()
            iv = None if init_vel is None else self._f32(init_vel, (B, D)).detach()
            params = out if out is not None else torch.empty((B, P), dtype=torch.float32, device=self.device)
            _lib.check(self._lib.mpk_trajectory_fit(self._h, pos.data_ptr(), _dptr(ip), _dptr(iv), None, float(init_time), reg,
                                                    params.data_ptr(), B, self._stream()))
        return params

    def fit_status(self) -> bool:
        """synchronise; True if an episode of the last per-episode-phase ``fit_trajectory`` launch had a Gram matrix that is not
        positive definite in float64 (its params row is NaN)"""
        flag = C.c_int32(0)
        _lib.check(self._lib.mpk_fit_status(self._h, C.byref(flag), self._stream()))
        return bool(flag.value)

    def _num_phase_params(self) -> int:
        return int(bool(self.config.learn_tau)) + int(bool(self.config.learn_delay))

    def trajectory_std(self, params_L, init_time: float = 0.0, *, pos: bool = True, vel: bool = True,
                       out: Optional[Sequence[Optional[torch.Tensor]]] = None
                       ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The trajectory's standard deviation under a Gaussian over the parameters (mpk.h: mpk_trajectory_std), one launch:
        ``params_L`` [B, Pl, Pl] -> ``(pos_std, vel_std)`` [B, T, D] float32 on the device, None for a disabled one, without an autograd
        graph.  ``params_L`` is the lower-triangular factor of the covariance of the non-phase parameters (Pl = ``num_params`` of a
        shared-phase handle), in the user's units and in the order they have in ``params`` -- a policy's ``scale_tril``; its strict
        upper triangle is never read.  ``pos_std[b, t, d]`` is the norm of the map's row times ``L_b`` (the factor form: non-negative
        by construction, exact zeros for ``L = 0``); ``init_pos`` / ``init_vel`` are deterministic and contribute nothing.  This stands
        in for mp_pytorch's ``get_traj_pos_std`` / ``get_traj_vel_std`` on a batch.  ``out``: a pair of buffers to write into (None for
        one to be allocated).  Every refusal is raised before any launch: ValueError for a shape other than [B, Pl, Pl], a wrong
        ``out``, ``pos = vel = False``; NotImplementedError for a handle that learns tau / delay, a DMP, and more than 16 DoF or 16
        table columns.
        """
        if not pos and not vel:
            raise ValueError("trajectory_std: pos and vel are both False: nothing to compute")
        if self.config.learn_tau or self.config.learn_delay:
            raise NotImplementedError("trajectory_std: a learned tau / delay gives every episode its own phase; only shared-phase "
                                      "handles have a standard-deviation kernel")
        if self.mp_type == "dmp":
            raise NotImplementedError("trajectory_std: a DMP has no probabilistic interface (promp / prodmp only)")
        D, T, Pl = self.num_dof, self.num_steps, self.num_params
        if D > 16:
            raise NotImplementedError(f"trajectory_std: at most 16 DoF and 16 table columns (this handle: {D} DoF)")
        shape = tuple(params_L.shape) if hasattr(params_L, "shape") else np.shape(params_L)
        if len(shape) != 3 or shape[0] < 1 or shape[1:] != (Pl, Pl):
            raise ValueError(f"trajectory_std: params_L must be [B, {Pl}, {Pl}] (the factor of the {Pl} non-phase parameters' covariance), "
                             f"got {shape}")
        B = shape[0]
        res = self._std_out_check("trajectory_std", out, pos, vel, B)
        with torch.no_grad():
            L = torch.as_tensor(params_L, dtype=torch.float32, device=self.device).detach().contiguous()
            res = [torch.empty((B, T, D), dtype=torch.float32, device=self.device) if r is False else r for r in res]
            _lib.check(self._lib.mpk_trajectory_std(self._h, L.data_ptr(), float(init_time), _dptr(res[0]), _dptr(res[1]), B,
                                                    self._stream()))
        return res[0], res[1]

    def _std_out_check(self, fn, out, pos, vel, B):
        """``out=(pos_std, vel_std)`` of the standard-deviation entry points: per array None (not wanted), the caller's buffer --
        contiguous float32 [B, T, D] on the device -- or False (to be allocated)"""
        D, T = self.num_dof, self.num_steps
        if out is not None and len(out) != 2:
            raise ValueError(f"{fn}: out must be a pair (pos_std, vel_std) of tensors or None")
        res = []
        for i, want in enumerate((pos, vel)):
            buf = out[i] if out is not None else None
            if not want:
                res.append(None)
            elif buf is not None:
                if tuple(buf.shape) != (B, T, D) or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != self.device:
                    raise ValueError(f"{fn}: out[{i}] must be a contiguous float32 tensor of shape {(B, T, D)} on {self.device}")
                res.append(buf)
            else:
                res.append(False)
        return res

    def trajectory_std_given_timing(self, params, params_L, init_time: float = 0.0, *, pos: bool = True, vel: bool = True,
                                    out: Optional[Sequence[Optional[torch.Tensor]]] = None
                                    ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        ``trajectory_std`` with every episode's timing GIVEN (mpk.h: mpk_trajectory_phase_std), for a handle that learns tau and / or
        delay, one launch: ``(pos_std, vel_std)`` [B, T, D] float32, None for a disabled one, each episode's band at its own tau /
        delay.  Of ``params`` [B, P] only the phase columns at the front are read (where ``trajectory`` reads them, clipped as it
        clips them); ``params_L`` [B, Pl, Pl] is the factor of the ``Pl = P - n_phase`` non-phase parameters' covariance.  The factor
        form on the episode's own float64 rows, ``| row tril(L) |``: ``L L^T`` is never formed, ``L = 0`` gives exact zeros, a
        rank-deficient covariance keeps its zeros, the strict upper triangle is never read.  ``init_time`` stays one float for the
        batch.  A ProDMP timing beyond the pre-computed range makes ``check_range`` raise.  Every refusal is raised before any
        launch: ValueError for a shared-phase handle (it has ``trajectory_std``), wrong shapes, a wrong ``out``, ``pos = vel =
        False``; NotImplementedError for a DMP and more than 16 DoF or 16 table columns.  Not built: gradients w.r.t. tau / delay,
        per-episode ``init_time`` tensors.
        """
        fn = "trajectory_std_given_timing"
        if not pos and not vel:
            raise ValueError(f"{fn}: pos and vel are both False: nothing to compute")
        self._timing_given(fn, "given")
        B = self._gaussian_checks(fn, "a standard-deviation kernel", params, params_L, self._num_phase_params())
        res = self._std_out_check(fn, out, pos, vel, B)
        with torch.no_grad():
            mean, L = self._mean_and_factor(params, params_L)
            res = [torch.empty((B, self.num_steps, self.num_dof), dtype=torch.float32, device=self.device) if r is False else r
                   for r in res]
            _lib.check(self._lib.mpk_trajectory_phase_std(self._h, mean.data_ptr(), L.data_ptr(), float(init_time), _dptr(res[0]),
                                                          _dptr(res[1]), B, self._stream()))
        return res[0], res[1]

    def condition(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None, init_vel=None,
                  init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None,
                  out: Optional[Sequence[torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        The Gaussian ``N(params, L L^T)`` over the parameters conditioned on observed trajectory points (mpk.h:
        mpk_trajectory_condition), one launch: ``(params_post, params_L_post)`` [B, P], [B, Pl, Pl] float32 on the device, without an
        autograd graph.  ``obs_steps``: a host sequence of M <= 32 strictly increasing step indices in [0, T), shared by the batch;
        ``obs_pos`` / ``obs_vel`` [B, M, D]: the observed positions / velocities at those steps (either may be None, not both);
        ``obs_std`` / ``obs_vel_std``: their standard deviations, a scalar, [M], [M, D] or [B, M, D], broadcast to [B, M, D].  A standard
        deviation of ``+inf`` (or NaN, or a negative one) skips that (episode, step, DoF) -- this is how some DoFs, or some episodes,
        only are observed -- and 0 is exact conditioning (more exact observations of a DoF than it has free parameters are the
        caller's error: unspecified, never a fault).  The update is sequential and in the factor form (float64, rounded once): the
        posterior factor is lower triangular with a non-negative diagonal and an exactly zero upper triangle, a valid ``scale_tril``
        even where the posterior covariance is singular; ``params_L``'s strict upper triangle is never read.  This stands in for
        conditioning an mp_pytorch ProMP on via-points, for a ProMP and a shared-phase ProDMP alike.  ``init_pos`` / ``init_vel``
        [B, D] are deterministic; None only for a ProMP (zeros).  ``out=(params, params_L)`` gives the in-place form (any pair of
        contiguous float32 buffers of the right shapes).  Every refusal is raised before any launch: ValueError for wrong shapes, no
        observation at all, values without standard deviations, bad steps, ``init_pos=None`` on a ProDMP; NotImplementedError for a
        handle that learns tau / delay, a DMP, more than 16 DoF or 16 table columns, and a Pl whose float64 triangle exceeds a CU's LDS.
        """
        return self._condition("condition", None, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time, obs_vel,
                               obs_vel_std, out)

    def condition_given_timing(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None, init_vel=None,
                               init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None,
                               out: Optional[Sequence[torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        ``condition`` with every episode's timing GIVEN (mpk.h: mpk_trajectory_phase_condition), for a handle that learns tau and / or
        delay, one launch: every episode is conditioned on the via-points at its own tau / delay, the values at the front of its
        ``params`` row (read where ``trajectory`` reads them, clipped to the handle's bounds as it clips them) -- a prior learned from
        demonstrations of different durations, conditioned at a new movement's speed.  The Gaussian is over the ``Pl = P - n_phase``
        non-phase parameters: ``params_L`` and the returned factor are [B, Pl, Pl]; the phase columns of the posterior ``params`` are
        the inputs' bits, unclipped.  Every convention is ``condition``'s: at most 32 shared, strictly increasing steps; the order
        steps ascending, positions by DoF, then velocities by DoF; ``sigma = 0`` conditions exactly; ``+inf``, NaN or a negative one
        skips the entry bit for bit; the factor form in float64, rounded once; exact zeros in the strict upper triangle, which is
        never read on input; ``out=(params, params_L)`` gives the in-place form.  The rows are the episode's own, in float64: an
        observed velocity is the velocity ``trajectory`` returns for that episode at that step.  ``init_time`` stays one float for the
        batch.  A ProDMP timing beyond the pre-computed range makes ``check_range`` raise.  A shared-phase handle is a ValueError (it
        has ``condition``); a ``params_L`` that is not [B, Pl, Pl] is a ValueError that names Pl; the other refusals are
        ``condition``'s, all before any launch.  Not built: gradients w.r.t. tau / delay, per-episode ``init_time`` tensors, DMP,
        correlated noise.
        """
        return self._condition("condition_given_timing", "given", params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel,
                               init_time, obs_vel, obs_vel_std, out)

    def _condition(self, fn, timing, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time, obs_vel, obs_vel_std,
                   out):
        phase = self._timing_given(fn, timing)
        n_phase = self._num_phase_params() if phase else 0
        B, steps = self._obs_checks(fn, "a conditioning kernel", params, params_L, obs_steps, obs_pos, obs_std, init_pos,
                                    init_vel, obs_vel, obs_vel_std, n_phase)
        P, M = self.num_params, int(steps.size)
        self._out_pair_check(fn, out, B, P, P - n_phase)
        ip, iv, yp, sp, yv, sv = self._log_prob_inputs(fn, B, M, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std)
        with torch.no_grad():
            mean, L = self._mean_and_factor(params, params_L)
            mean_out, L_out = out if out is not None else self._posterior_buffers(B, P, P - n_phase)
            entry = self._lib.mpk_trajectory_phase_condition if phase else self._lib.mpk_trajectory_condition
            _lib.check(entry(
                self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time),
                steps.ctypes.data_as(C.POINTER(C.c_int32)), M, _dptr(yp), _dptr(sp), _dptr(yv), _dptr(sv), mean_out.data_ptr(),
                L_out.data_ptr(), B, self._stream()))
        return mean_out, L_out

    def _obs_checks(self, fn, kernel, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std,
                    n_phase=0):
        """the refusals ``condition`` and ``trajectory_log_prob`` / ``_vjp`` share, all before anything touches the device (what only
        the library can judge -- the steps' range and order -- is refused by the launch's own checks, still before any launch);
        ``n_phase``: of the ``_given_timing`` methods (``_gaussian_checks``); returns (B, steps int32 [M])"""
        B = self._gaussian_checks(fn, kernel, params, params_L, n_phase)
        steps = np.asarray(list(obs_steps))
        if steps.ndim != 1 or (steps.size and not np.issubdtype(steps.dtype, np.integer)):
            raise ValueError(f"{fn}: obs_steps must be a sequence of ints, got {obs_steps!r}")
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        if obs_pos is None and obs_vel is None:
            raise ValueError(f"{fn}: obs_pos and obs_vel are both None: nothing is observed")
        for val, sd, names in ((obs_pos, obs_std, ("obs_pos", "obs_std")), (obs_vel, obs_vel_std, ("obs_vel", "obs_vel_std"))):
            if (val is None) != (sd is None):
                raise ValueError(f"{fn}: {names[0]} and {names[1]} come in pairs (observed values with their standard deviations)")
        self._start_check(fn, init_pos, init_vel)
        return B, steps

    def _gaussian_checks(self, fn, kernel, params, params_L, n_phase):
        """what every entry point that takes ``N(params, L L^T)`` refuses about the handle and the Gaussian's shape; returns B.
        ``n_phase`` = 0: the shared-phase route, a Gaussian over all P parameters (a learned tau / delay is refused; ``kernel``: the
        family's word); otherwise ``timing="given"``: over the Pl = P - n_phase non-phase parameters"""
        if not n_phase and (self.config.learn_tau or self.config.learn_delay):
            raise NotImplementedError(f"{fn}: a learned tau / delay gives every episode its own phase; only shared-phase handles have "
                                      f"{kernel}")
        if self.mp_type == "dmp":
            raise NotImplementedError(f"{fn}: a DMP has no probabilistic interface (promp / prodmp only)")
        D, P = self.num_dof, self.num_params
        Pl = P - n_phase
        if D > 16:
            raise NotImplementedError(f"{fn}: at most 16 DoF and 16 table columns (this handle: {D} DoF)")
        pshape = tuple(params.shape) if hasattr(params, "shape") else np.shape(params)
        if len(pshape) != 2 or pshape[0] < 1 or pshape[1] != P:
            raise ValueError(f"{fn}: params must be [B, {P}]" + (" (tau / delay in front, then the mean)" if n_phase else "") +
                             f", got {pshape}")
        B = pshape[0]
        lshape = tuple(params_L.shape) if hasattr(params_L, "shape") else np.shape(params_L)
        if lshape != (B, Pl, Pl):
            if n_phase:
                raise ValueError(f"{fn}: params_L must be [{B}, Pl, Pl] with Pl = {Pl} (the factor of the {Pl} non-phase parameters' "
                                 f"covariance; the timing is given, not distributed), got {lshape}")
            raise ValueError(f"{fn}: params_L must be [{B}, {P}, {P}] (the factor of the {P} non-phase parameters' covariance), "
                             f"got {lshape}")
        return B

    def _start_check(self, fn, init_pos, init_vel):
        if (init_pos is None or init_vel is None) and self.mp_type != "promp":
            raise ValueError(f"{fn}: init_pos / init_vel may be None only for a ProMP, which ignores them; a {self.mp_type} starts from "
                             "them")

    def _no_grad_check(self, fn, named):
        """the likelihood's inputs that have no gradient: (name, value) pairs, refused where a tensor among them requires grad"""
        if torch.is_grad_enabled():
            for name, t in named:
                if isinstance(t, torch.Tensor) and t.requires_grad:
                    raise NotImplementedError(f"{fn}: {name} requires grad, but the likelihood has a gradient w.r.t. params and params_L "
                                              "only; detach it")

    def _out_pair_check(self, fn, out, B, P, Pl):
        """``out=(params, params_L)`` of the conditioning entry points: None, or contiguous float32 [B, P] and [B, Pl, Pl] on the device"""
        if out is None:
            return
        if len(out) != 2:
            raise ValueError(f"{fn}: out must be a pair (params, params_L) of tensors")
        for i, (buf, shape) in enumerate(zip(out, ((B, P), (B, Pl, Pl)))):
            if (not isinstance(buf, torch.Tensor) or tuple(buf.shape) != shape or buf.dtype != torch.float32
                    or not buf.is_contiguous() or buf.device != self.device):
                raise ValueError(f"{fn}: out[{i}] must be a contiguous float32 tensor of shape {shape} on {self.device}")

    def _posterior_buffers(self, B, P, Pl):
        return (torch.empty((B, P), dtype=torch.float32, device=self.device),
                torch.empty((B, Pl, Pl), dtype=torch.float32, device=self.device))

    def _mean_and_factor(self, params, params_L):
        """the Gaussian's mean and factor as detached contiguous float32 device tensors"""
        return (torch.as_tensor(params, dtype=torch.float32, device=self.device).detach().contiguous(),
                torch.as_tensor(params_L, dtype=torch.float32, device=self.device).detach().contiguous())

    def _vjp_outputs(self, fn, g, mean, L, need):
        """the gradient launches' ``g`` as contiguous float64 [B] and their output buffers (None where ``need[i]`` is False), or None
        when no output is asked for"""
        B = mean.shape[0]
        g = torch.as_tensor(g, dtype=torch.float64, device=self.device).detach()
        if tuple(g.shape) != (B,):
            raise ValueError(f"{fn}: g must be [{B}], got {tuple(g.shape)}")
        g_mean = torch.empty_like(mean) if need[0] else None
        g_L = torch.empty_like(L) if need[1] else None
        return None if g_mean is None and g_L is None else (g.contiguous(), g_mean, g_L)

    def _log_prob_checks(self, fn, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std, n_phase=0):
        """the refusals of ``trajectory_log_prob`` / ``trajectory_log_prob_vjp`` -- ``condition``'s, plus the steps (here, so that no
        refusal needs the handle), the observation count and the inputs that have no gradient; returns (B, steps int32 [M])"""
        B, steps = self._obs_checks(fn, "a likelihood kernel", params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, obs_vel,
                                    obs_vel_std, n_phase)
        D = self.num_dof
        if not 1 <= steps.size <= 32:
            raise ValueError(f"{fn}: M must be 1..32 observed steps, got {steps.size}")
        if steps[0] < 0 or steps[-1] >= self.num_steps or (np.diff(steps) <= 0).any():
            raise ValueError(f"{fn}: obs_steps must be strictly increasing step indices in [0, {self.num_steps}), got "
                             f"{steps.tolist()}")
        n_obs = int(steps.size) * D * ((obs_pos is not None) + (obs_vel is not None))
        if n_obs > _lib.MPK_LOGPROB_MAX_OBS:
            raise NotImplementedError(f"{fn}: at most {_lib.MPK_LOGPROB_MAX_OBS} scalar observations per episode (steps x DoF x the "
                                      f"observation arrays given = {n_obs}); the whole-trajectory likelihood has no kernel here")
        self._no_grad_check(fn, (("init_pos", init_pos), ("init_vel", init_vel), ("obs_pos", obs_pos), ("obs_std", obs_std),
                                 ("obs_vel", obs_vel), ("obs_vel_std", obs_vel_std)))
        return B, steps

    def _obs_bcast(self, fn, x, name, B, M):
        """observed values or standard deviations -- a scalar, [M], [M, D] or [B, M, D] -- as a contiguous float32 [B, M, D] on the device"""
        t = torch.as_tensor(x, dtype=torch.float32, device=self.device).detach()
        if t.dim() == 1 and t.shape[0] == M:                        # [M]: one value per step
            t = t[:, None]
        try:
            return t.expand((B, M, self.num_dof)).contiguous()
        except RuntimeError:
            raise ValueError(f"{fn}: {name} does not broadcast to [{B}, {M}, {self.num_dof}], got {tuple(t.shape)}") from None

    def _log_prob_inputs(self, fn, B, M, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std):
        """(init_pos, init_vel, obs_pos, obs_std, obs_vel, obs_vel_std) as contiguous float32 device tensors or None, the standard
        deviations broadcast to [B, M, D] as ``condition`` broadcasts them"""
        D = self.num_dof

        def bcast(x, name):
            return self._obs_bcast(fn, x, name, B, M)
        with torch.no_grad():
            return (None if init_pos is None else self._f32(init_pos, (B, D)).detach(),
                    None if init_vel is None else self._f32(init_vel, (B, D)).detach(),
                    None if obs_pos is None else bcast(obs_pos, "obs_pos"), None if obs_pos is None else bcast(obs_std, "obs_std"),
                    None if obs_vel is None else bcast(obs_vel, "obs_vel"),
                    None if obs_vel is None else bcast(obs_vel_std, "obs_vel_std"))

    def _log_prob_launch(self, mean, L, steps, inputs, init_time, phase=False):
        ip, iv, yp, sp, yv, sv = inputs
        out = torch.empty((mean.shape[0],), dtype=torch.float64, device=self.device)
        entry = self._lib.mpk_trajectory_phase_log_prob if phase else self._lib.mpk_trajectory_log_prob
        _lib.check(entry(
            self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time), steps.ctypes.data_as(C.POINTER(C.c_int32)),
            int(steps.size), _dptr(yp), _dptr(sp), _dptr(yv), _dptr(sv), out.data_ptr(), mean.shape[0], self._stream()))
        return out

    def _log_prob_vjp_launch(self, g, mean, L, steps, inputs, init_time, need, phase=False):
        ip, iv, yp, sp, yv, sv = inputs
        outs = self._vjp_outputs("trajectory_log_prob_vjp_given_timing" if phase else "trajectory_log_prob_vjp", g, mean, L, need)
        if outs is None:
            return None, None
        g, g_mean, g_L = outs
        entry = self._lib.mpk_trajectory_phase_log_prob_vjp if phase else self._lib.mpk_trajectory_log_prob_vjp
        _lib.check(entry(
            self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time), steps.ctypes.data_as(C.POINTER(C.c_int32)),
            int(steps.size), _dptr(yp), _dptr(sp), _dptr(yv), _dptr(sv), g.data_ptr(), _dptr(g_mean), _dptr(g_L), mean.shape[0],
            self._stream()))
        return g_mean, g_L

    def trajectory_log_prob(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None, init_vel=None,
                            init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None) -> torch.Tensor:
        """
        The log-likelihood of observed trajectory points under the Gaussian ``N(params, L L^T)`` over the parameters (mpk.h:
        mpk_trajectory_log_prob), one launch: [B] float64 on the device.  The observations are ``condition``'s, argument by argument:
        ``obs_steps`` a host sequence of strictly increasing step indices shared by the batch, ``obs_pos`` / ``obs_vel`` [B, M, D] with
        ``obs_std`` / ``obs_vel_std`` (a scalar, [M], [M, D] or [B, M, D]); a standard deviation of ``+inf``, NaN or a negative one
        removes that (episode, step, DoF).  With the n that remain, ``log N(y; H mu + c, A A^T + diag(sigma^2))``, ``A = H tril(L)``, by
        a dense float64 Cholesky factorisation of the n x n covariance: n = 0 gives exactly 0.0, a singular covariance gives NaN for that
        episode alone.  At most 64 scalar observations per episode (steps x DoF x arrays given).  When ``params`` or ``params_L``
        requires grad the result carries the autograd graph: its backward is ONE mpk_trajectory_log_prob_vjp launch, which recomputes
        the factorisation from the inputs; a mean or factor expanded from one shared row gets the sum over the batch through torch as
        usual.  There is no gradient w.r.t. ``init_pos``, ``init_vel`` or the observations: a tensor among them that requires grad is
        a NotImplementedError, not a silent cut.  ``params_L``'s strict upper triangle is never read.  Refusals are ``condition``'s,
        raised before any launch, plus NotImplementedError for more than 64 observations.
        """
        return self._trajectory_log_prob("trajectory_log_prob", None, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel,
                                         init_time, obs_vel, obs_vel_std)

    def trajectory_log_prob_given_timing(self, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None, init_vel=None,
                                         init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None) -> torch.Tensor:
        """
        ``trajectory_log_prob`` with every episode's timing GIVEN (mpk.h: mpk_trajectory_phase_log_prob), for a handle that learns tau
        and / or delay, one launch: [B] float64, the observed points of episode b scored at its own tau / delay, the values at the
        front of its ``params`` row (clipped as ``trajectory`` clips them).  The Gaussian is over the ``Pl = P - n_phase`` non-phase
        parameters, ``params[b, n_phase:]`` its mean and ``params_L`` [B, Pl, Pl] its factor.  Everything else is
        ``trajectory_log_prob``'s: at most 64 scalar observations per episode, exactly 0.0 for none kept, NaN for a singular
        covariance in that episode alone, autograd with ONE backward launch (mpk_trajectory_phase_log_prob_vjp), a tensor among the
        observations or initial conditions that requires grad refused.  Timing is an input, not a random variable: the phase columns
        of ``params.grad`` are exact zeros (no gradient w.r.t. tau / delay is built).  ``init_time`` stays one float for the batch.  A
        shared-phase handle is a ValueError (it has ``trajectory_log_prob``); the other refusals are ``trajectory_log_prob``'s, all
        before any launch.
        """
        return self._trajectory_log_prob("trajectory_log_prob_given_timing", "given", params, params_L, obs_steps, obs_pos, obs_std,
                                         init_pos, init_vel, init_time, obs_vel, obs_vel_std)

    def _trajectory_log_prob(self, fn, timing, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time, obs_vel,
                             obs_vel_std):
        phase = self._timing_given(fn, timing)
        B, steps = self._log_prob_checks(fn, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std,
                                         self._num_phase_params() if phase else 0)
        inputs = self._log_prob_inputs(fn, B, int(steps.size), obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std)
        mean = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        L = torch.as_tensor(params_L, dtype=torch.float32, device=self.device)
        if torch.is_grad_enabled() and (mean.requires_grad or L.requires_grad):
            return _TrajectoryLogProbFn.apply(self, steps, inputs, float(init_time), mean.contiguous(), L.contiguous(), phase)
        return self._log_prob_launch(mean.detach().contiguous(), L.detach().contiguous(), steps, inputs, init_time, phase)

    def trajectory_log_prob_vjp(self, g, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None, init_vel=None,
                                init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None,
                                need: Sequence[bool] = (True, True)) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``trajectory_log_prob`` (mpk.h: mpk_trajectory_log_prob_vjp), one launch: ``g`` [B] float64, the
        gradient of a loss w.r.t. the log-likelihoods -> ``(g_params [B, P], g_params_L [B, Pl, Pl])`` float32 on the device, without
        an autograd graph.  The other arguments are ``trajectory_log_prob``'s.  ``g_params_L``'s strict upper triangle is exact zeros,
        and so are the rows of a DoF none of whose observations remain; an episode whose covariance is singular gets NaN rows.
        ``need[i]`` False: that output is not computed (None in its place).
        """
        return self._trajectory_log_prob_vjp("trajectory_log_prob_vjp", None, g, params, params_L, obs_steps, obs_pos, obs_std, init_pos,
                                             init_vel, init_time, obs_vel, obs_vel_std, need)

    def trajectory_log_prob_vjp_given_timing(self, g, params, params_L, obs_steps, obs_pos=None, obs_std=None, init_pos=None,
                                             init_vel=None, init_time: float = 0.0, *, obs_vel=None, obs_vel_std=None,
                                             need: Sequence[bool] = (True, True)
                                             ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``trajectory_log_prob_given_timing`` (mpk.h: mpk_trajectory_phase_log_prob_vjp), one launch:
        ``(g_params [B, P], g_params_L [B, Pl, Pl])`` as ``trajectory_log_prob_vjp`` returns them, with ``Pl = P - n_phase``.  The
        phase columns of ``g_params`` are exact zeros: the likelihood is differentiated at the given timing.
        """
        return self._trajectory_log_prob_vjp("trajectory_log_prob_vjp_given_timing", "given", g, params, params_L, obs_steps, obs_pos,
                                             obs_std, init_pos, init_vel, init_time, obs_vel, obs_vel_std, need)

    def _trajectory_log_prob_vjp(self, fn, timing, g, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time,
                                 obs_vel, obs_vel_std, need):
        phase = self._timing_given(fn, timing)
        B, steps = self._log_prob_checks(fn, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std,
                                         self._num_phase_params() if phase else 0)
        inputs = self._log_prob_inputs(fn, B, int(steps.size), obs_pos, obs_std, init_pos, init_vel, obs_vel, obs_vel_std)
        with torch.no_grad():
            mean, L = self._mean_and_factor(params, params_L)
            return self._log_prob_vjp_launch(g, mean, L, steps, inputs, init_time, need, phase)

    def _timing_given(self, fn, timing) -> bool:
        """``timing=None | "given"`` of the demonstration entry points: True for the per-episode-phase route"""
        if timing is None:
            return False
        if timing != "given":
            raise ValueError(f"{fn}: timing must be None or \"given\" (the tau / delay at the front of every params row are that "
                             f"episode's own), got {timing!r}")
        if not (self.config.learn_tau or self.config.learn_delay):
            raise ValueError(f"{fn}: timing=\"given\" on a handle that learns neither tau nor delay: every episode has the handle's phase "
                             "already; call without timing")
        return True

    def _demo_checks(self, fn, params, params_L, pos, obs_std, init_pos, init_vel, phase=False):
        """the refusals of ``demonstration_log_prob`` / ``demonstration_log_prob_vjp`` -- ``trajectory_log_prob``'s (for
        ``timing="given"`` with the Gaussian over the Pl = P - n_phase non-phase parameters) plus the demonstrations' shape and the
        inputs that have no gradient, all before anything touches the device; returns B"""
        if pos is None or obs_std is None:
            raise ValueError(f"{fn}: pos and obs_std are both required (the demonstrations with their standard deviations)")
        B = self._gaussian_checks(fn, "a likelihood kernel", params, params_L, self._num_phase_params() if phase else 0)
        self._start_check(fn, init_pos, init_vel)
        T, D = self.num_steps, self.num_dof
        shape = tuple(pos.shape) if hasattr(pos, "shape") else np.shape(pos)
        if shape != (B, T, D):
            raise ValueError(f"{fn}: pos must be [{B}, {T}, {D}] (whole demonstrations on the handle's {T} steps), got {shape}")
        self._no_grad_check(fn, (("init_pos", init_pos), ("init_vel", init_vel), ("pos", pos), ("obs_std", obs_std)))
        return B

    def _demo_inputs(self, fn, B, pos, obs_std, init_pos, init_vel):
        """(init_pos, init_vel, pos, obs_std) as contiguous float32 device tensors (the first two or None), obs_std broadcast to
        [B, T, D] as ``condition`` broadcasts its standard deviations"""
        D, T = self.num_dof, self.num_steps
        with torch.no_grad():
            return (None if init_pos is None else self._f32(init_pos, (B, D)).detach(),
                    None if init_vel is None else self._f32(init_vel, (B, D)).detach(),
                    self._f32(pos, (B, T, D)).detach(), self._obs_bcast(fn, obs_std, "obs_std", B, T))

    def _demo_log_prob_launch(self, mean, L, inputs, init_time, phase=False):
        ip, iv, y, sd = inputs
        out = torch.empty((mean.shape[0],), dtype=torch.float64, device=self.device)
        entry = self._lib.mpk_demonstration_phase_log_prob if phase else self._lib.mpk_demonstration_log_prob
        _lib.check(entry(
            self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time), y.data_ptr(), sd.data_ptr(), out.data_ptr(),
            mean.shape[0], self._stream()))
        return out

    def _demo_log_prob_vjp_launch(self, g, mean, L, inputs, init_time, need, phase=False):
        ip, iv, y, sd = inputs
        outs = self._vjp_outputs("demonstration_log_prob_vjp", g, mean, L, need)
        if outs is None:
            return None, None
        g, g_mean, g_L = outs
        entry = self._lib.mpk_demonstration_phase_log_prob_vjp if phase else self._lib.mpk_demonstration_log_prob_vjp
        _lib.check(entry(
            self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time), y.data_ptr(), sd.data_ptr(), g.data_ptr(),
            _dptr(g_mean), _dptr(g_L), mean.shape[0], self._stream()))
        return g_mean, g_L

    def demonstration_log_prob(self, params, params_L, pos, obs_std, init_pos=None, init_vel=None,
                               init_time: float = 0.0) -> torch.Tensor:
        """
        The log-likelihood of WHOLE demonstrations under the Gaussian ``N(params, L L^T)`` over the parameters (mpk.h:
        mpk_demonstration_log_prob), one launch: [B] float64 on the device.  ``pos`` [B, T, D]: the demonstrated positions on the
        handle's own T steps; ``obs_std`` a scalar, [D], [T, D] or [B, T, D].  An entry is kept when ``0 < sigma < inf``: ``+inf``,
        NaN or a negative one removes that (episode, step, DoF) -- missing samples, or a prefix of the movement.  Every kept entry is
        an observation of ``trajectory_log_prob``'s kind, ``log N(y; H mu + c, A A^T + diag(sigma^2))``, but evaluated in the
        information form: the Gram matrices of the basis per DoF and the Cholesky factor of the ``Pl x Pl`` matrix
        ``I + tril(L)^T G tril(L)``, all float64 -- ``T D`` may be in the thousands.  No entry kept gives exactly 0.0.  ``sigma == 0``
        cannot be expressed in this form: that episode is NaN (use ``trajectory_log_prob`` for exact observations).  When ``params``
        or ``params_L`` requires grad the result carries the autograd graph: its backward is ONE mpk_demonstration_log_prob_vjp
        launch, which recomputes everything from the inputs; a mean or factor expanded from one shared row gets the sum over the
        batch through torch as usual.  There is no gradient w.r.t. ``pos``, ``obs_std``, ``init_pos`` or ``init_vel``: a tensor among
        them that requires grad is a NotImplementedError, not a silent cut.  ``params_L``'s strict upper triangle is never read.
        Refusals are ``trajectory_log_prob``'s, raised before any launch (shapes, a learned tau / delay, a DMP, more than 16 DoF,
        ``init_pos`` / ``init_vel`` None on a ProDMP), plus ValueError for a ``pos`` that is not [B, T, D] with T the handle's steps.
        A handle that learns tau / delay refuses here; ``demonstration_log_prob_given_timing`` is its entry point.
        """
        return self._demonstration_log_prob("demonstration_log_prob", None, params, params_L, pos, obs_std, init_pos, init_vel, init_time)

    def demonstration_log_prob_given_timing(self, params, params_L, pos, obs_std, init_pos=None, init_vel=None,
                                            init_time: float = 0.0) -> torch.Tensor:
        """
        ``demonstration_log_prob`` with every episode's timing GIVEN (mpk.h: mpk_demonstration_phase_log_prob), for a handle that
        learns tau and / or delay, one launch: the tau / delay of episode b are the values at the front of its ``params`` row,
        exactly where ``trajectory`` reads them and clipped to the handle's bounds as it clips them -- demonstrations of different
        durations, each scored at its own timing.  They are given, not distributed: the Gaussian is over the ``Pl = P - n_phase``
        non-phase parameters, ``params[b, n_phase:]`` its mean and ``params_L`` [B, Pl, Pl] its factor.  Everything else is
        ``demonstration_log_prob``'s: the rule for kept entries, 0.0 for nothing kept, NaN for a ``sigma == 0``, autograd with ONE
        backward launch (mpk_demonstration_phase_log_prob_vjp).  Timing is an input, not a random variable: the phase columns of
        ``params.grad`` are exact zeros (no gradient w.r.t. tau / delay is built).  ``init_time`` stays one float for the batch.  A
        ProDMP timing beyond the pre-computed range makes ``check_range`` raise.  A shared-phase handle is a ValueError (it has
        ``demonstration_log_prob``); a ``params_L`` that is not [B, Pl, Pl] is a ValueError that names Pl; the other refusals are
        ``demonstration_log_prob``'s, all before any launch.
        """
        return self._demonstration_log_prob("demonstration_log_prob_given_timing", "given", params, params_L, pos, obs_std, init_pos,
                                            init_vel, init_time)

    def _demonstration_log_prob(self, fn, timing, params, params_L, pos, obs_std, init_pos, init_vel, init_time):
        phase = self._timing_given(fn, timing)
        B = self._demo_checks(fn, params, params_L, pos, obs_std, init_pos, init_vel, phase)
        inputs = self._demo_inputs(fn, B, pos, obs_std, init_pos, init_vel)
        mean = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        L = torch.as_tensor(params_L, dtype=torch.float32, device=self.device)
        if torch.is_grad_enabled() and (mean.requires_grad or L.requires_grad):
            return _DemonstrationLogProbFn.apply(self, inputs, float(init_time), mean.contiguous(), L.contiguous(), phase)
        return self._demo_log_prob_launch(mean.detach().contiguous(), L.detach().contiguous(), inputs, init_time, phase)

    def demonstration_log_prob_vjp(self, g, params, params_L, pos, obs_std, init_pos=None, init_vel=None, init_time: float = 0.0, *,
                                   need: Sequence[bool] = (True, True)) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``demonstration_log_prob`` (mpk.h: mpk_demonstration_log_prob_vjp), one launch: ``g`` [B]
        float64, the gradient of a loss w.r.t. the log-likelihoods -> ``(g_params [B, P], g_params_L [B, Pl, Pl])`` float32 on the
        device, without an autograd graph.  The other arguments are ``demonstration_log_prob``'s.  ``g_params_L``'s strict upper
        triangle is exact zeros, and so are the rows of a DoF none of whose entries remain; an episode with a ``sigma == 0`` gets NaN
        rows (use ``trajectory_log_prob`` for exact observations).  ``need[i]`` False: that output is not computed (None in its place).
        """
        return self._demonstration_log_prob_vjp("demonstration_log_prob_vjp", None, g, params, params_L, pos, obs_std, init_pos, init_vel,
                                                init_time, need)

    def demonstration_log_prob_vjp_given_timing(self, g, params, params_L, pos, obs_std, init_pos=None, init_vel=None,
                                                init_time: float = 0.0, *, need: Sequence[bool] = (True, True)
                                                ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        The vector-Jacobian product of ``demonstration_log_prob_given_timing`` (mpk.h: mpk_demonstration_phase_log_prob_vjp), one
        launch: ``(g_params [B, P], g_params_L [B, Pl, Pl])`` as ``demonstration_log_prob_vjp`` returns them, with ``Pl = P - n_phase``.
        The phase columns of ``g_params`` are exact zeros: the likelihood is differentiated at the given timing.
        """
        return self._demonstration_log_prob_vjp("demonstration_log_prob_vjp_given_timing", "given", g, params, params_L, pos, obs_std,
                                                init_pos, init_vel, init_time, need)

    def _demonstration_log_prob_vjp(self, fn, timing, g, params, params_L, pos, obs_std, init_pos, init_vel, init_time, need):
        phase = self._timing_given(fn, timing)
        B = self._demo_checks(fn, params, params_L, pos, obs_std, init_pos, init_vel, phase)
        inputs = self._demo_inputs(fn, B, pos, obs_std, init_pos, init_vel)
        with torch.no_grad():
            mean, L = self._mean_and_factor(params, params_L)
            return self._demo_log_prob_vjp_launch(g, mean, L, inputs, init_time, need, phase)

    def condition_on_demonstration(self, params, params_L, pos, obs_std, init_pos=None, init_vel=None, init_time: float = 0.0, *,
                                   out: Optional[Sequence[torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        The Gaussian ``N(params, L L^T)`` over the parameters conditioned on WHOLE demonstrations (mpk.h:
        mpk_demonstration_condition), one launch: ``(params_post, params_L_post)`` [B, P], [B, Pl, Pl] float32 on the device, without
        an autograd graph.  ``pos`` [B, T, D] and ``obs_std`` (a scalar, [D], [T, D] or [B, T, D]) are ``demonstration_log_prob``'s: an
        entry is kept when ``0 < sigma < inf``, so an observed prefix of a movement is the rest at ``inf`` and missing samples are
        ``inf`` one by one.  This is the information form of that likelihood -- the Gram matrices of the basis per DoF, the ``Pl x Pl``
        matrix ``M = I + tril(L)^T G tril(L)`` factored from its last row, ``L' = tril(L) K^-1`` -- where ``condition`` applies at most
        32 shared steps one scalar at a time: T D may be in the thousands.  The posterior factor is lower triangular with a
        non-negative diagonal and an exactly zero upper triangle, a valid ``scale_tril``; ``params_L``'s strict upper triangle is never
        read.  No entry kept returns the prior bit for bit.  ``sigma == 0`` cannot be expressed in this form: that episode's mean and
        the lower triangle of its factor are NaN (``condition`` takes exact observations); non-finite inputs do the same and stay
        inside their episode.  ``out=(params, params_L)`` gives the in-place form, validated as ``condition`` validates it.  A
        ``params`` or ``params_L`` that requires grad is detached: there is no gradient through the posterior.  Refusals are
        ``demonstration_log_prob``'s, raised before any launch.  A handle that learns tau / delay refuses here;
        ``condition_on_demonstration_given_timing`` is its entry point.
        """
        return self._condition_on_demonstration("condition_on_demonstration", None, params, params_L, pos, obs_std, init_pos, init_vel,
                                                init_time, out)

    def condition_on_demonstration_given_timing(self, params, params_L, pos, obs_std, init_pos=None, init_vel=None,
                                                init_time: float = 0.0, *,
                                                out: Optional[Sequence[torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        ``condition_on_demonstration`` with every episode's timing GIVEN (mpk.h: mpk_demonstration_phase_condition), for a handle that
        learns tau and / or delay, one launch: every episode is conditioned at its own tau / delay, the values at the front of its
        ``params`` row (clipped to the handle's bounds as ``trajectory`` clips them) -- the E-step of EM over demonstrations of
        different durations, prediction from a prefix at the movement's own speed.  The Gaussian is over the ``Pl = P - n_phase``
        non-phase parameters: ``params_L`` and the returned factor are [B, Pl, Pl]; the phase columns of the posterior ``params``
        are the inputs' bits, unclipped.  ``out=(params, params_L)`` gives the in-place form.  Refusals are
        ``demonstration_log_prob_given_timing``'s, raised before any launch.
        """
        return self._condition_on_demonstration("condition_on_demonstration_given_timing", "given", params, params_L, pos, obs_std,
                                                init_pos, init_vel, init_time, out)

    def _condition_on_demonstration(self, fn, timing, params, params_L, pos, obs_std, init_pos, init_vel, init_time, out):
        phase = self._timing_given(fn, timing)
        with torch.no_grad():                                       # (nothing here has a gradient: _demo_checks need not refuse one)
            B = self._demo_checks(fn, params, params_L, pos, obs_std, init_pos, init_vel, phase)
        P = self.num_params
        Pl = P - self._num_phase_params() if phase else P
        self._out_pair_check(fn, out, B, P, Pl)
        ip, iv, y, sd = self._demo_inputs(fn, B, pos, obs_std, init_pos, init_vel)
        with torch.no_grad():
            mean, L = self._mean_and_factor(params, params_L)
            mean_out, L_out = out if out is not None else self._posterior_buffers(B, P, Pl)
            entry = self._lib.mpk_demonstration_phase_condition if phase else self._lib.mpk_demonstration_condition
            _lib.check(entry(
                self._h, mean.data_ptr(), L.data_ptr(), _dptr(ip), _dptr(iv), float(init_time), y.data_ptr(), sd.data_ptr(),
                mean_out.data_ptr(), L_out.data_ptr(), B, self._stream()))
        return mean_out, L_out

    def condition_on_demonstration_plan(self, B: int, *, timing: Optional[str] = None) -> Tuple[int, int, int]:
        """``(workgroups, waves per workgroup, LDS bytes per workgroup)`` of a ``condition_on_demonstration`` launch of ``B`` episodes
        (mpk.h: mpk_demonstration_condition_plan; nothing is launched): wave w of workgroup g takes the episodes ``g waves + w``,
        ``+ workgroups waves``, ...  ``timing="given"``: the plan of the per-episode-phase launches (mpk_demonstration_phase_plan)"""
        nb, nw, lds = C.c_int32(), C.c_int32(), C.c_int32()
        entry = (self._lib.mpk_demonstration_phase_plan if self._timing_given("condition_on_demonstration_plan", timing)
                 else self._lib.mpk_demonstration_condition_plan)
        _lib.check(entry(self._h, int(B), C.byref(nb), C.byref(nw), C.byref(lds)))
        return nb.value, nw.value, lds.value

    def sample_trajectories(self, params, params_L, init_pos, init_vel, init_time: float = 0.0, *, num_samples: int,
                            generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        ``num_samples`` trajectories per episode from the Gaussian ``N(params, L L^T)`` over the non-phase parameters: ``(pos, vel)``
        [B, S, T, D] float32 on the device, without an autograd graph.  ``eps ~ N(0, I)`` [B, S, Pl] is drawn with torch on the device
        (``generator``: a device generator, for reproducible draws), the sampled parameters are ``params[:, None] + eps @ tril(L)^T``
        on the non-phase part (tau / delay, where learned, stay as given), and ONE ``trajectory`` launch over the B S rows evaluates
        them; every sample of an episode starts from that episode's ``init_pos`` / ``init_vel``.
        """
        S = int(num_samples)
        if S < 1:
            raise ValueError(f"sample_trajectories: num_samples must be >= 1, got {num_samples!r}")
        D, P = self.num_dof, self.num_params
        n_phase = self._num_phase_params()
        Pl = P - n_phase
        pshape = tuple(params.shape) if hasattr(params, "shape") else np.shape(params)
        if len(pshape) != 2 or pshape[1] != P:
            raise ValueError(f"sample_trajectories: params must be [B, {P}], got {pshape}")
        B = pshape[0]
        lshape = tuple(params_L.shape) if hasattr(params_L, "shape") else np.shape(params_L)
        if lshape != (B, Pl, Pl):
            raise ValueError(f"sample_trajectories: params_L must be [{B}, {Pl}, {Pl}], got {lshape}")
        with torch.no_grad():
            mean = torch.as_tensor(params, dtype=torch.float32, device=self.device).detach()
            L = torch.as_tensor(params_L, dtype=torch.float32, device=self.device).detach()
            eps = torch.randn((B, S, Pl), dtype=torch.float32, device=self.device, generator=generator)
            full = mean[:, None, :].repeat(1, S, 1)
            full[:, :, n_phase:] += eps @ torch.tril(L).transpose(1, 2)
            ip = self._f32(init_pos, (B, D))[:, None, :].expand(B, S, D).reshape(B * S, D)
            iv = self._f32(init_vel, (B, D))[:, None, :].expand(B, S, D).reshape(B * S, D)
            pos, vel = self._trajectory_launch(full.reshape(B * S, P), ip.contiguous(), iv.contiguous(), None, float(init_time), None)
        T = pos.shape[1]
        return pos.view(B, S, T, D), vel.view(B, S, T, D)

    def check_range(self):
        """synchronise and raise RuntimeError if a per-episode-phase ProDMP launch left the pre-computed table range"""
        _lib.check(self._lib.mpk_check_range(self._h, self._stream()))

    def poll_fault(self):
        """raise MPKLibraryError if a FINISHED launch of the ring kernels gave up waiting (outputs incomplete); synchronises nothing
        (mpk.h: mpk_poll_fault) -- for callers that synchronise themselves and make no further call that would report it"""
        _lib.check(self._lib.mpk_poll_fault(self._h))

    def gate_flags(self, valid: torch.Tensor, was_done: Optional[torch.Tensor], done: torch.Tensor):
        """(terminated, truncated) of a gated step as bool [B] tensors in ONE launch (mpk.h: mpk_gate_flags): an invalid plan terminates
        an episode that was live, a valid one that finished is truncated (black_box_wrapper.py:169-172,198-203); uint8 / bool inputs"""
        B = valid.shape[0]
        out = torch.empty((2, B), dtype=torch.uint8, device=self.device)
        u8 = lambda t: None if t is None else (t if t.dtype == torch.uint8 else t.view(torch.uint8))      # noqa: E731
        v, w, d = u8(valid), u8(was_done), u8(done)
        _lib.check(self._lib.mpk_gate_flags(self._h, v.data_ptr(), _dptr(w), d.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B,
                                            self._stream()))
        return out[0].view(torch.bool), out[1].view(torch.bool)

    def trajectory_host(self, params: np.ndarray, init_pos: np.ndarray, init_vel: np.ndarray, init_time: float
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        ONE episode, host arrays in, host tensors out (what BlackBoxWrapper.get_trajectory needs at B = 1): inputs travel
        in one pinned buffer, (pos | vel) come back in one, a single stream synchronisation.  Returns CPU float32
        tensors [T, D] -- like mp_pytorch on its default device, so fancy_gym's get_numpy does not copy again.
        """
        P, D, T = self.num_params, self.num_dof, self.num_steps
        st = self._host_stage
        if st is None or st[0] != (P, D, T):
            n_in = P + 2 * D + 1
            st = ((P, D, T), torch.empty(n_in, dtype=torch.float32).pin_memory(),
                  torch.empty(n_in, dtype=torch.float32, device=self.device),
                  torch.empty((2, T, D), dtype=torch.float32, device=self.device),
                  torch.empty((2, T, D), dtype=torch.float32).pin_memory())
            self._host_stage = st
        _, h_in, d_in, d_out, h_out = st
        buf = h_in.numpy()
        buf[:P] = np.asarray(params, np.float32).reshape(-1)
        buf[P:P + D] = np.asarray(init_pos, np.float32).reshape(-1)
        buf[P + D:P + 2 * D] = np.asarray(init_vel, np.float32).reshape(-1)
        buf[P + 2 * D] = init_time
        per_episode = bool(self.config.learn_tau or self.config.learn_delay)
        # zero copy (default): the kernel reads the inputs from, and writes (pos | vel) to, the pinned host buffers
        # themselves -- pinned host memory is device-accessible at the same address, and a few KB over PCIe cost less than
        # the two copy calls (MPK_B1_ZEROCOPY=0: staged copies through device buffers instead)
        zero_copy = self.b1_zero_copy
        if not zero_copy:
            d_in.copy_(h_in, non_blocking=True)
        base = (h_in if zero_copy else d_in).data_ptr()
        dst = h_out if zero_copy else d_out
        _lib.check(self._lib.mpk_trajectory(self._h, base, base + 4 * P, base + 4 * (P + D),
                                            base + 4 * (P + 2 * D) if per_episode else None, float(init_time),
                                            dst[0].data_ptr(), dst[1].data_ptr(), 1, self._stream()))
        if not zero_copy:
            h_out.copy_(d_out, non_blocking=True)
        if per_episode and self.mp_type == "prodmp":
            self.check_range()                       # synchronises
        else:
            torch.cuda.current_stream(self.device).synchronize()
        out = h_out.clone()
        return out[0], out[1]

    @staticmethod
    def _metaworld_state(c_pos: torch.Tensor):
        """current state as the motor kernels must see it for the metaworld controller: the gripper entry of the
        position is not subtracted (0), velocities play no part"""
        c_pos = c_pos.clone()
        c_pos[:, -1] = 0.0
        return c_pos, torch.zeros_like(c_pos)

    @staticmethod
    def _refuse_metaworld(spec, entry: str):
        """entry points that update the plant state in place cannot zero the gripper entry of the state the way
        _metaworld_state does for a frozen one: running the plain motor law there would turn the gripper action into
        des - q[-1] without a word"""
        if getattr(spec, "metaworld", False):
            raise ValueError(f"{entry}: the metaworld controller runs on the device for a frozen state only "
                             "(trajectory_actions / pd_rollout with plant='static'); step metaworld environments on the "
                             "host (VectorBlackBox)")

    def trajectory_actions(self, params, init_pos, init_vel, spec: RolloutSpec, c_pos, c_vel, init_time: float = 0.0,
                           out=None):
        """Fused trajectory + open-loop controller actions for a state frozen over the plan (MPK_PLANT_STATIC)."""
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B, D, T = params.shape[0], self.num_dof, self.num_steps
        init_pos, init_vel = self._f32(init_pos, (B, D)), self._f32(init_vel, (B, D))
        c_pos, c_vel = self._f64(c_pos, (B, D)), self._f64(c_vel, (B, D))
        if getattr(spec, "metaworld", False):
            c_pos, c_vel = self._metaworld_state(c_pos)
        if out is None:
            pos, vel, act = (torch.empty((B, T, D), dtype=torch.float32, device=self.device) for _ in range(3))
        else:
            pos, vel, act = out
        _lib.check(self._lib.mpk_trajectory_actions(
            self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
            c_pos.data_ptr(), c_vel.data_ptr(), pos.data_ptr(), vel.data_ptr(), act.data_ptr(), B, self._stream()))
        return pos, vel, act

    def trajectory_rollout(self, params, init_pos, init_vel, spec: RolloutSpec, q: torch.Tensor, qd: torch.Tensor,
                           n_steps: Optional[torch.Tensor] = None, init_time: float = 0.0, out=None):
        """
        One fused launch: trajectory + closed-loop controller / double-integrator rollout (BlackBoxWrapper.step for a
        GPU-resident plant).  q, qd float64 [B, D] are updated in place.  Returns (pos, vel, actions).
        """
        self._refuse_metaworld(spec, "trajectory_rollout")
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B, D, T = params.shape[0], self.num_dof, self.num_steps
        init_pos, init_vel = self._f32(init_pos, (B, D)), self._f32(init_vel, (B, D))
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        if out is None:
            pos, vel, act = (torch.empty((B, T, D), dtype=torch.float32, device=self.device) for _ in range(3))
        else:
            pos, vel, act = out
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self._lib.mpk_trajectory_rollout(
            self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
            q.data_ptr(), qd.data_ptr(), _dptr(n_steps), pos.data_ptr(), vel.data_ptr(), act.data_ptr(), B,
            self._stream()))
        return pos, vel, act

    def episode_reset(self, q: torch.Tensor, qd: torch.Tensor, traj_steps: torch.Tensor, plan_steps: torch.Tensor,
                      done: torch.Tensor, init_q: Optional[torch.Tensor] = None, init_qd: Optional[torch.Tensor] = None,
                      cond: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """BlackBoxWrapper.reset for device-resident episodes in one launch (mpk.h: mpk_episode_reset); everything in place"""
        B, D = q.shape
        for t, dt_ in ((q, torch.float64), (qd, torch.float64), (traj_steps, torch.int32), (plan_steps, torch.int32),
                       (done, torch.uint8)):
            assert t.dtype == dt_ and t.is_contiguous()
        for t in (init_q, init_qd):
            assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (B, D))
        cp, cv = cond if cond is not None else (None, None)
        _lib.check(self._lib.mpk_episode_reset(self._h, _dptr(init_q), _dptr(init_qd), q.data_ptr(), qd.data_ptr(),
                                               _dptr(cp), _dptr(cv), traj_steps.data_ptr(), plan_steps.data_ptr(),
                                               done.data_ptr(), B, self._stream()))

    def _gate(self, gate, B: int):
        """
        dict(pos_low, pos_high, check_tau_delay=False, tau_bound=None, delay_bound=None, raw_params=None, valid=None, penalty=None)
        -> (mpk_validity_gate, valid uint8 [B], penalty float64 [B], keep-alive); mpk.h: mpk_validity_gate
        """
        D = self.num_dof
        lo_p, lo_k = _dvec(gate["pos_low"], D)
        hi_p, hi_k = _dvec(gate["pos_high"], D)
        check = bool(gate.get("check_tau_delay"))
        g = _lib.mpk_validity_gate()
        g.pos_low, g.pos_high = lo_p, hi_p
        g.check_tau_delay = int(check)
        tb = gate.get("tau_bound") if check else None
        db = gate.get("delay_bound") if check else None
        if check and (tb is None or db is None):
            raise ValueError("check_tau_delay needs tau_bound and delay_bound")
        g.tau_bound[0], g.tau_bound[1] = (float(tb[0]), float(tb[1])) if check else (0.0, 0.0)
        g.delay_bound[0], g.delay_bound[1] = (float(db[0]), float(db[1])) if check else (0.0, 0.0)
        raw = gate.get("raw_params")
        if raw is not None:
            raw = torch.as_tensor(raw, dtype=torch.float32, device=self.device).contiguous()
            if tuple(raw.shape) != (B, self.num_params):
                raise ValueError(f"raw_params must be [{B}, {self.num_params}], got {tuple(raw.shape)}")
        valid = gate.get("valid")
        if valid is None:
            valid = torch.empty(B, dtype=torch.uint8, device=self.device)
        pen = gate.get("penalty")
        if pen is None:
            pen = torch.empty(B, dtype=torch.float64, device=self.device)
        assert valid.dtype == torch.uint8 and pen.dtype == torch.float64 and valid.is_contiguous() and pen.is_contiguous()
        g.raw_params, g.valid, g.penalty = _dptr(raw), valid.data_ptr(), pen.data_ptr()
        return g, valid, pen, (lo_k, hi_k, raw)

    def replan_step(self, params, init_pos, init_vel, spec: RolloutSpec, q: torch.Tensor, qd: torch.Tensor,
                    traj_steps: torch.Tensor, plan_steps: torch.Tensor, done: torch.Tensor, every: int,
                    max_planning_times: int, horizon: int, init_time: float = 0.0, condition: bool = False, out=None,
                    gate=None):
        """
        One replanning step of BlackBoxWrapper.step for every episode (mpk.h: mpk_replan_step): integer state, plan,
        controller + plant for the executed steps and -- ``condition`` -- the desired state at the last executed step, in
        ONE launch where the fused closed-loop kernel applies.  q, qd, traj_steps, plan_steps, done are updated in place.
        Returns dict(pos, vel, actions, seg_len int32 [B], done uint8 [B] snapshot, cond_pos, cond_vel (or None)).
        ``gate`` (see ``_gate``): the validity gate inside the step (mpk.h: mpk_replan_step_gated) -- additionally ``valid``
        uint8 [B] and ``penalty`` float64 [B]; an invalid plan finishes its episode without a step.
        """
        self._refuse_metaworld(spec, "replan_step")
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B, D, T = params.shape[0], self.num_dof, self.num_steps
        init_pos, init_vel = self._f32(init_pos, (B, D)), self._f32(init_vel, (B, D))
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        assert traj_steps.dtype == torch.int32 and plan_steps.dtype == torch.int32 and done.dtype == torch.uint8
        if out is None:
            pos, vel, act = (torch.empty((B, T, D), dtype=torch.float32, device=self.device) for _ in range(3))
        else:
            pos, vel, act = out
        seg = torch.empty(B, dtype=torch.int32, device=self.device)
        done_out = torch.empty(B, dtype=torch.uint8, device=self.device)
        cp = cv = None
        if condition:
            cp, cv = (torch.empty((B, D), dtype=torch.float32, device=self.device) for _ in range(2))
        st = _lib.mpk_replan_state(traj_steps.data_ptr(), plan_steps.data_ptr(), done.data_ptr(), seg.data_ptr(),
                                   done_out.data_ptr(), _dptr(cp), _dptr(cv), int(every),
                                   int(min(max_planning_times, 2 ** 31 - 1)), int(horizon), 0)
        if gate is not None:
            g, valid, pen, keep = self._gate(gate, B)
            _lib.check(self._lib.mpk_replan_step_gated(
                self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
                q.data_ptr(), qd.data_ptr(), C.byref(st), C.byref(g), pos.data_ptr(), vel.data_ptr(), act.data_ptr(), B,
                self._stream()))
            return dict(pos=pos, vel=vel, actions=act, seg_len=seg, done=done_out, cond_pos=cp, cond_vel=cv, valid=valid,
                        penalty=pen)
        _lib.check(self._lib.mpk_replan_step(
            self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
            q.data_ptr(), qd.data_ptr(), C.byref(st), pos.data_ptr(), vel.data_ptr(), act.data_ptr(), B,
            self._stream()))
        return dict(pos=pos, vel=vel, actions=act, seg_len=seg, done=done_out, cond_pos=cp, cond_vel=cv)

    def episode_return(self, params, init_pos, init_vel, spec: RolloutSpec, q: torch.Tensor, qd: torch.Tensor, *,
                       replan=None, n_steps: Optional[torch.Tensor] = None, reward: Optional[str] = None,
                       goal: Optional[torch.Tensor] = None, step0: Optional[torch.Tensor] = None,
                       steps_before_reward: int = 199, aggregation: str = "sum", init_time: float = 0.0,
                       condition: bool = False, gate=None, differentiable: bool = False, carry=None):
        """
        One plan of a ``verbose < 2`` step for every episode in ONE launch, nothing per step stored (mpk.h: mpk_episode_return):
        plan + controller + double-integrator plant + reward + reward_aggregation (+ the integer replanning state and the
        condition gather when ``replan = (traj_steps, plan_steps, done, every, max_planning_times, horizon)``).  q, qd (and
        the replanning state) are updated in place.  Returns dict(ret float64 [B], seg_len int32 [B], done uint8 [B] or None,
        cond_pos, cond_vel (or None)).  NotImplementedError where the fused kernel does not apply (per-episode phase, > 16
        columns / DoF, very long horizons): use replan_step / trajectory_rollout + reacher_rollout + reward_aggregate.

        ``differentiable=True`` (reward "simple_reacher", no gate): the same launch on a copy-protected plan-start state, and ``ret``
        carries a ``grad_fn`` whose backward is ONE mpk_episode_return_vjp launch (``episode_return_vjp``) to ``params``, ``init_pos``,
        ``init_vel`` and ``goal`` where they require grad; the plan-start state is a constant of that graph, and under replanning the
        gradient is that of this plan's return w.r.t. this plan's inputs.  NotImplementedError for what mpk_episode_return_vjp refuses (a
        learned tau / delay, a DMP off its response route, very long horizons) BEFORE anything is launched.  Without the flag nothing
        changes: inputs that require grad are treated as constants.

        ``carry=(q_in, qd_in)`` (with ``differentiable=True``): the carrying form for gradients that cross plan boundaries.  ``q_in``,
        ``qd_in`` are float64 [B, D] tensors with the bits of q, qd that may carry the graph of the plans before; the result gains
        ``carry = dict(q=, qd=[, cond_pos=, cond_vel=])``: clones of what the launch left in q, qd (and of the condition it wrote) that
        carry this plan's graph -- the backward, still ONE launch (mpk_episode_return_vjp_cond), takes their gradients as g_q, g_qd,
        g_cond_* and returns g_q0, g_qd0 to ``q_in``, ``qd_in``.  q, qd themselves and ``cond_pos`` / ``cond_vel`` stay graph-free.
        """
        self._refuse_metaworld(spec, "episode_return")
        if carry is not None and not differentiable:
            raise ValueError("episode_return(carry=...) is the carrying form of differentiable=True")
        if differentiable:
            if reward != "simple_reacher" or gate is not None:
                raise NotImplementedError("episode_return(differentiable=True) is built for reward='simple_reacher' without a validity gate")
            params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
            if params.dim() == 1:
                params = params[None]
            Bn = params.shape[0]
            init_pos, init_vel = self._f32(init_pos, (Bn, self.num_dof)), self._f32(init_vel, (Bn, self.num_dof))
            goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).expand(Bn, 2)
            if carry is not None:
                q_in, qd_in = (self._f64(t, (Bn, self.num_dof)) for t in carry)
            if torch.is_grad_enabled() and (carry is not None or any(t.requires_grad for t in (params, init_pos, init_vel, goal))):
                # what the backward would refuse is refused here, before the forward changes the state (B = 0: the checks alone, no launch)
                _lib.check(self._lib.mpk_episode_return_vjp(self._h, None, None, None, float(init_time), C.byref(spec.c), *([None] * 5),
                                                            int(steps_before_reward), _lib.AGG_MODES.get(aggregation, 0),
                                                            *([None] * 11), 0, self._stream()))
                res = {}

                def launch():
                    res.update(self.episode_return(params.detach(), init_pos.detach(), init_vel.detach(), spec, q, qd, replan=replan,
                                                   n_steps=n_steps, reward=reward, goal=goal.detach(), step0=step0,
                                                   steps_before_reward=steps_before_reward, aggregation=aggregation,
                                                   init_time=init_time, condition=condition))
                    return res
                s0 = replan[0] if replan is not None else step0
                if carry is not None:
                    ret, *tw = _EpisodeReturnCarryFn.apply(self, launch, spec, q, qd, s0, steps_before_reward, aggregation, init_time,
                                                           params.contiguous(), init_pos, init_vel, goal.contiguous(), q_in, qd_in)
                    return dict(res, ret=ret, carry=dict(zip(("q", "qd", "cond_pos", "cond_vel"), tw)))
                ret = _EpisodeReturnFn.apply(self, launch, spec, q, qd, s0, steps_before_reward,
                                             aggregation, init_time, params.contiguous(), init_pos, init_vel, goal.contiguous())
                return dict(res, ret=ret)
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device)
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B, D = params.shape[0], self.num_dof
        init_pos, init_vel = self._f32(init_pos, (B, D)), self._f32(init_vel, (B, D))
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        ret = torch.empty(B, dtype=torch.float64, device=self.device)
        seg = torch.empty(B, dtype=torch.int32, device=self.device)
        done_out = cp = cv = None
        st = None
        if replan is not None:
            traj_steps, plan_steps, done, every, max_planning_times, horizon = replan
            assert traj_steps.dtype == torch.int32 and plan_steps.dtype == torch.int32 and done.dtype == torch.uint8
            done_out = torch.empty(B, dtype=torch.uint8, device=self.device)
            if condition:
                cp, cv = (torch.empty((B, D), dtype=torch.float32, device=self.device) for _ in range(2))
            st = _lib.mpk_replan_state(traj_steps.data_ptr(), plan_steps.data_ptr(), done.data_ptr(), seg.data_ptr(),
                                       done_out.data_ptr(), _dptr(cp), _dptr(cv), int(every),
                                       int(min(max_planning_times, 2 ** 31 - 1)), int(horizon), 0)
        elif n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if goal is not None:
            goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).expand(B, 2).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        if reward not in _lib.REWARD_TYPES:
            raise ValueError(f"unknown device reward {reward!r}; choose one of {[k for k in _lib.REWARD_TYPES if k]}")
        if aggregation not in _lib.AGG_MODES:
            raise ValueError(f"unknown reward aggregation {aggregation!r}; choose one of {list(_lib.AGG_MODES)}")
        if gate is not None:
            g, valid, pen, keep = self._gate(gate, B)
            _lib.check(self._lib.mpk_episode_return_gated(
                self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
                q.data_ptr(), qd.data_ptr(), C.byref(st) if st is not None else None, C.byref(g), _dptr(n_steps), seg.data_ptr(),
                _lib.REWARD_TYPES[reward], _dptr(goal), _dptr(step0), int(steps_before_reward), _lib.AGG_MODES[aggregation],
                ret.data_ptr(), B, self._stream()))
            return dict(ret=ret, seg_len=seg, done=done_out, cond_pos=cp, cond_vel=cv, valid=valid, penalty=pen)
        _lib.check(self._lib.mpk_episode_return(
            self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c),
            q.data_ptr(), qd.data_ptr(), C.byref(st) if st is not None else None, _dptr(n_steps), seg.data_ptr(),
            _lib.REWARD_TYPES[reward], _dptr(goal), _dptr(step0), int(steps_before_reward), _lib.AGG_MODES[aggregation],
            ret.data_ptr(), B, self._stream()))
        return dict(ret=ret, seg_len=seg, done=done_out, cond_pos=cp, cond_vel=cv)

    def reward_aggregate(self, rewards: torch.Tensor, seg_len: torch.Tensor, aggregation: str = "sum") -> torch.Tensor:
        """reward_aggregation over each episode's executed steps (black_box_wrapper.py:216) of step rewards [B, T] float64, in the
        order of additions of episode_return (mpk.h: mpk_reward_aggregate): the two paths agree bit for bit"""
        assert rewards.dtype == torch.float64 and rewards.is_contiguous()
        seg_len = seg_len.to(device=self.device, dtype=torch.int32).contiguous()
        if torch.is_grad_enabled() and rewards.requires_grad:
            # differentiable step rewards (reacher_rollout under autograd): the same launch, a linear backward
            return _RewardAggregateFn.apply(self, seg_len, aggregation, rewards)
        return self._reward_aggregate_launch(rewards, seg_len, aggregation)

    def _reward_aggregate_launch(self, rewards, seg_len, aggregation):
        B, T = rewards.shape
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mpk_reward_aggregate(self._h, rewards.data_ptr(), seg_len.data_ptr(), _lib.AGG_MODES[aggregation],
                                                  out.data_ptr(), B, T, self._stream()))
        return out

    def pd_rollout(self, spec: RolloutSpec, des_pos: torch.Tensor, des_vel: torch.Tensor, q: torch.Tensor,
                   qd: torch.Tensor, n_steps: Optional[torch.Tensor] = None, want_actions: bool = True,
                   out: Optional[torch.Tensor] = None):
        """In-place closed-loop rollout; q, qd float64 [B, D] are updated to the state after the executed steps."""
        B, T, D = des_pos.shape
        assert des_pos.dtype == torch.float32 and des_vel.dtype == torch.float32
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        des_pos, des_vel = des_pos.contiguous(), des_vel.contiguous()
        act = out if out is not None else (
            torch.empty((B, T, D), dtype=torch.float32, device=self.device) if want_actions else None)
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if getattr(spec, "metaworld", False):
            q, qd = self._metaworld_state(q)         # static plant: the caller's state is left as it is
        _lib.check(self._lib.mpk_pd_rollout(self._h, C.byref(spec.c), des_pos.data_ptr(), des_vel.data_ptr(),
                                            q.data_ptr(), qd.data_ptr(), _dptr(n_steps), _dptr(act), B, T,
                                            self._stream()))
        return act

    def reacher_rollout(self, spec: RolloutSpec, des_pos: torch.Tensor, des_vel: torch.Tensor, q: torch.Tensor,
                        qd: torch.Tensor, goal: torch.Tensor, n_steps: Optional[torch.Tensor] = None,
                        step0: Optional[torch.Tensor] = None, steps_before_reward: int = 199,
                        want_actions: bool = True, out=None, carry=None, condition: bool = False):
        """
        pd_rollout + SimpleReacherEnv's per-step reward (simple_reacher.py:56-72) on the torque double integrator:
        returns (actions float32 [B, T, D] or None, rewards float64 [B, T]); q, qd are updated in place.

        Differentiable: with grad enabled and ``des_pos``, ``des_vel`` or ``goal`` requiring grad, the same launch runs on a copy-protected
        plan-start state (q, qd are cloned first) and ``rewards`` carries a ``grad_fn`` whose backward is ONE mpk_reacher_rollout_vjp
        launch (``reacher_rollout_vjp``); the actions and the in-place q, qd carry no graph.  The plan-start state is a constant of that
        graph.  Otherwise -- no requires_grad, or under no_grad -- nothing changes.

        ``carry=(q_in, qd_in)`` (grad enabled): the carrying form for gradients that cross plan boundaries.  ``q_in``, ``qd_in`` are
        float64 [B, D] tensors with the bits of q, qd that may carry the graph of the plans before.  Returns (actions, rewards, carry)
        with ``carry = dict(q=, qd=[, cond_pos=, cond_vel=])``: clones of what the launch left in q, qd that carry this plan's graph
        and, with ``condition``, clones of the condition gathered from this plan at ``n_steps`` (``condition_gather``, whose own
        graph-free outputs are ``carry["cond"]``).  The backward is still one launch (mpk_reacher_rollout_vjp_cond) and returns g_q0,
        g_qd0 to ``q_in``, ``qd_in``.
        """
        self._refuse_metaworld(spec, "reacher_rollout")
        B, T, D = des_pos.shape
        assert des_pos.dtype == torch.float32 and des_vel.dtype == torch.float32
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        des_pos, des_vel = des_pos.contiguous(), des_vel.contiguous()
        goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).expand(B, 2).contiguous()
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        if carry is not None:
            if not torch.is_grad_enabled():
                raise ValueError("reacher_rollout(carry=...) is the carrying form of the differentiable rollout: it needs grad enabled")
            q_in, qd_in = (self._f64(t, (B, D)) for t in carry)
            box = {}
            rew, *tw = _ReacherRolloutCarryFn.apply(self, spec, q, qd, n_steps, step0, steps_before_reward, want_actions, out,
                                                    bool(condition), box, des_pos, des_vel, goal, q_in, qd_in)
            tw = dict(zip(("q", "qd", "cond_pos", "cond_vel"), tw))
            if condition:
                tw["cond"] = (box["cond_pos"], box["cond_vel"])
            return box["actions"], rew, tw
        if torch.is_grad_enabled() and (des_pos.requires_grad or des_vel.requires_grad or goal.requires_grad):
            res = _ReacherRolloutFn.apply(self, spec, q, qd, n_steps, step0, steps_before_reward, want_actions, out, des_pos, des_vel,
                                          goal)
            return res if isinstance(res, tuple) else (None, res)
        return self._reacher_rollout_launch(spec, des_pos, des_vel, q, qd, goal, n_steps, step0, steps_before_reward, want_actions,
                                            out)

    def _reacher_rollout_launch(self, spec, des_pos, des_vel, q, qd, goal, n_steps, step0, steps_before_reward, want_actions, out):
        B, T, D = des_pos.shape
        if out is not None:
            act, rew = out
        else:
            act = torch.empty((B, T, D), dtype=torch.float32, device=self.device) if want_actions else None
            rew = torch.empty((B, T), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mpk_reacher_rollout(self._h, C.byref(spec.c), des_pos.data_ptr(), des_vel.data_ptr(),
                                                 q.data_ptr(), qd.data_ptr(), _dptr(n_steps), _dptr(step0),
                                                 goal.data_ptr(), int(steps_before_reward), _dptr(act),
                                                 rew.data_ptr(), B, T, self._stream()))
        return act, rew

    def reacher_rollout_vjp(self, spec: RolloutSpec, des_pos: torch.Tensor, des_vel: torch.Tensor, q0: torch.Tensor,
                            qd0: torch.Tensor, goal: torch.Tensor, g_rewards: Optional[torch.Tensor], *,
                            g_q: Optional[torch.Tensor] = None, g_qd: Optional[torch.Tensor] = None,
                            n_steps: Optional[torch.Tensor] = None, step0: Optional[torch.Tensor] = None,
                            steps_before_reward: int = 199, need: Sequence[bool] = (True, True, True, True, True),
                            out: Optional[Sequence[Optional[torch.Tensor]]] = None,
                            g_cond_pos: Optional[torch.Tensor] = None, g_cond_vel: Optional[torch.Tensor] = None):
        """
        The vector-Jacobian product of ``reacher_rollout`` (mpk.h: mpk_reacher_rollout_vjp), one launch: the gradients of a loss w.r.t.
        the step rewards [B, T] float64 and the final state (``g_q``, ``g_qd`` [B, D] float64; any of the three may be None = 0) ->
        (g_des_pos, g_des_vel float32 [B, T, D], g_q0, g_qd0 float64 [B, D], g_goal float64 [B, 2]).  ``q0``, ``qd0`` are the state at
        the START of the plan (reacher_rollout overwrites its q, qd: pass a copy taken before), and a constant here and there: under
        replanning this is the gradient of ONE plan's rewards w.r.t. that plan's trajectory.  ``need[i]`` False: that output is not
        computed (None in its place); ``out``: buffers for the needed ones.  NotImplementedError: more than 16 DoF, a plant other than
        the double integrator (the metaworld controller), horizons beyond about 2 100 steps.

        ``g_cond_pos`` / ``g_cond_vel`` (float32 [B, D], either may be None = 0): the gradient of a loss w.r.t. the condition a
        replanning forward gathered from this plan -- row ``clamp(n_steps - 1, 0, T - 1)`` of (des_pos, des_vel) -- is added to that row
        of (g_des_pos, g_des_vel) whatever the controller reads (mpk.h: mpk_reacher_rollout_vjp_cond, the entry taken when either is
        given).
        """
        if getattr(spec, "metaworld", False) or spec.plant != "double_integrator":
            raise NotImplementedError("reacher_rollout_vjp differentiates the torque double integrator only (plant='double_integrator'): "
                                      "the metaworld controller runs on a frozen state, HoleReacher's direct-velocity plant is not built")
        B, T, D = des_pos.shape
        assert des_pos.dtype == torch.float32 and des_vel.dtype == torch.float32
        des_pos, des_vel = des_pos.detach().contiguous(), des_vel.detach().contiguous()
        q0, qd0 = self._f64(q0, (B, D)).detach(), self._f64(qd0, (B, D)).detach()
        goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).detach().expand(B, 2).contiguous()
        ups = []
        for name, g, shape in (("g_rewards", g_rewards, (B, T)), ("g_q", g_q, (B, D)), ("g_qd", g_qd, (B, D))):
            if g is not None:
                g = torch.as_tensor(g, dtype=torch.float64, device=self.device)
                if tuple(g.shape) != shape:
                    raise ValueError(f"{name} must be {list(shape)}, got {list(g.shape)}")
                g = g.detach().contiguous()
            ups.append(g)
        gc = self._cond_upstreams(g_cond_pos, g_cond_vel, B, D)
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        res = []
        for i, (shape, dtype) in enumerate((((B, T, D), torch.float32), ((B, T, D), torch.float32), ((B, D), torch.float64),
                                            ((B, D), torch.float64), ((B, 2), torch.float64))):
            if not need[i]:
                res.append(None)
            elif out is not None and out[i] is not None:
                if tuple(out[i].shape) != shape or out[i].dtype != dtype or not out[i].is_contiguous() or out[i].device != self.device:
                    raise ValueError(f"out[{i}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
                res.append(out[i])
            else:
                res.append(torch.empty(shape, dtype=dtype, device=self.device))
        head = (self._h, C.byref(spec.c), des_pos.data_ptr(), des_vel.data_ptr(), q0.data_ptr(), qd0.data_ptr(), _dptr(n_steps),
                _dptr(step0), goal.data_ptr(), int(steps_before_reward), _dptr(ups[0]), _dptr(ups[1]), _dptr(ups[2]))
        tail = (_dptr(res[0]), _dptr(res[1]), _dptr(res[2]), _dptr(res[3]), _dptr(res[4]), B, T, self._stream())
        if gc is None:
            _lib.check(self._lib.mpk_reacher_rollout_vjp(*head, *tail))
        else:
            _lib.check(self._lib.mpk_reacher_rollout_vjp_cond(*head, _dptr(gc[0]), _dptr(gc[1]), *tail))
        return tuple(res)

    def _cond_upstreams(self, g_cond_pos, g_cond_vel, B: int, D: int):
        """the condition upstreams of a ``*_vjp`` product as the ``_cond`` entry points take them: float32 [B, D], contiguous, either may
        be None; None when neither is given (the plain entry point)"""
        if g_cond_pos is None and g_cond_vel is None:
            return None
        gc = []
        for name, g in (("g_cond_pos", g_cond_pos), ("g_cond_vel", g_cond_vel)):
            if g is not None:
                g = torch.as_tensor(g, device=self.device)
                if g.dtype != torch.float32:
                    raise ValueError(f"{name} must be float32 (the dtype of the condition), got {g.dtype}")
                if tuple(g.shape) != (B, D):
                    raise ValueError(f"{name} must be {[B, D]}, got {list(g.shape)}")
                g = g.detach().contiguous()
            gc.append(g)
        return gc

    def episode_return_vjp(self, params, init_pos, init_vel, spec: RolloutSpec, q0: torch.Tensor, qd0: torch.Tensor,
                           goal: torch.Tensor, g_ret: Optional[torch.Tensor], *, g_q: Optional[torch.Tensor] = None,
                           g_qd: Optional[torch.Tensor] = None, n_steps: Optional[torch.Tensor] = None,
                           step0: Optional[torch.Tensor] = None, steps_before_reward: int = 199, aggregation: str = "sum",
                           init_time: float = 0.0, need: Sequence[bool] = (True, True, True, True, True, True, False, False),
                           out: Optional[Sequence[Optional[torch.Tensor]]] = None,
                           g_cond_pos: Optional[torch.Tensor] = None, g_cond_vel: Optional[torch.Tensor] = None):
        """
        The vector-Jacobian product of ``episode_return`` with reward "simple_reacher" (mpk.h: mpk_episode_return_vjp), ONE launch --
        ``trajectory``, ``reacher_rollout_vjp`` and ``trajectory_vjp`` composed without the plan or its gradient in memory: the gradients
        of a loss w.r.t. the aggregated reward [B] float64 and the final state (``g_q``, ``g_qd`` [B, D] float64; any of the three may
        be None = 0) -> (g_params [B, P], g_init_pos, g_init_vel [B, D] float32, g_q0, g_qd0 [B, D], g_goal [B, 2] float64, q_end, qd_end
        [B, D] float64: the state after ``n_steps`` as the replay finds it, the bits ``episode_return`` leaves in q, qd).  ``q0``, ``qd0``
        are the state at the START of the plan (episode_return overwrites its q, qd: pass a copy taken before) and ``n_steps`` the
        executed steps (its ``seg_len``; None = all).  ``need[i]`` False: that output is not computed (None in its place); ``out``:
        buffers for the needed ones.  NotImplementedError: a learned tau / delay, a DMP off its response route, more than 16 DoF or
        contraction columns, a plant other than the double integrator, horizons beyond about 2 200 steps.

        ``g_cond_pos`` / ``g_cond_vel`` (float32 [B, D], either may be None = 0): the gradient of a loss w.r.t. the ``cond_pos`` /
        ``cond_vel`` a replanning ``episode_return(condition=True)`` returned -- row ``clamp(n_steps - 1, 0, T - 1)`` of the plan -- joins
        the plan's gradient at that row whatever the controller reads (mpk.h: mpk_episode_return_vjp_cond, the entry taken when either
        is given).
        """
        if getattr(spec, "metaworld", False) or spec.plant != "double_integrator":
            raise NotImplementedError("episode_return_vjp differentiates the torque double integrator only (plant='double_integrator'): "
                                      "the metaworld controller runs on a frozen state, HoleReacher's direct-velocity plant is not built")
        if aggregation not in _lib.AGG_MODES:
            raise ValueError(f"unknown reward aggregation {aggregation!r}; choose one of {list(_lib.AGG_MODES)}")
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device).detach()
        if params.dim() == 1:
            params = params[None]
        params = params.contiguous()
        B, D = params.shape[0], self.num_dof
        if params.shape[1] != self.num_params:
            raise ValueError(f"params has {params.shape[1]} entries per episode, expected {self.num_params}")
        init_pos, init_vel = self._f32(init_pos, (B, D)).detach(), self._f32(init_vel, (B, D)).detach()
        q0, qd0 = self._f64(q0, (B, D)).detach(), self._f64(qd0, (B, D)).detach()
        goal = torch.as_tensor(goal, dtype=torch.float64, device=self.device).detach().expand(B, 2).contiguous()
        ups = []
        for name, g, shape in (("g_ret", g_ret, (B,)), ("g_q", g_q, (B, D)), ("g_qd", g_qd, (B, D))):
            if g is not None:
                g = torch.as_tensor(g, dtype=torch.float64, device=self.device)
                if tuple(g.shape) != shape:
                    raise ValueError(f"{name} must be {list(shape)}, got {list(g.shape)}")
                g = g.detach().contiguous()
            ups.append(g)
        gc = self._cond_upstreams(g_cond_pos, g_cond_vel, B, D)
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        f32, f64 = torch.float32, torch.float64
        res = []
        for i, (shape, dtype) in enumerate((((B, self.num_params), f32), ((B, D), f32), ((B, D), f32), ((B, D), f64), ((B, D), f64),
                                            ((B, 2), f64), ((B, D), f64), ((B, D), f64))):
            if not need[i]:
                res.append(None)
            elif out is not None and out[i] is not None:
                if tuple(out[i].shape) != shape or out[i].dtype != dtype or not out[i].is_contiguous() or out[i].device != self.device:
                    raise ValueError(f"out[{i}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
                res.append(out[i])
            else:
                res.append(torch.empty(shape, dtype=dtype, device=self.device))
        head = (self._h, params.data_ptr(), init_pos.data_ptr(), init_vel.data_ptr(), float(init_time), C.byref(spec.c), q0.data_ptr(),
                qd0.data_ptr(), _dptr(n_steps), _dptr(step0), goal.data_ptr(), int(steps_before_reward), _lib.AGG_MODES[aggregation],
                _dptr(ups[0]), _dptr(ups[1]), _dptr(ups[2]))
        tail = (*(_dptr(r) for r in res), B, self._stream())
        if gc is None:
            _lib.check(self._lib.mpk_episode_return_vjp(*head, *tail))
        else:
            _lib.check(self._lib.mpk_episode_return_vjp_cond(*head, _dptr(gc[0]), _dptr(gc[1]), *tail))
        return tuple(res)

    def hole_reacher_rollout_vjp(self, spec: RolloutSpec, des_pos: Optional[torch.Tensor], des_vel: Optional[torch.Tensor],
                                 q0: torch.Tensor, qd0: torch.Tensor, hole: torch.Tensor, *, n_exec: Optional[torch.Tensor],
                                 collided: Optional[torch.Tensor], step0: Optional[torch.Tensor] = None,
                                 g_rewards: Optional[torch.Tensor] = None, g_ret: Optional[torch.Tensor] = None,
                                 aggregation: str = "sum", g_q: Optional[torch.Tensor] = None, g_qd: Optional[torch.Tensor] = None,
                                 rew_fct: str = "simple", collision_penalty: float = 100.0, steps_before_reward: int = 199,
                                 need: Sequence[bool] = (True, True, True, True, True),
                                 out: Optional[Sequence[Optional[torch.Tensor]]] = None,
                                 g_cond_pos: Optional[torch.Tensor] = None, g_cond_vel: Optional[torch.Tensor] = None):
        """
        The vector-Jacobian product of ``hole_reacher_rollout`` with the episode's end and collision verdict frozen (mpk.h:
        mpk_hole_reacher_rollout_vjp), one launch: the gradients of a loss w.r.t. the step rewards [B, T], their aggregate ``g_ret`` [B]
        (``aggregation``: how the forward formed it) and the final state (``g_q``, ``g_qd`` [B, D]; float64, any of the four may be
        None = 0) -> (g_des_pos, g_des_vel float32 [B, T, D], g_q0, g_qd0 float64 [B, D], g_hole float64 [B, 3]).  ``n_exec`` int32 [B]
        and ``collided`` uint8 [B] are the forward's outputs (None = T / no collision); ``q0``, ``qd0`` the state at the START of the
        plan (hole_reacher_rollout overwrites its q, qd: pass a copy taken before) and ``step0`` the env step counter there (a
        replanning forward: a copy of traj_steps before the plan).  The velocity controller reads ``des_vel`` only (``des_pos`` may be
        None, its gradient is zeros), the position controller the other way round.  ``need[i]`` False: that output is not computed (None
        in its place); ``out``: buffers for the needed ones.  ValueError: a plant other than 'velocity_direct'.  NotImplementedError:
        rew_fct 'unbounded', more than 16 DoF, horizons beyond about 2 200 steps.

        ``g_cond_pos`` / ``g_cond_vel`` (float32 [B, D], either may be None = 0): the gradient of a loss w.r.t. the condition a
        replanning forward gathered from this plan -- row ``clamp(n_exec - 1, 0, T - 1)`` of (des_pos, des_vel) -- is added to that row
        of (g_des_pos, g_des_vel) whatever the controller reads: the velocity controller's g_des_pos is then that row and zeros
        (mpk.h: mpk_hole_reacher_rollout_vjp_cond, the entry taken when either is given).
        """
        if spec.plant != "velocity_direct":
            raise ValueError("hole_reacher_rollout_vjp differentiates plant='velocity_direct' (reacher_rollout_vjp: the double integrator)")
        if aggregation not in _lib.AGG_MODES:
            raise ValueError(f"unknown reward aggregation {aggregation!r}; choose one of {list(_lib.AGG_MODES)}")
        rew = _lib.hole_rew_fct(rew_fct, steps_before_reward)
        ref = des_vel if des_vel is not None else des_pos
        if ref is None:
            raise ValueError("hole_reacher_rollout_vjp needs des_pos or des_vel")
        B, T, D = ref.shape
        des = []
        for t in (des_pos, des_vel):
            if t is not None:
                assert t.dtype == torch.float32 and tuple(t.shape) == (B, T, D)
                t = t.detach().contiguous()
            des.append(t)
        q0, qd0 = self._f64(q0, (B, D)).detach(), self._f64(qd0, (B, D)).detach()
        hole = torch.as_tensor(hole, dtype=torch.float64, device=self.device).detach().expand(B, 3).contiguous()
        ups = []
        for name, g, shape in (("g_ret", g_ret, (B,)), ("g_rewards", g_rewards, (B, T)), ("g_q", g_q, (B, D)), ("g_qd", g_qd, (B, D))):
            if g is not None:
                g = torch.as_tensor(g, dtype=torch.float64, device=self.device)
                if tuple(g.shape) != shape:
                    raise ValueError(f"{name} must be {list(shape)}, got {list(g.shape)}")
                g = g.detach().contiguous()
            ups.append(g)
        gc = self._cond_upstreams(g_cond_pos, g_cond_vel, B, D)
        if n_exec is not None:
            n_exec = n_exec.to(device=self.device, dtype=torch.int32).contiguous()
        if collided is not None:
            collided = collided.to(device=self.device, dtype=torch.uint8).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        res = []
        for i, (shape, dtype) in enumerate((((B, T, D), torch.float32), ((B, T, D), torch.float32), ((B, D), torch.float64),
                                            ((B, D), torch.float64), ((B, 3), torch.float64))):
            if not need[i]:
                res.append(None)
            elif out is not None and out[i] is not None:
                if tuple(out[i].shape) != shape or out[i].dtype != dtype or not out[i].is_contiguous() or out[i].device != self.device:
                    raise ValueError(f"out[{i}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
                res.append(out[i])
            else:
                res.append(torch.empty(shape, dtype=dtype, device=self.device))
        task = _lib.mpk_hole_task(float(collision_penalty), 0, 0, int(steps_before_reward), rew)
        head = (self._h, C.byref(spec.c), _dptr(des[0]), _dptr(des[1]), q0.data_ptr(), qd0.data_ptr(), _dptr(n_exec), _dptr(step0),
                C.byref(task), hole.data_ptr(), _dptr(collided), _lib.AGG_MODES[aggregation], _dptr(ups[0]), _dptr(ups[1]), _dptr(ups[2]),
                _dptr(ups[3]))
        tail = (*(_dptr(r) for r in res), B, T, self._stream())
        if gc is None:
            _lib.check(self._lib.mpk_hole_reacher_rollout_vjp(*head, *tail))
        else:
            _lib.check(self._lib.mpk_hole_reacher_rollout_vjp_cond(*head, _dptr(gc[0]), _dptr(gc[1]), *tail))
        return tuple(res)

    def hole_reacher_rollout(self, spec: RolloutSpec, des_pos: Optional[torch.Tensor], des_vel: torch.Tensor, q: torch.Tensor,
                             qd: torch.Tensor, hole: torch.Tensor, *, collision_penalty: float = 100.0,
                             allow_self_collision: bool = False, allow_wall_collision: bool = False, steps_before_reward: int = 199,
                             n_steps: Optional[torch.Tensor] = None, step0: Optional[torch.Tensor] = None, replan=None,
                             condition: bool = False, want_actions: bool = True, want_rewards: bool = True,
                             aggregation: Optional[str] = "sum", rew_fct: str = "simple",
                             reward_state: Optional[torch.Tensor] = None, differentiable: bool = False, carry=None):
        """
        The HoleReacher step loop on the device (mpk.h: mpk_hole_reacher_rollout2; spec.plant 'velocity_direct'): controller, clip,
        direct-velocity plant, collisions, reward, and the break on collision.  q, qd are updated in place.  ``rew_fct`` is the
        env's reward function ("simple", "vel_acc", "unbounded"; the last two need steps_before_reward = 199); "unbounded" keeps the
        end effector of step 180 in ``reward_state`` float64 [B, 2] on the device, read and written -- pass the same tensor to every
        plan of an episode (a reset need not clear it).  ``replan`` =
        (traj_steps, plan_steps, done, every, max_planning_times, horizon) lets the launch advance the integer state itself and commit
        the break (then n_steps / step0 must be None).  Returns a dict: actions [B, T, D] / rewards [B, T] (or None), ret [B] (or None
        when aggregation is None), n_exec [B] int32, collided / success [B] uint8, and with ``replan`` done (snapshot after the plan)
        plus cond_pos / cond_vel when ``condition``.

        ``differentiable=True`` (rew_fct "simple" / "vel_acc"; off by default, and then nothing changes -- no clone, no ``grad_fn`` even
        if the inputs require grad): with grad enabled and ``des_pos``, ``des_vel`` or ``hole`` requiring grad the launch is the plain
        call's -- the same state, integer outputs and values -- on a copy-protected plan-start state, and ``ret`` and ``rewards`` carry a
        ``grad_fn`` whose backward is ONE mpk_hole_reacher_rollout_vjp launch (``hole_reacher_rollout_vjp``) fed with the forward's own
        ``n_exec`` / ``collided``: the pathwise gradient with the episode's end and its collision verdict frozen.  The actions and the
        in-place q, qd carry no graph; the plan-start state is a constant of it.

        ``carry=(q_in, qd_in)`` (with ``differentiable=True``): the carrying form for gradients that cross plan boundaries.  ``q_in``,
        ``qd_in`` are float64 [B, D] tensors with the bits of q, qd that may carry the graph of the plans before; the dict gains
        ``carry = dict(q=, qd=[, cond_pos=, cond_vel=])``: clones of what the launch left in q, qd (and of the condition it wrote) that
        carry this plan's graph.  The backward is still one launch (mpk_hole_reacher_rollout_vjp_cond) and returns g_q0, g_qd0 to
        ``q_in``, ``qd_in``; q, qd and ``cond_pos`` / ``cond_vel`` stay graph-free.
        """
        if spec.plant != "velocity_direct":
            raise ValueError("hole_reacher_rollout integrates plant='velocity_direct'")
        if carry is not None and not differentiable:
            raise ValueError("hole_reacher_rollout(carry=...) is the carrying form of differentiable=True")
        if differentiable and rew_fct == "unbounded":
            raise NotImplementedError("hole_reacher_rollout(differentiable=True): rew_fct='unbounded' pays on the end effector stored at "
                                      "step 180, which may belong to an earlier plan -- its gradient crosses plans and is not built")
        if differentiable and torch.is_grad_enabled() and (carry is not None or (
                (want_rewards or aggregation is not None) and any(
                    isinstance(t, torch.Tensor) and t.requires_grad for t in (des_pos, des_vel, hole)))):
            kw = dict(collision_penalty=collision_penalty, allow_self_collision=allow_self_collision,
                      allow_wall_collision=allow_wall_collision, steps_before_reward=steps_before_reward, n_steps=n_steps, step0=step0,
                      replan=replan, condition=condition, want_actions=want_actions, want_rewards=want_rewards, aggregation=aggregation,
                      rew_fct=rew_fct, reward_state=reward_state)
            B = des_vel.shape[0]
            hole_t = torch.as_tensor(hole, dtype=torch.float64, device=self.device).expand(B, 3).contiguous()
            dp, dv = (des_pos.contiguous() if des_pos is not None else None), des_vel.contiguous()
            s0 = replan[0] if replan is not None else step0
            box = {}

            def launch():
                return self.hole_reacher_rollout(spec, None if dp is None else dp.detach(), dv.detach(), q, qd, hole_t.detach(), **kw)
            task_kw = dict(rew_fct=rew_fct, collision_penalty=collision_penalty, steps_before_reward=steps_before_reward)
            if carry is not None:
                D = dv.shape[2]
                q_in, qd_in = (self._f64(t, (B, D)) for t in carry)
                outs = _HoleRolloutCarryFn.apply(self, launch, box, spec, q, qd, s0, task_kw, aggregation, dp, dv, hole_t, q_in, qd_in)
            else:
                outs = _HoleRolloutFn.apply(self, launch, box, spec, q, qd, s0, task_kw, aggregation, dp, dv, hole_t)
            outs = list(outs)
            for k in ("ret", "rewards"):
                if box[k] is not None:
                    box[k] = outs.pop(0)
            if carry is not None:
                box["carry"] = dict(zip(("q", "qd", "cond_pos", "cond_vel"), outs))
            return box
        B, T, D = des_vel.shape
        assert des_vel.dtype == torch.float32 and (des_pos is None or des_pos.dtype == torch.float32)
        assert q.dtype == torch.float64 and qd.dtype == torch.float64 and q.is_contiguous() and qd.is_contiguous()
        des_vel = des_vel.contiguous()
        des_pos = des_pos.contiguous() if des_pos is not None else None
        hole = torch.as_tensor(hole, dtype=torch.float64, device=self.device).expand(B, 3).contiguous()
        f = dict(device=self.device)
        act = torch.empty((B, T, D), dtype=torch.float32, **f) if want_actions else None
        rews = torch.empty((B, T), dtype=torch.float64, **f) if want_rewards else None
        ret = torch.empty(B, dtype=torch.float64, **f) if aggregation is not None else None
        n_exec = torch.empty(B, dtype=torch.int32, **f)
        coll = torch.empty(B, dtype=torch.uint8, **f)
        succ = torch.empty(B, dtype=torch.uint8, **f)
        rew = _lib.hole_rew_fct(rew_fct, steps_before_reward)
        if rew_fct == "unbounded":
            if reward_state is None:
                raise ValueError("rew_fct='unbounded' keeps the end effector of step 180 across plans: pass reward_state "
                                 "(float64 [B, 2] on the device)")
            assert reward_state.dtype == torch.float64 and reward_state.shape == (B, 2) and reward_state.is_contiguous()
        task = _lib.mpk_hole_task(float(collision_penalty), int(bool(allow_self_collision)), int(bool(allow_wall_collision)),
                                  int(steps_before_reward), rew)
        st = done_out = cp = cv = None
        if replan is not None:
            traj_steps, plan_steps, done, every, max_planning_times, horizon = replan
            assert traj_steps.dtype == torch.int32 and plan_steps.dtype == torch.int32 and done.dtype == torch.uint8
            done_out = torch.empty(B, dtype=torch.uint8, **f)
            if condition:
                cp, cv = (torch.empty((B, D), dtype=torch.float32, **f) for _ in range(2))
            st = _lib.mpk_replan_state(traj_steps.data_ptr(), plan_steps.data_ptr(), done.data_ptr(), n_exec.data_ptr(),
                                       done_out.data_ptr(), _dptr(cp), _dptr(cv), int(every),
                                       int(min(max_planning_times, 2 ** 31 - 1)), int(horizon), 0)
        if n_steps is not None:
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).contiguous()
        if step0 is not None:
            step0 = step0.to(device=self.device, dtype=torch.int32).contiguous()
        agg = _lib.AGG_MODES[aggregation] if aggregation is not None else 0
        _lib.check(self._lib.mpk_hole_reacher_rollout2(
            self._h, C.byref(spec.c), _dptr(des_pos), des_vel.data_ptr(), q.data_ptr(), qd.data_ptr(), _dptr(n_steps), _dptr(step0),
            C.byref(task), hole.data_ptr(), _dptr(act), _dptr(rews), _dptr(ret), agg, n_exec.data_ptr(), coll.data_ptr(),
            succ.data_ptr(), C.byref(st) if st is not None else None, _dptr(reward_state) if rew_fct == "unbounded" else None,
            B, T, self._stream()))
        return dict(actions=act, rewards=rews, ret=ret, n_exec=n_exec, collided=coll, success=succ, done=done_out, cond_pos=cp,
                    cond_vel=cv)

    def reacher_reset(self, env: str, q: torch.Tensor, qd: torch.Tensor, traj_steps: torch.Tensor, plan_steps: torch.Tensor,
                      done: torch.Tensor, rng: torch.Tensor, task_out: torch.Tensor, *, seeds=None, seed_base: Optional[int] = None,
                      random_start: bool = True, target=None, hole_width=None, hole_x=None, hole_depth=None,
                      cond: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """
        The seeded resets of SimpleReacher (``env`` "simple_reacher") / HoleReacher ("hole_reacher") for B device-resident episodes in
        one launch (mpk.h: mpk_reacher_reset): what ``episode_reset`` writes, plus the goal [B, 2] / hole [B, 3] into ``task_out`` and
        each episode's numpy generator into ``rng`` (int64 [B, 5], the words of mpk_nprng_state; ``nprng_state`` reads it).
        ``seed_base`` seeds episode b with seed_base + b, ``seeds`` (uint64 [B] on the device, as int64) one seed per episode; neither
        continues every episode's stream.  The kwargs are the env's: None = drawn.  Everything in place; allocates nothing.
        """
        t = self._reset_task(env, q, qd, traj_steps, plan_steps, done, rng, task_out, seeds, seed_base, random_start, target,
                             hole_width, hole_x, hole_depth)
        B = q.shape[0]
        cp, cv = cond if cond is not None else (None, None)
        _lib.check(self._lib.mpk_reacher_reset(self._h, C.byref(t), _dptr(seeds), rng.data_ptr(), q.data_ptr(), qd.data_ptr(),
                                               _dptr(cp), _dptr(cv), traj_steps.data_ptr(), plan_steps.data_ptr(), done.data_ptr(),
                                               task_out.data_ptr(), B, self._stream()))

    @staticmethod
    def _reset_task(env, q, qd, traj_steps, plan_steps, done, rng, task_out, seeds, seed_base, random_start, target, hole_width, hole_x,
                    hole_depth):
        """the argument checks of a reacher reset and its mpk_reacher_reset_task"""
        B, D = q.shape
        for t, dt_ in ((q, torch.float64), (qd, torch.float64), (traj_steps, torch.int32), (plan_steps, torch.int32),
                       (done, torch.uint8), (rng, torch.int64), (task_out, torch.float64)):
            assert t.dtype == dt_ and t.is_contiguous() and t.shape[0] == B
        assert tuple(rng.shape) == (B, 5) and tuple(task_out.shape) == (B, 2 if env == "simple_reacher" else 3)
        if seeds is not None:
            assert seeds.dtype == torch.int64 and seeds.is_contiguous() and tuple(seeds.shape) == (B,)
        nan = float("nan")
        opt = lambda v: nan if v is None else float(v)        # noqa: E731
        t = _lib.mpk_reacher_reset_task()
        t.env = _lib.RESET_ENVS[env]
        t.random_start = int(bool(random_start))
        t.target[0], t.target[1] = (nan, nan) if target is None else (float(target[0]), float(target[1]))
        t.hole_width, t.hole_x, t.hole_depth = opt(hole_width), opt(hole_x), opt(hole_depth)
        t.seed_base_given = int(seed_base is not None)
        t.seed_base = int(seed_base) if seed_base is not None else 0
        return t

    def reacher_autoreset(self, env: str, q: torch.Tensor, qd: torch.Tensor, traj_steps: torch.Tensor, plan_steps: torch.Tensor,
                          done: torch.Tensor, rng: torch.Tensor, task: torch.Tensor, *, mask: Optional[torch.Tensor] = None,
                          observe: bool = True, col_mask: int = 0, time_div: float = 0.0, seeds=None, seed_base: Optional[int] = None,
                          random_start: bool = True, target=None, hole_width=None, hole_x=None, hole_depth=None,
                          cond: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, reset_mask: Optional[torch.Tensor] = None,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """
        The per-episode autoreset of a vector step in one launch (mpk.h: mpk_reacher_autoreset): ``final_obs`` [B, n_out] = the
        observation ``reacher_observation`` gives on entry; the episodes selected by ``mask`` (uint8 / bool [B] on the device; None:
        the ``done`` bytes) are reset as ``reacher_reset`` resets them (same arguments, in place; ``task`` is read and written); ``obs``
        = the new episode's first observation for them, ``final_obs`` for the others.  Returns (final_obs, obs, reset_mask) -- uint8
        [B], 1 = reset --; ``observe=False`` is the masked reset alone and returns (None, None, reset_mask).  ``out`` = (final_obs,
        obs) and ``reset_mask`` are allocated unless given.
        """
        t = self._reset_task(env, q, qd, traj_steps, plan_steps, done, rng, task, seeds, seed_base, random_start, target, hole_width,
                             hole_x, hole_depth)
        B = q.shape[0]
        if mask is not None:
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
            assert mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (B,) and mask.device == q.device
        if reset_mask is None:
            reset_mask = torch.empty(B, dtype=torch.uint8, device=self.device)
        assert reset_mask.dtype == torch.uint8 and reset_mask.is_contiguous() and tuple(reset_mask.shape) == (B,)
        c = final = obs = None
        if observe:
            c, n_out = self._obs_cfg(env, col_mask, time_div)
            final, obs = out if out is not None else (torch.empty((B, n_out), dtype=torch.float32, device=self.device) for _ in range(2))
            for o in (final, obs):
                assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (B, n_out)
            assert final.data_ptr() != obs.data_ptr() or B == 0
        cp, cv = cond if cond is not None else (None, None)
        _lib.check(self._lib.mpk_reacher_autoreset(
            self._h, C.byref(t), C.byref(c) if c is not None else None, _dptr(seeds), rng.data_ptr(), q.data_ptr(), qd.data_ptr(),
            _dptr(cp), _dptr(cv), traj_steps.data_ptr(), plan_steps.data_ptr(), done.data_ptr(), task.data_ptr(), _dptr(mask),
            reset_mask.data_ptr(), _dptr(final), _dptr(obs), B, self._stream()))
        return final, obs, reset_mask

    def reacher_env_step(self, env: str, actions: torch.Tensor, q: torch.Tensor, qd: torch.Tensor, traj_steps: torch.Tensor,
                         rng: torch.Tensor, task: torch.Tensor, out: dict, *, dt: float, max_episode_steps: int,
                         autoreset: bool = True, steps_before_reward: int = 199, rew_fct: str = "simple",
                         collision_penalty: float = 100.0, allow_self_collision: bool = False, allow_wall_collision: bool = False,
                         reward_state: Optional[torch.Tensor] = None, random_start: bool = True, target=None, hole_width=None,
                         hole_x=None, hole_depth=None):
        """
        One ``env.step(action)`` of the step-based reacher envs for B device-resident episodes plus the same-step autoreset, in one
        launch (mpk.h: mpk_reacher_env_step).  ``actions`` float32 [B, D] (not clipped); q, qd, traj_steps, rng, task (and
        ``reward_state`` for rew_fct "unbounded") are updated in place.  ``out`` holds the result tensors: reward float64 [B],
        terminated / truncated / reset_mask uint8 [B], final_obs / obs float32 [B, n], and for "hole_reacher" is_collided / is_success
        uint8 [B].  The reset kwargs are the env's (None = drawn), as for ``reacher_reset``.  Allocates nothing.
        """
        B, D = q.shape
        hole = env == "hole_reacher"
        n = 3 * D + (4 if hole else 3)
        assert actions.dtype == torch.float32 and actions.is_contiguous() and tuple(actions.shape) == (B, D)
        for t, dt_ in ((q, torch.float64), (qd, torch.float64), (traj_steps, torch.int32), (rng, torch.int64), (task, torch.float64),
                       (out["reward"], torch.float64)):
            assert t.dtype == dt_ and t.is_contiguous() and t.shape[0] == B
        assert tuple(rng.shape) == (B, 5) and tuple(task.shape) == (B, 3 if hole else 2)
        for key in ("terminated", "truncated", "reset_mask") + (("is_collided", "is_success") if hole else ()):
            assert out[key].dtype == torch.uint8 and out[key].is_contiguous() and tuple(out[key].shape) == (B,)
        for key in ("final_obs", "obs"):
            assert out[key].dtype == torch.float32 and out[key].is_contiguous() and tuple(out[key].shape) == (B, n)
        rew = _lib.hole_rew_fct(rew_fct, steps_before_reward) if hole else 0
        if hole and rew_fct == "unbounded":
            if reward_state is None:
                raise ValueError("rew_fct='unbounded' keeps the end effector of step 180 across steps: pass reward_state "
                                 "(float64 [B, 2] on the device)")
            assert reward_state.dtype == torch.float64 and tuple(reward_state.shape) == (B, 2) and reward_state.is_contiguous()
        nan = float("nan")
        opt = lambda v: nan if v is None else float(v)        # noqa: E731
        rt = _lib.mpk_reacher_reset_task()
        rt.env = _lib.RESET_ENVS[env]
        rt.random_start = int(bool(random_start))
        rt.target[0], rt.target[1] = (nan, nan) if target is None else (float(target[0]), float(target[1]))
        rt.hole_width, rt.hole_x, rt.hole_depth = opt(hole_width), opt(hole_x), opt(hole_depth)
        st = _lib.mpk_env_step_task()
        st.env, st.n_links, st.dt = rt.env, D, float(dt)
        st.max_episode_steps, st.autoreset = int(max_episode_steps), int(bool(autoreset))
        st.hole = _lib.mpk_hole_task(float(collision_penalty), int(bool(allow_self_collision)), int(bool(allow_wall_collision)),
                                     int(steps_before_reward), rew)
        _lib.check(self._lib.mpk_reacher_env_step(
            self._h, C.byref(st), C.byref(rt), actions.data_ptr(), rng.data_ptr(), q.data_ptr(), qd.data_ptr(), traj_steps.data_ptr(),
            task.data_ptr(), _dptr(reward_state) if hole and rew_fct == "unbounded" else None, out["reward"].data_ptr(),
            out["terminated"].data_ptr(), out["truncated"].data_ptr(), _dptr(out.get("is_collided")), _dptr(out.get("is_success")),
            out["reset_mask"].data_ptr(), out["final_obs"].data_ptr(), out["obs"].data_ptr(), B, self._stream()))
        return out

    def _obs_cfg(self, env: str, col_mask: int, time_div: float):
        c = _lib.mpk_obs_cfg()
        c.env = _lib.RESET_ENVS[env]
        c.n_links = self.num_dof
        c.col_mask = int(col_mask)
        c.time_div = float(time_div)
        n_full = 3 * self.num_dof + (4 if env == "hole_reacher" else 3)
        n_out = bin(int(col_mask)).count("1") if col_mask else n_full
        return c, n_out + int(time_div > 0)

    def reacher_observation(self, env: str, q: torch.Tensor, qd: torch.Tensor, task: torch.Tensor, steps: torch.Tensor, *,
                            col_mask: int = 0, time_div: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """
        The current observation of B reacher episodes (``env`` "simple_reacher" / "hole_reacher"; mpk.h: mpk_reacher_observation) as
        float32 [B, n_out] on the device, in one launch: the env's _get_obs() row from q, qd (float64 [B, D]), the goal [B, 2] / hole
        [B, 3] ``task`` and the step counter ``steps`` (int32 [B]); ``col_mask`` bit c keeps column c of the full row (0 = all),
        ``time_div`` > 0 appends steps / time_div.  Allocates ``out`` unless given.
        """
        B = q.shape[0]
        for t, dt_ in ((q, torch.float64), (qd, torch.float64), (task, torch.float64), (steps, torch.int32)):
            assert t.dtype == dt_ and t.is_contiguous() and t.shape[0] == B
        c, n_out = self._obs_cfg(env, col_mask, time_div)
        if out is None:
            out = torch.empty((B, n_out), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, n_out)
        _lib.check(self._lib.mpk_reacher_observation(self._h, C.byref(c), q.data_ptr(), qd.data_ptr(), task.data_ptr(),
                                                     steps.data_ptr(), out.data_ptr(), B, self._stream()))
        return out

    def reacher_step_observations(self, env: str, spec: RolloutSpec, des_pos: Optional[torch.Tensor], des_vel: Optional[torch.Tensor],
                                  q0: torch.Tensor, qd0: torch.Tensor, task: torch.Tensor, n_exec: torch.Tensor, step0: torch.Tensor, *,
                                  col_mask: int = 0, time_div: float = 0.0, end_state: bool = False):
        """
        ``infos['step_observations']`` of a verbose >= 2 step for B reacher episodes (mpk.h: mpk_reacher_step_observations): one launch
        replays the ``n_exec`` executed steps of the plan (des_pos, des_vel) [B, T, D] from the plan-start state (q0, qd0) with the
        rollout's controller and plant (``spec``: the double integrator for "simple_reacher", 'velocity_direct' for "hole_reacher"),
        starting at env step ``step0``, and writes the observation after every step: float32 [B, T, n_out], 0 behind n_exec.
        ``end_state`` also returns the replayed (q, qd) -- the state the rollout left.
        """
        ref = des_vel if des_vel is not None else des_pos
        B, T, D = ref.shape
        for t, dt_ in ((q0, torch.float64), (qd0, torch.float64), (task, torch.float64), (n_exec, torch.int32), (step0, torch.int32)):
            assert t.dtype == dt_ and t.is_contiguous() and t.shape[0] == B
        des_pos = des_pos.contiguous() if des_pos is not None else None
        des_vel = des_vel.contiguous() if des_vel is not None else None
        c, n_out = self._obs_cfg(env, col_mask, time_div)
        out = torch.empty((B, T, n_out), dtype=torch.float32, device=self.device)
        qe, qde = (torch.empty((B, D), dtype=torch.float64, device=self.device) for _ in range(2)) if end_state else (None, None)
        _lib.check(self._lib.mpk_reacher_step_observations(
            self._h, C.byref(c), C.byref(spec.c), _dptr(des_pos), _dptr(des_vel), q0.data_ptr(), qd0.data_ptr(), task.data_ptr(),
            n_exec.data_ptr(), step0.data_ptr(), out.data_ptr(), _dptr(qe), _dptr(qde), B, T, self._stream()))
        return (out, qe, qde) if end_state else out

    def condition_gather(self, pos: torch.Tensor, vel: torch.Tensor, seg_len: torch.Tensor,
                         out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """desired (pos, vel) [B, D] at the last executed step of each episode (condition_on_desired)"""
        B, T, D = pos.shape
        cp, cv = out if out is not None else (torch.empty((B, D), dtype=torch.float32, device=self.device),
                                              torch.empty((B, D), dtype=torch.float32, device=self.device))
        _lib.check(self._lib.mpk_condition_gather(self._h, pos.data_ptr(), vel.data_ptr(), seg_len.data_ptr(),
                                                  cp.data_ptr(), cv.data_ptr(), B, T, self._stream()))
        return cp, cv

    def unpin_tables(self):
        """release the basis-table slots pinned by captured graphs (mpk.h: mpk_unpin_tables); those graphs are dead then"""
        _lib.check(self._lib.mpk_unpin_tables(self._h))

    def replan_advance(self, traj_steps: torch.Tensor, plan_steps: torch.Tensor, done: torch.Tensor, every: int,
                       max_planning_times: int, horizon: int) -> torch.Tensor:
        """Integer replanning bookkeeping on device; returns seg_len int32 [B] and updates the state tensors in place."""
        B = traj_steps.shape[0]
        seg = torch.empty(B, dtype=torch.int32, device=self.device)
        mpt = int(min(max_planning_times, 2 ** 31 - 1))
        _lib.check(self._lib.mpk_replan_advance(self._h, traj_steps.data_ptr(), plan_steps.data_ptr(), seg.data_ptr(),
                                                done.data_ptr(), int(every), mpt, int(horizon), self.num_steps, B,
                                                self._stream()))
        return seg

    def traj_validity(self, pos: torch.Tensor, pos_low, pos_high, params: Optional[torch.Tensor] = None,
                      tau_bound=None, delay_bound=None, with_penalty: bool = False):
        """valid bool [B]; with_penalty: also the float64 reward of an invalid plan (table_tennis_env.py:282-289)"""
        B, T, D = pos.shape
        if with_penalty:
            lo_p, lo_k = _dvec(pos_low, D)
            hi_p, hi_k = _dvec(pos_high, D)
            check = int(params is not None and tau_bound is not None and delay_bound is not None)
            tb = (C.c_double * 2)(*(tau_bound if check else (0.0, 0.0)))
            db = (C.c_double * 2)(*(delay_bound if check else (0.0, 0.0)))
            valid = torch.empty(B, dtype=torch.uint8, device=self.device)
            pen = torch.empty(B, dtype=torch.float64, device=self.device)
            _lib.check(self._lib.mpk_traj_validity_penalty(
                self._h, pos.contiguous().data_ptr(), _dptr(params), C.cast(lo_p, C.c_void_p),
                C.cast(hi_p, C.c_void_p), check, C.cast(tb, C.c_void_p), C.cast(db, C.c_void_p), valid.data_ptr(),
                pen.data_ptr(), B, T, self._stream()))
            return valid.bool(), pen
        lo_p, lo_k = _dvec(pos_low, D)
        hi_p, hi_k = _dvec(pos_high, D)
        check = int(params is not None and tau_bound is not None and delay_bound is not None)
        tb = (C.c_double * 2)(*(tau_bound if check else (0.0, 0.0)))
        db = (C.c_double * 2)(*(delay_bound if check else (0.0, 0.0)))
        valid = torch.empty(B, dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.mpk_traj_validity(self._h, pos.contiguous().data_ptr(), _dptr(params),
                                               C.cast(lo_p, C.c_void_p), C.cast(hi_p, C.c_void_p), check,
                                               C.cast(tb, C.c_void_p), C.cast(db, C.c_void_p), valid.data_ptr(), B, T,
                                               self._stream()))
        return valid.bool()

    # ---- introspection -----------------------------------------------------------------------------------------
    def prodmp_tables(self):
        n = self._lib.mpk_prodmp_tables(self._h, None, None, None, None, None, None, None)
        _lib.check(n)
        K = self.config.num_basis + 1
        arrs = [np.empty(n, np.float64) for _ in range(4)] + [np.empty((n, K), np.float64) for _ in range(2)] + \
               [np.empty(K, np.float64)]
        _lib.check(self._lib.mpk_prodmp_tables(self._h, *[a.ctypes.data for a in arrs]))
        return dict(zip(("y1", "y2", "dy1", "dy2", "pos_basis", "vel_basis", "scale"), arrs))

    def prodmp_indices(self, init_time: float = 0.0):
        T = self.num_steps
        idx = np.empty(T, np.int32)
        ib = np.empty(1, np.int32)
        _lib.check(self._lib.mpk_prodmp_indices(self._h, float(init_time), idx.ctypes.data, ib.ctypes.data,
                                                self._stream()))
        return idx, int(ib[0])

    def scaled_basis(self, times) -> np.ndarray:
        """basis functions x their parameter scale at ``times`` [n] -> float32 [n, K] (mpk.h: mpk_scaled_basis)"""
        t = np.ascontiguousarray(np.asarray(times, np.float32).reshape(-1))
        K = self.config.num_basis + (1 if self.mp_type == "prodmp" else 0)
        out = np.empty((t.shape[0], K), np.float32)
        _lib.check(self._lib.mpk_scaled_basis(self._h, t.ctypes.data, int(t.shape[0]), out.ctypes.data, self._stream()))
        return out

    def last_kernel(self) -> str:
        return self._lib.mpk_last_kernel(self._h).decode()
