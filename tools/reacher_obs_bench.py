#!/usr/bin/env python3
"""
Reacher observations on the device: k_reacher_obs (mpk_reacher_observation, the context row of the registered ids) and
k_reacher_step_obs (mpk_reacher_step_observations, full rows of every executed step) for SimpleReacher (2 links, torque double
integrator) and HoleReacher (5 links, direct velocity plant), beside the rollout kernel of the same step at the same B.  Captured graphs
of 20 launches, median of rounds (tools/closed_bench.py graph_time).  Then BatchedBlackBox(reward="hole_reacher") at 4 096 episodes:
the eager verbose = 2 step with and without observations=True, and a captured episode of one plan.
    python tools/reacher_obs_bench.py [B ...] [--once]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import BatchedBlackBox, RolloutSpec, TrajectoryEngine, _gym  # noqa: E402
from tools.closed_bench import graph_time  # noqa: E402
from tools.hole_reacher_bench import plans  # noqa: E402

T = 200
LIM = float(np.float32(2 * np.pi))
HBM = 8.0e12          # bytes / s, the MI355X's peak HBM bandwidth


def family(kind, B):
    D = 5 if kind == "hole_reacher" else 2
    eng = TrajectoryEngine("promp", "linear", "zero_rbf", D, 5, dt=0.01, duration=2.0, tau=2.0, num_basis_zero_start=1, device=0)
    dev = dict(device="cuda")
    if kind == "hole_reacher":
        q0, vel, hole = plans(B)
        spec = RolloutSpec("velocity", D, 0.0, 0.0, -LIM, LIM, plant="velocity_direct", dt=0.01)
        pos = torch.zeros((B, T, D), dtype=torch.float32, **dev)
        vel = torch.as_tensor(vel, **dev)
        task = torch.as_tensor(hole, dtype=torch.float64, **dev)
        col_mask = (1 << (3 * D + 3)) - 1           # the context row of random start, width drawn: all but steps
    else:
        rng = np.random.default_rng(0)
        q0 = np.zeros((B, D)); q0[:, 0] = rng.uniform(np.pi / 4, 3 * np.pi / 4, B)
        spec = RolloutSpec("motor", D, 0.6, 0.075, -1000.0, 1000.0, plant="double_integrator", dt=0.01)
        pos = torch.as_tensor(rng.standard_normal((B, T, D)).cumsum(1).astype(np.float32) * 0.05, **dev)
        vel = torch.as_tensor(rng.standard_normal((B, T, D)).astype(np.float32), **dev)
        task = torch.as_tensor(rng.uniform(-1, 1, (B, 2)), dtype=torch.float64, **dev)
        col_mask = (1 << (3 * D + 2)) - 1           # the context row of random start: all but steps
    q0 = torch.as_tensor(q0, dtype=torch.float64, **dev)
    qd0 = torch.zeros_like(q0)
    q, qd = q0.clone(), qd0.clone()
    n_exec = torch.full((B,), T, dtype=torch.int32, **dev)
    step0 = torch.zeros(B, dtype=torch.int32, **dev)
    steps = torch.full((B,), T, dtype=torch.int32, **dev)
    out = torch.empty((B, bin(col_mask).count("1")), dtype=torch.float32, **dev)

    def obs():
        eng.reacher_observation(kind, q, qd, task, steps, col_mask=col_mask, out=out)

    def step_obs():
        eng.reacher_step_observations(kind, spec, pos, vel, q0, qd0, task, n_exec, step0)

    def rollout():
        q.copy_(q0); qd.copy_(qd0)
        if kind == "hole_reacher":
            eng.hole_reacher_rollout(spec, None, vel, q, qd, task, n_steps=n_exec, step0=step0, want_actions=False, want_rewards=False)
        else:
            eng.reacher_rollout(spec, pos, vel, q, qd, task, n_steps=n_exec, step0=step0)

    n_full = 3 * D + (4 if kind == "hole_reacher" else 3)
    if "--once" in sys.argv:          # one launch of each (counter collection: rocprofv3 --pmc WRITE_SIZE FETCH_SIZE)
        obs(); step_obs(); rollout()
        torch.cuda.synchronize()
        return dict(kind=kind, B=B, step_obs_bytes_written=B * T * n_full * 4, obs_bytes_written=out.numel() * 4)
    t_obs, t_step, t_roll = graph_time(obs), graph_time(step_obs), graph_time(rollout)
    written = B * T * n_full * 4
    read = B * T * D * 4 * (1 if kind == "hole_reacher" else 2)
    return dict(kind=kind, B=B, obs_us=t_obs * 1e6, step_obs_us=t_step * 1e6, rollout_us=t_roll * 1e6,
                step_obs_bytes_written=written, step_obs_roofline_share=(written + read) / HBM / t_step,
                step_obs_over_rollout=t_step / t_roll)


def eager_and_graph(B=4096, reps=20):
    env = _gym.make("fancy_ProMP/HoleReacher-v0")
    params = torch.as_tensor(np.random.default_rng(1).standard_normal((B, env.action_space.shape[0])).astype(np.float32) * 0.1,
                             device="cuda")
    res = {}
    for flag in (False, True):
        bb = BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=0.01, duration=2.0, act_low=-LIM, act_high=LIM,
                             plant="velocity_direct", reward="hole_reacher", max_episode_steps=200, observations=flag)
        bb.reset(seed=0)
        for _ in range(3):
            bb.reset(sample=True); bb.step(params)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            bb.reset(sample=True); bb.step(params)
        torch.cuda.synchronize()
        res[f"eager_reset_step_us obs={flag}"] = (time.perf_counter() - t0) / reps * 1e6
        g = bb.capture_episode(1, sample=True)
        g.params[0].copy_(params)
        g.replay(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            g.replay()
        torch.cuda.synchronize()
        res[f"graph_replay_us obs={flag}"] = (time.perf_counter() - t0) / reps * 1e6
    return res


def main():
    batches = [int(a) for a in sys.argv[1:] if a.isdigit()] or [1024, 8192, 65536]
    torch.cuda.set_device(0)
    for kind in ("simple_reacher", "hole_reacher"):
        for B in batches:
            print(json.dumps(family(kind, B)), flush=True)
    if "--once" not in sys.argv:
        print(json.dumps(eager_and_graph()), flush=True)


if __name__ == "__main__":
    main()
