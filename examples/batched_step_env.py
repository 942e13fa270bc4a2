#!/usr/bin/env python3
"""
The step-based twin of the black-box examples: `fancy/HoleReacher-v0` as a device vector env (`make_batched_step_vec(id, n)`), one
environment step of every episode per kernel launch.  A linear policy on the observation (or `--random`: uniform draws from the
action space) drives `n` arms for `--steps` environment steps through the captured step -- actions are written into the graph's
buffer, one replay is one launch (mpk_reacher_env_step: plant, collisions, reward, TimeLimit, same-step autoreset, observations).
Everything stays on the GPU; the only read-back is the printed statistics.

    python examples/batched_step_env.py [--envs 4096] [--steps 2000] [--seed 0] [--random] [--eager]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import make_batched_step_vec  # noqa: E402

ENV_ID = "fancy/HoleReacher-v0"


def run(envs: int = 4096, steps: int = 2000, seed: int = 0, random: bool = False, eager: bool = False, verbose: bool = True):
    vec = make_batched_step_vec(ENV_ID, envs)
    n_obs, n_act = vec.single_observation_space.shape[0], vec.single_action_space.shape[0]
    dev = vec.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    high = torch.as_tensor(vec.single_action_space.high, device=dev)
    W = 0.05 * torch.randn((n_obs, n_act), generator=gen, device=dev)
    W[-1] = 0.0                                                     # (the step counter is not a feature)
    obs, _ = vec.reset(seed=seed)
    captured = None if eager else vec.capture()
    actions = torch.zeros((envs, n_act), device=dev) if eager else captured.actions
    returns = torch.zeros(envs, dtype=torch.float64, device=dev)
    episodes = torch.zeros((), dtype=torch.int64, device=dev)
    collisions = torch.zeros((), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        if random:
            actions.uniform_(-1.0, 1.0, generator=gen).mul_(high)
        else:
            torch.clamp(obs @ W, -high, high, out=actions)
        obs, rewards, terminated, truncated, info = vec.step(actions) if eager else captured.replay()
        returns += rewards
        episodes += info["_final_obs"].sum()
        collisions += terminated.sum()
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    rate = envs * steps / wall
    if verbose:
        print(f"{ENV_ID}: {envs} envs x {steps} steps in {wall:.3f} s = {rate / 1e6:.2f} M env steps / s "
              f"({'eager' if eager else 'captured'} step, {'random' if random else 'linear'} policy)")
        print(f"episodes finished {int(episodes)}, of them collided {int(collisions)}, mean reward per step "
              f"{float(returns.mean()) / steps:.4f}")
    return rate


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--eager", action="store_true")
    a = ap.parse_args()
    run(a.envs, a.steps, a.seed, a.random, a.eager)
