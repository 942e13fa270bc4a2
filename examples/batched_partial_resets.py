#!/usr/bin/env python3
"""
Random search on `fancy_ProMP/HoleReacher-v0` with replanning (`replanning_every=50`: a vector step is one plan of 50 env steps, an
episode is four of them), once in the default mode of `make_batched_vec` and once with `partial_resets=True`.

In the default mode an episode that collides stays done until the last episode of the batch reaches the step limit: its lane executes
nothing in the vector steps in between.  With `partial_resets=True` it starts anew in the step that ended it, from its own stream, and
`info["_final_obs"]` marks the rows whose `info["final_obs"]` closes an episode.  The script prints the executed env steps of every
vector step in both modes, and the share of lanes that executed nothing.

    python examples/batched_partial_resets.py [--envs 4096] [--steps 16] [--seed 0] [--scale 0.3] [--graph]

`--graph` replays the partial-resets step as one hipGraph (`BatchedVectorEnv.capture`: allowed with replanning in this mode only).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import make_batched_vec  # noqa: E402

ENV_ID = "fancy_ProMP/HoleReacher-v0"
EVERY = 50


def run(partial_resets: bool, envs: int, steps: int, seed: int, scale: float, graph: bool = False, verbose: bool = True):
    vec = make_batched_vec(ENV_ID, envs, partial_resets=partial_resets,
                           mp_config_override={"black_box_kwargs": {"replanning_every": EVERY}})
    dev = vec.bb.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    n_act = vec.single_action_space.shape[0]
    vec.reset(seed=seed)
    step = vec.step
    if graph and partial_resets:
        captured = vec.capture()

        def step(actions):
            captured.actions.copy_(actions)
            return captured.replay()
    executed, idle, best = [], [], -float("inf")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        actions = scale * torch.randn((envs, n_act), generator=gen, device=dev)
        obs, rewards, terminated, truncated, info = step(actions)
        length = info["trajectory_length"]
        executed.append(length.sum())
        idle.append((length == 0).float().mean())
        best = max(best, float(rewards.max()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    executed = [int(e) for e in executed]
    idle = [float(i) for i in idle]
    if verbose:
        mode = "partial_resets=True " if partial_resets else "reset all together  "
        print(f"{mode} executed env steps per vector step: {executed}")
        print(f"{mode} idle lanes per vector step: {' '.join(f'{i:.0%}' for i in idle)}")
        print(f"{mode} {sum(executed)} env steps in {dt:.3f} s = {sum(executed) / dt:.3e} env steps/s, best plan return {best:.2f}")
    return executed, idle


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scale", type=float, default=0.3)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    for mode in (False, True):
        run(mode, a.envs, a.steps, a.seed, a.scale, a.graph)
