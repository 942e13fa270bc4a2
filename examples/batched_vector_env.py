#!/usr/bin/env python3
"""
Contextual random search on `fancy_ProDMP/HoleReacher-v0`, written only against the vector-env front door: `make_batched_vec(id, n)`
gives `n` device-resident episodes with the id's own dt, duration, basis, gains, action bounds, reward and hole settings -- no constant
is typed here.  Every `step(actions)` runs one whole episode of every env (plan, rollout with collision break, reward) and, same-step
autoreset, hands back the first observation of the next episodes: the context (start pose, hole width, offset to the hole's bottom) the
next parameters are chosen for.

The policy is linear in the context, params = W [context, 1]; each iteration perturbs W once per env, evaluates every perturbation on
that env's own freshly drawn context, and moves W along the return-weighted perturbations (the better half, ranks as weights).
Everything stays on the GPU; the only read-back is the printed statistics.

    python examples/batched_vector_env.py [--envs 4096] [--iters 30] [--seed 0] [--graph]

`--graph` replays the whole vector step as one hipGraph (`BatchedVectorEnv.capture`).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import make_batched_vec  # noqa: E402

ENV_ID = "fancy_ProDMP/HoleReacher-v0"


def search(envs: int = 4096, iters: int = 30, seed: int = 0, graph: bool = False, verbose: bool = True):
    vec = make_batched_vec(ENV_ID, envs)
    n_obs, n_act = vec.single_observation_space.shape[0], vec.single_action_space.shape[0]
    dev = vec.bb.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = torch.zeros((n_act, n_obs + 1), device=dev)
    sigma, lr, elite = 0.3, 0.5, envs // 2
    obs, _ = vec.reset(seed=seed)
    step = vec.step
    if graph:
        captured = vec.capture()

        def step(actions):
            captured.actions.copy_(actions)
            return captured.replay()
    history = []
    t0 = time.perf_counter()
    for it in range(iters):
        context = torch.cat([obs, torch.ones((envs, 1), device=dev)], dim=1)
        noise = sigma * torch.randn((envs, n_act, n_obs + 1), generator=gen, device=dev)
        noise[0] = 0.0                                              # env 0 evaluates the unperturbed policy
        actions = torch.einsum("bpc,bc->bp", W + noise, context)
        obs, rewards, terminated, truncated, info = step(actions)
        best = rewards.topk(elite).indices
        weights = torch.linspace(1.0, 0.0, elite, device=dev, dtype=noise.dtype)
        W = W + lr * (weights[:, None, None] * noise[best]).sum(0) / weights.sum()
        history.append((float(rewards[0]), float(rewards.mean()), float(info["is_collided"].float().mean()),
                        float(info["is_success"].float().mean())))
        if verbose:
            print(f"iteration {it:3d}: policy return {history[-1][0]:10.3f}   population mean {history[-1][1]:10.3f}   "
                  f"collided {history[-1][2]:5.1%}   in the hole {history[-1][3]:5.1%}")
    torch.cuda.synchronize()
    if verbose:
        dt = time.perf_counter() - t0
        print(f"{iters} iterations x {envs} episodes in {dt:.2f} s = {iters * envs / dt:.3e} episodes/s")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    search(a.envs, a.iters, a.seed, a.graph)
