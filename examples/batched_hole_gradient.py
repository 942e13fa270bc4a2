#!/usr/bin/env python3
"""
Gradient ascent on the return of `fancy_ProDMP/HoleReacher-v0`, all on the device.

HoleReacher's return jumps where a collision starts and where the episode's end moves, so the gradient taken here is the one
`collision_gradient="frozen"` defines: each episode's end and collision verdict are held at what the forward found, and everything else
-- plan, PD controller, clip, direct-velocity plant, the squared distance to the hole's bottom, the acceleration cost -- is
differentiated.  The collision penalty is a constant of that gradient; the distance paid on the colliding step still pulls the arm
towards the hole.  Every episode of the batch (its own start pose and hole, drawn by the seeded device reset) gets its own ProDMP
parameter vector, and Adam climbs the return through `BatchedBlackBox.step(params, differentiable=True)`: the plain step's two
launches forward, two launches backward (`mpk_hole_reacher_rollout_vjp`, `mpk_trajectory_vjp`).

This gradient does not see a collision coming: followed blindly it steers many arms through the floor on their way to the hole (run
with `--no-safeguard` and watch the collided fraction).  So the return decides what the gradient proposed: an episode whose return
fell below its best so far goes back to its best parameters (the forward of the next iteration is the check, nothing extra is
launched).  Prints the mean return of the proposals, the mean of the best returns and the collided fraction of every iteration.

    python examples/batched_hole_gradient.py [--envs 4096] [--iters 100] [--lr 0.02] [--seed 0] [--no-safeguard]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import make_batched  # noqa: E402

ID = "fancy_ProDMP/HoleReacher-v0"


def optimise(envs: int = 4096, iters: int = 100, lr: float = 0.02, seed: int = 0, verbose: bool = True, safeguard: bool = True):
    """returns ((mean return, collided fraction) of the initial parameters, the same for what ``iters`` Adam steps leave -- with the
    safeguard every episode's best parameters) on the same seeded episodes"""
    bb = make_batched(ID, envs, observations=False, collision_gradient="frozen")
    params = torch.zeros((envs, bb.engine.num_params), device=bb.device, requires_grad=True)
    opt = torch.optim.Adam([params], lr=lr)
    best_ret = torch.full((envs,), -float("inf"), dtype=torch.float64, device=bb.device)
    best_params = params.detach().clone()
    first = None
    t0 = time.perf_counter()
    for it in range(iters):
        bb.reset(seed=seed)                      # the same episodes every iteration
        out = bb.step(params, differentiable=True)
        rets = out["rewards"]
        opt.zero_grad(set_to_none=True)
        (-rets.mean()).backward()
        with torch.no_grad():
            better = rets.detach() > best_ret
            best_ret = torch.where(better, rets.detach(), best_ret)
            best_params[better] = params.detach()[better]
        opt.step()
        if safeguard:
            with torch.no_grad():                # a proposal that lost return is withdrawn before the optimiser's step lands on it
                params[~better] = best_params[~better]
        now = (float(rets.detach().mean()), float(out["is_collided"].double().mean()))
        first = first or now
        if verbose:
            print(f"iteration {it:4d}: mean return {now[0]:10.4f}   best so far {float(best_ret.mean()):10.4f}   "
                  f"collided {100 * now[1]:5.1f} %")
    bb.reset(seed=seed)
    with torch.no_grad():
        out = bb.step(best_params if safeguard else params.detach())
    last = (float(out["rewards"].mean()), float(out["is_collided"].double().mean()))
    torch.cuda.synchronize()
    if verbose:
        print(f"mean return {first[0]:.4f} -> {last[0]:.4f}, collided {100 * first[1]:.1f} % -> {100 * last[1]:.1f} % after {iters} "
              f"Adam steps on {envs} episodes ({(time.perf_counter() - t0) / max(iters, 1) * 1e3:.2f} ms per iteration)")
    return first, last


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-safeguard", action="store_true", help="follow the gradient blindly")
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    optimise(a.envs, a.iters, a.lr, a.seed, safeguard=not a.no_safeguard)
