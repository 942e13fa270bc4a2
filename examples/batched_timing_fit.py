#!/usr/bin/env python3
"""
Fitting demonstrations of DIFFERENT DURATIONS: weights and the timing parameter tau by gradient descent, all on the device.

`--envs` demonstrations are generated from a BeerPong-shaped ProMP (7 DoF, 2 basis functions behind 2 zero-padded ones, linear phase, 300
steps of 10 ms) with a known tau per episode between 1.2 and 2.7 s.  Adam then fits every episode's weights AND its tau, starting from
zero weights and tau = 2.005 s, on the mean squared position error plus a small velocity term.  The handle learns tau, so every episode has
its own phase: `TrajectoryEngine.trajectory(..., phase_gradient="pathwise")` keeps the autograd graph through it -- the forward is the usual
one launch (`k_traj_phase`), the backward one `mpk_trajectory_phase_vjp` launch (`k_phase_vjp`), which recomputes each episode's phase
and basis rows and transposes them, the derivative w.r.t. tau included (clamped to its bounds as torch.clamp does it).

    python examples/batched_timing_fit.py [--envs 4096] [--iters 300] [--lr 0.05] [--seed 0]

The loss falls by two to three orders of magnitude and tau comes within a few per cent of the demonstration's.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU_BOUND = (0.5, 3.0)
TAU_START = 2.005     # between two grid times: no step starts on the clip of the linear phase (s = 1), where its derivative jumps
VEL_WEIGHT = 1e-2


def make_engine(device=0):
    from fancy_gym_amd import TrajectoryEngine
    return TrajectoryEngine("promp", "linear", "zero_rbf", 7, 2, dt=0.01, duration=3.0, tau=3.0, learn_tau=True, tau_bound=TAU_BOUND,
                            basis_bandwidth_factor=3, num_basis_zero_start=2, num_basis_zero_goal=0, device=device)


def demo_parameters(envs: int, seed: int = 0):
    """(params [envs, 1 + 7 * 2] with the known tau in column 0, init_pos [envs, 7]) float32 numpy"""
    rng = np.random.default_rng(seed)
    params = rng.standard_normal((envs, 15)).astype(np.float32)
    params[:, 0] = rng.uniform(1.2, 2.7, envs)
    return params, rng.uniform(-1, 1, (envs, 7)).astype(np.float32)


def loss_of(pos, vel, want_pos, want_vel):
    return ((pos - want_pos) ** 2).mean() + VEL_WEIGHT * ((vel - want_vel) ** 2).mean()


def fit_loop(trajectory, theta0, want_pos, want_vel, iters: int, lr: float, verbose: bool = False):
    """Adam on ``theta`` (a leaf made from ``theta0``) through ``trajectory(theta) -> (pos, vel)``; returns (theta, losses: iters + 1 floats)"""
    theta = theta0.clone().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=lr)
    losses = []
    for it in range(iters):
        loss = loss_of(*trajectory(theta), want_pos, want_vel)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        if verbose and it % 50 == 0:
            print(f"iteration {it:4d}: loss {float(losses[-1]):.4e}")
    with torch.no_grad():
        losses.append(loss_of(*trajectory(theta), want_pos, want_vel))
    return theta.detach(), [float(x) for x in losses]


def fit(envs: int = 4096, iters: int = 300, lr: float = 0.05, seed: int = 0, verbose: bool = True, engine=None):
    """returns (loss per iteration as a list of floats, mean relative error of the fitted tau)"""
    eng = engine or make_engine()
    dev = eng.device
    demo, init_pos = (torch.from_numpy(a).to(dev) for a in demo_parameters(envs, seed))
    init_vel = torch.zeros_like(init_pos)
    with torch.no_grad():
        want_pos, want_vel = eng.trajectory(demo, init_pos, init_vel)
    theta0 = torch.zeros_like(demo)
    theta0[:, 0] = TAU_START
    t0 = time.perf_counter()
    theta, losses = fit_loop(lambda th: eng.trajectory(th, init_pos, init_vel, phase_gradient="pathwise"), theta0, want_pos, want_vel,
                             iters, lr, verbose)
    torch.cuda.synchronize()
    tau_err = float(((theta[:, 0].clamp(*TAU_BOUND) - demo[:, 0]).abs() / demo[:, 0]).mean())
    if verbose:
        dt = time.perf_counter() - t0
        print(f"final loss {losses[-1]:.4e} ({losses[-1] / losses[0]:.1e} of the start), mean relative tau error {tau_err:.3f}")
        print(f"{iters} iterations x {envs} episodes in {dt:.2f} s (last launch {eng.last_kernel()})")
    return losses, tau_err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    fit(a.envs, a.iters, a.lr, a.seed)
