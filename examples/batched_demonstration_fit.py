#!/usr/bin/env python3
"""
Fitting movement-primitive parameters to demonstrations in closed form, one launch for the whole batch.

Demonstrations are drawn for `--envs` episodes at the BoxPushing shape (7 DoF, 5 basis functions, 100 steps): the trajectories of random
ProDMP parameters plus noise.  For a fixed phase the trajectory is linear in the parameters, so the best fit is a regularised
least-squares problem per (episode, DoF): `TrajectoryEngine.fit_trajectory` contracts the demonstrations with the basis table on the
matrix cores and solves the 6 x 6 systems inside the same launch (`mpk_trajectory_fit`) -- what mp_pytorch's
`learn_mp_params_from_trajs` does on the host.  Beside it, the Adam loop of examples/batched_trajectory_fit.py on the same demonstrations
(positions only), for the error it reaches and the time it takes.

    python examples/batched_demonstration_fit.py [--envs 4096] [--noise 0.05] [--reg 1e-9] [--adam-iters 300] [--seed 0]

Many parameter vectors reproduce a demonstration almost equally well (the late basis functions of an exponential phase barely move the
trajectory), so the two are compared on the reconstruction, not on the parameters.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402


def make_engine(device=0) -> TrajectoryEngine:
    return TrajectoryEngine("prodmp", "exp", "prodmp", 7, 5, dt=0.02, duration=2.0, tau=1.5, alpha_phase=3.0,
                            basis_bandwidth_factor=2, basis_alpha=10, device=device)


def demonstrations(eng: TrajectoryEngine, envs: int, noise: float, seed: int):
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    target = torch.randn((envs, eng.num_params), generator=gen, device=dev)
    init_pos = 2.0 * torch.rand((envs, eng.num_dof), generator=gen, device=dev) - 1.0
    init_vel = torch.zeros((envs, eng.num_dof), device=dev)
    clean = eng.trajectory(target, init_pos, init_vel)[0]
    return clean + noise * torch.randn(clean.shape, generator=gen, device=dev), init_pos, init_vel


def rms(eng, params, init_pos, init_vel, want) -> float:
    return float(((eng.trajectory(params, init_pos, init_vel)[0] - want) ** 2).mean().sqrt())


def adam_fit(eng, want, init_pos, init_vel, iters: int, lr: float = 0.1):
    theta = torch.zeros((want.shape[0], eng.num_params), device=eng.device, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=lr)
    for _ in range(iters):
        loss = ((eng.trajectory(theta, init_pos, init_vel)[0] - want) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return theta.detach()


def run(envs: int = 4096, noise: float = 0.05, reg: float = 1e-9, adam_iters: int = 300, seed: int = 0, verbose: bool = True,
        engine: TrajectoryEngine = None):
    """returns (RMS reconstruction error of the closed-form fit, of the Adam loop (None with adam_iters = 0), the fitted params)"""
    eng = engine or make_engine()
    with torch.no_grad():
        want, init_pos, init_vel = demonstrations(eng, envs, noise, seed)
        eng.fit_trajectory(want, init_pos, init_vel, reg=reg)           # builds and caches the Gram factor of (init_time, reg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        params = eng.fit_trajectory(want, init_pos, init_vel, reg=reg)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        kernel = eng.last_kernel()
        e_fit = rms(eng, params, init_pos, init_vel, want)
    if verbose:
        print(f"closed form: RMS reconstruction error {e_fit:.4e} (noise {noise:g}) for {envs} episodes in {1e3 * t_fit:.3f} ms, "
              f"one launch of {kernel}")
    e_adam = None
    if adam_iters > 0:
        t0 = time.perf_counter()
        theta = adam_fit(eng, want, init_pos, init_vel, adam_iters)
        torch.cuda.synchronize()
        t_adam = time.perf_counter() - t0
        with torch.no_grad():
            e_adam = rms(eng, theta, init_pos, init_vel, want)
        if verbose:
            print(f"Adam, {adam_iters} iterations: RMS reconstruction error {e_adam:.4e} in {1e3 * t_adam:.1f} ms")
    return e_fit, e_adam, params


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--reg", type=float, default=1e-9)
    ap.add_argument("--adam-iters", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.envs, a.noise, a.reg, a.adam_iters, a.seed)
