#!/usr/bin/env python3
"""
Learning a ProMP by maximum likelihood: a shared mean and covariance factor over the parameters, trained with Adam on the
log-likelihood of demonstrated points -- observation noise kept apart from the weight covariance -- through
`TrajectoryEngine.trajectory_log_prob` (one launch forward, one launch backward per iteration, `mpk_trajectory_log_prob` / `_vjp`).

1. `--demos` demonstrations: the trajectories of ProMP parameters drawn from a known Gaussian N(centre, G G^T), plus observation noise.
2. A shared `mean [P]` and `scale_tril [P, P]` (a lower triangle with an exponentiated diagonal) are learned with Adam on
   `-log_prob.mean()`; every iteration scores the demonstrations at `--steps` steps of the horizon, redrawn each time.
3. Printed, all at one fixed set of steps: the mean log-likelihood at the start and at the end, under the generating Gaussian itself,
   and under the closed-form route (`fit_trajectory` -> `torch.cov` -> Cholesky), which folds the observation noise into the weights.

    python examples/batched_promp_likelihood.py [--demos 512] [--iters 300] [--steps 8] [--noise 0.05] [--lr 0.05] [--seed 0]

Shape: a ProMP with 4 DoF and 6 basis functions (P = 24), 100 steps; 8 steps x 4 DoF = 32 scalar observations per episode and launch.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402


def make_engine(device=0) -> TrajectoryEngine:
    return TrajectoryEngine("promp", "linear", "rbf", 4, 6, dt=0.02, duration=2.0, tau=2.0, device=device)


def scale_tril(raw):
    """a valid factor from an unconstrained square matrix: its strict lower triangle, and exp of its diagonal"""
    return torch.tril(raw, -1) + torch.diag_embed(torch.exp(torch.diagonal(raw)))


def run(demos: int = 512, iters: int = 300, steps: int = 8, noise: float = 0.05, lr: float = 0.05, seed: int = 0, verbose: bool = True,
        engine: TrajectoryEngine = None):
    """returns the mean log-likelihoods (start, end, under the generating Gaussian, under the closed-form route) at the fixed steps"""
    eng = engine or make_engine()
    dev, T, D, P = eng.device, eng.num_steps, eng.num_dof, eng.num_params
    assert steps * D <= 64, "at most 64 scalar observations per episode"
    gen = torch.Generator(device=dev).manual_seed(seed)
    rng = np.random.default_rng(seed)
    # 1. demonstrations of a known Gaussian over the parameters, plus observation noise
    centre = torch.randn(P, generator=gen, device=dev)
    G = torch.tril(0.2 * torch.randn((P, P), generator=gen, device=dev))
    G.diagonal().abs_().add_(0.05)
    truth = centre + torch.randn((demos, P), generator=gen, device=dev) @ G.T
    z = torch.zeros((demos, D), device=dev)
    with torch.no_grad():
        clean = eng.trajectory(truth, z, z)[0]
    demo = clean + noise * torch.randn(clean.shape, generator=gen, device=dev)

    def draw():
        return sorted(int(t) for t in rng.choice(T, size=steps, replace=False))

    def score(mean, L, at):
        return eng.trajectory_log_prob(mean.expand(demos, -1), L.expand(demos, -1, -1), at, demo[:, at], noise)
    fixed = [int(t) for t in np.linspace(0, T - 1, steps).round()]
    # 2. Adam on the negative mean log-likelihood
    mean = torch.zeros(P, device=dev, requires_grad=True)
    raw = torch.zeros((P, P), device=dev)
    raw.diagonal().fill_(float(np.log(0.3)))
    raw.requires_grad_(True)
    opt = torch.optim.Adam([mean, raw], lr=lr)
    with torch.no_grad():
        start = float(score(mean, scale_tril(raw), fixed).mean())
    for _ in range(iters):
        opt.zero_grad(set_to_none=True)
        loss = -score(mean, scale_tril(raw), draw()).mean()
        loss.backward()
        opt.step()
    kernels = eng.last_kernel()
    with torch.no_grad():
        end = float(score(mean, scale_tril(raw), fixed).mean())
        generating = float(score(centre, G, fixed).mean())
        # 3. the closed-form route: every demonstration's least-squares parameters, their sample mean and covariance
        params = eng.fit_trajectory(demo, z, z)
        cov = torch.cov(params.T.double())
        cov += 1e-9 * torch.diagonal(cov).mean() * torch.eye(P, device=dev, dtype=torch.float64)
        closed = float(score(params.mean(dim=0), torch.linalg.cholesky(cov).float(), fixed).mean())
    if verbose:
        print(f"{demos} demonstrations, {iters} iterations of Adam at {steps} redrawn steps x {D} DoF = {steps * D} observations per "
              f"episode; the backward is one launch of {kernels}")
        print(f"mean log-likelihood: start {start:.4f}  end {end:.4f}")
        print(f"under the generating Gaussian {generating:.4f}; under the closed-form route (fit_trajectory -> cov -> Cholesky) "
              f"{closed:.4f}")
    return start, end, generating, closed


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--demos", type=int, default=512)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.demos, a.iters, a.steps, a.noise, a.lr, a.seed)
