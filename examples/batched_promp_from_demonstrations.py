#!/usr/bin/env python3
"""
Learning a ProMP from whole demonstrations by maximum likelihood: a shared mean and covariance factor over the parameters, trained
with Adam on the log-likelihood of complete noisy trajectories -- some of them with missing samples -- through
`TrajectoryEngine.demonstration_log_prob` (one launch forward, one launch backward per iteration, `mpk_demonstration_log_prob` / `_vjp`;
the information form: every one of the T x D samples of a demonstration counts, and a 24 x 24 matrix is factored per episode).

1. `--demos` demonstrations: the trajectories of ProMP parameters drawn from a known Gaussian N(centre, G G^T), plus observation noise;
   a fraction `--missing` of the samples is lost (their sigma is `inf`, their value garbage), and every fourth demonstration stops after
   60 % of the movement (a prefix).
2. A shared `mean [P]` and `scale_tril [P, P]` (a lower triangle with an exponentiated diagonal) are learned with Adam on
   `-log_prob.mean()` over the whole demonstrations.
3. Printed: the mean log-likelihood at the start and at the end and under the generating Gaussian itself, and how far the learned mean
   is from the generating centre.

    python examples/batched_promp_from_demonstrations.py [--demos 512] [--iters 300] [--noise 0.05] [--missing 0.2] [--lr 0.05] [--seed 0]

Shape: a ProMP with 4 DoF and 6 basis functions (P = 24), 100 steps: up to 400 scalar observations per episode and launch.
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


def run(demos: int = 512, iters: int = 300, noise: float = 0.05, missing: float = 0.2, lr: float = 0.05, seed: int = 0,
        verbose: bool = True, engine: TrajectoryEngine = None):
    """returns (the mean log-likelihood at the start, at the end, under the generating Gaussian, |mean - centre| / |centre|)"""
    eng = engine or make_engine()
    dev, T, D, P = eng.device, eng.num_steps, eng.num_dof, eng.num_params
    gen = torch.Generator(device=dev).manual_seed(seed)
    # 1. demonstrations of a known Gaussian over the parameters, plus observation noise, with samples missing
    centre = torch.randn(P, generator=gen, device=dev)
    G = torch.tril(0.2 * torch.randn((P, P), generator=gen, device=dev))
    G.diagonal().abs_().add_(0.05)
    truth = centre + torch.randn((demos, P), generator=gen, device=dev) @ G.T
    z = torch.zeros((demos, D), device=dev)
    with torch.no_grad():
        clean = eng.trajectory(truth, z, z)[0]
    demo = clean + noise * torch.randn(clean.shape, generator=gen, device=dev)
    sigma = torch.full(clean.shape, noise, device=dev)
    lost = torch.rand(clean.shape, generator=gen, device=dev) < missing
    lost[::4, int(0.6 * T):] = True                                         # every fourth demonstration is a prefix
    sigma[lost] = float("inf")
    demo[lost] = float("nan")                                               # a lost sample's value is never used

    def score(mean, L):
        return eng.demonstration_log_prob(mean.expand(demos, -1), L.expand(demos, -1, -1), demo, sigma)
    # 2. Adam on the negative mean log-likelihood
    mean = torch.zeros(P, device=dev, requires_grad=True)
    raw = torch.zeros((P, P), device=dev)
    raw.diagonal().fill_(float(np.log(0.3)))
    raw.requires_grad_(True)
    opt = torch.optim.Adam([mean, raw], lr=lr)
    with torch.no_grad():
        start = float(score(mean, scale_tril(raw)).mean())
    for _ in range(iters):
        opt.zero_grad(set_to_none=True)
        loss = -score(mean, scale_tril(raw)).mean()
        loss.backward()
        opt.step()
    kernels = eng.last_kernel()
    with torch.no_grad():
        end = float(score(mean, scale_tril(raw)).mean())
        generating = float(score(centre, G).mean())
        off = float((mean - centre).norm() / centre.norm())
    if verbose:
        kept = int((~lost).sum()) / demos
        print(f"{demos} demonstrations of {T} steps x {D} DoF, {kept:.0f} samples kept per demonstration on average, {iters} iterations "
              f"of Adam; the backward is one launch of {kernels}")
        print(f"mean log-likelihood: start {start:.4f}  end {end:.4f}")
        print(f"under the generating Gaussian {generating:.4f}; learned mean off the generating centre by {off:.3f} of its norm")
    return start, end, generating, off


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--demos", type=int, default=512)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--missing", type=float, default=0.2)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.demos, a.iters, a.noise, a.missing, a.lr, a.seed)
