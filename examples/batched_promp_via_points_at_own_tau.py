#!/usr/bin/env python3
"""
Via-points at a movement's own speed.  examples/batched_promp_time_aligned.py learns a ProMP prior N(mean, L L^T) from demonstrations that
each last as long as their own tau says; this example takes such a prior and does what a ProMP is for, at a NEW movement's tau:

1. the prior is learned as there (`em` of that example: the E-step is one launch of `condition_on_demonstration_given_timing`);
2. its uncertainty band at two different tau, `trajectory_std_given_timing` (one launch of `mpk_trajectory_phase_std`; the plain
   `trajectory_std` refuses a handle that learns tau);
3. the prior conditioned on ONE via-point -- a position 0.3 beside the prior mean and the prior mean's own velocity at one step, each
   with its standard deviation -- at the two tau, `condition_given_timing` (one launch of `mpk_trajectory_phase_condition`): the same
   step is another phase at another tau, so the two posteriors differ;
4. the band after conditioning, again at each movement's own tau: it collapses at the via-point and stays wide elsewhere;
5. `trajectory_log_prob_given_timing` scores the via-point under the prior and under the posterior;
6. trajectories sampled from the two posteriors (`sample_trajectories`, which takes a learned phase as it stands) scatter around the
   posterior mean's trajectory as the posterior band says they should.

    python examples/batched_promp_via_points_at_own_tau.py [--demos 128] [--iters 6] [--noise 0.02] [--seed 0]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batched_promp_time_aligned import em, make_engine, rows  # noqa: E402


def run(demos: int = 128, iters: int = 6, noise: float = 0.02, seed: int = 0, verbose: bool = True, engine=None, samples: int = 64,
        taus=(1.25, 1.9), via_step: int = 60, via_std: float = 0.01):
    """returns (pos_std at the via-point before and after conditioning [2 tau, D] each, the via-point's log-likelihood under the prior and
    under the posterior [2 tau] each, and how the samples sit in the posterior band at the via-point: the largest distance of their mean
    from the posterior mean's trajectory in standard errors (band / sqrt(samples)), the smallest and largest ratio of their standard
    deviation to the band)"""
    eng = engine or make_engine()
    dev, D, Pl = eng.device, eng.num_dof, eng.num_params - 1
    gen = torch.Generator(device=dev).manual_seed(seed)
    # 1. a prior from demonstrations played at their own speeds
    centre = torch.randn(Pl, generator=gen, device=dev)
    G = torch.tril(0.15 * torch.randn((Pl, Pl), generator=gen, device=dev))
    G.diagonal().abs_().add_(0.05)
    weights = centre + torch.randn((demos, Pl), generator=gen, device=dev) @ G.T
    tau_demo = 1.2 + 0.8 * torch.rand(demos, generator=gen, device=dev)
    z = torch.zeros((demos, D), device=dev)
    demo = eng.trajectory(torch.cat([tau_demo[:, None], weights], dim=1), z, z)[0]
    demo = demo + noise * torch.randn(demo.shape, generator=gen, device=dev)
    mean, L, _ = em(eng, tau_demo, demo, torch.full(demo.shape, noise, device=dev), iters, False, "")
    # 2. the prior's band at two tau
    tau = torch.tensor(taus, device=dev)
    B = tau.shape[0]
    prior, prior_L = rows(tau, mean), L.expand(B, -1, -1).contiguous()
    band = eng.trajectory_std_given_timing(prior, prior_L)
    # 3. one via-point (position and velocity) at step via_step, the same values for both movements
    zt = torch.zeros((B, D), device=dev)
    prior_pos, prior_vel = eng.trajectory(prior, zt, zt)
    way_pos = prior_pos[:1, via_step].expand(B, D)[:, None, :] + 0.3
    way_vel = prior_vel[:, via_step][:, None, :].contiguous()
    obs = dict(obs_steps=[via_step], obs_pos=way_pos, obs_std=via_std, obs_vel=way_vel, obs_vel_std=10.0 * via_std)
    post, post_L = eng.condition_given_timing(prior, prior_L, **obs)
    kernel = eng.last_kernel()
    # 4. the band after conditioning; 5. the via-point's score before and after
    band_post = eng.trajectory_std_given_timing(post, post_L)
    lp_prior = eng.trajectory_log_prob_given_timing(prior, prior_L, **obs)
    lp_post = eng.trajectory_log_prob_given_timing(post, post_L, **obs)
    # 6. samples from the posteriors
    smp = eng.sample_trajectories(post, post_L, zt, zt, num_samples=samples, generator=gen)[0]
    at_via = smp[:, :, via_step]                                            # [B, S, D]
    post_pos = eng.trajectory(post, zt, zt)[0][:, via_step]
    miss = float(((at_via.mean(dim=1) - post_pos).abs() / (band_post[0][:, via_step] / samples ** 0.5)).max())
    ratio = at_via.std(dim=1) / band_post[0][:, via_step]
    passes = float(((post_pos - way_pos[:, 0]).abs() / via_std).max())
    if verbose:
        print(f"prior from {demos} demonstrations at tau in [{float(tau_demo.min()):.2f}, {float(tau_demo.max()):.2f}]; conditioning is one "
              f"launch of {kernel}")
        for b in range(B):
            print(f"tau {taus[b]:.2f}: pos_std at step {via_step} {float(band[0][b, via_step].mean()):.4f} -> "
                  f"{float(band_post[0][b, via_step].mean()):.4f} (via-point std {via_std}); at the last step "
                  f"{float(band[0][b, -1].mean()):.4f} -> {float(band_post[0][b, -1].mean()):.4f}; log-likelihood of the via-point "
                  f"{float(lp_prior[b]):.2f} -> {float(lp_post[b]):.2f}")
        print(f"the two posterior means differ by up to {float((post[0, 1:] - post[1, 1:]).abs().max()):.4f}; the posterior mean's trajectory "
              f"passes the via-point within {passes:.2f} via-point std; {samples} sampled trajectories: their mean within {miss:.2f} standard "
              f"errors of it, their std {float(ratio.min()):.2f} .. {float(ratio.max()):.2f} of the posterior band")
    return band[0][:, via_step], band_post[0][:, via_step], lp_prior, lp_post, miss, float(ratio.min()), float(ratio.max())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--demos", type=int, default=128)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.demos, a.iters, a.noise, a.seed)
