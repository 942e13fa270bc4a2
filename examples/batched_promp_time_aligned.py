#!/usr/bin/env python3
"""
Learning a ProMP from demonstrations that do not all last equally long: every demonstration is the same movement distribution played at
its own speed, so it has its own tau.  A BeerPong-like handle (ProMP, 7 DoF, linear phase, learned tau) takes each demonstration's tau at
the front of its `params` row; `TrajectoryEngine.condition_on_demonstration_given_timing` conditions the shared prior on every
demonstration AT THAT DEMONSTRATION'S TAU (one launch of `mpk_demonstration_phase_condition`), and
`demonstration_log_prob_given_timing` scores it there.

1. `--demos` demonstrations: ProMP weights drawn from a known Gaussian N(centre, G G^T), played at a tau drawn per demonstration, plus
   observation noise; a fraction `--missing` of the samples is lost (sigma `inf`, value garbage).
2. EM for the shared prior N(mean, L L^T) over the weights:
     E-step  one launch: the posterior of every demonstration under the current prior at its own tau;
     M-step  in torch (float64), examples/batched_promp_em.py's.
   The mean log-likelihood of the demonstrations is printed per iteration; EM never lowers it.
3. For contrast the same EM with every demonstration forced to the mean tau -- what a shared-phase handle could do -- and both priors
   scored on held-out demonstrations (the time-aligned prior at each one's own tau, the other at the mean tau).
4. Prefix prediction at a held-out demonstration's own tau: the time-aligned prior conditioned on the first 40 % (one launch), the
   posterior mean's trajectory against the held-out rest, and the predictive spread from samples `params' + eps tril(L')^T` through
   `trajectory` (`sample_trajectories`; `trajectory_std` is shared-phase only).

    python examples/batched_promp_time_aligned.py [--demos 256] [--iters 8] [--noise 0.02] [--missing 0.2] [--seed 0]

Shape: a ProMP with 7 DoF and 5 basis functions (Pl = 35, P = 36 with tau), 100 steps: up to 700 scalar observations per demonstration.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402

TAU_LO, TAU_HI = 1.0, 2.0


def make_engine(device=0) -> TrajectoryEngine:
    return TrajectoryEngine("promp", "linear", "rbf", 7, 5, dt=0.02, duration=2.0, tau=2.0, learn_tau=True, tau_bound=(TAU_LO, TAU_HI),
                            device=device)


def m_step(post_mean, post_L):
    """the prior that maximises the expected complete-data log-likelihood: (mean [Pl], L [Pl, Pl]) float32 from the posteriors [N, ..]"""
    m, Lp = post_mean.double(), torch.tril(post_L.double())
    mean = m.mean(0)
    d = m - mean
    cov = (Lp @ Lp.transpose(1, 2) + d[:, :, None] * d[:, None, :]).mean(0)
    return mean.float(), torch.linalg.cholesky(0.5 * (cov + cov.T)).float()


def rows(tau, mean):
    """params [N, 1 + Pl]: tau in front, then the shared mean"""
    return torch.cat([tau[:, None], mean.expand(tau.shape[0], -1)], dim=1).contiguous()


def em(eng, tau, demo, sigma, iters, verbose, label):
    """EM from a broad prior at zero with the demonstrations at the timings `tau`; returns (mean, L, the mean log-likelihood before the
    first and after every iteration)"""
    N, Pl = tau.shape[0], eng.num_params - 1
    mean = torch.zeros(Pl, device=eng.device)
    L = 0.3 * torch.eye(Pl, device=eng.device)

    def score():
        return float(eng.demonstration_log_prob_given_timing(rows(tau, mean), L.expand(N, -1, -1), demo, sigma).mean())
    lls = [score()]
    for it in range(iters):
        post, post_L = eng.condition_on_demonstration_given_timing(rows(tau, mean), L.expand(N, -1, -1), demo, sigma)     # E-step
        mean, L = m_step(post[:, 1:], post_L)                                                                             # M-step
        lls.append(score())
        if verbose:
            print(f"{label} iteration {it + 1:2d}: mean log-likelihood {lls[-1]:.4f}")
    return mean, L, lls


def run(demos: int = 256, iters: int = 8, noise: float = 0.02, missing: float = 0.2, seed: int = 0, verbose: bool = True,
        engine: TrajectoryEngine = None, held_out: int = 32, samples: int = 64):
    """returns (the time-aligned EM's mean log-likelihood before the first and after every iteration, the held-out mean log-likelihood
    under the time-aligned prior and under the forced-mean-tau prior, the rms error on the held-out rest of the prior mean's trajectory
    and of the posterior mean's, the fraction of held-out samples within 3 predicted standard deviations)"""
    eng = engine or make_engine()
    dev, T, D, P = eng.device, eng.num_steps, eng.num_dof, eng.num_params
    Pl, N = P - 1, demos + held_out
    gen = torch.Generator(device=dev).manual_seed(seed)
    # 1. one movement distribution, played at per-demonstration speeds
    centre = torch.randn(Pl, generator=gen, device=dev)
    G = torch.tril(0.15 * torch.randn((Pl, Pl), generator=gen, device=dev))
    G.diagonal().abs_().add_(0.05)
    weights = centre + torch.randn((N, Pl), generator=gen, device=dev) @ G.T
    tau = 1.2 + 0.8 * torch.rand(N, generator=gen, device=dev)
    z = torch.zeros((N, D), device=dev)                                     # (a ProMP without zero padding ignores init_pos / init_vel)
    clean = eng.trajectory(torch.cat([tau[:, None], weights], dim=1), z, z)[0]
    noisy = clean + noise * torch.randn(clean.shape, generator=gen, device=dev)
    demo, test = noisy[:demos].clone(), noisy[demos:]
    tau_demo, tau_test = tau[:demos].contiguous(), tau[demos:].contiguous()
    sigma = torch.full(demo.shape, noise, device=dev)
    lost = torch.rand(demo.shape, generator=gen, device=dev) < missing
    sigma[lost] = float("inf")
    demo[lost] = float("nan")                                               # a lost sample's value is never used
    # 2. EM at every demonstration's own tau; 3. the same EM with every demonstration forced to the mean tau
    mean, L, lls = em(eng, tau_demo, demo, sigma, iters, verbose, "own tau ")
    kernel = eng.last_kernel()
    tau_mean = tau_demo.mean()
    mean_f, L_f, lls_f = em(eng, tau_mean.expand(demos).contiguous(), demo, sigma, iters, verbose, "mean tau")
    sd_test = torch.full(test.shape, noise, device=dev)
    held = float(eng.demonstration_log_prob_given_timing(rows(tau_test, mean), L.expand(held_out, -1, -1), test, sd_test).mean())
    held_f = float(eng.demonstration_log_prob_given_timing(rows(tau_mean.expand(held_out).contiguous(), mean_f),
                                                           L_f.expand(held_out, -1, -1), test, sd_test).mean())
    # 4. the rest of a held-out movement from its first 40 %, at its own tau
    cut = int(0.4 * T)
    sd = torch.full((T, D), noise, device=dev)
    sd[cut:] = float("inf")
    prior = rows(tau_test, mean)
    post, post_L = eng.condition_on_demonstration_given_timing(prior, L.expand(held_out, -1, -1), test, sd)
    zt = z[:held_out]
    pred = eng.trajectory(post, zt, zt)[0]
    prior_pred = eng.trajectory(prior, zt, zt)[0]
    spread = eng.sample_trajectories(post, post_L, zt, zt, num_samples=samples, generator=gen)[0].std(dim=1)
    rest = test[:, cut:]
    err_prior = float((prior_pred[:, cut:] - rest).pow(2).mean().sqrt())
    err_post = float((pred[:, cut:] - rest).pow(2).mean().sqrt())
    inside = float(((pred[:, cut:] - rest).abs() <= 3.0 * (spread[:, cut:] ** 2 + noise ** 2).sqrt()).float().mean())
    if verbose:
        print(f"{demos} demonstrations of {T} steps x {D} DoF at tau in [{float(tau_demo.min()):.2f}, {float(tau_demo.max()):.2f}]; the "
              f"E-step is one launch of {kernel}")
        print(f"mean log-likelihood at each demonstration's own tau: start {lls[0]:.4f}  end {lls[-1]:.4f}; forced to the mean tau "
              f"{float(tau_mean):.3f}: end {lls_f[-1]:.4f}")
        print(f"{held_out} held-out demonstrations: mean log-likelihood {held:.4f} under the time-aligned prior, {held_f:.4f} under the "
              f"prior learned at the mean tau")
        print(f"seen for {cut} of {T} steps at their own tau: rms error on the rest {err_prior:.4f} from the prior mean, {err_post:.4f} "
              f"from the posterior mean (noise {noise}); {100 * inside:.1f} % of the rest within 3 predicted std ({samples} samples)")
    return lls, held, held_f, err_prior, err_post, inside


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--demos", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--missing", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.demos, a.iters, a.noise, a.missing, a.seed)
