#!/usr/bin/env python3
"""
Learning a ProMP from noisy, partly missing demonstrations by EM, and predicting the rest of a movement from its beginning -- both through
`TrajectoryEngine.condition_on_demonstration` (one launch of `mpk_demonstration_condition` over all demonstrations: the posterior over
the parameters given every kept sample, in the information form).  The closed-form counterpart of the Adam loop in
examples/batched_promp_from_demonstrations.py.

1. `--demos` demonstrations: the trajectories of ProMP parameters drawn from a known Gaussian N(centre, G G^T), plus observation noise;
   a fraction `--missing` of the samples is lost (their sigma is `inf`, their value garbage), and every fourth demonstration stops after
   60 % of the movement.
2. EM for the shared prior N(mean, L L^T):
     E-step  one launch: the posterior N(m_n, L'_n L'_n^T) of every demonstration n under the current prior, expanded over the batch;
     M-step  in torch (float64): mean = the mean of the m_n, L = the Cholesky factor of the mean of L'_n L'_n^T + (m_n - mean)(m_n - mean)^T.
   The mean log-likelihood of the demonstrations (`demonstration_log_prob`) is printed per iteration; EM never lowers it.
3. Prefix prediction: held-out movements of the same Gaussian, observed for their first 40 %; the learned prior conditioned on that
   prefix (one launch), then `trajectory` of the posterior mean and `trajectory_std` of the posterior factor against the held-out rest.

    python examples/batched_promp_em.py [--demos 512] [--iters 10] [--noise 0.05] [--missing 0.2] [--seed 0]

Shape: a ProMP with 4 DoF and 6 basis functions (P = 24), 100 steps: up to 400 scalar observations per demonstration.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402


def make_engine(device=0) -> TrajectoryEngine:
    return TrajectoryEngine("promp", "linear", "rbf", 4, 6, dt=0.02, duration=2.0, tau=2.0, device=device)


def m_step(post_mean, post_L):
    """the prior that maximises the expected complete-data log-likelihood: (mean [P], L [P, P]) float32 from the posteriors [N, ..]"""
    m, Lp = post_mean.double(), torch.tril(post_L.double())
    mean = m.mean(0)
    d = m - mean
    cov = (Lp @ Lp.transpose(1, 2) + d[:, :, None] * d[:, None, :]).mean(0)
    return mean.float(), torch.linalg.cholesky(0.5 * (cov + cov.T)).float()


def run(demos: int = 512, iters: int = 10, noise: float = 0.05, missing: float = 0.2, seed: int = 0, verbose: bool = True,
        engine: TrajectoryEngine = None, held_out: int = 32):
    """returns (the mean log-likelihood before the first and after every iteration, the rms error on the held-out rest of the prior
    mean's trajectory and of the posterior mean's, the fraction of held-out samples within 3 predicted standard deviations)"""
    eng = engine or make_engine()
    dev, T, D, P = eng.device, eng.num_steps, eng.num_dof, eng.num_params
    gen = torch.Generator(device=dev).manual_seed(seed)
    # 1. demonstrations of a known Gaussian over the parameters, plus observation noise, with samples missing
    centre = torch.randn(P, generator=gen, device=dev)
    G = torch.tril(0.2 * torch.randn((P, P), generator=gen, device=dev))
    G.diagonal().abs_().add_(0.05)
    truth = centre + torch.randn((demos + held_out, P), generator=gen, device=dev) @ G.T
    z = torch.zeros((demos + held_out, D), device=dev)
    clean = eng.trajectory(truth, z, z)[0]
    noisy = clean + noise * torch.randn(clean.shape, generator=gen, device=dev)
    demo, test = noisy[:demos].clone(), noisy[demos:]
    sigma = torch.full(demo.shape, noise, device=dev)
    lost = torch.rand(demo.shape, generator=gen, device=dev) < missing
    lost[::4, int(0.6 * T):] = True                                         # every fourth demonstration stops early
    sigma[lost] = float("inf")
    demo[lost] = float("nan")                                               # a lost sample's value is never used

    def score(mean, L):
        return float(eng.demonstration_log_prob(mean.expand(demos, -1), L.expand(demos, -1, -1), demo, sigma).mean())
    # 2. EM from a broad prior at zero
    mean = torch.zeros(P, device=dev)
    L = 0.3 * torch.eye(P, device=dev)
    lls = [score(mean, L)]
    for it in range(iters):
        post_mean, post_L = eng.condition_on_demonstration(mean.expand(demos, -1), L.expand(demos, -1, -1), demo, sigma)   # E-step
        kernel = eng.last_kernel()
        mean, L = m_step(post_mean, post_L)                                                                                  # M-step
        lls.append(score(mean, L))
        if verbose:
            print(f"iteration {it + 1:2d}: mean log-likelihood {lls[-1]:.4f}")
    # 3. the rest of a held-out movement from its first 40 %
    cut = int(0.4 * T)
    sd = torch.full((T, D), noise, device=dev)
    sd[cut:] = float("inf")
    zt = torch.zeros((held_out, D), device=dev)
    post_mean, post_L = eng.condition_on_demonstration(mean.expand(held_out, -1), L.expand(held_out, -1, -1), test, sd)
    pred = eng.trajectory(post_mean, zt, zt)[0]
    pred_std = eng.trajectory_std(post_L, vel=False)[0]
    prior_pred = eng.trajectory(mean.expand(held_out, -1).contiguous(), zt, zt)[0]
    rest = test[:, cut:]
    err_prior = float((prior_pred[:, cut:] - rest).pow(2).mean().sqrt())
    err_post = float((pred[:, cut:] - rest).pow(2).mean().sqrt())
    inside = float(((pred[:, cut:] - rest).abs() <= 3.0 * (pred_std[:, cut:] ** 2 + noise ** 2).sqrt()).float().mean())
    if verbose:
        kept = int((~lost).sum()) / demos
        print(f"{demos} demonstrations of {T} steps x {D} DoF, {kept:.0f} samples kept per demonstration on average; the E-step is one "
              f"launch of {kernel}")
        print(f"mean log-likelihood: start {lls[0]:.4f}  end {lls[-1]:.4f}; learned mean off the generating centre by "
              f"{float((mean - centre).norm() / centre.norm()):.3f} of its norm")
        print(f"{held_out} held-out movements seen for {cut} of {T} steps: rms error on the rest {err_prior:.4f} from the prior mean, "
              f"{err_post:.4f} from the posterior mean (noise {noise}); {100 * inside:.1f} % of the rest within 3 predicted std")
    return lls, err_prior, err_post, inside


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--demos", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--missing", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.demos, a.iters, a.noise, a.missing, a.seed)
