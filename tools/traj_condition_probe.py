"""
mpk_trajectory_condition against what a user could do without it, on the same device (profiles/r20_traj_condition.md):

  yardstick   the batch formula in float32 torch.  Not timed: the observation matrix H [M D, Pl] from one forward launch over Pl + 1
              unit-vector rows, and the offsets c from one forward launch at zero parameters.  Timed, per call:
              Sigma = L L^T, S = H Sigma H^T + R, torch.linalg.cholesky(S), two cholesky_solve, mu' and Sigma' = Sigma - G S^-1 G^T,
              and the re-factorisation torch.linalg.cholesky(Sigma' + jitter I) -- the posterior covariance is near-singular, without
              the jitter the factorisation fails
  kernel      TrajectoryEngine.condition(..., out=...): one launch of k_traj_condition, nothing materialised

M = 3 position via-points on all DoFs, sigma = 0.01.  Device events around groups of `--group` back-to-back calls, warm (30 calls
first, which also brings the clocks up), the two alternating in one process; per shape the median (10th .. 90th percentile) time per
call over the groups, the ratio, and the largest difference of the two posterior means and covariances.

    python tools/traj_condition_probe.py [--groups 40] [--group 10] [--shapes cfg2:4096,pl160:4096] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fancy_gym_amd import TrajectoryEngine  # noqa: E402


def engine(name):
    if name == "cfg2":      # ProDMP, 7 DoF, 5 basis functions + goal, 100 steps: Pl = 42
        return TrajectoryEngine("prodmp", "exp", "prodmp", 7, 5, dt=0.02, duration=2.0, tau=1.5, alpha_phase=3.0,
                                basis_bandwidth_factor=2, basis_alpha=10, device=0)
    if name == "pl160":     # ProDMP, 16 DoF, 9 basis functions + goal, 30 steps: Pl = 160, one wave per workgroup
        return TrajectoryEngine("prodmp", "exp", "prodmp", 16, 9, dt=0.02, duration=0.6, tau=1.0, alpha_phase=3.0, basis_alpha=15,
                                device=0)
    raise SystemExit(f"unknown shape {name}")


def timed(fn, groups, group, warm=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / group)
    return np.asarray(out)


def markdown(recs):
    us = lambda x: f"{x[0]:,.1f} ({x[1]:,.1f} .. {x[2]:,.1f})".replace(",", " ")       # noqa: E731
    rows = ["| shape | B | kernel us | kernel again us | torch composition us | composition / kernel | LDS / workgroup, waves | "
            "largest relative difference (mean, covariance) |", "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        rows.append(f"| {r['shape']} (T = {r['T']}, D = {r['D']}, Pl = {r['Pl']}) | {r['B']} | `{r['kernel']}` {us(r['kernel_us'])} | "
                    f"{us(r['kernel_again_us'])} | {us(r['torch_us'])} | {r['ratio']:.2f} | {r['lds_bytes']} B, {r['waves']} | "
                    f"{r['diff_mean']:.1e}, {r['diff_cov']:.1e} |")
    return "\n".join(rows) + "\n"


def lds_plan(Pl, M, KT):
    """traj_cond_limits restated: (bytes per workgroup, waves per workgroup, waves per CU)"""
    per_wave, shared, cu = 8 * (Pl * (Pl + 1) // 2 + 4 * Pl), 16 * M * KT, 160 * 1024
    best = max((w * (cu // (w * per_wave + shared)), w) for w in range(1, 5) if w * per_wave + shared <= cu)
    return best[1] * per_wave + shared, best[1], best[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--shapes", default="cfg2:4096,pl160:4096")
    ap.add_argument("--sigma", type=float, default=0.01)
    ap.add_argument("--markdown", metavar="FILE", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    recs = []
    for item in args.shapes.split(","):
        name, B = item.split(":")
        B = int(B)
        eng = engine(name)
        D, T, Pl, M = eng.num_dof, eng.num_steps, eng.num_params, 3
        steps = [T // 4, T // 2, T - 1]
        gen = torch.Generator(device="cuda").manual_seed(1)
        rows = torch.zeros((Pl + 1, Pl), device="cuda")
        rows[:Pl] = torch.eye(Pl, device="cuda")
        z = torch.zeros((Pl + 1, D), device="cuda")
        pos = eng.trajectory(rows, z, z)[0]
        H = (pos[:Pl] - pos[Pl])[:, steps].permute(1, 2, 0).reshape(M * D, Pl).contiguous()     # [(m, d), Pl]
        mu = torch.randn((B, Pl), device="cuda", generator=gen)
        L = torch.tril(0.3 * torch.randn((B, Pl, Pl), device="cuda", generator=gen))
        L.diagonal(dim1=1, dim2=2).abs_().add_(0.1)
        ip = 2.0 * torch.rand((B, D), device="cuda", generator=gen) - 1.0
        iv = torch.zeros((B, D), device="cuda")
        c = eng.trajectory(torch.zeros((B, Pl), device="cuda"), ip, iv)[0][:, steps].reshape(B, M * D).contiguous()
        w = mu + torch.einsum("bpq,bq->bp", L, torch.randn((B, Pl), device="cuda", generator=gen))
        y = (w @ H.T + c + args.sigma * torch.randn((B, M * D), device="cuda", generator=gen)).contiguous()
        sd = torch.full((B, M, D), args.sigma, device="cuda")
        R = (args.sigma ** 2) * torch.eye(M * D, device="cuda")
        eye = torch.eye(Pl, device="cuda")

        def composed():
            Sigma = L @ L.transpose(1, 2)
            G = Sigma @ H.T                                               # [B, Pl, MD]
            S = H @ G + R
            Sc = torch.linalg.cholesky(S)
            r = (y - c - mu @ H.T)[:, :, None]
            mean = mu + (G @ torch.cholesky_solve(r, Sc))[:, :, 0]
            cov = Sigma - G @ torch.cholesky_solve(G.transpose(1, 2), Sc)
            cov = 0.5 * (cov + cov.transpose(1, 2))
            jitter = 1e-5 * cov.diagonal(dim1=1, dim2=2).mean(dim=1)
            return mean, torch.linalg.cholesky(cov + jitter[:, None, None] * eye), cov

        out = (torch.empty_like(mu), torch.empty_like(L))
        y3 = y.view(B, M, D)

        def kernel():
            return eng.condition(mu, L, steps, y3, sd, ip, iv, out=out)

        got, want = kernel(), composed()
        torch.cuda.synchronize()
        got_cov = torch.tril(got[1]) @ torch.tril(got[1]).transpose(1, 2)
        diff_mean = float((got[0] - want[0]).abs().max() / want[0].abs().max())
        diff_cov = float((got_cov - want[2]).abs().max() / want[2].abs().max())
        del want, got_cov
        tk = timed(kernel, args.groups, args.group)
        tc = timed(composed, max(args.groups // 4, 5), max(args.group // 5, 1), warm=3)
        tk2 = timed(kernel, args.groups, args.group)
        q = lambda x: [float(np.percentile(x, p)) for p in (50, 10, 90)]       # noqa: E731
        KT = Pl // D + 2
        lds, waves, on_cu = lds_plan(Pl, M, KT)
        rec = dict(shape=name, B=B, T=T, D=D, Pl=Pl, M=M, sigma=args.sigma, kernel=eng.last_kernel(), kernel_us=q(tk),
                   kernel_again_us=q(tk2), torch_us=q(tc), ratio=float(np.median(tc) / np.median(tk)), diff_mean=diff_mean,
                   diff_cov=diff_cov, lds_bytes=lds, waves=waves, waves_per_cu=on_cu,
                   bytes_per_episode=4 * (Pl * (Pl + 1) // 2 + Pl * Pl + 2 * Pl + 2 * M * D + 2 * D))
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del L, out, mu
        torch.cuda.empty_cache()
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
