"""
mpk_trajectory_log_prob / _vjp against what a user could do without them, on the same device (profiles/r21_traj_log_prob.md):

  yardstick   the float32 torch composition.  Not timed: the observation matrix H [n, Pl] from one forward launch over Pl + 1 unit-vector
              rows, and the offsets c from one forward launch at zero parameters.  Timed, per call: A = H tril(L), S = A A^T + R,
              torch.linalg.cholesky(S), torch.distributions.MultivariateNormal(loc, scale_tril=C).log_prob(y); forward + backward adds
              the autograd backward of its sum w.r.t. the mean and the factor
  kernel      TrajectoryEngine.trajectory_log_prob: one launch of k_traj_log_prob; forward + backward: the same under autograd, whose
              backward is one launch of k_traj_log_prob<.., grad>

Shapes: cfg2 with M = 2 position steps (n = 14, Pl = 42) and Pl = 160 with M = 2 position and velocity steps (n = 64).  Device events
around groups of `--group` back-to-back calls, warm (30 calls first, which also brings the clocks up), kernel and composition alternating
in one process; per shape the median (10th .. 90th percentile) time per call over the groups, the ratios, and the largest difference of
the two results.

    python tools/traj_log_prob_probe.py [--groups 40] [--group 10] [--shapes cfg2:4096,pl160:4096] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.traj_condition_probe import engine, timed  # noqa: E402


def lds_plan(Pl, nmax, M, KT):
    """traj_log_prob_limits restated: (bytes per workgroup, waves per workgroup, waves per CU)"""
    per_wave, shared, cu = 8 * (nmax * (Pl | 1) + nmax * (nmax + 1) // 2 + 3 * nmax), 16 * M * KT + 64, 160 * 1024
    best = max((w * (cu // (w * per_wave + shared)), w) for w in range(1, 5) if w * per_wave + shared <= cu)
    return best[1] * per_wave + shared, best[1], best[0]


def markdown(recs):
    us = lambda x: f"{x[0]:,.1f} ({x[1]:,.1f} .. {x[2]:,.1f})".replace(",", " ")       # noqa: E731
    rows = ["| shape | B | forward us | composition forward us | ratio | forward + backward us | composition forward + backward us | "
            "ratio | LDS / workgroup, waves, waves / CU | largest relative difference (log_prob, g_params, g_params_L) |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        rows.append(f"| {r['shape']} (D = {r['D']}, Pl = {r['Pl']}, n = {r['n']}) | {r['B']} | `{r['kernel']}` {us(r['fwd_us'])} | "
                    f"{us(r['torch_fwd_us'])} | {r['ratio_fwd']:.2f} | {us(r['fwdbwd_us'])} | {us(r['torch_fwdbwd_us'])} | "
                    f"{r['ratio_fwdbwd']:.2f} | {r['lds_bytes']} B, {r['waves']}, {r['waves_per_cu']} | "
                    f"{r['diff_lp']:.1e}, {r['diff_gm']:.1e}, {r['diff_gL']:.1e} |")
    return "\n".join(rows) + "\n"


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
        D, T, Pl, M = eng.num_dof, eng.num_steps, eng.num_params, 2
        with_vel = name == "pl160"                                            # 2 x 16 x 2 = 64 observations
        steps = [T // 2, T - 1]
        n = M * D * (2 if with_vel else 1)
        gen = torch.Generator(device="cuda").manual_seed(1)
        rows = torch.zeros((Pl + 1, Pl), device="cuda")
        rows[:Pl] = torch.eye(Pl, device="cuda")
        z = torch.zeros((Pl + 1, D), device="cuda")
        mu = torch.randn((B, Pl), device="cuda", generator=gen)
        L = torch.tril(0.3 * torch.randn((B, Pl, Pl), device="cuda", generator=gen))
        L.diagonal(dim1=1, dim2=2).abs_().add_(0.1)
        ip = 2.0 * torch.rand((B, D), device="cuda", generator=gen) - 1.0
        iv = torch.zeros((B, D), device="cuda")
        with torch.no_grad():
            unit = eng.trajectory(rows, z, z)
            zero = eng.trajectory(torch.zeros((B, Pl), device="cuda"), ip, iv)
        # rows in the kernel's order: step, then positions by DoF, then velocities by DoF
        arrays = (0, 1) if with_vel else (0,)
        H = torch.stack([(unit[o][:Pl] - unit[o][Pl])[:, steps] for o in arrays], dim=2)          # [Pl, M, arrays, D]
        H = H.permute(1, 2, 3, 0).reshape(n, Pl).contiguous()
        c = torch.stack([zero[o][:, steps] for o in arrays], dim=2).reshape(B, n).contiguous()
        w = mu + torch.einsum("bpq,bq->bp", L, torch.randn((B, Pl), device="cuda", generator=gen))
        y = (w @ H.T + c + args.sigma * torch.randn((B, n), device="cuda", generator=gen)).contiguous()
        y4 = y.view(B, M, len(arrays), D)
        yp, yv = y4[:, :, 0].contiguous(), (y4[:, :, 1].contiguous() if with_vel else None)
        R = (args.sigma ** 2) * torch.eye(n, device="cuda")

        def composed(mean, fac):
            A = H @ torch.tril(fac)                                       # [B, n, Pl]
            S = A @ A.transpose(1, 2) + R
            dist = torch.distributions.MultivariateNormal(mean @ H.T + c, scale_tril=torch.linalg.cholesky(S), validate_args=False)
            return dist.log_prob(y)

        def kernel(mean, fac):
            return eng.trajectory_log_prob(mean, fac, steps, yp, args.sigma, ip, iv, obs_vel=yv,
                                           obs_vel_std=args.sigma if with_vel else None)

        def fwdbwd(fn):
            def call():
                mean, fac = mu.detach().requires_grad_(True), L.detach().requires_grad_(True)
                fn(mean, fac).sum().backward()
                return mean.grad, fac.grad
            return call

        def fwd(fn):
            def call():
                with torch.no_grad():
                    return fn(mu, L)
            return call

        got, want = fwd(kernel)(), fwd(composed)()
        name_k = eng.last_kernel()
        got_g, want_g = fwdbwd(kernel)(), fwdbwd(composed)()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())    # noqa: E731
        diffs = rel(got, want), rel(got_g[0], want_g[0]), rel(got_g[1], torch.tril(want_g[1]))
        del got, want, got_g, want_g
        tk = timed(fwd(kernel), args.groups, args.group)
        tc = timed(fwd(composed), max(args.groups // 4, 5), max(args.group // 5, 1), warm=3)
        tkb = timed(fwdbwd(kernel), args.groups, args.group)
        tcb = timed(fwdbwd(composed), max(args.groups // 4, 5), max(args.group // 5, 1), warm=3)
        tk2 = timed(fwd(kernel), args.groups, args.group)
        q = lambda x: [float(np.percentile(x, p)) for p in (50, 10, 90)]       # noqa: E731
        KT = Pl // D + 2
        lds, waves, on_cu = lds_plan(Pl, n, M, KT)
        rec = dict(shape=name, B=B, T=T, D=D, Pl=Pl, M=M, n=n, sigma=args.sigma, kernel=name_k, fwd_us=q(tk), fwd_again_us=q(tk2),
                   torch_fwd_us=q(tc), ratio_fwd=float(np.median(tc) / np.median(tk)), fwdbwd_us=q(tkb), torch_fwdbwd_us=q(tcb),
                   ratio_fwdbwd=float(np.median(tcb) / np.median(tkb)), diff_lp=diffs[0], diff_gm=diffs[1], diff_gL=diffs[2],
                   lds_bytes=lds, waves=waves, waves_per_cu=on_cu)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del L, mu
        torch.cuda.empty_cache()
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
