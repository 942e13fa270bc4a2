"""
mpk_demonstration_log_prob / _vjp against what a user could do without them, on the same device (profiles/r22_demo_log_prob.md):

  kernel      TrajectoryEngine.demonstration_log_prob: one launch of k_demo_log_prob; forward + backward: the same under autograd, whose
              backward is one launch of k_demo_log_prob<.., grad>
  low rank    torch.distributions.LowRankMultivariateNormal(H mu + c, cov_factor = A = H tril(L) [B, n, Pl], cov_diag = sigma^2) -- torch's
              own information form (the Pl x Pl capacitance matrix) -- in float32 and in float64.  Timed, per call: A, the distribution,
              log_prob(y); forward + backward adds the autograd backward of its sum w.r.t. the mean and the factor
  dense       torch.distributions.MultivariateNormal(H mu + c, scale_tril = cholesky(A A^T + sigma^2 I)), float32, the n x n form, at
              `--dense-batch` episodes (its [B, n, n] covariance is 8 GB at B = 4096, n = 700); the kernel is timed at that batch too
  Not timed: the observation matrix H [n, Pl], n = T D, from one forward launch over Pl + 1 unit-vector rows, and the offsets c from one
  forward launch at zero parameters.

Shapes: cfg2 (7 DoF x 100 steps, Pl = 42, n = 700) and Pl = 160 (16 DoF x 30 steps, n = 480), every entry kept.  Device events around
groups of `--group` back-to-back calls, warm, kernel and baselines in one process; per shape the median (10th .. 90th percentile) time per
call over the groups, the ratios baseline / kernel, and the largest relative difference of the kernel's results from the float64 low-rank
ones.

    python tools/demo_log_prob_probe.py [--groups 20] [--group 5] [--shapes cfg2:4096,pl160:4096] [--dense-batch 256] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.traj_condition_probe import engine, timed  # noqa: E402


def lds_plan(D, Kloc, T, KT):
    """demo_log_prob_limits restated: (bytes per workgroup, waves per workgroup, waves per CU)"""
    Pl, cu = D * Kloc, 160 * 1024
    ld = Pl | 1
    tc = min(T, max(32, Kloc * ld // (2 * D)))
    per_wave = 8 * (Pl * (Pl + 1) // 2 + D * Kloc * Kloc + 2 * Pl + max(Kloc * ld, 2 * tc * D) + (Kloc * ld + 1) // 2 + 8)
    shared = 8 * T * KT + 64
    best = max((w * (cu // (w * per_wave + shared)), w) for w in range(1, 5) if w * per_wave + shared <= cu)
    return best[1] * per_wave + shared, best[1], best[0]


def markdown(recs):
    def us(x):
        return "failed" if x is None else f"{x[0]:,.1f} ({x[1]:,.1f} .. {x[2]:,.1f})".replace(",", " ")

    def rt(x):
        return "-" if x is None else f"{x:.2f}"
    rows = ["| shape | | B | kernel us | low rank float32 us (ratio) | low rank float64 us (ratio) | dense float32 us (ratio) | "
            "LDS / workgroup, waves, waves / CU | largest relative difference from low rank float64 (log_prob, g_params, g_params_L) |",
            "|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        head = f"| {r['shape']} (D = {r['D']}, T = {r['T']}, Pl = {r['Pl']}, n = {r['n']}) "
        tail = f"| {r['lds_bytes']} B, {r['waves']}, {r['waves_per_cu']} | {r['diff_lp']:.1e}, {r['diff_gm']:.1e}, {r['diff_gL']:.1e} |"
        for what, label in (("fwd", "forward"), ("fwdbwd", "forward + backward")):
            rows.append(head + f"| {label} | {r['B']} | `{r['kernel_' + what]}` {us(r[what + '_us'])} | {us(r['lr32_' + what + '_us'])} "
                        f"({rt(r['ratio_lr32_' + what])}) | {us(r['lr64_' + what + '_us'])} ({rt(r['ratio_lr64_' + what])}) | not run | "
                        + tail)
            rows.append(head + f"| {label} | {r['dense_B']} | {us(r['small_' + what + '_us'])} | {us(r['lr32_small_' + what + '_us'])} "
                        f"({rt(r['ratio_lr32_small_' + what])}) | {us(r['lr64_small_' + what + '_us'])} "
                        f"({rt(r['ratio_lr64_small_' + what])}) | {us(r['dense_' + what + '_us'])} ({rt(r['ratio_dense_' + what])}) " + tail)
        for k, v in r["failed"].items():
            rows.append(f"\n`{r['shape']}` `{k}` did not run: {v}")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--shapes", default="cfg2:4096,pl160:4096")
    ap.add_argument("--dense-batch", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.01)
    ap.add_argument("--markdown", metavar="FILE", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    recs = []
    for item in args.shapes.split(","):
        name, B = item.split(":")
        B = int(B)
        Bd = min(B, args.dense_batch)
        eng = engine(name)
        D, T, Pl = eng.num_dof, eng.num_steps, eng.num_params
        n = T * D
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
            unit = eng.trajectory(rows, z, z)[0]
            zero = eng.trajectory(torch.zeros((B, Pl), device="cuda"), ip, iv)[0]
        H = (unit[:Pl] - unit[Pl]).reshape(Pl, n).T.contiguous()             # [n, Pl], rows in (t, d) order
        c = zero.reshape(B, n).contiguous()
        w = mu + torch.einsum("bpq,bq->bp", L, torch.randn((B, Pl), device="cuda", generator=gen))
        y = (w @ H.T + c + args.sigma * torch.randn((B, n), device="cuda", generator=gen)).contiguous()
        y3 = y.view(B, T, D)

        def low_rank(dtype, nb=B):
            Hd, cd, yd = H.to(dtype), c[:nb].to(dtype), y[:nb].to(dtype)
            diag = torch.full((nb, n), args.sigma ** 2, device="cuda", dtype=dtype)

            def fn(mean, fac):
                mean, fac = mean.to(dtype), fac.to(dtype)
                dist = torch.distributions.LowRankMultivariateNormal(mean @ Hd.T + cd, Hd @ torch.tril(fac), diag, validate_args=False)
                return dist.log_prob(yd)
            return fn

        def dense(mean, fac):
            A = H @ torch.tril(fac)
            S = A @ A.transpose(1, 2) + (args.sigma ** 2) * torch.eye(n, device="cuda")
            dist = torch.distributions.MultivariateNormal(mean @ H.T + c[:Bd], scale_tril=torch.linalg.cholesky(S), validate_args=False)
            return dist.log_prob(y[:Bd])

        def kernel(nb=B):
            def fn(mean, fac):
                return eng.demonstration_log_prob(mean, fac, y3[:nb], args.sigma, ip[:nb], iv[:nb])
            return fn

        def fwdbwd(fn, nb=B):
            def call():
                mean, fac = mu[:nb].detach().requires_grad_(True), L[:nb].detach().requires_grad_(True)
                fn(mean, fac).sum().backward()
                return mean.grad, fac.grad
            return call

        def fwd(fn, nb=B):
            def call():
                with torch.no_grad():
                    return fn(mu[:nb], L[:nb])
            return call

        # the differences at the dense batch: torch's float64 low-rank backward does not run at every batch (see `attempt`)
        got, want = fwd(kernel(Bd), Bd)(), fwd(low_rank(torch.float64, Bd), Bd)()
        name_f = eng.last_kernel()
        got_g, want_g = fwdbwd(kernel(Bd), Bd)(), fwdbwd(low_rank(torch.float64, Bd), Bd)()
        name_b = eng.last_kernel()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())    # noqa: E731
        diffs = rel(got, want), rel(got_g[0], want_g[0]), rel(got_g[1], torch.tril(want_g[1]))
        del got, want, got_g, want_g
        q = lambda x: None if x is None else [float(np.percentile(x, p)) for p in (50, 10, 90)]       # noqa: E731
        few = dict(groups=max(args.groups // 4, 5), group=max(args.group // 5, 1), warm=3)
        failed = {}

        def attempt(key, fn):
            """a baseline that torch cannot run at this batch (a library allocation failure) is recorded, not fatal"""
            try:
                return timed(fn, **few)
            except RuntimeError as e:
                failed[key] = str(e).splitlines()[0][:160]
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                return None
        t = {}
        for what, wrap in (("fwd", fwd), ("fwdbwd", fwdbwd)):
            t[what] = timed(wrap(kernel()), args.groups, args.group)
            t["small_" + what] = timed(wrap(kernel(Bd), Bd), args.groups, args.group)
            for tag, dtype in (("lr32_", torch.float32), ("lr64_", torch.float64)):
                t[tag + what] = attempt(tag + what, wrap(low_rank(dtype)))
                t[tag + "small_" + what] = attempt(tag + "small_" + what, wrap(low_rank(dtype, Bd), Bd))
            t["dense_" + what] = attempt("dense_" + what, wrap(dense, Bd))
            torch.cuda.empty_cache()
        KT = Pl // D + 2
        lds, waves, on_cu = lds_plan(D, Pl // D, T, KT)
        rec = dict(shape=name, B=B, T=T, D=D, Pl=Pl, n=n, sigma=args.sigma, kernel_fwd=name_f, kernel_fwdbwd=name_b, dense_B=Bd,
                   diff_lp=diffs[0], diff_gm=diffs[1], diff_gL=diffs[2], lds_bytes=lds, waves=waves, waves_per_cu=on_cu, failed=failed)
        for k, v in t.items():
            rec[k + "_us"] = q(v)
        ratio = lambda a, b: None if t[a] is None else float(np.median(t[a]) / np.median(t[b]))      # noqa: E731
        for what in ("fwd", "fwdbwd"):
            for tag in ("lr32_", "lr64_"):
                rec["ratio_" + tag + what] = ratio(tag + what, what)
                rec["ratio_" + tag + "small_" + what] = ratio(tag + "small_" + what, "small_" + what)
            rec["ratio_dense_" + what] = ratio("dense_" + what, "small_" + what)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del L, mu
        torch.cuda.empty_cache()
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
