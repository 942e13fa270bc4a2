"""
mpk_demonstration_condition against what a user could do without it, on the same device (profiles/r23_demo_condition.md):

  kernel       TrajectoryEngine.condition_on_demonstration: one launch of k_demo_condition
  composition  the same information form in float64 torch: the Gram matrices by einsum (G = H^T W H per episode, q = H^T W r),
               M = I + tril(L)^T G tril(L), torch.linalg.cholesky, solve_triangular (X = C^-1 tril(L)^T, so Sigma' = X^T X and
               mu' = mu + X^T C^-1 v), and a SECOND Cholesky of Sigma' to get a triangular factor back; where torch cannot run the
               batch at once (a library allocation failure), `--chunk` episodes at a time
  condition    where the horizon has at most 32 steps: the existing sequential kernel, TrajectoryEngine.condition on every step
  Not timed: the observation matrix H [n, Pl], n = T D, from one forward launch over Pl + 1 unit-vector rows, and the offsets c from one
  forward launch at zero parameters.

Shapes: cfg2 (7 DoF x 100 steps, Pl = 42, n = 700) and Pl = 160 (16 DoF x 30 steps, n = 480), every entry kept.  Device events around
groups of `--group` back-to-back calls, warm, kernel and baselines in one process; per shape the median (10th .. 90th percentile) time per
call over the groups, the ratios baseline / kernel, and the largest relative difference of the kernel's mean and covariance from the
composition's.

    python tools/demo_condition_probe.py [--groups 20] [--group 5] [--shapes cfg2:4096,pl160:256,pl160:4096] [--chunk 256] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.traj_condition_probe import engine, timed  # noqa: E402


def markdown(recs):
    def us(x):
        return "not run" if x is None else f"{x[0]:,.1f} ({x[1]:,.1f} .. {x[2]:,.1f})".replace(",", " ")

    def rt(x):
        return "-" if x is None else f"{x:.2f}"
    rows = ["| shape | B | kernel us | float64 torch composition us (ratio) | `condition`, every step us (ratio) | workgroups x waves, "
            "LDS / workgroup | largest relative difference from the composition (mean, covariance) |", "|---|---|---|---|---|---|---|"]
    for r in recs:
        rows.append(f"| {r['shape']} (D = {r['D']}, T = {r['T']}, Pl = {r['Pl']}, n = {r['n']}) | {r['B']} | `{r['kernel']}` "
                    f"{us(r['kernel_us'])} | {us(r['torch_us'])}, {r['composition']} ({rt(r['ratio_torch'])}) | {us(r['cond_us'])} ({rt(r['ratio_cond'])}) | "
                    f"{r['blocks']} x {r['waves']}, {r['lds_bytes']} B | {r['diff_mean']:.1e}, {r['diff_cov']:.1e} |")
        for k, v in r["failed"].items():
            rows.append(f"\n`{r['shape']}` B = {r['B']} `{k}` did not run: {v}")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--shapes", default="cfg2:4096,pl160:256,pl160:4096")
    ap.add_argument("--sigma", type=float, default=0.01)
    ap.add_argument("--chunk", type=int, default=256, help="episodes per call of the composition when torch cannot run the batch at once")
    ap.add_argument("--markdown", metavar="FILE", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    recs = []
    for item in args.shapes.split(","):
        name, B = item.split(":")
        B = int(B)
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
        unit = eng.trajectory(rows, z, z)[0]
        zero = eng.trajectory(torch.zeros((B, Pl), device="cuda"), ip, iv)[0]
        H = (unit[:Pl] - unit[Pl]).reshape(Pl, n).T.contiguous().double()    # [n, Pl], rows in (t, d) order
        c = zero.reshape(B, n).contiguous()
        w = mu + torch.einsum("bpq,bq->bp", L, torch.randn((B, Pl), device="cuda", generator=gen))
        y = (w @ H.float().T + c + args.sigma * torch.randn((B, n), device="cuda", generator=gen)).contiguous()
        y3 = y.view(B, T, D)
        sd = torch.full((B, T, D), args.sigma, device="cuda")
        out = (torch.empty_like(mu), torch.empty_like(L))
        eye = torch.eye(Pl, device="cuda", dtype=torch.float64)

        def kernel():
            return eng.condition_on_demonstration(mu, L, y3, sd, ip, iv, out=out)

        def composition(factor=True, lo=0, hi=B):
            m, Ld = mu[lo:hi].double(), torch.tril(L[lo:hi]).double()
            wt = sd[lo:hi].reshape(hi - lo, n).double().pow(-2)
            r = y[lo:hi].double() - c[lo:hi].double() - m @ H.T
            G = torch.einsum("np,bnq->bpq", H, wt[:, :, None] * H)
            q = torch.einsum("bn,np->bp", wt * r, H)
            M = eye + Ld.transpose(1, 2) @ G @ Ld
            C = torch.linalg.cholesky(M)
            X = torch.linalg.solve_triangular(C, Ld.transpose(1, 2), upper=False)
            t = torch.linalg.solve_triangular(C, (Ld.transpose(1, 2) @ q[:, :, None]), upper=False)
            mean = m + (X.transpose(1, 2) @ t)[:, :, 0]
            S = X.transpose(1, 2) @ X
            return mean, (torch.linalg.cholesky(S) if factor else S)

        def chunked(factor=True):
            return [composition(factor, lo, min(lo + args.chunk, B)) for lo in range(0, B, args.chunk)]

        def sequential():
            return eng.condition(mu, L, list(range(T)), y3, sd, ip, iv, out=out)

        failed = {}

        def attempt(key, fn, **kw):
            """a baseline that torch cannot run at this batch (an allocation failure, a Cholesky that meets a pivot <= 0) is recorded"""
            try:
                return timed(fn, **kw)
            except RuntimeError as e:
                failed[key] = str(e).splitlines()[0][:160]
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                return None
        got = tuple(x.clone() for x in kernel())
        kname = eng.last_kernel()
        nd = min(B, args.chunk)                                              # (the differences on the first chunk)
        want = composition(factor=False, hi=nd)
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())    # noqa: E731
        gl = torch.tril(got[1][:nd]).double()
        diffs = rel(got[0][:nd], want[0]), rel(gl @ gl.transpose(1, 2), want[1])
        del got, want, gl
        torch.cuda.empty_cache()
        few = dict(groups=max(args.groups // 4, 5), group=1, warm=3)
        t = dict(kernel=timed(kernel, args.groups, args.group), torch=None,
                 cond=attempt("condition", sequential, groups=args.groups, group=args.group) if T <= 32 else None)
        # the composition as far as torch runs it: the batch at once or `--chunk` episodes at a time (an allocation failure of the
        # batched solve), with the second Cholesky or -- where Sigma' is not positive definite in float64 -- without a factor
        how = "did not run"
        for factor, tag in ((True, ""), (False, ", WITHOUT the second Cholesky (no factor comes back)")):
            for fn, label in ((lambda: composition(factor), "the batch at once"), (lambda: chunked(factor), f"{args.chunk} at a time")):
                if t["torch"] is None and (label == "the batch at once" or B > args.chunk):
                    t["torch"] = attempt(f"composition, {label}{tag}", fn, **few)
                    how = label + tag
        blocks, waves, lds = eng.condition_on_demonstration_plan(B)
        q3 = lambda x: None if x is None else [float(np.percentile(x, p)) for p in (50, 10, 90)]       # noqa: E731
        ratio = lambda a: None if t[a] is None else float(np.median(t[a]) / np.median(t["kernel"]))   # noqa: E731
        rec = dict(shape=name, B=B, composition=how, T=T, D=D, Pl=Pl, n=n, sigma=args.sigma, kernel=kname, blocks=blocks, waves=waves, lds_bytes=lds,
                   diff_mean=diffs[0], diff_cov=diffs[1], kernel_us=q3(t["kernel"]), torch_us=q3(t["torch"]), cond_us=q3(t["cond"]),
                   ratio_torch=ratio("torch"), ratio_cond=ratio("cond"), failed=failed)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del L, mu, out
        torch.cuda.empty_cache()
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
