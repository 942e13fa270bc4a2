"""
mpk_trajectory_std against what a user could do without it, on the same device (profiles/r19_traj_std.md):

  yardstick   J by one forward launch over P + 1 unit-vector rows (not timed), then float32 torch on the device:
              einsum("tdp,bpj->btdj", J, tril(L)) -> square -> sum over j -> sqrt, for pos and vel -- it writes and re-reads an
              intermediate of B T D Pl floats per output
  kernel      TrajectoryEngine.trajectory_std(L): one launch of k_traj_std_tile, nothing materialised

Device events around each call, warm, the two alternating in one process.  Prints per shape the median (10th .. 90th percentile)
times, their ratio, the largest difference of the two results, and what the kernel moves and contracts per episode, computed from the
shape: bytes read (the Pl x Pl factor as the caller stores it; the lower triangle is what is loaded) and written, and MFMA instructions
(v_mfma_f32_16x16x4_f32: DoF x row tiles x j tiles below the DoF's last row x table-column chunks x outputs).

    python tools/traj_std_probe.py [--reps 200] [--shapes cfg2:4096,cfg2:65536,cfg1:4096] [--markdown FILE]

One JSON line per shape on stdout; --markdown FILE also writes them to FILE as the table that profiles/r19_traj_std.md carries under
"Probe output"; --render LOG prints that table from the JSON lines of an earlier run, without a device.
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
    if name == "cfg2":      # ProDMP, 7 DoF, 5 basis functions, 100 steps
        return TrajectoryEngine("prodmp", "exp", "prodmp", 7, 5, dt=0.02, duration=2.0, tau=1.5, alpha_phase=3.0,
                                basis_bandwidth_factor=2, basis_alpha=10, device=0)
    if name == "cfg1":      # zero-padded ProMP, 5 DoF, 5 basis functions, 200 steps
        return TrajectoryEngine("promp", "linear", "zero_rbf", 5, 5, dt=0.02, duration=4.0, tau=4.0, num_basis_zero_start=1,
                                num_basis_zero_goal=0, basis_bandwidth_factor=3, device=0)
    raise SystemExit(f"unknown shape {name}")


def counts(eng):
    """per episode: bytes the caller's factor holds, bytes of its lower triangle, bytes written, MFMA instructions"""
    D, T, Pl = eng.num_dof, eng.num_steps, eng.num_params
    Kloc = Pl // D
    KT = Kloc + (2 if eng.mp_type == "prodmp" else 1)        # + init_pos, init_vel | + the zero-padding column
    km, nrt = (KT + 3) // 4, (T + 15) // 16
    mfma = sum(((d + 1) * Kloc + 15) // 16 for d in range(D)) * nrt * km * 2
    return dict(factor_bytes=4 * Pl * Pl, triangle_bytes=4 * Pl * (Pl + 1) // 2, written_bytes=2 * 4 * T * D, mfma=mfma)


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return np.asarray(out)


def markdown(recs):
    """the records as a table: median (10th .. 90th percentile) us, ratio, bytes and MFMA instructions per episode"""
    us = lambda x: f"{x[0]:,.1f} ({x[1]:,.1f} .. {x[2]:,.1f})".replace(",", " ")       # noqa: E731
    rows = ["| shape | B | kernel us | kernel again us | torch composition us | ratio | factor bytes (lower triangle) / episode | "
            "bytes written / episode | MFMA / episode | composition's intermediate |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        rows.append(f"| {r['shape']} (T = {r['T']}, D = {r['D']}, Pl = {r['Pl']}) | {r['B']} | `{r['kernel']}` {us(r['kernel_us'])} | "
                    f"{us(r['kernel_again_us'])} | {us(r['torch_us'])} | {r['ratio']:.1f} | {r['factor_bytes']} ({r['triangle_bytes']}) | "
                    f"{r['written_bytes']} | {r['mfma']} | " + f"{r['intermediate_bytes'] / 1e6:,.0f} MB |".replace(",", " "))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--shapes", default="cfg2:4096,cfg2:65536,cfg1:4096")
    ap.add_argument("--markdown", metavar="FILE", default=None, help="also write the results as a markdown table")
    ap.add_argument("--render", metavar="LOG", default=None, help="print the table from the JSON lines of an earlier run and exit")
    args = ap.parse_args()
    if args.render:
        with open(args.render) as f:
            print(markdown([json.loads(line) for line in f if line.startswith("{")]), end="")
        return
    recs = []
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    for item in args.shapes.split(","):
        name, B = item.split(":")
        B = int(B)
        eng = engine(name)
        D, T, Pl = eng.num_dof, eng.num_steps, eng.num_params
        # J from one forward launch over the unit vectors (not timed)
        rows = torch.zeros((Pl + 1, Pl), device="cuda")
        rows[:Pl] = torch.eye(Pl, device="cuda")
        z = torch.zeros((Pl + 1, D), device="cuda")
        pos, vel = eng.trajectory(rows, z, z)
        J = [(y[:Pl] - y[Pl]).permute(1, 2, 0).contiguous() for y in (pos, vel)]        # [T, D, Pl]
        gen = torch.Generator(device="cuda").manual_seed(1)
        L = torch.tril(0.3 * torch.randn((B, Pl, Pl), device="cuda", generator=gen))
        L.diagonal(dim1=1, dim2=2).abs_().add_(0.1)

        def composed():
            res = []
            for j in J:
                y = torch.einsum("tdp,bpj->btdj", j, L)
                res.append((y * y).sum(-1).sqrt())
            return res

        out = (torch.empty((B, T, D), device="cuda"), torch.empty((B, T, D), device="cuda"))

        def kernel():
            return eng.trajectory_std(L, out=out)

        got, want = kernel(), composed()
        torch.cuda.synchronize()
        diff = max(float(((g - w).abs().max() / w.abs().max())) for g, w in zip(got, want))
        del want
        heavy = B * T * D * Pl * 4 > 2 ** 31          # the intermediate alone is gigabytes: fewer repetitions of the yardstick
        tk = timed(kernel, args.reps, 30)
        tc = timed(composed, max(args.reps // (20 if heavy else 4), 5), 3)
        tk2 = timed(kernel, args.reps, 30)             # again behind the yardstick: the spread of the same code
        q = lambda x: [float(np.percentile(x, p)) for p in (50, 10, 90)]       # noqa: E731
        c = counts(eng)
        rec = dict(shape=name, B=B, T=T, D=D, Pl=Pl, kernel=eng.last_kernel(), kernel_us=q(tk), kernel_again_us=q(tk2), torch_us=q(tc),
                   ratio=float(np.median(tc) / np.median(tk)), max_rel_diff=diff, intermediate_bytes=B * T * D * Pl * 4 * 2, **c,
                   kernel_bytes=B * (c["factor_bytes"] + c["written_bytes"]),
                   mfma_rate_per_us=B * c["mfma"] / float(np.median(tk)))
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del L, out, J
        torch.cuda.empty_cache()
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
