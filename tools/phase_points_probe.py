#!/usr/bin/env python3
"""
Times the point-wise entry points with a per-episode phase (condition_given_timing, trajectory_log_prob_given_timing + its vjp,
trajectory_std_given_timing) against (a) the shared-phase kernels on a twin handle with a FIXED phase and (b) the float64 torch
composition with per-episode design matrices (built ahead of the timed window; B = 256 only: they are [B, T, D, Pl] float64).

HIP events around ONE call through the Python entry point, `--warmup` untimed calls of every route first, then `--reps` timed ones with
the routes ALTERNATING inside a repetition; prints median (min .. max) in microseconds per route.  profiles/r26_phase_points.md.

    python tools/phase_points_probe.py [--reps 15] [--warmup 3] [--batches 256 4096]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402

def shapes():
    """name: ((pc, bc, tc, dt, duration), observed steps for conditioning, for the likelihood, velocities too): the reference's two
    learned-phase families as the tests configure them, and Pl = 160 on 30 steps"""
    from oracle import mp_oracle as O
    from tests import demonstration_phase_ref as DP
    limit = (O.PhaseCfg("linear", tau=0.6, learn_tau=True, tau_bound=(0.4, 0.6)), O.BasisCfg("rbf", num_basis=10, basis_bandwidth_factor=3),
             O.TrajCfg("promp", action_dim=16), 0.02, 0.6)
    return {"TableTennis-ProDMP": (DP.cfg("tt_prodmp_350_steps"), 5, 4, True), "BeerPong-ProMP": (DP.cfg("beerpong_promp"), 5, 4, True),
            "Pl=160": (limit, 5, 4, False)}


def engines(cfg):
    import dataclasses
    from tests.test_gpu_trajectory import make_engine
    pc, bc, tc, dt, duration = cfg
    return make_engine(pc, bc, tc, dt, duration), make_engine(dataclasses.replace(pc, learn_tau=False, learn_delay=False), bc, tc, dt, duration)


def timed(fns, reps, warmup):
    """{label: sorted microseconds}: the routes alternate inside every repetition"""
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(1e3 * a.elapsed_time(b))
    return {k: sorted(v) for k, v in out.items()}


def fmt(v):
    return f"{statistics.median(v):.0f} ({v[0]:.0f} .. {v[-1]:.0f})"


def design(eng, mu, ip, iv, n_phase):
    """H [2][B, T, D, Pl] float64 and c [2][B, T, D] of the forward at every episode's own timing: Pl + 1 trajectory launches"""
    B, P = mu.shape
    base = mu.clone()
    base[:, n_phase:] = 0.0
    c = [x.double() for x in eng.trajectory(base, ip, iv)]
    z = torch.zeros_like(ip)
    zero = [x.double() for x in eng.trajectory(base, z, z)]
    H = [torch.empty(c[0].shape + (P - n_phase,), dtype=torch.float64, device=mu.device) for _ in range(2)]
    for p in range(P - n_phase):
        row = base.clone()
        row[:, n_phase + p] = 1.0
        for o, x in enumerate(eng.trajectory(row, z, z)):
            H[o][..., p] = x.double() - zero[o]
    return H, c


def run(name, B, reps, warmup, torch_too):
    cfg, Mc, Ml, vel = shapes()[name]
    eng, twin = engines(cfg)
    pc = cfg[0]
    dev, D, T, P = eng.device, eng.num_dof, eng.num_steps, eng.num_params
    n_phase = P - twin.num_params
    Pl = P - n_phase
    gen = torch.Generator(device=dev).manual_seed(0)
    mu = torch.randn((B, P), generator=gen, device=dev)
    bounds = ([pc.tau_bound] if pc.learn_tau else []) + ([pc.delay_bound] if pc.learn_delay else [])
    lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
    for i in range(n_phase):
        mu[:, i] = lo[i] + (hi[i] - lo[i]) * torch.rand(B, generator=gen, device=dev)
    L = torch.tril(0.3 * torch.randn((B, Pl, Pl), generator=gen, device=dev))
    L.diagonal(dim1=1, dim2=2).abs_().add_(0.1)
    ip, iv = torch.rand((B, D), generator=gen, device=dev) - 0.5, torch.rand((B, D), generator=gen, device=dev) - 0.5
    pos, velo = eng.trajectory(mu, ip, iv)
    g = torch.randn(B, generator=gen, device=dev, dtype=torch.float64)
    mu_s = mu[:, n_phase:].contiguous()

    def obs(M):
        steps = [int(x) for x in torch.linspace(1, T - 2, M).round().tolist()]
        kws = dict(obs_vel=velo[:, steps].contiguous() + 0.05, obs_vel_std=0.5) if vel else {}
        return (steps, pos[:, steps].contiguous() + 0.05, 0.05, ip, iv), kws
    (ac, kc), (al, kl) = obs(Mc), obs(Ml)
    rows = {}
    fns = {"phase": lambda: eng.condition_given_timing(mu, L, *ac, **kc), "shared": lambda: twin.condition(mu_s, L, *ac, **kc)}
    rows["condition"] = fns
    rows["log_prob"] = {"phase": lambda: eng.trajectory_log_prob_given_timing(mu, L, *al, **kl),
                        "shared": lambda: twin.trajectory_log_prob(mu_s, L, *al, **kl)}
    rows["log_prob_vjp"] = {"phase": lambda: eng.trajectory_log_prob_vjp_given_timing(g, mu, L, *al, **kl),
                            "shared": lambda: twin.trajectory_log_prob_vjp(g, mu_s, L, *al, **kl)}
    rows["std"] = {"phase": lambda: eng.trajectory_std_given_timing(mu, L), "shared": lambda: twin.trajectory_std(L)}
    if torch_too:
        H, c = design(eng, mu, ip, iv, n_phase)
        L64, m64 = L.double(), mu_s.double()

        def system(args, kws):
            steps, y, sd = args[:3]
            Hs = [H[0][:, steps].reshape(B, -1, Pl)] + ([H[1][:, steps].reshape(B, -1, Pl)] if vel else [])
            r = [(y.double() - c[0][:, steps]).reshape(B, -1)] + ([(kws["obs_vel"].double() - c[1][:, steps]).reshape(B, -1)] if vel else [])
            s2 = [torch.full_like(r[0], sd ** 2)] + ([torch.full_like(r[0], kws["obs_vel_std"] ** 2)] if vel else [])
            return torch.cat(Hs, 1), torch.cat(r, 1), torch.cat(s2, 1)
        Hc, rc, sc = system(ac, kc)
        Hl, rl, sl = system(al, kl)

        def t_condition():
            A = Hc @ L64
            S = A @ A.transpose(1, 2) + torch.diag_embed(sc)
            G = L64 @ A.transpose(1, 2)
            C = torch.linalg.cholesky(S)
            m = m64 + (G @ torch.cholesky_solve((rc - (Hc @ m64[..., None])[..., 0])[..., None], C))[..., 0]
            W = torch.linalg.solve_triangular(C, G.transpose(1, 2), upper=False)
            return m, L64 @ L64.transpose(1, 2) - W.transpose(1, 2) @ W

        def t_log_prob(m=m64, Lx=L64):
            A = Hl @ torch.tril(Lx)
            C = torch.linalg.cholesky(A @ A.transpose(1, 2) + torch.diag_embed(sl))
            z = torch.linalg.solve_triangular(C, (rl - (Hl @ m[..., None])[..., 0])[..., None], upper=False)[..., 0]
            return -0.5 * (z * z).sum(1) - torch.log(torch.diagonal(C, dim1=1, dim2=2)).sum(1) - 0.5 * rl.shape[1] * 1.8378770664093453

        def t_backward():
            m, Lx = m64.clone().requires_grad_(True), L64.clone().requires_grad_(True)
            (t_log_prob(m, Lx) * g).sum().backward()
            return m.grad, Lx.grad

        def t_std():
            return [torch.einsum("btdp,bpj->btdj", H[o], L64).norm(dim=-1) for o in range(2)]
        rows["condition"]["torch f64"] = t_condition
        rows["log_prob"]["torch f64"] = t_log_prob
        rows["log_prob_vjp"]["torch f64 (forward + backward)"] = t_backward
        rows["std"]["torch f64"] = t_std
    for op, fns in rows.items():
        res = timed(fns, reps, warmup)
        fns["phase"]()
        kern = eng.last_kernel()
        print(f"| {name} | {B} | {op} | {kern} | " + " | ".join(f"{k}: {fmt(v)}" for k, v in res.items()) + " |", flush=True)
    eng.check_range()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--shapes", nargs="+", default=list(shapes()))
    a = ap.parse_args()
    for name in a.shapes:
        for B in a.batches:
            run(name, B, a.reps, a.warmup, torch_too=B <= 256)
