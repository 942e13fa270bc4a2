"""
The float64 reference of TrajectoryEngine.trajectory_log_prob / trajectory_log_prob_vjp (mpk_trajectory_log_prob, _vjp), shared by
tests/test_gpu_traj_log_prob.py and tests/test_traj_log_prob_host.py.  Built on tests/trajectory_condition_ref.py: its `case` (the
inputs), `observations` (the scalar observations of an episode in the kernel's order, rows from the float64 Jacobian of the CPU oracle,
offsets from the oracle's trajectory at zero parameters), `tril64`, `draw_steps` and the std reference's `random_factor(nan_upper=True)`.

Forward, per episode, in float64 numpy with np.linalg.cholesky, over the n observations whose standard deviation is a finite number >= 0:

    A = H tril(L),   S = A A^T + diag(sigma^2),   r = y - c - H mu,   log_prob = -1/2 r^T S^-1 r - 1/2 log det S - n / 2 log 2 pi

(n = 0: 0.0; S not positive definite: NaN).  Gradients: float64 torch autograd of the same formula on the CPU, for an upstream g [B].
Floor: the same quantities with H and c rounded to float32 (`observations(..., f32_table=True)`) -- what any evaluation through a
float32 table pays.

Bounds (the project's RTOL = 1e-5 rule, as trajectory_condition_ref.bound applies it):
    log_prob          |got - ref| <= max(1e-5 (max_b |ref| + n), 4 x floor)    n is in the scale: log p is a sum of n terms of order one
                                                                               and passes through zero
    g_params, g_L     |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x floor)
and `floor_cap` states the condition that keeps the floor term from making a bound vacuous: 4 x floor <= 1e-2 x scale.
"""
import functools

import numpy as np
import torch

from .test_gpu_trajectory import RTOL
from . import trajectory_condition_ref as R
from .trajectory_condition_ref import config, engine_for, jacobian, observations, random_factor, tril64  # noqa: F401

LABELS = ("log_prob", "g_params", "g_params_L")
LOG_2PI = float(np.log(2.0 * np.pi))
FLOOR_CAP = 1e-2


def system(ob):
    """(H [n, P], y - c [n], sigma^2 [n]) of the list `observations` returns"""
    return np.stack([x[0] for x in ob]), np.array([x[2] - x[1] for x in ob]), np.array([x[3] ** 2 for x in ob])


def log_prob(mu64, L64, ob):
    """the forward of one episode in float64 numpy"""
    if not ob:
        return 0.0
    H, r0, s2 = system(ob)
    A = H @ L64
    S = A @ A.T + np.diag(s2)
    try:
        C = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return float("nan")
    z = np.linalg.solve(C, r0 - H @ mu64)
    return float(-0.5 * z @ z - np.log(np.diag(C)).sum() - 0.5 * len(ob) * LOG_2PI)


def autograd(mu64, L64, ob, g):
    """(log_prob, g_params [P], g_params_L [P, P]) of one episode: float64 torch autograd of the formula on the CPU"""
    P = mu64.size
    if not ob:
        return 0.0, np.zeros(P), np.zeros((P, P))
    H, r0, s2 = (torch.from_numpy(x) for x in system(ob))
    mu = torch.tensor(mu64, dtype=torch.float64, requires_grad=True)
    L = torch.tensor(L64, dtype=torch.float64, requires_grad=True)
    A = H @ torch.tril(L)
    S = A @ A.T + torch.diag(s2)
    C, info = torch.linalg.cholesky_ex(S)
    if int(info) != 0:
        return float("nan"), np.full(P, np.nan), np.full((P, P), np.nan)
    z = torch.linalg.solve_triangular(C, (r0 - H @ mu)[:, None], upper=False)[:, 0]
    lp = -0.5 * (z * z).sum() - torch.log(torch.diagonal(C)).sum() - 0.5 * len(ob) * LOG_2PI
    (float(g) * lp).backward()
    return float(lp.detach()), mu.grad.numpy(), np.tril(L.grad.numpy())


def closed_form(mu64, L64, ob, g):
    """(g_params, g_params_L) as include/mpk.h states them: alpha = S^-1 r, g H^T alpha, g tril(H^T (alpha alpha^T - S^-1) A)"""
    P = mu64.size
    if not ob:
        return np.zeros(P), np.zeros((P, P))
    H, r0, s2 = system(ob)
    A = H @ L64
    S = A @ A.T + np.diag(s2)
    alpha = np.linalg.solve(S, r0 - H @ mu64)
    return g * (H.T @ alpha), g * np.tril(H.T @ (np.outer(alpha, alpha) - np.linalg.inv(S)) @ A)


def references(name, mu, L, steps, c, obs, g):
    """dict(ref_lp [B], ref_gmu [B, P], ref_gL [B, P, P], n [B], floor_lp, floor_gmu, floor_gL: the error of the same through a float32
    table); obs: ((values, stds) of the positions or None, the same of the velocities)"""
    B = mu.shape[0]
    L64 = tril64(L)
    out = {k: [] for k in ("ref_lp", "ref_gmu", "ref_gL", "n", "floor_lp", "floor_gmu", "floor_gL")}
    for b in range(B):
        m64 = mu[b].astype(np.float64)
        ob = observations(name, b, steps, c, obs)
        lp, gm, gL = autograd(m64, L64[b], ob, g[b])
        lp_np = log_prob(m64, L64[b], ob)
        assert (np.isnan(lp) and np.isnan(lp_np)) or abs(lp - lp_np) <= 1e-9 * (abs(lp_np) + len(ob)), (lp, lp_np)
        lp32, gm32, gL32 = autograd(m64, L64[b], observations(name, b, steps, c, obs, f32_table=True), g[b])
        for k, v in zip(out, (lp_np, gm, gL, len(ob), abs(lp32 - lp_np), np.abs(gm32 - gm), np.abs(gL32 - gL))):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case(name, B, M, sigma, seed=0, vel=False):
    """the inputs of trajectory_condition_ref.case (float32-exact; the factor's strict upper triangle is NaN), a random non-uniform
    upstream gradient g [B] float64 and the float64 references, computed once and shared"""
    cs = dict(R.case(name, B, M, sigma, seed=seed, vel=vel, nan_upper=True))
    for k in ("ref_mu", "ref_Sigma", "floor_mu", "floor_Sigma"):
        del cs[k]
    rng = np.random.default_rng(77 + 1000 * seed + B)
    cs["g"] = rng.standard_normal(B) * rng.uniform(0.5, 2.0, B)
    cs.update(references(name, cs["mu"], cs["L"], cs["steps"], cs["c"], (cs["pos"], cs["vel"]), cs["g"]))
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def scales(ref):
    """per output array: the scale its 1e-5 rule and its floor cap are stated in (log_prob: per episode, max_b |ref| + n_b)"""
    fin = ref["ref_lp"][np.isfinite(ref["ref_lp"])]
    lp = (np.abs(fin).max() if fin.size else 0.0) + ref["n"]
    return lp, np.nanmax(np.abs(ref["ref_gmu"]), initial=0.0), np.nanmax(np.abs(ref["ref_gL"]), initial=0.0)


def floor_cap(ref, what):
    """4 x floor <= 1e-2 x scale for every output array: the floor term cannot make a bound vacuous"""
    s_lp, s_gm, s_gL = scales(ref)
    for label, floor, scale in zip(LABELS, (ref["floor_lp"], ref["floor_gmu"], ref["floor_gL"]), (np.min(s_lp), s_gm, s_gL)):
        worst = float(np.nanmax(floor, initial=0.0))
        print(f"[logp] {what} {label}: f32-table floor {worst:.3e}  scale {scale:.3e}  floor / scale {worst / scale if scale else 0.0:.2e}")
        assert 4.0 * worst <= FLOOR_CAP * scale, f"{what} {label}: floor {worst:.3e} against scale {scale:.3e}"


def bounds(ref):
    """the per-element tolerance of (log_prob, g_params, g_params_L)"""
    s_lp, s_gm, s_gL = scales(ref)
    fl = [float(np.nanmax(ref[k], initial=0.0)) for k in ("floor_lp", "floor_gmu", "floor_gL")]
    return (np.maximum(RTOL * s_lp, 4.0 * fl[0]),
            np.maximum(RTOL * s_gm + RTOL * np.abs(ref["ref_gmu"]), 4.0 * fl[1]),
            np.maximum(RTOL * s_gL + RTOL * np.abs(ref["ref_gL"]), 4.0 * fl[2]))


def to_np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def check(got, ref, what):
    """got: (log_prob [B], g_params [B, P], g_params_L [B, P, P]) tensors or arrays (None: not compared); the bounds above; prints the
    measured maxima first"""
    refs = (ref["ref_lp"], ref["ref_gmu"], ref["ref_gL"])
    floors = (ref["floor_lp"], ref["floor_gmu"], ref["floor_gL"])
    tols = bounds(ref)
    for o in range(3):
        if got[o] is None:
            continue
        g, r = to_np(got[o]), refs[o]
        assert g.shape == r.shape, (what, LABELS[o], g.shape, r.shape)
        err = np.abs(g - r)
        print(f"[logp] {what} {LABELS[o]}: max|ref| {np.abs(r).max():.3e}  max err {np.nanmax(err):.3e}  f32-table floor "
              f"{np.max(floors[o]):.3e}  project rule {RTOL * np.max(scales(ref)[o]):.3e}")
        assert np.isfinite(g).all(), f"{what} {LABELS[o]}: {(~np.isfinite(g)).sum()} entries are not finite"
        assert not (err > tols[o]).any(), f"{what} {LABELS[o]}: max err {err.max():.3e}, {(err > tols[o]).sum()} outside"


# ---- the cases of tests/test_gpu_traj_log_prob.py's parity test, stated once: the host test checks the floor cap on every one ----------
PARITY = ("cfg1_promp_zero_padded", "cfg2_prodmp", "prodmp_relative_goal", "promp_16_columns_3_dof", "prodmp_12_columns_16_dof",
          "prodmp_1_dof", "cfg4_prodmp_init_time", "cfg2_prodmp_97_steps")        # tests/test_gpu_traj_condition.py's list
WITH_VEL = ("cfg2_prodmp", "cfg1_promp_zero_padded")
LIMIT = "prodmp_12_columns_16_dof"                                                # M = 2 with velocities: n = 64, Pl = 160
SEED = 1


def gpu_cases():
    """(name, vel, B, M, sigma): M = 2 on every name at B in {1, 3, 65}; M = 4 at B = 3 where that keeps n <= 64"""
    out = []
    for sigma in (0.1, 1e-3):
        for name in PARITY:
            for vel in (False, True) if name in WITH_VEL + (LIMIT,) else (False,):
                out += [(name, vel, B, 2, sigma) for B in (1, 3, 65)]
        out += [(name, False, 3, 4, sigma) for name in ("cfg2_prodmp", "cfg1_promp_zero_padded", LIMIT)]
        out.append(("cfg2_prodmp", True, 3, 4, sigma))
    return out
