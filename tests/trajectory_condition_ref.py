"""
The float64 reference of TrajectoryEngine.condition (mpk_trajectory_condition), shared by tests/test_gpu_traj_condition.py and
tests/test_traj_condition_host.py.

With a shared phase the trajectory is affine in the parameters, so the float64 Jacobian J of tests/test_gpu_traj_vjp.py (built from the
CPU oracle, cached per configuration) gives every observation row, H = J[o][steps][..., :P], and the oracle's trajectory at zero
parameters with the episode's init_pos / init_vel gives the offset c.  The reference is the BATCH formula per episode in float64 numpy,

    S = H Sigma H^T + R,   mu' = mu + Sigma H^T S^-1 (y - H mu - c),   Sigma' = Sigma - Sigma H^T S^-1 H Sigma,   Sigma = L L^T,

over the observations whose standard deviation is a finite number >= 0 (R = diag(sigma^2)) -- not the arithmetic the kernel uses.
Beside it: `sequential`, a float64 numpy restatement of the kernel's sequential square-root update (mpk.h), and the batch formula
with H and c rounded to float32 -- what any evaluation through a float32 table pays, the rounding floor of the bound.

Bound (per output array), the project's own as test_gpu_traj_vjp.check applies it:
    |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the float32-table floor)
applied to the posterior mean and to the posterior COVARIANCE tril(L') tril(L')^T formed in float64 from the returned float32 factor.

Never compare L' with np.linalg.cholesky(Sigma'): the posterior is near-singular by design (every observation with a small sigma takes
a direction out of it), and the Cholesky factor of a near-singular matrix is ill-posed -- the two factors of the SAME covariance were
measured up to 4e-3 apart at sigma = 1e-3, and at Pl = 160 the reference covariance is not even positive definite in float64, so
np.linalg.cholesky raises.  L' L'^T is the well-posed quantity.  Do not "tighten" the check to the factor.
"""
import functools

import numpy as np
import torch

from oracle import mp_oracle as O

from .test_gpu_trajectory import RTOL
from .test_gpu_traj_vjp import config, engine_for, jacobian  # noqa: F401  (re-exported: the tests take them from here)
from .trajectory_std_ref import random_factor, tile_names, tril64  # noqa: F401

LABELS = ("params_post", "Sigma_post")


def offsets(name, ip, iv):
    """[2][B, T, D] float64: the oracle's (pos, vel) at zero parameters from each episode's init_pos / init_vel"""
    pc, bc, tc, dt, duration, init_time, _ = config(name)
    P = O.num_params(pc, bc, tc)
    B = ip.shape[0]
    pos, vel = O.get_trajectory(pc, bc, tc, np.zeros((B, P)), duration, dt, init_time, ip.astype(np.float64), iv.astype(np.float64),
                                dtype=np.float64)
    return pos, vel


def observations(name, b, steps, c, obs, f32_table=False):
    """the scalar observations of episode b in the kernel's order -- steps ascending; within a step the positions, DoF ascending, then the
    velocities -- as a list of (h [P], c, y, sigma, (o, m, d)); obs: ((values, stds) of the positions or None, the same of the
    velocities), each [B, M, D]; entries whose sigma is +inf, NaN or negative are left out"""
    J, P, D, _ = jacobian(name)
    out = []
    for m, t in enumerate(steps):
        for o in range(2):
            if obs[o] is None:
                continue
            y, sd = obs[o]
            for d in range(D):
                sigma = float(sd[b, m, d])
                if not (sigma >= 0.0) or np.isinf(sigma):
                    continue
                h, cc = J[o][t, d, :P], c[o][b, t, d]
                if f32_table:
                    h, cc = h.astype(np.float32).astype(np.float64), float(np.float32(cc))
                out.append((h, cc, float(y[b, m, d]), sigma, (o, m, d)))
    return out


def batch(mu, L64, ob):
    """(mu', Sigma') of the batch formula for one episode; ob: the list `observations` returns"""
    Sigma = L64 @ L64.T
    if not ob:
        return mu.copy(), Sigma
    H = np.stack([x[0] for x in ob])
    r = np.array([x[2] - x[1] for x in ob]) - H @ mu
    S = H @ Sigma @ H.T + np.diag([x[3] ** 2 for x in ob])
    G = Sigma @ H.T
    return mu + G @ np.linalg.solve(S, r), Sigma - G @ np.linalg.solve(S, G.T)


def sequential(mu, L64, ob):
    """(mu', L') of the kernel's arithmetic restated in float64 numpy: Carlson's square-root measurement update in its lower-triangular
    form, one scalar observation after the other (mpk.h: mpk_trajectory_condition)"""
    mu, L = mu.copy(), L64.copy()
    n = mu.size
    for h, c, y, sigma, _ in ob:
        if not (sigma >= 0.0) or np.isinf(sigma):
            continue
        v = L.T @ h
        b = np.empty(n + 1)
        b[n] = sigma * sigma
        for j in range(n - 1, -1, -1):
            b[j] = b[j + 1] + v[j] * v[j]
        if not b[0] > 0.0:
            continue
        r = y - c - h @ mu
        w = np.zeros(n)
        for j in range(n - 1, -1, -1):
            col = L[:, j].copy()
            if b[j] > 0.0 and b[j + 1] > 0.0:
                L[:, j] = col * np.sqrt(b[j + 1] / b[j]) - w * (v[j] / (np.sqrt(b[j + 1]) * np.sqrt(b[j])))
            elif b[j] > 0.0:
                L[:, j] = 0.0
            w += col * v[j]
        mu = mu + w * (r / b[0])
    return mu, L


def draw_steps(rng, T, M):
    """M observed steps from 1 .. T - 1, one from each of M equal bands of the horizon.  Via-points that crowd together (three of the
    last twenty steps, say) make H Sigma H^T nearly singular, and at sigma = 0 the BATCH formula -- the reference -- then loses what
    its condition number takes: at cond 1e12 it was measured 1e-6 off while the sequential update met the via-points to 1e-15.  Spread
    steps keep the reference's own error below the bounds the tests state."""
    edges = np.linspace(1, T, M + 1).astype(int)
    assert (np.diff(edges) >= 1).all(), (T, M)
    return tuple(int(rng.integers(edges[m], edges[m + 1])) for m in range(M))


@functools.lru_cache(maxsize=None)
def case(name, B, M, sigma, seed=0, vel=False, nan_upper=True):
    """inputs (float32-exact values) and the float64 references of one test case, computed once and shared:
    dict(mu, L, ip, iv, steps, pos=(y, sd), vel=(y, sd) or None, ref_mu, ref_Sigma, floor_mu, floor_Sigma)"""
    J, P, D, T = jacobian(name)
    rng = np.random.default_rng(1000 * seed + 7 * B + M)
    mu = rng.standard_normal((B, P)).astype(np.float32)
    L = random_factor(P, B, seed=seed + B, nan_upper=nan_upper)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    steps = draw_steps(rng, T, M)
    c = offsets(name, ip, iv)
    # observed values: the trajectory of parameters drawn from the prior, plus noise of the observation's own size
    w = mu.astype(np.float64) + np.einsum("bpq,bq->bp", tril64(L), rng.standard_normal((B, P)))
    obs = []
    for o in range(2):
        if o == 1 and not vel:
            obs.append(None)
            continue
        y = np.einsum("mdp,bp->bmd", J[o][list(steps)][..., :P], w) + c[o][:, list(steps)] + sigma * rng.standard_normal((B, M, D))
        obs.append((y.astype(np.float32), np.full((B, M, D), sigma, np.float32)))
    out = dict(mu=mu, L=L, ip=ip, iv=iv, steps=steps, pos=obs[0], vel=obs[1], c=c)
    out.update(references(name, mu, L, steps, c, obs))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def references(name, mu, L, steps, c, obs):
    """dict(ref_mu [B, P], ref_Sigma [B, P, P], floor_mu, floor_Sigma: the error of the batch formula through a float32 table)"""
    B = mu.shape[0]
    L64 = tril64(L)
    ref_mu, ref_S, f_mu, f_S = [], [], [], []
    for b in range(B):
        m64 = mu[b].astype(np.float64)
        a, s = batch(m64, L64[b], observations(name, b, steps, c, obs))
        a32, s32 = batch(m64, L64[b], observations(name, b, steps, c, obs, f32_table=True))
        ref_mu.append(a); ref_S.append(s); f_mu.append(np.abs(a32 - a)); f_S.append(np.abs(s32 - s))
    return dict(ref_mu=np.stack(ref_mu), ref_Sigma=np.stack(ref_S), floor_mu=np.stack(f_mu), floor_Sigma=np.stack(f_S))


def covariance(L32):
    """tril(L') tril(L')^T in float64 from a float32 factor [B, P, P] (tensor or array)"""
    L = L32.detach().cpu().numpy() if isinstance(L32, torch.Tensor) else np.asarray(L32)
    L64 = np.tril(L).astype(np.float64)
    return np.einsum("bpj,bqj->bpq", L64, L64)


def bound(r, floor):
    scale = np.abs(r).max() if r.size else 0.0
    return np.maximum(RTOL * scale + RTOL * np.abs(r), 4.0 * (floor.max() if floor.size else 0.0))


def check(got_mu, got_L, ref, what):
    """the bound on the posterior mean and on the posterior covariance; prints the measured maxima first"""
    g_mu = got_mu.detach().cpu().numpy() if isinstance(got_mu, torch.Tensor) else np.asarray(got_mu)
    pairs = ((g_mu.astype(np.float64), ref["ref_mu"], ref["floor_mu"]), (covariance(got_L), ref["ref_Sigma"], ref["floor_Sigma"]))
    for label, (g, r, fl) in zip(LABELS, pairs):
        assert g.shape == r.shape, (what, label, g.shape, r.shape)
        err = np.abs(g - r)
        tol = bound(r, fl)
        print(f"[cond] {what} {label}: max|ref| {np.abs(r).max():.3e}  max err {np.nanmax(err):.3e}  f32-table floor {fl.max():.3e}  "
              f"project rule {RTOL * np.abs(r).max():.3e}")
        assert np.isfinite(g).all(), f"{what} {label}: {(~np.isfinite(g)).sum()} entries are not finite"
        assert not (err > tol).any(), f"{what} {label}: max err {err.max():.3e}, {(err > tol).sum()} outside"
