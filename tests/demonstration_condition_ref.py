"""
The float64 reference of TrajectoryEngine.condition_on_demonstration (mpk_demonstration_condition), shared by
tests/test_gpu_demo_condition.py and tests/test_demo_condition_host.py.  Inputs are tests/demonstration_log_prob_ref.py's (`draw`: whole
demonstrations with about 30 % of the entries missing at sigma = 0.1, complete ones at 1e-2 and 1e-3; the factor's strict upper triangle
is NaN), the cases are its `gpu_cases()`, and the reference is tests/trajectory_condition_ref.py's DENSE batch formula (`batch`: S = H
Sigma H^T + R is n x n, n up to 1000) over the kept entries of a demonstration, every (step, DoF) with 0 < sigma < inf one of ITS scalar
observations (`observations(name, b, range(T), ..)`) -- not the information form the kernel evaluates.  The float32-table floor
(`f32_table=True`) and the bound are that module's:

    |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x floor)

on the posterior mean and on the posterior COVARIANCE tril(L') tril(L')^T formed in float64 from the returned float32 factor -- never on
the factor (that module's docstring says why).

`information_form` restates the kernel's algebra (include/mpk.h: the reverse Cholesky M = K^T K, L' = tril(L) K^-1, mu' = mu + L' K^-T
v) in float64 numpy, for the host test that checks it against the dense formula.
"""
import functools

import numpy as np

from fancy_gym_amd import _lib

from . import trajectory_condition_ref as R
from .demonstration_log_prob_ref import SIGMAS, config, draw, engine_for, gpu_cases, jacobian, tril64  # noqa: F401
from .trajectory_condition_ref import bound, check, covariance  # noqa: F401

SIGNATURE = _lib.SIGNATURES["mpk_demonstration_condition"]                        # the entry under test: without it nothing here applies


def kept(name, b, c, pos, sd, f32_table=False):
    """the scalar observations of episode b: every (step, DoF) whose sigma is > 0 and finite, steps ascending, DoF ascending"""
    T = pos.shape[1]
    return [x for x in R.observations(name, b, range(T), c, ((pos, sd), None), f32_table=f32_table) if x[3] > 0.0]


def references(name, mu, L, c, pos, sd):
    """dict(ref_mu [B, P], ref_Sigma [B, P, P], floor_mu, floor_Sigma, n [B]): the dense batch formula over the kept entries of every
    episode, and its error through a float32 table"""
    B = mu.shape[0]
    L64 = tril64(L)
    ref_mu, ref_S, f_mu, f_S, n = [], [], [], [], []
    for b in range(B):
        m64 = mu[b].astype(np.float64)
        ob = kept(name, b, c, pos, sd)
        a, s = R.batch(m64, L64[b], ob)
        a32, s32 = R.batch(m64, L64[b], kept(name, b, c, pos, sd, f32_table=True))
        ref_mu.append(a); ref_S.append(s); f_mu.append(np.abs(a32 - a)); f_S.append(np.abs(s32 - s)); n.append(len(ob))
    return dict(ref_mu=np.stack(ref_mu), ref_Sigma=np.stack(ref_S), floor_mu=np.stack(f_mu), floor_Sigma=np.stack(f_S), n=np.array(n))


@functools.lru_cache(maxsize=None)
def case(name, B, sigma, missing, seed=1):
    """the inputs of demonstration_log_prob_ref.draw and the float64 references, computed once and shared (read-only)"""
    cs = draw(name, B, sigma, missing, seed)
    cs.update(references(name, cs["mu"], cs["L"], cs["c"], cs["pos"], cs["sd"]))
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def gram(ob, mu64):
    """(G [P, P], q [P]) of the kept observations: G = H^T W H (block diagonal: a row of H lives in its DoF's block), q = H^T W r"""
    H = np.stack([x[0] for x in ob])
    w = 1.0 / np.array([x[3] ** 2 for x in ob])
    r = np.array([x[2] - x[1] for x in ob]) - H @ mu64
    return H.T @ (w[:, None] * H), H.T @ (w * r)


def reverse_cholesky(M):
    """K lower triangular with M = K^T K: the left-looking Cholesky loop over reversed indices, from the bottom-right corner"""
    n = M.shape[0]
    K = np.zeros_like(M)
    for jc in range(n - 1, -1, -1):
        x = M[jc, :jc + 1] - K[jc + 1:, jc] @ K[jc + 1:, :jc + 1]
        if not x[jc] > 0.0:
            raise np.linalg.LinAlgError(f"pivot {jc} is not > 0")
        K[jc, :jc + 1] = x / np.sqrt(x[jc])
        K[jc, jc] = np.sqrt(x[jc])
    return K


def lower_inverse(K):
    """K^-1 of a lower-triangular K row by row, as the kernel does it in place: row j from the rows above it"""
    n = K.shape[0]
    Ki = np.zeros_like(K)
    for j in range(n):
        inv = 1.0 / K[j, j]
        Ki[j, :j] = (0.0 - K[j, :j] @ Ki[:j, :j]) * inv
        Ki[j, j] = inv
    return Ki


def information_form(mu64, L64, ob):
    """(mu' [P], L' [P, P]) of one episode as include/mpk.h states mpk_demonstration_condition, in float64 numpy; ob: the kept
    observations (every sigma > 0).  Nothing kept: the prior"""
    if not ob:
        return mu64.copy(), L64.copy()
    assert all(x[3] > 0.0 for x in ob), "sigma == 0 cannot be expressed in the information form"
    P = mu64.size
    G, q = gram(ob, mu64)
    M = np.eye(P) + L64.T @ G @ L64
    K = reverse_cholesky(M)
    t = np.linalg.solve(K.T, L64.T @ q)
    Lp = L64 @ lower_inverse(K)
    return mu64 + Lp @ t, Lp
