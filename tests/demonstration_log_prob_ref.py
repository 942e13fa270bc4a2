"""
The float64 reference of TrajectoryEngine.demonstration_log_prob / demonstration_log_prob_vjp (mpk_demonstration_log_prob, _vjp), shared
by tests/test_gpu_demo_log_prob.py and tests/test_demo_log_prob_host.py.  Built on tests/trajectory_log_prob_ref.py: every (step, DoF)
of a demonstration whose sigma is kept is one of ITS scalar observations (`observations(name, b, range(T), ..)`: rows from the float64
Jacobian of the CPU oracle, offsets from the oracle's trajectory at zero parameters), and the reference stays ITS dense n x n formula
(`log_prob`, numpy Cholesky of A A^T + diag(sigma^2)) with float64 torch autograd of it (`autograd`) -- not the information form the
kernel evaluates.  The float32-table floor (`f32_table=True`), the bounds and the floor cap are that module's:

    log_prob          |got - ref| <= max(1e-5 (max_b |ref| + n), 4 x floor)
    g_params, g_L     |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x floor)
    floor cap         4 x floor <= 1e-2 x scale

`information_form` restates the kernel's algebra (include/mpk.h) in float64 numpy, for the host test that checks it against the dense
formula.
"""
import functools

import numpy as np

from . import trajectory_condition_ref as R
from . import trajectory_log_prob_ref as LP
from .trajectory_log_prob_ref import bounds, check, config, engine_for, floor_cap, jacobian, observations, tril64  # noqa: F401

MISSING = 0.3                                                                     # the fraction of entries at sigma = inf


def references(name, mu, L, c, pos, sd, g):
    """dict(ref_lp [B], ref_gmu [B, P], ref_gL [B, P, P], n [B], floor_*): the dense formula over the kept entries of every episode"""
    T = pos.shape[1]
    return LP.references(name, mu, L, range(T), c, ((pos, sd), None), g)


def draw(name, B, sigma, missing, seed):
    """inputs as trajectory_condition_ref.case draws them (float32-exact; the factor's strict upper triangle is NaN): parameters from the
    prior, their whole trajectory plus noise of size sigma; `missing`: about 30 % of the entries at sigma = inf, with garbage values"""
    J, P, D, T = jacobian(name)
    rng = np.random.default_rng(1000 * seed + 7 * B + T)
    mu = rng.standard_normal((B, P)).astype(np.float32)
    L = R.random_factor(P, B, seed=seed + B, nan_upper=True)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    c = R.offsets(name, ip, iv)
    w = mu.astype(np.float64) + np.einsum("bpq,bq->bp", tril64(L), rng.standard_normal((B, P)))
    y = (np.einsum("tdp,bp->btd", J[0][..., :P], w) + c[0] + sigma * rng.standard_normal((B, T, D))).astype(np.float32)
    sd = np.full((B, T, D), sigma, np.float32)
    if missing:
        gone = rng.random((B, T, D)) < MISSING
        sd[gone] = np.inf
        y[gone] = 1e6                                                              # a removed entry's value is never used
    g = rng.standard_normal(B) * rng.uniform(0.5, 2.0, B)
    return dict(mu=mu, L=L, ip=ip, iv=iv, c=c, pos=y, sd=sd, g=g)


@functools.lru_cache(maxsize=None)
def case(name, B, sigma, missing, seed=1):
    """the inputs, a random non-uniform upstream gradient g [B] float64 and the float64 references, computed once and shared"""
    cs = draw(name, B, sigma, missing, seed)
    cs.update(references(name, cs["mu"], cs["L"], cs["c"], cs["pos"], cs["sd"], cs["g"]))
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def information_form(mu64, L64, ob, g):
    """(log_prob, g_params [P], g_params_L [P, P]) of one episode as include/mpk.h states the information form, in float64 numpy: the
    Gram matrix G = H^T W H is block diagonal because a row of H lives in its DoF's block"""
    P = mu64.size
    if not ob:
        return 0.0, np.zeros(P), np.zeros((P, P))
    H, r0, s2 = LP.system(ob)
    w = 1.0 / s2
    r = r0 - H @ mu64
    G = H.T @ (w[:, None] * H)
    q = H.T @ (w * r)
    s, lsig, n = float(w @ (r * r)), float(np.log(s2).sum()), len(ob)
    M = np.eye(P) + L64.T @ G @ L64
    C = np.linalg.cholesky(M)
    v = L64.T @ q
    z = np.linalg.solve(C, v)
    lp = -0.5 * (s - z @ z) - 0.5 * (lsig + 2.0 * np.log(np.diag(C)).sum()) - 0.5 * n * LP.LOG_2PI
    x = np.linalg.solve(M, v)
    X = G @ L64
    gm = q - X @ x
    return float(lp), g * gm, g * np.tril(np.outer(gm, L64.T @ gm) - X @ np.linalg.inv(M))


# ---- the cases of tests/test_gpu_demo_log_prob.py's parity test, stated once: the host test checks the floor cap on every one --------
PARITY = ("cfg1_promp_zero_padded", "cfg2_prodmp", "prodmp_relative_goal", "promp_16_columns_3_dof", "prodmp_12_columns_16_dof",
          "prodmp_1_dof", "cfg4_prodmp_init_time", "cfg2_prodmp_97_steps")
BATCH_65 = ("prodmp_1_dof", "cfg4_prodmp_init_time")
SIGMAS = ((0.1, True), (1e-2, False), (1e-3, False))                              # (sigma, about 30 % of the entries missing)


def gpu_cases():
    """(name, B, sigma, missing)"""
    out = []
    for sigma, missing in SIGMAS:
        for name in PARITY:
            out += [(name, B, sigma, missing) for B in ((1, 3, 65) if name in BATCH_65 else (1, 3))]
    return out
