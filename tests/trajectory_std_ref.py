"""
The float64 reference of TrajectoryEngine.trajectory_std (mpk_trajectory_std), shared by tests/test_gpu_traj_std.py and
tests/test_traj_std_host.py.

With a shared phase the trajectory is affine in the parameters, so the float64 Jacobian J of tests/test_gpu_traj_vjp.py (built from the
CPU oracle, cached per configuration) is the whole map: for parameters ~ N(mean, L L^T) the standard deviation of pos / vel [t, d] is the
norm of J's row times L,

    ref[o] = sqrt(((J[o][..., :P] @ L64) ** 2).sum(-1)),      L64 = tril(L32) in float64

(the factor form; equal to sqrt(diag(J Sigma J^T)), Sigma = L L^T, which test_traj_std_host.py checks).  Beside it the float32 CPU einsum
of the same expression: what any float32 evaluation of the factor form pays, the rounding floor of the bound.

Bound (per output array), the project's own as test_gpu_traj_vjp.check applies it:
    |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the float32 einsum's max error)
"""
import numpy as np
import torch

from .test_gpu_trajectory import RTOL
from .test_gpu_traj_vjp import CONFIGS, config, engine_for, jacobian  # noqa: F401  (re-exported: the tests take them from here)

LABELS = ("pos_std", "vel_std")
# the configurations of the rank-deficient case, and of the comparison with the forward kernels
RANK_DEFICIENT = ("cfg1_promp_zero_padded", "cfg2_prodmp", "promp_16_columns_3_dof")
FORWARD = ("cfg1_promp_zero_padded", "cfg2_prodmp", "prodmp_relative_goal")


def tile_names():
    """every ProMP / ProDMP entry of CONFIGS whose route is the tile route (<= 16 DoF, <= 16 table columns)"""
    return [n for n, cfg in CONFIGS.items() if cfg[6] == "tile" and cfg[2].trajectory_generator_type in ("promp", "prodmp")]


def random_factor(P, B, seed, nan_upper=True):
    """[B, P, P] float32: a dense lower triangle 0.3 N(0, 1) with diagonal |.| + 0.1; the strict upper triangle NaN (never to be read)"""
    rng = np.random.default_rng(seed)
    L = np.tril(0.3 * rng.standard_normal((B, P, P)))
    idx = np.arange(P)
    L[:, idx, idx] = np.abs(L[:, idx, idx]) + 0.1
    L = L.astype(np.float32)
    if nan_upper:
        L[:, np.triu(np.ones((P, P), bool), 1)] = np.nan
    return L


def tril64(L32):
    return np.tril(np.nan_to_num(np.asarray(L32), nan=0.0)).astype(np.float64)


def reference(name, L32):
    """(ref [2][B, T, D] float64, e32 [2][B, T, D]: the error of the float32 CPU einsum of the same expression against it)"""
    J, P, D, T = jacobian(name)
    L64 = tril64(L32)
    assert L64.shape[1:] == (P, P), (name, L64.shape, P)
    L32t = torch.from_numpy(L64.astype(np.float32))
    ref, e32 = [], []
    for o in range(2):
        Jp = J[o][..., :P]                                                  # [T, D, P]
        r = np.sqrt((np.einsum("tdp,bpj->btdj", Jp, L64) ** 2).sum(-1))
        y32 = torch.einsum("tdp,bpj->btdj", torch.from_numpy(Jp.astype(np.float32)), L32t)
        s32 = torch.sqrt((y32 * y32).sum(-1)).numpy().astype(np.float64)
        ref.append(r)
        e32.append(np.abs(s32 - r))
    return ref, e32


def quadratic_form32(name, L32):
    """[2][B, T, D] float32 VARIANCES of the arithmetic the kernel must not use: Sigma = L L^T first, then r^T Sigma r, all float32"""
    J, P, _, _ = jacobian(name)
    L = tril64(L32).astype(np.float32)
    S = np.einsum("bpj,bqj->bpq", L, L)
    out = []
    for o in range(2):
        Jp = J[o][..., :P].astype(np.float32)
        out.append(np.einsum("tdp,bpq,tdq->btd", Jp, S, Jp))
    return out


def factor_form32(name, L32):
    """[2][B, T, D] float32: the factor form in float32 (numpy), the arithmetic the kernel has to use"""
    J, P, _, _ = jacobian(name)
    L = tril64(L32).astype(np.float32)
    out = []
    for o in range(2):
        y = np.einsum("tdp,bpj->btdj", J[o][..., :P].astype(np.float32), L)
        out.append(np.sqrt((y * y).sum(-1, dtype=np.float32)))
    return out


def bound(r, e):
    """the per-element tolerance of one output array"""
    scale = np.abs(r).max() if r.size else 0.0
    return np.maximum(RTOL * scale + RTOL * np.abs(r), 4.0 * (e.max() if e.size else 0.0))


def check(got, ref, e32, what, arrays=(0, 1)):
    """per output array: finite, non-negative, |got - ref| <= bound; prints the measured maxima first.  got[o]: a tensor or an array"""
    for o in arrays:
        g = got[o].cpu().numpy() if isinstance(got[o], torch.Tensor) else np.asarray(got[o])
        g = g.astype(np.float64)
        r, e = ref[o], e32[o]
        assert g.shape == r.shape, (what, LABELS[o], g.shape, r.shape)
        err = np.abs(g - r)
        tol = bound(r, e)
        print(f"[std] {what} {LABELS[o]}: max|ref| {np.abs(r).max():.3e}  max err {np.nanmax(err):.3e}  max f32-einsum err {e.max():.3e}  "
              f"project rule {RTOL * np.abs(r).max():.3e}")
        assert np.isfinite(g).all(), f"{what} {LABELS[o]}: {(~np.isfinite(g)).sum()} entries are not finite"
        assert (g >= 0.0).all(), f"{what} {LABELS[o]}: negative entries"
        assert not (err > tol).any(), f"{what} {LABELS[o]}: max err {err.max():.3e}, {(err > tol).sum()} outside"


def rank_deficient_factor(name, B, seed):
    """
    [B, P, P] float32 whose covariance is rank deficient with a trajectory row in its null space: DoF 0's diagonal block is the
    Cholesky factor of M M^T + 1e-12 tr(M M^T) I, the columns of M [Kloc, Kloc - 1] orthogonal in float64 to the position row of DoF 0
    at step T // 2 (the other right-singular vectors of that row, mixed by a random square matrix); the other DoFs get random
    lower-triangular blocks.  pos_std[:, T // 2, 0] is then ~1e-6 of the array's maximum: the factor form keeps it there, the
    quadratic form r^T (L L^T) r cancels to rounding noise of either sign.  Returns (L, T // 2).
    """
    J, P, D, T = jacobian(name)
    Kloc, t0 = P // D, T // 2
    rng = np.random.default_rng(seed)
    L = np.zeros((B, P, P))
    r = J[0, t0, 0, :Kloc]
    Q = np.linalg.svd(r[None], full_matrices=True)[2][1:].T             # [Kloc, Kloc - 1], orthogonal to r
    for b in range(B):
        M = Q @ rng.standard_normal((Kloc - 1, Kloc - 1))
        S = M @ M.T
        L[b, :Kloc, :Kloc] = np.linalg.cholesky(S + 1e-12 * np.trace(S) * np.eye(Kloc))
        for d in range(1, D):
            L[b, d * Kloc:(d + 1) * Kloc, d * Kloc:(d + 1) * Kloc] = np.tril(rng.standard_normal((Kloc, Kloc)))
    return L.astype(np.float32), t0
