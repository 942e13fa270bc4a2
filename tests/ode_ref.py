"""
A check of the HIP path that does NOT go through the oracle's recollection of mp_pytorch: the movement-primitive
trajectories are, by their published definition (Ijspeert et al. 2013, eq. 2.1-2.3; Li et al. 2023 "ProDMP", eq. 1-4),
solutions of the second-order system

        tau^2 y'' = alpha (beta (g - y) - tau y') + f(x),     f(x) = x * sum_k phi_k(x) w_k,     beta = alpha / 4,

with x the canonical phase and phi_k normalised Gaussian basis functions.  In scaled time s = (t - delay) / tau:

        y_ss + alpha y_s + alpha beta y = alpha beta g + f(x(s)),      x(s) = exp(-alpha_x s).

(the linear phase generator has x(s) = min(s, 1): ``solve(..., phase=linear_phase)``.)  The explicit Euler recurrence of the DMP
is first order in dt: ``extrapolate`` combines a run at dt with one at dt / 2 so that the leading error term cancels and the
comparison with the ODE becomes tight without any reference for the recurrence itself.

This module integrates that system with SciPy (``solve_ivp``, rtol 1e-10) from a boundary condition; the tests compare
it with what libmpk's kernels return.  The ONLY things taken from the library are its construction-time constants --
basis centres / bandwidths (``mpk_host_rbf``) and the per-column scale factors (``mpk_prodmp_tables``) -- i.e. *which*
ODE is solved is the library's statement of its basis; *that the kernels solve it* (closed form, boundary-condition
solve, scale folding, replanning, table lookup) is what is verified.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from scipy.integrate import solve_ivp


def rbf_constants(engine):
    """centres (phase space) and bandwidths of the engine's normalised RBFs, float64 (library construction-time values)"""
    from fancy_gym_amd import _lib
    lib = _lib.load()
    n = lib.mpk_host_rbf(C.byref(engine.config), None, None)
    assert n > 0
    cen, bw = np.empty(n), np.empty(n)
    assert lib.mpk_host_rbf(C.byref(engine.config), cen.ctypes.data, bw.ctypes.data) == n
    return cen, bw


def forcing(x, cen, bw, w, first=0):
    """x: [...]; w: [..., nb] -> x * sum_k phi_k(x) w_k with phi normalised over ALL centres, learnable columns first.."""
    e = np.exp(-0.5 * bw * (x[..., None] - cen) ** 2)
    phi = e / e.sum(axis=-1, keepdims=True) if cen.shape[0] > 1 else e
    nb = w.shape[-1]
    return x * np.sum(phi[..., first:first + nb] * w, axis=-1)


def linear_phase(s):
    """the linear phase generator's bounded phase: clip(s, 0, 1) -- not smooth at s = 1"""
    return min(max(s, 0.0), 1.0)


linear_phase.smooth = False


def solve(alpha, alpha_x, cen, bw, w, g, s_b, y_b, ys_b, s_eval, first=0, phase=None):
    """
    Integrate  y_ss = alpha (alpha/4 (g - y) - y_s) + f(x(s))  for N independent scalar problems at once.
      w [N, nb], g [N], y_b, ys_b [N] (ys = dy/ds = tau * dy/dt), s_b scalar, s_eval [M] increasing (>= s_b)
      phase: a callable x(s) of a scalar s >= 0; default exp(-alpha_x s).  A callable is taken as NOT smooth unless it carries
      ``smooth = True``: the solver's step is then capped at 1/200 of a phase unit, small against the width of a basis
      function (the centres of nb functions lie 1 / (nb - 1) apart), so that no step jumps a kink unnoticed.
    Returns y [N, M], ys [N, M].
    """
    N = w.shape[0]
    beta = alpha / 4.0
    max_step = np.inf if phase is None or getattr(phase, "smooth", False) else 5e-3

    def rhs(s, u):
        y, z = u[:N], u[N:]
        x = np.exp(-alpha_x * max(s, 0.0)) if phase is None else phase(max(s, 0.0))
        f = forcing(np.full(N, x), cen, bw, w, first)
        return np.concatenate([z, alpha * (beta * (g - y) - z) + f])

    s_eval = np.asarray(s_eval, np.float64)
    out_y, out_z = np.empty((N, s_eval.size)), np.empty((N, s_eval.size))
    # samples marginally before the boundary (index rounding) are integrated backwards: the two directions separately
    for mask, direction in ((s_eval >= s_b, 1.0), (s_eval < s_b, -1.0)):
        if not mask.any():
            continue
        # distinct points in integration order (several samples may share one table grid point, e.g. before the delay)
        pts, inv = np.unique(direction * s_eval[mask], return_inverse=True)
        pts = direction * pts
        y_u, z_u = np.empty((N, pts.size)), np.empty((N, pts.size))
        at_b = pts == s_b
        y_u[:, at_b] = y_b[:, None]; z_u[:, at_b] = ys_b[:, None]
        if (~at_b).any():
            sol = solve_ivp(rhs, [s_b, pts[~at_b][-1]], np.concatenate([y_b, ys_b]), t_eval=pts[~at_b], rtol=1e-10,
                            atol=1e-12, method="DOP853", max_step=max_step)
            assert sol.success, sol.message
            y_u[:, ~at_b] = sol.y[:N]; z_u[:, ~at_b] = sol.y[N:]
        out_y[:, mask] = y_u[:, inv]
        out_z[:, mask] = z_u[:, inv]
    return out_y, out_z


def table_indices(times32, tau32, delay32, scaled_dt32):
    """the integer part of the ProDMP path, fp32 recipe: round_half_even(max((t - delay)/tau, 0) / scaled_dt)"""
    f = np.float32
    s = np.maximum((times32.astype(f) - f(delay32)) / f(tau32), f(0)).astype(f)
    return np.rint((s / f(scaled_dt32)).astype(f)).astype(np.int64)


def extrapolate(coarse, fine, t_coarse, t_fine, first_sample="init"):
    """
    Richardson extrapolation of a first-order scheme: 2 y(dt/2) - y(dt) at the coarse run's sample times, which removes the
    leading error term.  coarse [B, T, D] with times t_coarse [T] or [B, T]; fine [B, 2T, D] from a run at dt / 2 with times
    t_fine.  Which fine samples are the coarse ones follows from where the boundary lies:
      'init': the first sample IS the boundary (init_time + dt); the fine run was started at init_time + dt / 2, so its first
              sample is the same instant, and its samples 0, 2, 4, ... are the coarse samples;
      'step': the boundary is init_time for both runs, and the fine samples 1, 3, 5, ... are the coarse ones.
    The two time grids must coincide to 1e-6.
    """
    off = {"init": 0, "step": 1}[first_sample]
    T = coarse.shape[1]
    assert fine.shape[1] == 2 * T, (coarse.shape, fine.shape)
    tc, tf = np.asarray(t_coarse, np.float64), np.asarray(t_fine, np.float64)[..., off::2]
    assert tc.shape[-1] == T and tf.shape[-1] == T
    assert np.abs(tc - tf).max() <= 1e-6, np.abs(tc - tf).max()
    return 2.0 * np.asarray(fine, np.float64)[:, off::2] - np.asarray(coarse, np.float64)
