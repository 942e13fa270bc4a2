"""
The float64 reference of the point-wise entry points with a PER-EPISODE phase (``condition_given_timing``,
``trajectory_log_prob_given_timing`` / ``_vjp_given_timing``, ``trajectory_std_given_timing``: mpk_trajectory_phase_*), shared by
tests/test_gpu_phase_points.py and tests/test_phase_points_host.py.

Per episode it builds the float64 position AND velocity Jacobians ``J [2][T, D, Pl]`` of the CPU oracle
(``oracle.mp_oracle.get_trajectory(dtype=float64)``) at that episode's tau / delay -- the oracle clips them to the bounds as the forward
does -- and the offsets ``c [2][T, D]``, the oracle's trajectory at zero parameters from the episode's init_pos / init_vel: what
tests/trajectory_fit_ref.Design does for positions, with the velocity beside it.  The trajectory is affine in the non-phase parameters,
so these are the whole map.  An observation list in tests/trajectory_condition_ref.observations' format -- steps ascending; within a
step the positions by DoF, then the velocities by DoF -- goes to the EXISTING dense references, never to the arithmetic the kernels use:

    the batch posterior (mean and covariance)           tests/trajectory_condition_ref.batch
    log N(y; H mu + c, H L L^T H^T + diag(sigma^2))     tests/trajectory_log_prob_ref.log_prob / autograd
    std[o][b, t, d] = | J[o][b, t, d] tril(L_b) |       the factor form with the per-episode Jacobian

The bounds are the project's, unchanged (those modules' ``check`` / ``bounds`` / ``bound`` / ``floor_cap``):

    posterior mean, covariance tril(L') tril(L')^T, gradients   |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x floor)
    log_prob                                                    |got - ref| <= max(1e-5 (max_b |ref| + n), 4 x floor)
    std                                                         tests/trajectory_std_ref.bound
    floor cap                                                   4 x floor <= 1e-2 x scale, for every output array of every case

``floor``: the same reference with each episode's rows and offsets rounded to float32.  Inputs: configurations and timings from
tests/demonstration_phase_ref (``CONFIGS``, ``timings``: episode b inside, on or outside the bounds by b % 3), steps from
tests/trajectory_condition_ref.draw_steps (spread steps keep the reference's own conditioning error small), float32-exact values, NaN in
the factor's strict upper triangle, a non-uniform upstream g.
"""
import functools

import numpy as np
import torch

from oracle import mp_oracle as O

from . import demonstration_phase_ref as DP
from . import trajectory_condition_ref as R
from . import trajectory_log_prob_ref as LP
from . import trajectory_std_ref as SR
from .demonstration_phase_ref import BATCHES, CONFIGS, LIMIT, OVER_LIMIT, cfg, engine_for, shape, timings  # noqa: F401
from .trajectory_std_ref import random_factor, tril64  # noqa: F401

SEED = 1
# one name per rows-per-lane count NS = 1, 2, 3 (Pl = 21, 110, 160), the two of the reference's own learned-phase families
NS_NAMES = ("tt_prodmp_70_steps", "promp_10_basis_11_dof", LIMIT)
TIMING_NAMES = ("beerpong_promp", "tt_prodmp_70_steps")
FREE = "promp_9_basis_5_dof"                # more free parameters per DoF than the composition tests' exact observations


@functools.lru_cache(maxsize=None)
def _jacobian(name, phase_bytes):
    pc, bc, tc, dt, duration = cfg(name)
    P, Pl, off, D, T = shape(name)
    phase = np.frombuffer(phase_bytes, np.float32).astype(np.float64)
    x = np.zeros((Pl + 1, P))
    x[:, :off] = phase
    x[1:, off:] = np.eye(Pl)
    z = np.zeros((Pl + 1, D))
    pos, vel = O.get_trajectory(pc, bc, tc, x, duration, dt, 0.0, z, z, dtype=np.float64)
    J = np.stack([np.moveaxis(pos[1:] - pos[0], 0, -1), np.moveaxis(vel[1:] - vel[0], 0, -1)])      # [2][T, D, Pl]
    J.setflags(write=False)
    return J


def jacobian(name, phase_row):
    """J [2][T, D, Pl] float64 of the oracle at the episode's tau / delay"""
    return _jacobian(name, np.ascontiguousarray(phase_row, np.float32).tobytes())


def offsets(name, phase, ip, iv):
    """c [2][B, T, D] float64: the oracle's (pos, vel) at zero non-phase parameters from each episode's init_pos / init_vel"""
    pc, bc, tc, dt, duration = cfg(name)
    P, Pl, off, D, T = shape(name)
    x = np.zeros((phase.shape[0], P))
    x[:, :off] = phase
    pos, vel = O.get_trajectory(pc, bc, tc, x, duration, dt, 0.0, ip.astype(np.float64), iv.astype(np.float64), dtype=np.float64)
    return np.stack([pos, vel])


def rows(name, phase, ip, iv):
    """(H [2][B, T, D, Pl], c [2][B, T, D]) float64"""
    H = np.stack([jacobian(name, phase[b]) for b in range(phase.shape[0])], axis=1)
    return H, offsets(name, phase, ip, iv)


def observations(H, c, b, steps, obs, f32=False):
    """the scalar observations of episode b in trajectory_condition_ref.observations' format and order; obs: ((values, stds) of the
    positions or None, the same of the velocities), each [B, M, D]; entries whose sigma is +inf, NaN or negative are left out"""
    D = H.shape[3]
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
                h, cc = H[o, b, t, d], c[o, b, t, d]
                if f32:
                    h, cc = h.astype(np.float32).astype(np.float64), float(np.float32(cc))
                out.append((h, cc, float(y[b, m, d]), sigma, (o, m, d)))
    return out


def draw(name, B, M, sigma, vel, seed=SEED, phase=None):
    """inputs as trajectory_condition_ref.case draws them, with the timings in front of mu [B, P] (`phase` [n_phase]: that one timing for
    every episode) and a factor [B, Pl, Pl]"""
    P, Pl, off, D, T = shape(name)
    rng = np.random.default_rng(1000 * seed + 7 * B + M)
    mu = rng.standard_normal((B, P)).astype(np.float32)
    mu[:, :off] = timings(name, B, seed) if phase is None else phase
    L = random_factor(Pl, B, seed=seed + B, nan_upper=True)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    steps = R.draw_steps(rng, T, M)
    H, c = rows(name, mu[:, :off], ip, iv)
    w = mu[:, off:].astype(np.float64) + np.einsum("bpq,bq->bp", tril64(L), rng.standard_normal((B, Pl)))
    obs = []
    for o in range(2):
        if o == 1 and not vel:
            obs.append(None)
            continue
        y = np.einsum("bmdp,bp->bmd", H[o][:, list(steps)], w) + c[o][:, list(steps)] + sigma * rng.standard_normal((B, M, D))
        obs.append((y.astype(np.float32), np.full((B, M, D), sigma, np.float32)))
    g = rng.standard_normal(B) * rng.uniform(0.5, 2.0, B)
    return dict(mu=mu, L=L, ip=ip, iv=iv, steps=steps, pos=obs[0], vel=obs[1], H=H, c=c, g=g, off=off)


def condition_references(cs, obs=None, mu=None, L=None, steps=None):
    """dict(ref_mu [B, Pl], ref_Sigma [B, Pl, Pl], floor_mu, floor_Sigma) of the dense batch formula; obs / mu / L / steps override"""
    obs = (cs["pos"], cs["vel"]) if obs is None else obs
    mu, L = cs["mu"] if mu is None else mu, cs["L"] if L is None else L
    steps = cs["steps"] if steps is None else steps
    off, B = cs["off"], cs["mu"].shape[0]
    L64 = tril64(L)
    ref_mu, ref_S, f_mu, f_S = [], [], [], []
    for b in range(B):
        m64 = np.asarray(mu)[b, off:].astype(np.float64)
        a, s = R.batch(m64, L64[b], observations(cs["H"], cs["c"], b, steps, obs))
        a32, s32 = R.batch(m64, L64[b], observations(cs["H"], cs["c"], b, steps, obs, f32=True))
        ref_mu.append(a); ref_S.append(s); f_mu.append(np.abs(a32 - a)); f_S.append(np.abs(s32 - s))
    return dict(ref_mu=np.stack(ref_mu), ref_Sigma=np.stack(ref_S), floor_mu=np.stack(f_mu), floor_Sigma=np.stack(f_S))


def log_prob_references(cs, obs=None, mu=None, L=None, steps=None):
    """dict(ref_lp [B], ref_gmu [B, P], ref_gL [B, Pl, Pl], n [B], floor_*) of the dense formula; exact zeros in the phase columns"""
    obs = (cs["pos"], cs["vel"]) if obs is None else obs
    mu, L = cs["mu"] if mu is None else mu, cs["L"] if L is None else L
    steps = cs["steps"] if steps is None else steps
    off, B = cs["off"], cs["mu"].shape[0]
    L64 = tril64(L)
    out = {k: [] for k in ("ref_lp", "ref_gmu", "ref_gL", "n", "floor_lp", "floor_gmu", "floor_gL")}
    front = np.zeros(off)
    for b in range(B):
        m64 = np.asarray(mu)[b, off:].astype(np.float64)
        ob = observations(cs["H"], cs["c"], b, steps, obs)
        lp, gm, gL = LP.autograd(m64, L64[b], ob, cs["g"][b])
        lp_np = LP.log_prob(m64, L64[b], ob)
        assert (np.isnan(lp) and np.isnan(lp_np)) or abs(lp - lp_np) <= 1e-9 * (abs(lp_np) + len(ob)), (lp, lp_np)
        lp32, gm32, gL32 = LP.autograd(m64, L64[b], observations(cs["H"], cs["c"], b, steps, obs, f32=True), cs["g"][b])
        vals = (lp_np, np.concatenate([front, gm]), gL, len(ob), abs(lp32 - lp_np), np.concatenate([front, np.abs(gm32 - gm)]),
                np.abs(gL32 - gL))
        for k, v in zip(out, vals):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


def std_reference(H, L32):
    """(ref [2][B, T, D] float64: the factor-form norm with each episode's own Jacobian; e32 [2][B, T, D]: the error of the float32 CPU
    einsum of the same expression against it, the rounding floor of trajectory_std_ref.bound)"""
    L64 = tril64(L32)
    L32t = torch.from_numpy(L64.astype(np.float32))
    ref, e32 = [], []
    for o in range(2):
        r = np.sqrt((np.einsum("btdp,bpj->btdj", H[o], L64) ** 2).sum(-1))
        y32 = torch.einsum("btdp,bpj->btdj", torch.from_numpy(H[o].astype(np.float32)), L32t)
        s32 = torch.sqrt((y32 * y32).sum(-1)).numpy().astype(np.float64)
        ref.append(r)
        e32.append(np.abs(s32 - r))
    return ref, e32


def std_floor_cap(ref, e32, what):
    """the std's float32 floor against the cap: 4 x floor <= 1e-2 x scale, per output array"""
    for o in range(2):
        scale, worst = float(np.abs(ref[o]).max()), float(e32[o].max())
        print(f"[std] {what} {SR.LABELS[o]}: f32 floor {worst:.3e}  scale {scale:.3e}  floor / scale {worst / scale if scale else 0.0:.2e}")
        assert 4.0 * worst <= LP.FLOOR_CAP * scale, f"{what} {SR.LABELS[o]}: floor {worst:.3e} against scale {scale:.3e}"


def condition_floor_cap(ref, what):
    for label, r, fl in zip(R.LABELS, (ref["ref_mu"], ref["ref_Sigma"]), (ref["floor_mu"], ref["floor_Sigma"])):
        scale, worst = float(np.abs(r).max()), float(fl.max())
        print(f"[cond] {what} {label}: f32 floor {worst:.3e}  scale {scale:.3e}  floor / scale {worst / scale if scale else 0.0:.2e}")
        assert 4.0 * worst <= LP.FLOOR_CAP * scale, f"{what} {label}: floor {worst:.3e} against scale {scale:.3e}"


def _freeze(cs):
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def n_obs(name, M, vel):
    return M * shape(name)[3] * (2 if vel else 1)


@functools.lru_cache(maxsize=None)
def case(name, B, M, sigma, vel, seed=SEED):
    """the inputs and every float64 reference of one case, computed once and shared (read-only): the posterior's, the likelihood's where
    n <= 64 (``has_lp``), the std's (of the PRIOR factor)"""
    cs = draw(name, B, M, sigma, vel, seed)
    cs.update(condition_references(cs))
    cs["has_lp"] = n_obs(name, M, vel) <= 64
    if cs["has_lp"]:
        cs.update(log_prob_references(cs))
    cs["ref_std"], cs["e32_std"] = std_reference(cs["H"], cs["L"])
    return _freeze(cs)


def max_steps(name):
    return min(shape(name)[4] - 1, 32)


def gpu_cases():
    """(name, B, M, sigma, vel) of the parity test: every configuration at B = 3, M = 3, both sigmas, positions alone and with
    velocities; the three NS names at B = 1 and 9 too; M = 1 and the configuration's largest M (32 on tt_prodmp_70_steps) on the NS
    names and the reference's own two families"""
    out = []
    for sigma in (0.1, 1e-3):
        for name in CONFIGS:
            out += [(name, 3, 3, sigma, vel) for vel in (False, True)]
    for name in NS_NAMES:
        out += [(name, B, 3, 1e-3, True) for B in (1, 9)]
    for name in dict.fromkeys(NS_NAMES + TIMING_NAMES):
        out += [(name, 3, 1, 1e-3, True), (name, 3, max_steps(name), 1e-3, False)]
    out.append((LIMIT, 3, 4, 1e-3, False))                  # Pl = 160 at n = 64 (conditioning: M = 5 is max_steps above)
    return out


def check_condition(got_mu, got_L, cs, what, ref=None):
    DP.check_condition(got_mu, got_L, cs if ref is None else dict(ref, mu=cs["mu"], off=cs["off"]), what)


def check_log_prob(got, cs, what, ref=None):
    DP.check_log_prob(got, cs if ref is None else dict(ref, off=cs["off"]), what)
