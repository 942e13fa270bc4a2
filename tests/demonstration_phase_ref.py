"""
The float64 reference of the demonstration entry points with a PER-EPISODE phase (``timing="given"``: mpk_demonstration_phase_log_prob,
_vjp, _condition), shared by tests/test_gpu_demo_phase.py and tests/test_demo_phase_host.py.

Per episode it builds ``tests/trajectory_fit_ref.Design(pc, bc, tc, dt, duration, init_time, phase[b])``: the float64 CPU oracle at that
episode's tau / delay (the oracle clips them to the bounds as the forward does) -- what tests/test_gpu_traj_fit.py trusts for k_phase_fit.
``Psi [D, T, Kloc]`` and ``offset()`` give every kept (t, d) one scalar observation ``(h [Pl], c, y, sigma)``, h living in its DoF's
block, and the reference is the DENSE formula over them, never the information form the kernel evaluates:

    log N(y; H mu + c, H L L^T H^T + diag(sigma^2))     tests/trajectory_log_prob_ref.log_prob / autograd (float64 torch autograd)
    the batch posterior (mean and covariance)           tests/trajectory_condition_ref.batch

The bounds are the project's (those modules' ``check`` / ``bounds`` / ``bound`` / ``floor_cap``):

    log_prob                         |got - ref| <= max(1e-5 (max_b |ref| + n), 4 x floor)
    gradients, posterior mean, cov   |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x floor)
    floor cap                        4 x floor <= 1e-2 x scale

``floor``: the same reference with each episode's Psi and c rounded to float32.  The posterior covariance is tril(L') tril(L')^T formed
in float64, never the factor.  Gradients are [B, P] / [B, Pl, Pl] with exact zeros in the phase columns of g_params: the likelihood is
differentiated at the given timing.

Inputs are drawn as tests/demonstration_log_prob_ref.draw draws them (float32-exact, NaN in the factor's strict upper triangle, y = 1e6
where sigma = inf, a non-uniform upstream g); timings from tests/test_gpu_traj_fit.phase_values (episode b inside, on or outside the
bounds by b % 3); configurations from tests/test_gpu_traj_fit.phase_configs() plus LIMIT, defined here at the LDS limit the shared route
documents (Pl = 160).
"""
import functools

import numpy as np

from oracle import mp_oracle as O

from . import trajectory_condition_ref as R
from . import trajectory_fit_ref as F
from . import trajectory_log_prob_ref as LP
from .demonstration_condition_ref import information_form as cond_information_form  # noqa: F401
from .demonstration_log_prob_ref import MISSING, SIGMAS, information_form  # noqa: F401
from .trajectory_condition_ref import bound, covariance  # noqa: F401
from .trajectory_log_prob_ref import bounds, floor_cap  # noqa: F401
from .trajectory_std_ref import random_factor, tril64

TABLE = ("tt_prodmp_70_steps", "tt_prodmp_350_steps", "beerpong_promp", "promp_exp_learn_both", "promp_zero_12_basis_3_dof",
         "prodmp_13_basis_1_dof_no_goal", "prodmp_4_basis_12_dof_goal_offset_add", "promp_9_basis_5_dof", "promp_10_basis_11_dof")
LIMIT = "promp_10_basis_16_dof_6_steps"                                           # Pl = 160: one wave on a CU
CONFIGS = TABLE + (LIMIT,)
OVER_LIMIT = ("prodmp_13_basis_16_dof_relative_goal", "promp_16_basis_16_dof")    # Pl = 224, 256: refused
BATCHES = (1, 3, 9)


@functools.lru_cache(maxsize=None)
def cfg(name):
    """(pc, bc, tc, dt, duration) of a learned-phase configuration without per-episode clocks"""
    if name == LIMIT:
        return (O.PhaseCfg("linear", tau=0.6, learn_tau=True, tau_bound=(0.4, 0.6)),
                O.BasisCfg("rbf", num_basis=10, basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=16), 0.1, 0.6)
    if name == "promp_17_dof":
        return (O.PhaseCfg("linear", tau=0.6, learn_tau=True, tau_bound=(0.4, 0.6)),
                O.BasisCfg("rbf", num_basis=2, basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=17), 0.1, 0.6)
    from .test_gpu_traj_fit import phase_configs
    pc, bc, tc, dt, duration, clocks = phase_configs()[name]
    assert clocks is None and (pc.learn_tau or pc.learn_delay), name
    return pc, bc, tc, dt, duration


def engine_for(name):
    from .test_gpu_trajectory import make_engine
    return make_engine(*cfg(name))


def shape(name):
    """(P, Pl, n_phase, D, T)"""
    pc, bc, tc, dt, duration = cfg(name)
    P = O.num_params(pc, bc, tc)
    off = int(bool(pc.learn_tau)) + int(bool(pc.learn_delay))
    return P, P - off, off, tc.action_dim, O.num_steps(duration, dt)


def timings(name, B, seed=1):
    from .test_gpu_traj_fit import phase_values
    return phase_values(cfg(name)[0], B, np.random.default_rng(100 + seed + B))


@functools.lru_cache(maxsize=None)
def _design(name, phase_bytes):
    return F.Design(*cfg(name), 0.0, np.frombuffer(phase_bytes, np.float32))


def design(name, phase_row):
    """the episode's own Design: the oracle at its tau / delay"""
    return _design(name, np.ascontiguousarray(phase_row, np.float32).tobytes())


def rows(name, phase, ip, iv):
    """(H [B, T, D, Pl], c [B, T, D]) float64: row (t, d) of episode b lives in block d of the Pl non-phase parameters"""
    P, Pl, off, D, T = shape(name)
    B = phase.shape[0]
    H, c = np.zeros((B, T, D, Pl)), np.empty((B, T, D))
    for b in range(B):
        ds = design(name, phase[b])
        for d in range(D):
            H[b, :, d, d * ds.Kloc:(d + 1) * ds.Kloc] = ds.Psi[d]
        c[b] = ds.offset(ip[b:b + 1], iv[b:b + 1])[0]
    return H, c


def kept(H, c, pos, sd, b, f32=False):
    """the scalar observations of episode b in trajectory_condition_ref.observations' format: every (step, DoF) with 0 < sigma < inf"""
    out = []
    T, D = pos.shape[1:]
    for t in range(T):
        for d in range(D):
            sigma = float(sd[b, t, d])
            if not (sigma > 0.0) or np.isinf(sigma):
                continue
            h, cc = H[b, t, d], c[b, t, d]
            if f32:
                h, cc = h.astype(np.float32).astype(np.float64), float(np.float32(cc))
            out.append((h, cc, float(pos[b, t, d]), sigma, (0, t, d)))
    return out


def draw(name, B, sigma, missing, seed=1):
    """inputs as demonstration_log_prob_ref.draw draws them, with the timings in front of mu [B, P] and a factor [B, Pl, Pl]"""
    P, Pl, off, D, T = shape(name)
    rng = np.random.default_rng(1000 * seed + 7 * B + T)
    mu = rng.standard_normal((B, P)).astype(np.float32)
    mu[:, :off] = timings(name, B, seed)
    L = random_factor(Pl, B, seed=seed + B, nan_upper=True)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    H, c = rows(name, mu[:, :off], ip, iv)
    w = mu[:, off:].astype(np.float64) + np.einsum("bpq,bq->bp", tril64(L), rng.standard_normal((B, Pl)))
    y = (np.einsum("btdp,bp->btd", H, w) + c + sigma * rng.standard_normal((B, T, D))).astype(np.float32)
    sd = np.full((B, T, D), sigma, np.float32)
    if missing:
        gone = rng.random((B, T, D)) < MISSING
        sd[gone] = np.inf
        y[gone] = 1e6                                                              # a removed entry's value is never used
    g = rng.standard_normal(B) * rng.uniform(0.5, 2.0, B)
    return dict(mu=mu, L=L, ip=ip, iv=iv, H=H, c=c, pos=y, sd=sd, g=g, off=off)


def log_prob_references(cs, pos=None, sd=None, mu=None, L=None):
    """dict(ref_lp [B], ref_gmu [B, P], ref_gL [B, Pl, Pl], n [B], floor_*) of the dense formula; pos / sd / mu / L override the case's"""
    pos, sd = cs["pos"] if pos is None else pos, cs["sd"] if sd is None else sd
    mu, L = cs["mu"] if mu is None else mu, cs["L"] if L is None else L
    off, B = cs["off"], cs["mu"].shape[0]
    L64 = tril64(L)
    out = {k: [] for k in ("ref_lp", "ref_gmu", "ref_gL", "n", "floor_lp", "floor_gmu", "floor_gL")}
    front = np.zeros(off)
    for b in range(B):
        m64 = mu[b, off:].astype(np.float64)
        ob = kept(cs["H"], cs["c"], pos, sd, b)
        lp, gm, gL = LP.autograd(m64, L64[b], ob, cs["g"][b])
        lp_np = LP.log_prob(m64, L64[b], ob)
        assert abs(lp - lp_np) <= 1e-9 * (abs(lp_np) + len(ob)), (lp, lp_np)
        lp32, gm32, gL32 = LP.autograd(m64, L64[b], kept(cs["H"], cs["c"], pos, sd, b, f32=True), cs["g"][b])
        vals = (lp_np, np.concatenate([front, gm]), gL, len(ob), abs(lp32 - lp_np), np.concatenate([front, np.abs(gm32 - gm)]),
                np.abs(gL32 - gL))
        for k, v in zip(out, vals):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


def condition_references(cs, pos=None, sd=None, mu=None, L=None):
    """dict(ref_mu [B, Pl], ref_Sigma [B, Pl, Pl], floor_mu, floor_Sigma) of the dense batch formula over the kept entries"""
    pos, sd = cs["pos"] if pos is None else pos, cs["sd"] if sd is None else sd
    mu, L = cs["mu"] if mu is None else mu, cs["L"] if L is None else L
    off, B = cs["off"], cs["mu"].shape[0]
    L64 = tril64(L)
    ref_mu, ref_S, f_mu, f_S = [], [], [], []
    for b in range(B):
        m64 = mu[b, off:].astype(np.float64)
        a, s = R.batch(m64, L64[b], kept(cs["H"], cs["c"], pos, sd, b))
        a32, s32 = R.batch(m64, L64[b], kept(cs["H"], cs["c"], pos, sd, b, f32=True))
        ref_mu.append(a); ref_S.append(s); f_mu.append(np.abs(a32 - a)); f_S.append(np.abs(s32 - s))
    return dict(ref_mu=np.stack(ref_mu), ref_Sigma=np.stack(ref_S), floor_mu=np.stack(f_mu), floor_Sigma=np.stack(f_S))


def _freeze(cs):
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


@functools.lru_cache(maxsize=None)
def inputs(name, B, sigma, missing, seed=1):
    return _freeze(draw(name, B, sigma, missing, seed))


@functools.lru_cache(maxsize=None)
def log_prob_case(name, B, sigma, missing, seed=1):
    """the inputs and the likelihood's float64 references, computed once and shared (read-only)"""
    cs = dict(inputs(name, B, sigma, missing, seed))
    cs.update(log_prob_references(cs))
    return _freeze(cs)


@functools.lru_cache(maxsize=None)
def condition_case(name, B, sigma, missing, seed=1):
    """the inputs and the posterior's float64 references, computed once and shared (read-only)"""
    cs = dict(inputs(name, B, sigma, missing, seed))
    cs.update(condition_references(cs))
    return _freeze(cs)


def gpu_cases():
    """(name, B, sigma, missing): every configuration at every batch size and every sigma"""
    return [(name, B, sigma, missing) for sigma, missing in SIGMAS for name in CONFIGS for B in BATCHES]


def check_log_prob(got, ref, what):
    """LP.check with the phase columns of g_params held to exact zeros and the strict upper triangle of g_params_L too"""
    LP.check(got, ref, what)
    off = ref["off"]
    if got[1] is not None:
        assert not LP.to_np(got[1])[:, :off].any(), f"{what}: the phase columns of g_params are exact zeros"
    if got[2] is not None:
        gL = LP.to_np(got[2])
        assert not np.triu(gL, 1).any(), f"{what}: the strict upper triangle of g_params_L is exact zeros"


def check_condition(got_mu, got_L, ref, what):
    """R.check on the non-phase part; the factor is lower triangular with a non-negative diagonal and an exact-zero upper triangle; the
    phase columns are the inputs' bits"""
    off = ref["off"]
    g_mu = got_mu.detach().cpu().numpy() if hasattr(got_mu, "detach") else np.asarray(got_mu)
    g_L = got_L.detach().cpu().numpy() if hasattr(got_L, "detach") else np.asarray(got_L)
    assert np.array_equal(g_mu[:, :off].view(np.int32), np.asarray(ref["mu"])[:, :off].view(np.int32)), \
        f"{what}: the phase columns leave as given, unclipped"
    R.check(g_mu[:, off:], g_L, ref, what)
    assert not np.triu(g_L, 1).any(), f"{what}: the strict upper triangle is exact zeros"
    assert (np.diagonal(g_L, axis1=1, axis2=2) >= 0.0).all(), f"{what}: the diagonal is non-negative"
