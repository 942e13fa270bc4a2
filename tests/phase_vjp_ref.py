"""
A torch restatement of the oracle's ``promp_trajectory`` / ``prodmp_trajectory`` (oracle/mp_oracle.py) with a per-episode phase -- learned
tau / delay, clipped to their bounds, and a per-episode ``init_time`` -- so that torch autograd gives the gradient the reference's
formulation (mp_pytorch: ordinary torch graphs) has: clamp's mask on tau / delay, the phase clips, zero-padded bases, disabled blocks, both
relative-goal modes, the goal offset.  Usable in float64 and float32.  ProDMP's table indices are integers: they come from the oracle's
fp32 recipe (``prodmp_indices``) in every dtype and are constants of the graph.  The reference for tests/test_gpu_phase_vjp.py; checked
against the float64 oracle in tests/test_phase_vjp_host.py.
"""
import numpy as np
import torch

from oracle import mp_oracle as O

NP = {torch.float64: np.float64, torch.float32: np.float32}


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, NP[dtype])))


def clipped_phase(pc, params, dtype):
    """(tau, delay, local start): learned values clamped as ``get_trajectory(clip=True)`` (bounds held in fp32), else the config's"""
    f = NP[dtype]
    tau = torch.tensor(O._q(pc.tau, f), dtype=dtype)
    delay = torch.tensor(O._q(pc.delay, f), dtype=dtype)
    i = 0
    if pc.learn_tau:
        lo, hi = (float(np.float32(b)) for b in pc.tau_bound)
        tau = torch.clamp(params[:, i], lo, hi); i += 1
    if pc.learn_delay:
        lo, hi = (float(np.float32(b)) for b in pc.delay_bound)
        delay = torch.clamp(params[:, i], lo, hi); i += 1
    return tau, delay, i


def scaled_times(pc, params, init_time, dt, duration, dtype):
    """s = (t - delay) / tau [B, T] (unclipped), detached: what the tests inspect for steps on a phase clip"""
    with torch.no_grad():
        tau, delay, _ = clipped_phase(pc, params.detach().to(dtype), dtype)
        times = _t(O.make_times(duration, dt, init_time, dtype=NP[dtype]), dtype)
        B = params.shape[0]
        tt = times.expand(B, -1) if times.dim() == 1 else times
        return (tt - delay.reshape(-1, 1)) / tau.reshape(-1, 1)


def trajectory(pc, bc, tc, params, init_pos, init_vel, init_time, dt, duration, dtype=torch.float64, tables=None):
    """params [B, P], init_pos / init_vel [B, D] torch tensors of ``dtype`` (any may require grad); init_time a float or an array [B]
    (no gradient) -> pos, vel [B, T, D]"""
    f = NP[dtype]
    B, D = params.shape[0], tc.action_dim
    tau, delay, i0 = clipped_phase(pc, params, dtype)
    tau_b = tau.expand(B) if tau.dim() == 0 else tau
    delay_b = delay.expand(B) if delay.dim() == 0 else delay
    local = params[:, i0:].reshape(B, D, -1)
    times = _t(O.make_times(duration, dt, init_time, dtype=f), dtype)
    tt = times.expand(B, -1) if times.dim() == 1 else times                             # [B, T]
    kind = tc.trajectory_generator_type
    if kind == "promp":
        s = (tt - delay_b[:, None]) / tau_b[:, None]
        if pc.phase_generator_type == "linear":
            x = torch.clamp(s, 0.0, 1.0)
        else:
            x = torch.exp(-float(O._q(pc.alpha_phase, f)) * torch.clamp(s, min=0.0))
        cen, bw = (_t(a, dtype) for a in O.rbf_centers_bandwidth(pc, bc, f))
        b = torch.exp(-((x[..., None] - cen) ** 2 * bw) / 2.0)
        if cen.shape[0] > 1:
            b = b / b.sum(dim=-1, keepdim=True)
        if bc.basis_generator_type == "zero_rbf":
            zs = bc.num_basis_zero_start
            b = b[..., zs: zs + bc.num_basis]
        phi = b * float(O._q(tc.weights_scale, f))
        pos = torch.einsum("btk,bdk->btd", phi, local)
        if bc.basis_generator_type == "zero_rbf":
            pos = pos + init_pos[:, None, :]
        v = (pos[:, 1:] - pos[:, :-1]) / (tt[:, 1:] - tt[:, :-1])[..., None]
        return pos, torch.cat((v, v[:, -1:]), dim=1)
    if kind != "prodmp":
        raise NotImplementedError(kind)
    tab = tables if tables is not None else O.prodmp_tables(pc, bc, f)
    nb = bc.num_basis
    c = 0
    cols = []
    if not tc.disable_weights:
        cols.append(local[..., :nb]); c = nb
    else:
        cols.append(torch.zeros((B, D, nb), dtype=dtype))
    cols.append(local[..., c:c + 1] if not tc.disable_goal else torch.zeros((B, D, 1), dtype=dtype))
    full = torch.cat(cols, dim=-1)
    goal = full[..., -1]
    if tc.relative_goal and tc.relative_goal_mode == "before_scale":
        goal = goal + init_pos
    scale = _t(O.prodmp_weights_goal_scale(tc, bc, tab, f), dtype)
    w = full[..., :nb] * scale[:nb]
    goal = goal * scale[nb]
    if tc.relative_goal and tc.relative_goal_mode == "after_scale":
        goal = goal + init_pos
    if tc.goal_offset_mode == "add":
        goal = goal + float(O._q(tc.goal_offset, f))
    wg = torch.cat((w, goal[..., None]), dim=-1)                                        # [B, D, nb + 1]
    v_b = init_vel * tau_b[:, None]
    # the integer part of the path: the oracle's fp32 recipe on the fp32-held clipped tau / delay
    g = np.float32
    tau32 = tau_b.detach().numpy().astype(g)
    delay32 = delay_b.detach().numpy().astype(g)
    tt32 = tt.detach().numpy().astype(g)
    idx = O.prodmp_indices(tt32, tau32, delay32, tab.scaled_dt, bc.pre_compute_length_factor, g)
    it = np.broadcast_to(np.asarray(init_time, f), (B,)).astype(g)
    idx_b = O.prodmp_indices(it[:, None], tau32, delay32, tab.scaled_dt, bc.pre_compute_length_factor, g)[:, 0]
    idx, idx_b = torch.from_numpy(idx), torch.from_numpy(idx_b)
    T1, T2, D1, D2 = (_t(a, dtype) for a in (tab.y1, tab.y2, tab.dy1, tab.dy2))
    PB, VB = _t(tab.pos_basis, dtype), _t(tab.vel_basis, dtype)
    y1, y2, dy1, dy2 = T1[idx], T2[idx], D1[idx], D2[idx]
    y1b, y2b, dy1b, dy2b = T1[idx_b], T2[idx_b], D1[idx_b], D2[idx_b]
    det = y1b * dy2b - y2b * dy1b
    a, b_, c_, d_ = (dy2b / det)[:, None], (dy1b / det)[:, None], (y1b / det)[:, None], (y2b / det)[:, None]
    xi1, xi2 = a * y1 - b_ * y2, c_ * y2 - d_ * y1
    xi3, xi4 = a * dy1 - b_ * dy2, c_ * dy2 - d_ * dy1
    psi_b, dpsi_b = PB[idx_b], VB[idx_b]
    H = PB[idx] - (xi1[..., None] * psi_b[:, None, :] + xi2[..., None] * dpsi_b[:, None, :])
    Hv = VB[idx] - (xi3[..., None] * psi_b[:, None, :] + xi4[..., None] * dpsi_b[:, None, :])
    pos = xi1[..., None] * init_pos[:, None, :] + xi2[..., None] * v_b[:, None, :] + torch.einsum("btk,bdk->btd", H, wg)
    vel = xi3[..., None] * init_pos[:, None, :] + xi4[..., None] * v_b[:, None, :] + torch.einsum("btk,bdk->btd", Hv, wg)
    return pos, vel / tau_b[:, None, None]


def vjp(pc, bc, tc, params, init_pos, init_vel, init_time, dt, duration, g_pos, g_vel, dtype=torch.float64, tables=None):
    """numpy in -> (g_params, g_init_pos, g_init_vel) numpy float64 arrays by autograd of ``trajectory`` in ``dtype``; g_pos / g_vel None: skipped"""
    p, ip, iv = (_t(a, dtype).requires_grad_(True) for a in (params, init_pos, init_vel))
    pos, vel = trajectory(pc, bc, tc, p, ip, iv, init_time, dt, duration, dtype, tables)
    loss = torch.zeros((), dtype=dtype)
    if g_pos is not None:
        loss = loss + (pos * _t(g_pos, dtype)).sum()
    if g_vel is not None:
        loss = loss + (vel * _t(g_vel, dtype)).sum()
    grads = torch.autograd.grad(loss, (p, ip, iv), allow_unused=True)
    return tuple((torch.zeros_like(x) if g is None else g).numpy().astype(np.float64) for g, x in zip(grads, (p, ip, iv)))


# ---- configurations beside tests/test_gpu_learned_phase.py's -------------------------------------------------------------------------
EXTRA = {
    # an exp-phase ProMP that learns both tau and delay
    "promp_exp_learn_both": (O.PhaseCfg("exp", tau=1.2, alpha_phase=2.5, learn_tau=True, learn_delay=True, tau_bound=(0.6, 1.4),
                                        delay_bound=(0.0, 0.2)),
                             O.BasisCfg("rbf", num_basis=5, basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=4, weights_scale=0.8),
                             0.02, 1.0),
    # ProDMP: init_pos joins the SCALED goal, the weights are disabled, tau is learned
    "prodmp_after_scale_no_weights": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0, learn_tau=True, tau_bound=(0.6, 1.1)),
                                      O.BasisCfg("prodmp", num_basis=3, alpha=15, basis_bandwidth_factor=2),
                                      O.TrajCfg("prodmp", action_dim=3, goal_scale=1.5, relative_goal=True, disable_weights=True,
                                                relative_goal_mode="after_scale"), 0.02, 0.9),
}


def grid_config(kind, D, T):
    """ProMP (linear phase, zero-padded basis) / ProDMP (relative goal before the scale) learning tau and delay at D DoF and T steps"""
    dt = 0.01
    if kind == "promp":
        return (O.PhaseCfg("linear", tau=1.0, learn_tau=True, learn_delay=True, tau_bound=(0.4, 1.0), delay_bound=(0.0, 0.008)),
                O.BasisCfg("zero_rbf", num_basis=3, num_basis_zero_start=1, num_basis_zero_goal=1, basis_bandwidth_factor=3),
                O.TrajCfg("promp", action_dim=D, weights_scale=0.9), dt, T * dt)
    return (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.4, 1.0), delay_bound=(0.0, 0.008)),
            O.BasisCfg("prodmp", num_basis=3, alpha=20, basis_bandwidth_factor=3),
            O.TrajCfg("prodmp", action_dim=D, weights_scale=0.6, goal_scale=1.2, auto_scale_basis=True, relative_goal=True), dt, T * dt)


def make_inputs(pc, bc, tc, dt, duration, B, init_time=0.0, seed=0):
    """(params, init_pos, init_vel, seed used): tau / delay at least 5 % of the bound's width inside the bounds except row 0 (above tau_hi)
    and row 1 (below tau_lo); the seed is advanced until no step sits within 1e-4 of a phase clip (linear: s = 0 or 1, exp: s = 0)"""
    P = O.num_params(pc, bc, tc)
    seed0 = seed
    while True:
        rng = np.random.default_rng(seed)
        params = rng.standard_normal((B, P)).astype(np.float32)
        i = 0
        if pc.learn_tau:
            lo, hi = pc.tau_bound
            w = hi - lo
            params[:, i] = rng.uniform(lo + 0.05 * w, hi - 0.05 * w, B)
            params[0, i] = hi + 0.07 * w
            if B > 1:
                params[1, i] = lo - 0.07 * w
            i += 1
        if pc.learn_delay:
            lo, hi = pc.delay_bound
            w = hi - lo
            params[:, i] = rng.uniform(lo + 0.05 * w, hi - 0.05 * w, B)
            i += 1
        ip = rng.uniform(-1, 1, (B, tc.action_dim)).astype(np.float32)
        iv = rng.uniform(-1, 1, (B, tc.action_dim)).astype(np.float32)
        ok = True
        if tc.trajectory_generator_type == "promp":
            ok = phase_clip_margin(pc, params, init_time, dt, duration) >= 1e-4
        if ok:
            return params, ip, iv, seed
        seed += 1
        assert seed < seed0 + 100, "no seed keeps every step off the phase clips"


def phase_clip_margin(pc, params, init_time, dt, duration):
    """the smallest distance of a step's scaled time s from a clip of the phase (linear: 0 and 1, exp: 0) over the rows whose phase
    derivative reaches an output.  A row whose tau was clipped on a handle that learns no delay is left out: its d x / d s is multiplied
    by the clamp's 0 and goes nowhere -- and it cannot be kept off the clip where tau_hi is the duration (BeerPong: row 0 is above
    tau_hi by construction, so its last step sits at s = 1 exactly)."""
    s = scaled_times(pc, torch.from_numpy(np.asarray(params, np.float32)), init_time, dt, duration, torch.float64).numpy()
    if pc.learn_tau and not pc.learn_delay:
        lo, hi = (np.float32(b) for b in pc.tau_bound)
        s = s[(params[:, 0] >= lo) & (params[:, 0] <= hi)]
    if s.size == 0:
        return np.inf
    edge = np.abs(s).min()
    if pc.phase_generator_type == "linear":
        edge = min(edge, np.abs(s - 1.0).min())
    return edge
