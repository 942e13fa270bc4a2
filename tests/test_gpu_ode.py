"""
GPU suite: the HIP path against an INDEPENDENT statement of what a movement primitive is -- SciPy's solution of the
DMP / ProDMP differential equation (tests/ode_ref.py) -- instead of against the oracle's recollection of mp_pytorch.
Covers BASELINE cfg2, cfg4 (all four replanning boundary conditions, auto_scale_basis, disable_goal), the reference's
TableTennis ProDMP configuration with learned tau / delay (auto_scale_basis, relative_goal, disable_goal), and cfg3
(explicit Euler: first-order convergence to the ODE in dt); further ProDMP cases at the same bounds (an init_time of each
episode's own with learned tau / delay, init_vel and an enabled scaled relative goal in both relative_goal_mode settings;
disable_weights with a goal scale; goal_offset_mode = add; cfg2 with an init_time array); and every DMP route -- response
rows, serial Euler, the four per-episode kernels, linear phase, first sample 'step' -- against the ODE by Richardson
extrapolation, positions and velocities, at bounds of a few 1e-4 of the scale (the table in front of DMP_MEASURED below).

Tolerances are derived from the ProDMP table step h = basis_dt / tau0 (scaled time):
  * against the ODE evaluated AT the table's grid points (s = idx * h, boundary at idx_b * h) the only error is the
    cumulative-trapezoid quadrature of the pre-computed integrals, O(h^2): measured 3e-6 .. 2e-5 of the trajectory scale for
    the configurations here; bound used: 40 * h^2 * scale (h = 1/150: 1.8e-3 ... the constant covers alpha = 25);
  * against the ODE at the EXACT sample times the table lookup adds |dy/ds| * h / 2 (index rounding, half a grid step).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import ode_ref as R
from tests.test_gpu_trajectory import CFG2, CFG3, CFG4, make_engine
from oracle import mp_oracle as O

pytestmark = pytest.mark.gpu


def _prodmp_case(pc, bc, tc, dt, duration, params, ip, iv, init_time, tau=None, delay=None, factory=None):
    """returns (pos, vel) from the GPU and the ODE solution at the table grid points, plus the table step"""
    eng = (factory or make_engine)(pc, bc, tc, dt, duration)
    B, D = ip.shape
    it_arg = init_time
    if isinstance(init_time, np.ndarray):
        it_arg = torch.tensor(init_time.astype(np.float32), device=eng.device)
    pos, vel = eng.trajectory(params, ip, iv, it_arg)
    if pc.learn_tau or pc.learn_delay:
        eng.check_range()                   # synchronises
    pos, vel = pos.cpu().numpy().astype(np.float64), vel.cpu().numpy().astype(np.float64)
    tabs = eng.prodmp_tables()
    cen, bw = R.rbf_constants(eng)
    nb = bc.num_basis
    scale = np.ones(nb + 1)
    if tc.auto_scale_basis:
        scale = tabs["scale"].astype(np.float32).astype(np.float64)
    scale[:nb] *= np.float32(tc.weights_scale); scale[nb] *= np.float32(tc.goal_scale)
    h = float(np.float32(bc.dt) / np.float32(pc.tau))
    off = int(pc.learn_tau) + int(pc.learn_delay)
    local = params[:, off:].reshape(B, D, -1).astype(np.float64)
    w = np.zeros((B, D, nb)); g = np.zeros((B, D))
    c = 0
    if not tc.disable_weights:
        w = local[..., :nb] * scale[:nb]; c = nb
    if not tc.disable_goal:
        g = local[..., c] * scale[nb]
    if tc.relative_goal:                       # default mode: init_pos joins the RAW goal parameter, the scale applies to both
        g = g + ip.astype(np.float64) * (scale[nb] if tc.relative_goal_mode == "before_scale" else 1.0)
    if tc.goal_offset_mode == "add":           # the offset joins the goal itself, behind the scale
        g = g + float(np.float32(tc.goal_offset))
    # a learned tau / delay: what the episode uses is the parameter clipped to its bound (black_box_wrapper.py:104-105)
    if tau is None and pc.learn_tau:
        tau = np.clip(params[:, 0], np.float32(pc.tau_bound[0]), np.float32(pc.tau_bound[1]))
    if delay is None and pc.learn_delay:
        delay = np.clip(params[:, int(pc.learn_tau)], np.float32(pc.delay_bound[0]), np.float32(pc.delay_bound[1]))
    base = eng.times()
    out_y, out_v = np.empty_like(pos), np.empty_like(vel)
    slope = np.zeros(B)
    for b in range(B):
        tau_b = np.float32(pc.tau if tau is None else tau[b])
        delay_b = np.float32(pc.delay if delay is None else delay[b])
        it_b = np.float32(init_time[b] if isinstance(init_time, np.ndarray) else init_time)
        idx = R.table_indices(base + it_b, tau_b, delay_b, np.float32(h))
        idx_b = R.table_indices(np.array([it_b], np.float32), tau_b, delay_b, np.float32(h))[0]
        y, ys = R.solve(float(np.float32(bc.alpha)), float(np.float32(pc.alpha_phase)), cen, bw, w[b], g[b],
                        idx_b * h, ip[b].astype(np.float64), iv[b].astype(np.float64) * float(tau_b), idx * h)
        out_y[b] = y.T
        out_v[b] = ys.T / float(tau_b)
        slope[b] = np.abs(ys).max()
    return pos, vel, out_y, out_v, h, slope


def _check(pos, vel, y, v, h, alpha):
    sp = max(np.abs(y).max(), 1e-3)
    sv = max(np.abs(v).max(), 1e-3)
    # O(h^2) trapezoid residual of the pre-computed integrals (+ the fp32 contract of the kernels, 1e-5)
    tol_p = (40.0 * h * h + 1e-5) * sp
    tol_v = (40.0 * h * h * alpha / 4 + 1e-5) * sv       # the velocity rows carry an extra factor ~alpha/2 of curvature
    ep, ev = np.abs(pos - y).max(), np.abs(vel - v).max()
    assert ep <= tol_p, f"pos: {ep:.3e} > {tol_p:.3e} (scale {sp:.3e})"
    assert ev <= tol_v, f"vel: {ev:.3e} > {tol_v:.3e} (scale {sv:.3e})"
    return ep / sp, ev / sv


def _inputs(P, D, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, P)).astype(np.float32), rng.uniform(-1, 1, (B, D)).astype(np.float32),
            rng.uniform(-1, 1, (B, D)).astype(np.float32))


def check_cfg2(init_time, factory=None):
    pc, bc, tc, dt, dur = CFG2
    params, ip, iv = _inputs(42, 7, 6, 11)
    pos, vel, y, v, h, _ = _prodmp_case(pc, bc, tc, dt, dur, params, ip, iv, init_time, factory=factory)
    _check(pos, vel, y, v, h, bc.alpha)


@pytest.mark.parametrize("mapping", ["1", "2"])
@pytest.mark.parametrize("init_time", [0.0, 0.5])
def test_cfg2_prodmp_solves_the_ode(init_time, mapping, mpk_option):
    mpk_option("mapping", mapping)
    check_cfg2(init_time)


def test_cfg4_all_four_replanning_boundary_conditions_solve_the_ode():
    check_cfg4()


def check_cfg4(factory=None):
    """
    BoxPushingDenseReplan (box_pushing/mp_wrapper.py:68-92): weights_scale = goal_scale = 0.3, auto_scale_basis,
    disable_goal, plans at t = 0, 25, 50, 75 steps, each conditioned on the DESIRED state where the previous plan broke
    (condition_on_desired, black_box_wrapper.py:199-201).  Every plan must solve the ODE from its own boundary state;
    with unchanged parameters consecutive plans continue ONE solution, so plan k must also reproduce plan 0's tail.
    """
    pc, bc, tc, dt, dur = CFG4
    B, D = 5, 7
    rng = np.random.default_rng(4)
    prm_same = rng.standard_normal((B, 35)).astype(np.float32)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    first = None
    for same in (True, False):
        cp, cv = ip, iv
        for k in range(4):
            prm = prm_same if same else rng.standard_normal((B, 35)).astype(np.float32)
            init_time = float(np.float32(25 * k * dt))
            pos, vel, y, v, h, _ = _prodmp_case(pc, bc, tc, dt, dur, prm, cp, cv, init_time, factory=factory)
            _check(pos, vel, y, v, h, bc.alpha)
            if same:
                if k == 0:
                    first = (pos, vel)
                else:
                    # plan k from the desired state at step 25k - 1 of plan k-1 == the tail of plan 0.  The boundary
                    # state is an fp32 sample of plan k-1, so the continuation is exact up to that rounding carried
                    # through the (stable) dynamics
                    n = 100 - 25 * k
                    sp, sv = np.abs(first[0]).max(), np.abs(first[1]).max()
                    assert np.abs(pos[:, :n] - first[0][:, 25 * k:]).max() <= 2e-5 * sp
                    assert np.abs(vel[:, :n] - first[1][:, 25 * k:]).max() <= 2e-5 * sv * bc.alpha
            # condition_on_desired: the next plan starts from the desired state at the last executed step
            cp, cv = pos[:, 24].astype(np.float32), vel[:, 24].astype(np.float32)


@pytest.mark.parametrize("phase_opt", ["1", "0"])
def test_tabletennis_prodmp_with_learned_tau_and_delay_solves_the_ode(phase_opt, mpk_option):
    mpk_option("phase", phase_opt)
    check_tabletennis_prodmp()


def check_tabletennis_prodmp(factory=None):
    """
    table_tennis/mp_wrapper.py:33-55: learn_tau, learn_delay, tau_bound [0.8, 1.5], delay_bound [0.05, 0.15],
    alpha_phase 3, 3 basis functions, alpha 25, weights_scale 0.7, auto_scale_basis, relative_goal, disable_goal;
    dt = 0.008, 350 steps.  Per-episode phase -> the per-episode kernels (wave-per-episode and workgroup-per-episode).
    """
    pc = O.PhaseCfg("exp", tau=2.8, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.8, 1.5),
                    delay_bound=(0.05, 0.15))
    bc = O.BasisCfg("prodmp", num_basis=3, basis_bandwidth_factor=3, alpha=25)
    tc = O.TrajCfg("prodmp", action_dim=7, weights_scale=0.7, auto_scale_basis=True, relative_goal=True,
                   disable_goal=True)
    B, D = 6, 7
    rng = np.random.default_rng(8)
    params = rng.standard_normal((B, 2 + 21)).astype(np.float32)
    params[:, 0] = rng.uniform(0.8, 1.5, B)
    params[:, 1] = rng.uniform(0.05, 0.15, B)
    params[0, 0], params[1, 0] = 0.3, 9.0            # outside the bounds: clipped to 0.8 / 1.5 (black_box_wrapper.py:104-105)
    tau = np.clip(params[:, 0], 0.8, 1.5)
    delay = np.clip(params[:, 1], 0.05, 0.15)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = np.zeros((B, D), np.float32)
    pos, vel, y, v, h, slope = _prodmp_case(pc, bc, tc, 0.008, 2.8, params, ip, iv, 0.0, tau=tau, delay=delay,
                                            factory=factory)
    _check(pos, vel, y, v, h, bc.alpha)
    # against the ODE at the EXACT sample times: + half a table step of slope (index rounding)
    eng = (factory or make_engine)(pc, bc, tc, 0.008, 2.8)
    base = eng.times().astype(np.float64)
    cen, bw = R.rbf_constants(eng)
    tabs = eng.prodmp_tables()
    sc = tabs["scale"].astype(np.float32).astype(np.float64)
    for b in (2, 3):
        w = params[b, 2:].reshape(D, 3).astype(np.float64) * sc[:3] * np.float32(0.7)
        g = ip[b].astype(np.float64)                                  # disabled goal + relative goal: goal = init_pos
        s = np.maximum((base - delay[b]) / tau[b], 0.0)
        ye, _ = R.solve(25.0, 3.0, cen, bw, w, g, 0.0, ip[b].astype(np.float64), np.zeros(D), s)
        bound = slope[b] * h / 2 + (40 * h * h + 1e-5) * np.abs(ye).max()
        assert np.abs(pos[b] - ye.T).max() <= bound


# ---- ProDMP: the cases the checks above leave out, at the same bounds ---------------------------------------------------------------
TT_DT, TT_DUR = 0.008, 2.8


def check_tabletennis_prodmp_own_init_time(relative_goal_mode, factory=None):
    """
    The TableTennis shape with everything the case above switches off: an init_time of each episode's own (a multiple of dt, up
    to 59 dt -- some episodes start before their delay has passed, some after), non-zero init_vel, the goal ENABLED with
    goal_scale 0.4 under relative_goal (x auto_scale_basis).  Each relative_goal_mode is compared with the ODE its own
    definition states; the two goals differ by (1 - s_g) init_pos, so a handle that ignored the switch fails.
    """
    pc = O.PhaseCfg("exp", tau=2.8, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.8, 1.5),
                    delay_bound=(0.05, 0.15))               # (as check_tabletennis_prodmp: table step h = 0.01 / 2.8)
    bc = O.BasisCfg("prodmp", num_basis=3, basis_bandwidth_factor=3, alpha=25)
    tc = O.TrajCfg("prodmp", action_dim=7, weights_scale=0.7, goal_scale=0.4, auto_scale_basis=True, relative_goal=True,
                   relative_goal_mode=relative_goal_mode)
    B, D = 6, 7
    rng = np.random.default_rng(18)
    params = rng.standard_normal((B, 2 + 28)).astype(np.float32)
    params[:, 0] = rng.uniform(0.8, 1.5, B)
    params[:, 1] = rng.uniform(0.05, 0.15, B)
    params[0, 0], params[1, 0], params[2, 1] = 0.3, 9.0, 0.5       # outside the bounds: clipped
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    init_time = (np.array([0, 59, 7, 13, 30, 2]) * np.float32(TT_DT)).astype(np.float32)
    pos, vel, y, v, h, _ = _prodmp_case(pc, bc, tc, TT_DT, TT_DUR, params, ip, iv, init_time, factory=factory)
    return _check(pos, vel, y, v, h, bc.alpha)


@pytest.mark.parametrize("phase_opt", ["1", "0"])
@pytest.mark.parametrize("relative_goal_mode", ["before_scale", "after_scale"])
def test_tabletennis_prodmp_with_own_init_time_and_a_scaled_relative_goal_solves_the_ode(relative_goal_mode, phase_opt, mpk_option):
    mpk_option("phase", phase_opt)
    check_tabletennis_prodmp_own_init_time(relative_goal_mode)


def check_prodmp_flags(which, factory=None):
    """cfg2's shape with one more flag each: 'disable_weights' (the goal alone, goal_scale 0.5, shared init_time 0.5),
    'goal_offset' (goal_offset_mode = add, goal_offset 1.0), 'own_init_time' (cfg2 itself, fixed phase, with an init_time array:
    the per-episode kernels reached through init_time alone)"""
    pc, bc, tc, dt, dur = CFG2
    B, D = 6, 7
    init_time = 0.5
    if which == "disable_weights":
        tc = dataclasses.replace(tc, disable_weights=True, goal_scale=0.5)
    elif which == "goal_offset":
        tc = dataclasses.replace(tc, goal_offset_mode="add", goal_offset=1.0)
    else:
        assert which == "own_init_time"
        init_time = (np.array([0, 25, 3, 50, 11, 74]) * np.float32(dt)).astype(np.float32)
    params, ip, iv = _inputs(O.num_params(pc, bc, tc), D, B, 21)
    pos, vel, y, v, h, _ = _prodmp_case(pc, bc, tc, dt, dur, params, ip, iv, init_time, factory=factory)
    return _check(pos, vel, y, v, h, bc.alpha)


@pytest.mark.parametrize("which", ["disable_weights", "goal_offset", "own_init_time"])
def test_cfg2_prodmp_flags_solve_the_ode(which):
    check_prodmp_flags(which)


def test_cfg3_dmp_euler_on_the_gpu_converges_to_the_ode_first_order():
    check_cfg3_dmp()


def check_cfg3_dmp(factory=None):
    """explicit Euler: the trajectory approaches the ODE solution linearly in dt"""
    pc, bc, tc, _, dur = CFG3
    B, D = 4, 7
    rng = np.random.default_rng(6)
    params = (rng.standard_normal((B, 42)) * 20.0).astype(np.float32)
    params[:, 5::6] = rng.standard_normal((B, 7))          # goals O(1)
    ip = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    iv = np.zeros((B, D), np.float32)
    errs = []
    for dt in (0.02, 0.01, 0.005):
        eng = (factory or make_engine)(pc, bc, tc, dt, dur)
        pos, vel = eng.trajectory(params, ip, iv, 0.0)
        pos = pos.cpu().numpy().astype(np.float64)
        cen, bw = R.rbf_constants(eng)
        t = eng.times().astype(np.float64)
        s = t / 4.0
        local = params.reshape(B, D, 6).astype(np.float64)
        e = 0.0
        for b in range(B):
            # the first sample carries the initial condition (MPK_DMP_FIRST_IS_INIT): the boundary is at s[0]
            y, _ = R.solve(25.0, 2.0, cen, bw, local[b, :, :5], local[b, :, 5], s[0], ip[b].astype(np.float64),
                           np.zeros(D), s)
            e = max(e, np.abs(pos[b] - y.T).max())
        errs.append(e)
    assert errs[1] < 0.6 * errs[0] and errs[2] < 0.6 * errs[1], errs
    assert errs[2] < 0.05 * np.abs(pos).max(), errs


# ---- DMP against the ODE, tightly: Richardson extrapolation of the explicit Euler recurrence ---------------------------------------
# The recurrence is first order in dt, so 2 y(dt/2) - y(dt) at the common sample times removes the leading error term and what
# is left falls by 4 per halving of dt (second order) whenever the delay's onset lies on the coarse time grid.  That turns the
# 5 % of check_cfg3_dmp into a few 1e-4 of the trajectory scale WITHOUT a reference for the recurrence itself: positions and
# velocities, vel = z / tau, z_0 = tau * init_vel, both scales, the delay's hold, the tau / delay clips, each episode's own
# init_time, both first-sample modes and the linear phase with its clip at 1 all enter the ODE's statement
# (tests/ode_ref.py) and nothing of oracle/mp_oracle.py does.
#
# Shape: cfg3's (7 DoF, five basis functions, alpha 25, duration 4) with weights_scale 0.8, goal_scale 1.2, weights of magnitude
# 20, init_vel uniform in [-1, 1].  The kernels get DMP_B episodes (37: the batch at which the pipeline kernel is reached with a
# ragged last block); the ODE is solved for the first DMP_N of them.
#
# Bounds.  For each case the residual of the FLOAT64 ORACLE's extrapolation against SciPy was measured on the CPU (columns
# "oracle"; tests/test_oracle_pins.py asserts that the oracle still gives these figures); the bound is twice that plus 3e-5 of
# the scale -- the extrapolation triples the 1e-5 fp32 contract of the kernels, and the kernels differ from the float64 oracle
# by that contract only, one to two orders below the residual.  All figures are fractions of the scale (max |y|, max |y'| of the
# ODE solution), pos / vel; "plain" is the unextrapolated recurrence at the coarse dt; "GPU" the largest residual any route
# of the case showed on an MI355X (profiles/dmp_ode_extrapolation.md has the per-route figures).
#
#   case          what it is                                                  dt    plain            oracle           bound            GPU
#   shared        shared exp phase, init_time 0                               0.02  1.9e-2 / 2.8e-2  2.09e-4/1.11e-3  4.5e-4 / 2.2e-3  2.09e-4/1.11e-3
#                                                                             0.01                   5.00e-5/2.60e-4  1.3e-4 / 5.5e-4  5.01e-5/2.60e-4
#   learned       learned tau in [2, 6] (two raw values clipped), delay a     0.02  3.1e-2 / 6.4e-2  7.81e-4/5.15e-3  1.6e-3 / 1.0e-2  7.81e-4/5.15e-3
#                 multiple of 0.02 (one 0), own init_time per episode         0.01                   1.79e-4/1.15e-3  3.9e-4 / 2.3e-3  1.79e-4/1.15e-3
#   offgrid       the same with delays uniform in [0, 0.4] (the ordinary      0.02  2.8e-2 / 6.6e-2  5.65e-4/4.78e-3  1.2e-3 / 9.6e-3  5.65e-4/4.78e-3
#                 case: the onset kink is first order, no order assertion)
#   linear        linear phase, learned tau in [2, 3.6] < duration (every     0.02  3.3e-2 / 5.7e-2  7.20e-4/4.06e-3  1.5e-3 / 8.2e-3  7.20e-4/4.06e-3
#                 episode crosses the clip at s = 1; tau a multiple of 0.02)  0.01                   1.66e-4/9.03e-4  3.6e-4 / 1.8e-3  1.66e-4/9.03e-4
#   step_shared   first sample 'step' (k_dmp_prestep), shared phase,          0.02  2.3e-2 / 2.9e-2  2.75e-4/1.13e-3  5.8e-4 / 2.3e-3  2.75e-4/1.13e-3
#                 init_time 0.06: the boundary is AT init_time                0.01                   6.59e-5/2.66e-4  1.6e-4 / 5.6e-4  6.59e-5/2.66e-4
#   step_learned  first sample 'step' on the 'learned' configuration          0.02  3.2e-2 / 7.5e-2  7.46e-4/6.08e-3  1.5e-3 / 1.2e-2  7.46e-4/6.08e-3
#                                                                             0.01                   1.71e-4/1.36e-3  3.7e-4 / 2.7e-3  1.71e-4/1.36e-3
#
DMP_MEASURED = {
    # case: {coarse dt of the pair: (oracle pos, oracle vel)}
    "shared": {0.02: (2.088e-4, 1.107e-3), 0.01: (5.004e-5, 2.596e-4)},
    "learned": {0.02: (7.806e-4, 5.153e-3), 0.01: (1.794e-4, 1.149e-3)},
    "offgrid": {0.02: (5.648e-4, 4.782e-3)},
    "linear": {0.02: (7.195e-4, 4.064e-3), 0.01: (1.661e-4, 9.031e-4)},
    "step_shared": {0.02: (2.748e-4, 1.132e-3), 0.01: (6.590e-5, 2.655e-4)},
    "step_learned": {0.02: (7.459e-4, 6.083e-3), 0.01: (1.713e-4, 1.355e-3)},
}
DMP_B, DMP_N, DMP_DUR = 37, 8, 4.0


def _dmp_bound(name, dt):
    op, ov = DMP_MEASURED[name][dt]
    return 2.0 * op + 3e-5, 2.0 * ov + 3e-5


@functools.lru_cache(maxsize=None)
def _dmp_case(name):
    """(pc, bc, tc, coarse dt, levels, on_grid, params, init_pos, init_vel, init_time): init_time a float (shared) or [B]"""
    phase = "linear" if name == "linear" else "exp"
    first = "step" if name.startswith("step") else "init"
    learned = name in ("learned", "offgrid", "step_learned")
    dt = 0.02
    pc = O.PhaseCfg(phase, tau=4.0, alpha_phase=2.0)
    if learned:
        pc = dataclasses.replace(pc, learn_tau=True, learn_delay=True, tau_bound=(2.0, 6.0), delay_bound=(0.0, 0.4))
    if name == "linear":
        pc = dataclasses.replace(pc, learn_tau=True, tau_bound=(2.0, 3.6))      # every tau below the duration: all cross s = 1
    bc = O.BasisCfg("rbf", num_basis=5, basis_bandwidth_factor=3)
    tc = O.TrajCfg("dmp", action_dim=7, alpha=25.0, weights_scale=0.8, goal_scale=1.2, dmp_first_sample=first)
    B = DMP_N if name in ("shared", "step_shared") else DMP_B
    rng = np.random.default_rng(sum(map(ord, name)))
    local = rng.standard_normal((B, 7, 6)) * 20.0
    local[..., 5] = rng.standard_normal((B, 7))                          # goals O(1)
    head = []
    init_time = 0.0
    if learned:
        tau = rng.uniform(2.0, 6.0, B)
        tau[0], tau[1] = 1.0, 9.0                                         # outside the bound: clipped to 2 / 6
        delay = rng.integers(0, 21, B) * dt if name != "offgrid" else rng.uniform(0.0, 0.4, B)
        delay[2] = 0.0
        head = [tau, delay]
        init_time = rng.integers(0, 30, B) * dt
        init_time[[0, 3, 4, 6]] = 0.0                                     # these start before their delay has passed: a hold
        init_time = init_time.astype(np.float32)
    elif name == "linear":
        # multiples of the coarse dt, so that the clip's kink at t = tau lies on every grid (as the delay's onset does)
        head = [rng.integers(100, 181, B) * dt]
    elif name == "step_shared":
        init_time = 0.06
    params = np.concatenate([h[:, None] for h in head] + [local.reshape(B, 42)], axis=1).astype(np.float32)
    ip = rng.uniform(-1, 1, (B, 7)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, 7)).astype(np.float32)
    for a in (params, ip, iv):
        a.setflags(write=False)
    levels = 2 if name == "offgrid" else 3
    return pc, bc, tc, dt, levels, name != "offgrid", params, ip, iv, init_time


def _dmp_times(eng, init_time, n):
    """[n, T] float64: the library's time grid, base + init_time in float32"""
    it = np.asarray(init_time, np.float32)
    it = it[:n] if it.ndim else np.full(n, it)
    return (eng.times().astype(np.float32)[None, :] + it[:, None]).astype(np.float32).astype(np.float64)


_DMP_ODE = {}


def _dmp_ode(name, eng_ref, t_ref):
    """SciPy's solution for the first DMP_N episodes at the sample times t_ref [n, M] (of the finest run that is extrapolated
    TO); solved once per case and shared, read-only, by every route and factory"""
    if name in _DMP_ODE:
        assert np.array_equal(_DMP_ODE[name][2], t_ref)
        return _DMP_ODE[name]
    pc, bc, tc, dt, levels, on_grid, params, ip, iv, init_time = _dmp_case(name)
    cen, bw = R.rbf_constants(eng_ref)
    n = t_ref.shape[0]
    f32 = np.float32
    off = int(pc.learn_tau) + int(pc.learn_delay)
    local = params[:n, off:].reshape(n, 7, 6).astype(np.float64)
    w = local[..., :5] * float(f32(tc.weights_scale))
    g = local[..., 5] * float(f32(tc.goal_scale))
    y, v = np.empty((n, t_ref.shape[1], 7)), np.empty((n, t_ref.shape[1], 7))
    onset = []
    for b in range(n):
        tau = float(np.clip(params[b, 0], f32(pc.tau_bound[0]), f32(pc.tau_bound[1]))) if pc.learn_tau else float(f32(pc.tau))
        delay = float(np.clip(params[b, 1], f32(pc.delay_bound[0]), f32(pc.delay_bound[1]))) if pc.learn_delay else float(f32(pc.delay))
        it_b = float(np.asarray(init_time, f32).reshape(-1)[b if isinstance(init_time, np.ndarray) else 0])
        # 'init': the first sample carries the boundary state; 'step': the boundary is at init_time itself
        t_b = t_ref[b, 0] if tc.dmp_first_sample == "init" else it_b
        s = np.maximum((t_ref[b] - delay) / tau, 0.0)
        s_b = max((t_b - delay) / tau, 0.0)
        yy, ys = R.solve(float(f32(tc.alpha)), float(f32(pc.alpha_phase)), cen, bw, w[b], g[b], s_b, ip[b].astype(np.float64),
                         iv[b].astype(np.float64) * tau, s, phase=R.linear_phase if pc.phase_generator_type == "linear" else None)
        y[b], v[b] = yy.T, ys.T / tau
        # the ODE's right-hand side at s = 0 with the boundary state (for the onset check below)
        x0 = 0.0 if pc.phase_generator_type == "linear" else 1.0
        a0 = float(f32(tc.alpha)) * (float(f32(tc.alpha)) / 4 * (g[b] - ip[b]) - iv[b] * tau) + R.forcing(np.full(7, x0), cen, bw, w[b])
        onset.append((s, a0))
    for a in (y, v, t_ref):
        a.setflags(write=False)
    _DMP_ODE[name] = (y, v, t_ref, onset)
    return _DMP_ODE[name]


def _dmp_onset(name, pos, y, onset, sp):
    """
    Where an episode is still held at its boundary state by the delay (scaled time s = 0 up to sample k), sample k + 1 is ONE step
    of the recurrence from exactly that state: y_b + ds (z_b + ds a_0) against the ODE's y_b + ds z_b + ds^2 a_0 / 2 + O(ds^3), a
    local error of ds^2 |a_0| / 2, a_0 the ODE's right-hand side at s = 0.  Bound: twice that, plus the fp32 contract.  The
    extrapolation cannot see an onset that comes a step late -- a first-order error like the recurrence's own, which it
    removes -- but here it is ds |z_b| = dt |init_vel| against a bound of order dt^2.
    """
    seen = 0
    for b, (s, a0) in enumerate(onset):
        held = np.nonzero(s <= 1e-6)[0]
        if held.size == 0 or held[-1] + 1 >= s.size:
            continue
        k = held[-1] + 1
        lim = s[k] ** 2 * np.abs(a0) + 1e-5 * sp
        err = np.abs(pos[b, k] - y[b, k])
        assert (err <= lim).all(), f"{name}: episode {b} leaves its hold with {err.max():.3e} off the ODE (bound {lim[err.argmax()]:.3e})"
        seen += 1
    return seen


def check_dmp_extrapolated(name, factory=None, expect_kernel=None):
    """
    One case on one route (the process-wide options the caller set): runs at dt, dt / 2 (and dt / 4 with the delay on the grid),
    extrapolates, compares positions AND velocities of the first DMP_N episodes with the ODE.  Asserts
      * the measured bound (module table) for every extrapolated pair,
      * extrapolated residual < a tenth of the plain recurrence's error at the same coarse dt,
      * delay on the grid: residual(dt / 2, dt / 4) <= 0.35 residual(dt, dt / 2)  (second order gives 0.25),
      * the first sample after a delay's hold within the one-step local error (_dmp_onset),
      * expect_kernel (a name, or a substring with a leading '~': absent with '!~') on the COARSE engine, GPU only.
    Returns the figures {"plain": (p, v), dt: (p, v), ...} as fractions of the scale.
    """
    pc, bc, tc, dt, levels, on_grid, params, ip, iv, init_time = _dmp_case(name)
    params, ip, iv = params.copy(), ip.copy(), iv.copy()                 # (the shared inputs stay read-only)
    mode = tc.dmp_first_sample
    B = params.shape[0]
    n = min(B, DMP_N)
    runs = []
    for k in range(levels):
        dt_k = dt / 2 ** k
        eng = (factory or make_engine)(pc, bc, tc, dt_k, DMP_DUR)
        # 'init': every run's first sample is the instant init_time + dt of the coarse run
        it_k = init_time if mode == "step" else (np.asarray(init_time, np.float64) + (dt - dt_k))
        if isinstance(init_time, np.ndarray):
            it_k = np.asarray(it_k, np.float32)
            it_arg = torch.tensor(it_k, device=eng.device)
        else:
            it_arg = it_k = float(it_k)
        pos, vel = eng.trajectory(params, ip, iv, it_arg)
        if k == 0 and expect_kernel and factory is None:
            got = eng.last_kernel()
            if expect_kernel.startswith("!~"):
                assert expect_kernel[2:] not in got and "dmp" in got, got
            elif expect_kernel.startswith("~"):
                assert expect_kernel[1:] in got, got
            else:
                assert got == expect_kernel, got
        runs.append((pos[:n].cpu().numpy().astype(np.float64), vel[:n].cpu().numpy().astype(np.float64),
                     _dmp_times(eng, it_k, n), eng))
    # the ODE at the sample times of the finest run that is extrapolated TO (levels - 2); coarser ones are subsets of it
    y, v, _, onset = _dmp_ode(name, runs[levels - 2][3], runs[levels - 2][2])
    sp, sv = np.abs(y).max(), np.abs(v).max()
    held = _dmp_onset(name, runs[levels - 2][0], y, onset, sp)
    assert held >= 3 or not pc.learn_delay, held           # (the learned-delay cases do hold some of their episodes)
    off = {"init": 0, "step": 1}[mode]
    fig = {}
    for k in range(levels - 1):
        ext_p = R.extrapolate(runs[k][0], runs[k + 1][0], runs[k][2], runs[k + 1][2], mode)
        ext_v = R.extrapolate(runs[k][1], runs[k + 1][1], runs[k][2], runs[k + 1][2], mode)
        yk, vk = y, v
        for _ in range(levels - 2 - k):
            yk, vk = yk[:, off::2], vk[:, off::2]
        if k == 0:
            fig["plain"] = (np.abs(runs[0][0] - yk).max() / sp, np.abs(runs[0][1] - vk).max() / sv)
        fig[dt / 2 ** k] = (np.abs(ext_p - yk).max() / sp, np.abs(ext_v - vk).max() / sv)
    print(f"dmp-ode {name} {expect_kernel or ''} " + " ".join(f"{k}: {p:.3e}/{q:.3e}" for k, (p, q) in fig.items()))
    for k in range(levels - 1):
        d = dt / 2 ** k
        (ep, ev), (bp, bv) = fig[d], _dmp_bound(name, d)
        assert ep <= bp, f"{name} dt {d}: pos {ep:.3e} > {bp:.3e} of the scale"
        assert ev <= bv, f"{name} dt {d}: vel {ev:.3e} > {bv:.3e} of the scale"
    assert fig[dt][0] < 0.1 * fig["plain"][0] and fig[dt][1] < 0.1 * fig["plain"][1], fig
    if on_grid:
        assert fig[dt / 2][0] <= 0.35 * fig[dt][0] and fig[dt / 2][1] <= 0.35 * fig[dt][1], fig
    return fig


_PER_EPISODE = {"rows": ({"phase": 0}, "k_traj_rows<dmp>"), "wave": ({"phase_flat": 0}, "k_traj_phase<dmp>"),
                "wg": ({"phase_flat": 1, "pipe": 0}, "k_traj_phase<dmp,wg>"),
                "pipe": ({"phase_flat": 1, "pipe": -1}, "k_traj_phase<dmp,wg,pipe>")}
_SHARED = {"response": ({"dmp_response": -1}, "~dmp_resp"), "serial": ({"dmp_response": 0}, "!~dmp_resp")}
# (case, route, phase_table): every per-episode kernel with the exact forcing rows (0) and the interpolated ones (1)
DMP_ROUTES = ([("shared", r, -1) for r in _SHARED] +
              [("learned", r, t) for t in (0, 1) for r in _PER_EPISODE] +
              [("offgrid", r, 1) for r in ("wave", "pipe")] +
              [("linear", r, 1) for r in ("wave", "pipe")] +
              [("step_shared", r, -1) for r in _SHARED] +
              [("step_learned", r, 1) for r in ("wave", "pipe")])


@pytest.mark.parametrize("name,route,table", DMP_ROUTES, ids=[f"{n}-{r}-table{t}" if t >= 0 else f"{n}-{r}" for n, r, t in DMP_ROUTES])
def test_dmp_routes_solve_the_ode_by_extrapolation(name, route, table, mpk_option):
    opts, kernel = (_SHARED if route in _SHARED else _PER_EPISODE)[route]
    for k, v in opts.items():
        mpk_option(k, v)
    if table >= 0:
        mpk_option("phase_table", table)
    check_dmp_extrapolated(name, expect_kernel=kernel)
