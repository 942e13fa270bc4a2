"""
CPU suite, part 1: what pins the ORACLE (oracle/mp_oracle.py), since the reference's arithmetic (mp_pytorch) cannot be
imported or compiled here ("parity unpinned"):
  * committed golden fixtures (tests/golden/*.npz) incl. a second, torch-CPU formulation
  * an independent SciPy ODE solve of the ProDMP / DMP dynamics
  * the reference's own behavioural tests, restated: action-dim formula, parameter order, tau / delay plateaus with
    ``==``, PD formula with ``array_equal``, planning counts
"""
import os
import sys

import numpy as np
import pytest
from scipy.integrate import solve_ivp

from oracle import mp_oracle as O
from tests.golden.make_golden import CONFIGS

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- golden fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_reproduces_golden(name):
    cfg = CONFIGS[name]
    z = np.load(os.path.join(GOLD, name + ".npz"))
    pc, bc, tc = cfg["pc"], cfg["bc"], cfg["tc"]
    for k, it in enumerate(z["init_times"]):
        p, v = O.get_trajectory(pc, bc, tc, z["params"], cfg["duration"], cfg["dt"], float(it), z["init_pos"],
                                z["init_vel"], dtype=np.float32)
        np.testing.assert_allclose(p, z[f"pos32_{k}"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(v, z[f"vel32_{k}"], rtol=2e-6, atol=2e-5)
        assert p.dtype == np.float32 and p.shape == (z["params"].shape[0], O.num_steps(cfg["duration"], cfg["dt"]),
                                                     tc.action_dim)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_agrees_with_torch_formulation(name):
    """two independent restatements (numpy vs torch CPU fp32 in the recalled mp_pytorch op order)"""
    cfg = CONFIGS[name]
    z = np.load(os.path.join(GOLD, name + ".npz"))
    fd = cfg["tc"].trajectory_generator_type == "promp"
    for k in range(len(z["init_times"])):
        sp, sv = np.abs(z[f"pos32_{k}"]).max(), np.abs(z[f"vel32_{k}"]).max()
        assert np.abs(z[f"pos32_{k}"] - z[f"tpos_{k}"]).max() <= 5e-6 * sp
        # ProMP velocity = forward difference of fp32 positions: conditioning 1/dt (see tests/test_gpu_trajectory.py)
        tol_v = 1e-5 * sv + (2 * np.finfo(np.float32).eps * sp / cfg["dt"] if fd else 0.0)
        assert np.abs(z[f"vel32_{k}"] - z[f"tvel_{k}"]).max() <= tol_v
        assert z[f"err64_{k}"][0] < 5e-6            # fp32 oracle vs fp64 oracle, relative to the array maximum
    # the oracle's scalar linspace recipe vs torch's vectorised kernel: <= 2 ulp, and the ProDMP table indices
    # (asserted identical inside make_golden.py) do not move
    assert np.abs(z["times_torch"] - z["times_oracle"]).max() <= 2.4e-7 * max(1.0, cfg["duration"])


def test_golden_indices_are_what_the_oracle_computes():
    cfg = CONFIGS["cfg4_prodmp_replan"]
    z = np.load(os.path.join(GOLD, "cfg4_prodmp_replan.npz"))
    tabs = O.prodmp_tables(cfg["pc"], cfg["bc"], np.float32)
    for k, it in enumerate(z["init_times"]):
        times = O.make_times(cfg["duration"], cfg["dt"], float(it))
        idx = O.prodmp_indices(times, np.float32(1.5), np.float32(0.0), tabs.scaled_dt)
        assert np.array_equal(idx.astype(np.int32), z[f"idx_{k}"][0])
        # dt = 0.02 on a 0.01 grid: every index is an exact multiple -> 2 * step + init offset
        assert np.array_equal(idx, 2 * np.arange(1, 101) + int(round(float(it) / 0.01)))


# ---- independent maths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init_time", [0.0, 0.5, 1.0])
def test_prodmp_closed_form_solves_the_ode(init_time):
    """tau^2 y'' = alpha (beta (g - y) - tau y') + x Phi(x)^T w from the boundary condition at init_time"""
    pc = O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0)
    bc = O.BasisCfg("prodmp", num_basis=5, basis_bandwidth_factor=2, alpha=10)
    tc = O.TrajCfg("prodmp", action_dim=1)
    rng = np.random.default_rng(3)
    params = rng.standard_normal((1, 6))
    y0, v0 = 0.3, -0.2
    times = O.make_times(2.0, 0.02, init_time, dtype=np.float64)
    pos, vel = O.prodmp_trajectory(pc, bc, tc, params, times, init_time, np.array([[y0]]), np.array([[v0]]),
                                   dtype=np.float64)
    w, g = params[0, :5], params[0, 5]
    alpha, beta, tau = 10.0, 2.5, 1.5
    rb = O.BasisCfg(**{**bc.__dict__, "basis_generator_type": "rbf"})

    def rhs(t, s):
        y, z = s
        tt = np.array([t])
        f = O.phase(pc, tt, dtype=np.float64)[0] * (O.rbf_basis(pc, rb, tt, dtype=np.float64)[0] @ w)
        return [z / tau, (alpha * (beta * (g - y) - z) + f) / tau]

    sol = solve_ivp(rhs, [init_time, times[-1]], [y0, v0 * tau], t_eval=times, rtol=1e-10, atol=1e-12)
    assert np.abs(sol.y[0] - pos[0, :, 0]).max() < 2e-5      # residual = trapezoid rule on the dt = 0.01 grid
    assert np.abs(sol.y[1] / tau - vel[0, :, 0]).max() < 1e-4


def test_dmp_euler_converges_to_the_ode():
    pc = O.PhaseCfg("exp", tau=2.0, alpha_phase=2.0)
    bc = O.BasisCfg("rbf", num_basis=5)
    tc = O.TrajCfg("dmp", action_dim=1, alpha=25.0)
    rng = np.random.default_rng(5)
    params = rng.standard_normal((1, 6)) * np.array([50, 50, 50, 50, 50, 1.0])
    errs = []
    for dt in (0.004, 0.002, 0.001):
        times = O.make_times(2.0, dt, 0.0, dtype=np.float64)
        pos, vel = O.dmp_trajectory(pc, bc, tc, params, times, np.array([[0.1]]), np.array([[0.0]]), dtype=np.float64)
        w, g = params[0, :5], params[0, 5]

        def rhs(t, s):
            y, z = s
            tt = np.array([t])
            f = O.phase(pc, tt, dtype=np.float64)[0] * (O.rbf_basis(pc, bc, tt, dtype=np.float64)[0] @ w)
            return [z / 2.0, (25.0 * (6.25 * (g - y) - z) + f) / 2.0]

        sol = solve_ivp(rhs, [times[0], times[-1]], [0.1, 0.0], t_eval=times, rtol=1e-10, atol=1e-12)
        errs.append(np.abs(sol.y[0] - pos[0, :, 0]).max())
    assert errs[1] < 0.6 * errs[0] and errs[2] < 0.6 * errs[1]     # first-order convergence of explicit Euler


# ---- the reference's behavioural pins, restated ----------------------------------------------------------------------
@pytest.mark.parametrize("mp_type", ["promp", "dmp", "prodmp"])
@pytest.mark.parametrize("num_dof", [0, 1, 2, 5])
@pytest.mark.parametrize("num_basis", [1, 2, 5])
@pytest.mark.parametrize("learn_tau", [True, False])
@pytest.mark.parametrize("learn_delay", [True, False])
def test_action_dim_formula(mp_type, num_dof, num_basis, learn_tau, learn_delay):
    """test/test_black_box.py:168-193"""
    pc = O.PhaseCfg("exp", learn_tau=learn_tau, learn_delay=learn_delay)
    bc = O.BasisCfg("prodmp" if mp_type == "prodmp" else "rbf", num_basis=num_basis)
    tc = O.TrajCfg(mp_type, action_dim=num_dof)
    expect = num_dof * num_basis + int(learn_tau) + int(learn_delay) + (num_dof if "dmp" in mp_type else 0)
    assert O.num_params(pc, bc, tc) == expect
    assert O.params_bounds(pc, bc, tc).shape == (2, expect)


def _toy(mp_type, learn_tau, learn_delay):
    """make_bb('toy-v0', ...) with mp_pytorch defaults: 1 DoF, 10 basis, tau = duration = 1.0, dt = 0.02"""
    linear = mp_type == "promp"
    pc = O.PhaseCfg("linear" if linear else "exp", tau=1.0, learn_tau=learn_tau, learn_delay=learn_delay,
                    tau_bound=(0.04, 1.0), delay_bound=(0.0, 0.96))
    bc = O.BasisCfg("rbf" if linear else "prodmp", num_basis=10)
    return pc, bc, O.TrajCfg(mp_type, action_dim=1)


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("tau", [0.25, 0.5, 0.75, 1.0])
def test_learn_tau_plateau(mp_type, tau):
    """test/test_black_box.py:219-261 -- param order: action[0] = tau"""
    pc, bc, tc = _toy(mp_type, True, False)
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1, O.num_params(pc, bc, tc))).astype(np.float32)
    a[0, 0] = tau
    pos, vel = O.get_trajectory(pc, bc, tc, a, 1.0, 0.02, 0.0, np.ones((1, 1)), np.zeros((1, 1)))
    pos, vel = pos.flatten(), vel.flatten()
    n = int(np.round(tau / 0.02))
    assert pos.shape == (50,)
    if mp_type == "promp":                      # exact plateau only for the linear phase
        assert np.all(pos[n:] == pos[-1]) and np.all(vel[n:] == vel[-1])
    assert np.all(pos[:n - 1] != pos[-1]) and np.all(vel[:n - 2] != vel[-1])


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("delay", [0, 0.25, 0.5, 0.75])
def test_learn_delay_plateau(mp_type, delay):
    """test/test_black_box.py:266-307"""
    pc, bc, tc = _toy(mp_type, False, True)
    rng = np.random.default_rng(2)
    a = rng.standard_normal((1, O.num_params(pc, bc, tc))).astype(np.float32)
    a[0, 0] = delay
    pos, vel = O.get_trajectory(pc, bc, tc, a, 1.0, 0.02, 0.0, np.ones((1, 1)), np.zeros((1, 1)))
    pos, vel = pos.flatten(), vel.flatten()
    n = int(np.round(delay / 0.02))
    assert np.all(pos[:max(1, n - 1)] == pos[0]) and np.all(vel[:max(1, n - 2)] == vel[0])
    assert np.all(pos[max(1, n):] != pos[0]) and np.all(vel[max(1, n)] != vel[0])


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("tau", [0.25, 0.5, 0.75])
@pytest.mark.parametrize("delay", [0.25, 0.5])
def test_learn_tau_and_delay_plateaus(mp_type, tau, delay):
    """test/test_black_box.py:312-368 -- action[0] = tau, action[1] = delay"""
    if 1.0 < delay + tau:
        pytest.skip("as in the reference")
    pc, bc, tc = _toy(mp_type, True, True)
    rng = np.random.default_rng(4)
    a = rng.standard_normal((1, O.num_params(pc, bc, tc))).astype(np.float32)
    a[0, 0], a[0, 1] = tau, delay
    pos, vel = O.get_trajectory(pc, bc, tc, a, 1.0, 0.02, 0.0, np.ones((1, 1)), np.zeros((1, 1)))
    pos, vel = pos.flatten(), vel.flatten()
    nt, nd = int(np.round(tau / 0.02)), int(np.round(delay / 0.02))
    if mp_type == "promp":
        assert np.all(pos[nd + nt:] == pos[-1]) and np.all(vel[nd + nt:] == vel[-1])
    assert np.all(pos[:nd - 1] == pos[0]) and np.all(vel[:nd - 2] == vel[0])
    act_p, act_v = pos[nd: nd + nt - 1], vel[nd: nd + nt - 2]
    assert np.all(act_p != pos[-1]) and np.all(act_p != pos[0])
    assert np.all(act_v != vel[-1]) and np.all(act_v != vel[0])


def test_sub_trajectory_length_is_round_tau_over_dt():
    """test/test_replanning_sequencing.py:104-105"""
    pc, bc, tc = _toy("promp", True, False)
    for tau in (0.1, 0.33, 0.5, 0.97):
        a = np.zeros((1, O.num_params(pc, bc, tc)), np.float32)
        a[0, 0] = tau
        pos, _ = O.get_trajectory(pc, bc, tc, a, None, 0.02, 0.0, np.ones((1, 1)), np.zeros((1, 1)))
        assert pos.shape[1] == int(np.round(np.float32(tau) / 0.02))


@pytest.mark.parametrize("pd", [(0, 0), (0.5, 0.5), (1.0, -0.25), (np.array([1.0, 2.0]), np.array([0.1, 0.2]))])
def test_pd_formula_is_exact(pd):
    """test/test_controller.py:30-44"""
    p, d = pd
    rng = np.random.default_rng(0)
    for _ in range(10):
        q_d, qd_d, q, qd = (rng.uniform(-1, 1, 2) for _ in range(4))
        assert np.array_equal(O.pd_action(p, d, q_d, qd_d, q, qd), p * (q_d - q) + d * (qd_d - qd))


def test_controller_shape_mismatch_raises():
    """test/test_controller.py:47-54, :68-73"""
    with pytest.raises(ValueError):
        O.pd_action(1, 1, np.ones(2), np.ones(2), np.ones(3), np.ones(2))
    with pytest.raises(ValueError):
        O.pd_action(1, 1, np.ones(2), np.ones(2), np.ones(2), np.ones(3))
    with pytest.raises(ValueError):
        O.metaworld_action(np.ones(4), None, np.ones(5), None)
    a = O.metaworld_action(np.array([1., 2., 3., 9.]), None, np.array([.5, .5, .5, 0.]), None)
    assert np.array_equal(a, np.array([.5, 1.5, 2.5, 9.]))


# ---- the reference's OWN controller code (the one arithmetic of the path that lives in /root/reference) ------------------
REF_CTRL = os.path.join(GOLD, "ref_controllers.npz")
REF_CFGS = ("cfg1", "cfg2", "cfg3", "cfg4", "cfg5")


def test_reference_controller_fixture_provenance():
    """tests/golden/ref_controllers.npz holds outputs of the reference's fancy_gym/black_box/controller/*.py loaded
    unmodified (tests/golden/make_ref_controller_golden.py); it is the committed generator's product, and it records the
    sha256 of each of the four reference files it was generated from"""
    import hashlib
    import re
    z = np.load(REF_CTRL)
    meta = str(z["meta"])
    assert "generated from /root/reference controller/*.py" in meta
    gen = hashlib.sha256(open(os.path.join(GOLD, "make_ref_controller_golden.py"), "rb").read()).hexdigest()
    assert "generator sha256 " + gen in meta, "ref_controllers.npz predates the committed generator: re-run it"
    assert list(z["shape_errors"]) == ["ValueError"] * 3            # pd_controller.py:22-27 / test_controller.py:47-54
    for f in ("pd_controller.py", "pos_controller.py", "vel_controller.py", "meta_world_controller.py"):
        assert re.search(re.escape(f) + r" sha256 [0-9a-f]{64}\b", meta), f


REF_VALID = os.path.join(GOLD, "ref_validity.npz")
REF_VALID_CASES = tuple(str(c) for c in np.load(REF_VALID)["cases"])


def test_reference_validity_fixture_provenance():
    """tests/golden/ref_validity.npz holds the verdicts / penalties of the reference's check_traj_validity and
    _get_traj_invalid_penalty compiled alone (tests/golden/make_ref_validity_golden.py); it is the committed generator's product
    and records the sha256 of both reference files it read"""
    import hashlib
    import re
    z = np.load(REF_VALID)
    meta = str(z["meta"])
    assert "check_traj_validity and _get_traj_invalid_penalty compiled alone with ast" in meta
    gen = hashlib.sha256(open(os.path.join(GOLD, "make_ref_validity_golden.py"), "rb").read()).hexdigest()
    assert "generator sha256 " + gen in meta, "ref_validity.npz predates the committed generator: re-run it"
    for f in ("table_tennis_env.py", "table_tennis_utils.py"):
        assert re.search(re.escape(f) + r" sha256 [0-9a-f]{64}\b", meta), f
    # what the fixture has to cover: NaN / +-inf positions and tau / delay, both verdicts, NaN and infinite penalties
    act = np.concatenate([z[c + "_action"] for c in REF_VALID_CASES])
    pos_nan = np.concatenate([np.isnan(z[c + "_pos"]).any(axis=(1, 2)) for c in REF_VALID_CASES])
    valid = np.concatenate([z[c + "_valid"] for c in REF_VALID_CASES])
    pen = np.concatenate([z[c + "_penalty"] for c in REF_VALID_CASES])
    assert np.isnan(act).any() and np.isinf(act).any() and (pos_nan & valid).any() and (pos_nan & ~valid).any()
    assert np.isnan(pen[~valid]).any() and np.isinf(pen[~valid]).any() and valid.sum() > 100 and (~valid).sum() > 100


@pytest.mark.parametrize("case", REF_VALID_CASES)
def test_oracle_validity_equals_the_reference(case):
    """O.traj_validity == check_traj_validity bit for bit, O.traj_invalid_penalty == _get_traj_invalid_penalty with NaN where
    the reference's is NaN -- on positions exactly on / one float32 beside the limits, NaN / +-inf positions, raw tau / delay
    and limits, lo > hi and limits beyond the float32 range"""
    z = np.load(REF_VALID)
    g = lambda n: z[f"{case}_{n}"]
    pos, act, lo, hi, tb, db = g("pos"), g("action"), g("lo"), g("hi"), g("tb"), g("db")
    with np.errstate(invalid="ignore"):
        valid = O.traj_validity(act, pos, lo, hi, tb, db)
        pen = O.traj_invalid_penalty(act, pos, lo, hi, tb, db)
    np.testing.assert_array_equal(valid, g("valid"))
    np.testing.assert_array_equal(pen, g("penalty"))            # (NaN == NaN here)
    np.testing.assert_array_equal(pen[~valid], g("penalty")[~valid])


@pytest.mark.parametrize("cfg", REF_CFGS)
def test_oracle_controllers_equal_the_reference_controllers(cfg):
    """oracle pd / pos / vel actions == what the reference's classes returned on the same inputs, bit for bit; the
    oracle's rollout loop (frozen state and double integrator) == the per-step loop with the reference's PDController in it"""
    z = np.load(REF_CTRL)
    g = lambda n: z[f"{cfg}_{n}"]
    dp, dv, q0, qd0, lo, hi = g("des_pos"), g("des_vel"), g("q0"), g("qd0"), g("lo"), g("hi")
    pg, dg, dt = g("p_gains"), g("d_gains"), float(g("dt"))
    pg = float(pg) if pg.ndim == 0 else pg
    dg = float(dg) if dg.ndim == 0 else dg
    B, T, D = dp.shape
    for b in range(B):
        for t in range(0, T, 7):
            a = O.pd_action(pg, dg, dp[b, t], dv[b, t], q0[b], qd0[b])
            assert a.dtype == np.float64 and np.array_equal(a, g("pd")[b, t])
    # batched form (what the GPU tests compare against)
    for ctrl, key in (("motor", "pd_clip"), ("position", "pos_clip"), ("velocity", "vel_clip")):
        ra, rq, rqd = O.rollout(dp, dv, ctrl, pg, dg, lo, hi, "static", dt, q0, qd0)
        assert np.array_equal(ra, g(key)), (cfg, ctrl)
        assert np.array_equal(rq, q0) and np.array_equal(rqd, qd0)
    assert np.array_equal(O.pos_action(dp[0, 0], dv[0, 0], q0[0], qd0[0]), dp[0, 0])
    assert np.array_equal(O.vel_action(dp[0, 0], dv[0, 0], q0[0], qd0[0]), dv[0, 0])
    ra, rq, rqd = O.rollout(dp, dv, "motor", pg, dg, lo, hi, "double_integrator", dt, q0, qd0)
    assert np.array_equal(ra, g("loop_act")) and np.array_equal(rq, g("loop_q")) and np.array_equal(rqd, g("loop_qd"))


def test_oracle_and_host_controllers_on_the_reference_grid():
    """the reference's known-answer grid (test/test_controller.py:14-73), with the REFERENCE's outputs as the expectation,
    against the oracle and against the host classes of the drop-in (fancy_gym_amd/black_box/controller)"""
    from fancy_gym_amd.black_box.factory import get_controller
    z = np.load(REF_CTRL)
    gi, go = z["grid_in"], z["grid_pd"]
    assert gi.shape == (3 ** 4 * 36, 18)
    for row, want in zip(gi[::5], go[::5]):
        dp, dv, cp, cv, pg, dg = (row[3 * i:3 * i + 3] for i in range(6))
        assert np.array_equal(O.pd_action(pg, dg, dp, dv, cp, cv), want)
        assert np.array_equal(get_controller("motor", p_gains=pg, d_gains=dg)(dp, dv, cp, cv), want)
    # vectorised over the whole grid
    assert np.array_equal(O.pd_action(gi[:, 12:15], gi[:, 15:18], gi[:, 0:3], gi[:, 3:6], gi[:, 6:9], gi[:, 9:12]), go)
    mi, mo = z["metaworld_in"], z["metaworld_out"]
    mw = get_controller("metaworld")
    for row, want in zip(mi, mo):
        assert np.array_equal(O.metaworld_action(row[:4], None, row[4:], None), want)
        assert np.array_equal(mw(row[:4], np.zeros(4), row[4:], np.zeros(4)), want)
    assert np.array_equal(O.metaworld_action(mi[:, :4], None, mi[:, 4:], None), mo)


@pytest.mark.parametrize("max_planning_times", [1, 2, 3, 4])
@pytest.mark.parametrize("every", [5, 10, 25])
def test_planning_counts(max_planning_times, every):
    """test/test_replanning_sequencing.py:165-194,338-364: #step() calls per episode == max_planning_times"""
    horizon = 50 if every < 25 else 100
    segs = O.replanning_segments(horizon, every, max_planning_times)
    assert len(segs) == max_planning_times
    assert sum(n for _, n in segs) == horizon
    for k, (start, n) in enumerate(segs):
        assert start == k * every
        assert n == (every if k < max_planning_times - 1 else horizon - start)


# ---- the same differential-equation checks the GPU suite applies to the HIP path (tests/test_gpu_ode.py), here on the
# oracle: cfg2, cfg4's four replanning boundary conditions (auto_scale_basis, disable_goal), the TableTennis ProDMP
# configuration with learned tau / delay (relative_goal), DMP Euler convergence ----------------------------------------
def test_oracle_solves_the_ode_for_every_baseline_prodmp_and_dmp_configuration():
    from tests import test_gpu_ode as G
    from tests.oracle_engine import OracleEngine
    G.check_cfg2(0.0, factory=OracleEngine)
    G.check_cfg2(0.5, factory=OracleEngine)
    G.check_cfg4(factory=OracleEngine)
    G.check_tabletennis_prodmp(factory=OracleEngine)
    G.check_cfg3_dmp(factory=OracleEngine)


def test_oracle_solves_the_ode_for_the_prodmp_cases_with_own_init_time_and_the_remaining_flags():
    """learned tau / delay with an init_time per episode, init_vel, an enabled scaled relative goal in both relative_goal_mode
    settings; disable_weights with goal_scale 0.5; goal_offset_mode = add; cfg2 with an init_time array -- at the bounds of _check"""
    from tests import test_gpu_ode as G
    from tests.oracle_engine import OracleEngine
    for mode in ("before_scale", "after_scale"):
        G.check_tabletennis_prodmp_own_init_time(mode, factory=OracleEngine)
    for which in ("disable_weights", "goal_offset", "own_init_time"):
        G.check_prodmp_flags(which, factory=OracleEngine)


@pytest.mark.parametrize("name", ["shared", "learned", "offgrid", "linear", "step_shared", "step_learned"])
def test_oracle_dmp_extrapolation_solves_the_ode_and_gives_the_recorded_residuals(name):
    """the Richardson-extrapolated Euler recurrence of the float64 oracle against SciPy, positions and velocities: the check
    the GPU suite applies to every DMP route (its conditions included: a tenth of the plain error, second order with the delay
    on the grid) -- and the residuals the GPU bounds are derived from (tests/test_gpu_ode.py DMP_MEASURED) are what the oracle
    gives"""
    from tests import test_gpu_ode as G
    from tests.oracle_engine import OracleEngine
    fig = G.check_dmp_extrapolated(name, factory=OracleEngine)
    for dt, (rp, rv) in G.DMP_MEASURED[name].items():
        assert abs(fig[dt][0] / rp - 1) < 0.02 and abs(fig[dt][1] / rv - 1) < 0.02, (name, dt, fig[dt], (rp, rv))


def _misreading(kind):
    """OracleEngine with ONE thing of the DMP semantics read differently"""
    import dataclasses
    import torch
    from tests.oracle_engine import OracleEngine

    class Misread(OracleEngine):
        def __init__(self, pc, bc, tc, dt, duration):
            super().__init__(pc, bc, tc, dt, duration)          # (the construction-time constants stay the handle's)
            self.delay_bound = pc.delay_bound
            if kind == "goal_scale_ignored":
                self.tc = dataclasses.replace(tc, goal_scale=1.0)
            if kind == "tau_unclipped":
                self.pc = dataclasses.replace(pc, tau_bound=(1e-5, np.inf))
            if kind == "delay_hold_one_step_late":
                self.pc = dataclasses.replace(pc, delay_bound=(pc.delay_bound[0], np.inf))

        def trajectory(self, params, init_pos, init_vel, init_time=0.0):
            pc = self.pc
            params = np.array(params, np.float32)
            tau = np.float32(pc.tau)
            if pc.learn_tau:
                tau = np.clip(params[:, 0], *np.float32(pc.tau_bound))[:, None]
            if kind == "init_vel_not_times_tau":
                init_vel = np.asarray(init_vel) / tau
            if kind == "delay_hold_one_step_late" and pc.learn_delay:
                c = int(pc.learn_tau)
                params[:, c] = np.clip(params[:, c], *np.float32(self.delay_bound)) + np.float32(self.dt)
            pos, vel = super().trajectory(params, init_pos, init_vel, init_time)
            if kind == "vel_not_divided_by_tau":
                vel = vel * torch.as_tensor(np.asarray(tau, np.float64))[..., None]
            return pos, vel

    return Misread


@pytest.mark.parametrize("kind", ["vel_not_divided_by_tau", "init_vel_not_times_tau", "goal_scale_ignored",
                                  "delay_hold_one_step_late", "tau_unclipped"])
def test_the_extrapolated_dmp_checks_reject_misreadings_the_first_order_check_accepts(kind):
    """why the extrapolated checks exist: each of these one-line misreadings of the DMP semantics passes check_cfg3_dmp (shared
    phase, init_vel 0, unit scales, no delay, positions only, 5 %) and fails the learned-phase or the shared-phase check"""
    from tests import test_gpu_ode as G
    factory = _misreading(kind)
    G.check_cfg3_dmp(factory=factory)                      # let through
    caught = []
    for name in ("learned", "shared"):
        try:
            G.check_dmp_extrapolated(name, factory=factory)
        except AssertionError:
            caught.append(name)
    print(kind, "caught by", caught)
    assert "learned" in caught, (kind, caught)


def test_golden_fixtures_record_their_provenance():
    """every fixture names the numpy / torch versions it was produced with and carries the hash of the generator script
    and of the oracle it came from; the committed generator AND the committed oracle are the ones that produced the
    committed fixtures (an oracle edit without regenerating them fails here)"""
    import hashlib
    gen = hashlib.sha256(open(os.path.join(GOLD, "make_golden.py"), "rb").read()).hexdigest()
    orc = hashlib.sha256(open(os.path.join(ROOT, "oracle", "mp_oracle.py"), "rb").read()).hexdigest()
    for name in sorted(CONFIGS):
        z = np.load(os.path.join(GOLD, name + ".npz"))
        assert "numpy" in str(z["versions"]) and "torch" in str(z["versions"])
        assert str(z["generator_sha256"]) == gen, f"{name}.npz was not produced by the committed make_golden.py"
        assert str(z["oracle_sha256"]) == orc, f"{name}.npz predates the committed oracle/mp_oracle.py: re-run make_golden.py"
        assert "NOT from mp_pytorch" in str(z["meta"])


# ---- one-command pinning against the real mp_pytorch (tools/pin_against_mp_pytorch.py) ----------------------------------
def _run_pin(args, behaviour=None):
    import subprocess
    code = "import sys; sys.path.insert(0, %r)\n" % ROOT
    if behaviour:
        code += "import tests.fake_mp_pytorch as F; F.BEHAVIOUR.update(%r)\n" % (behaviour,)
    code += "from tools import pin_against_mp_pytorch as P; sys.exit(P.main(%r))\n" % (list(args),)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)


def test_oracle_against_mp_pytorch_reference_outputs(tmp_path):
    """
    THE pin: oracle/mp_oracle.py against outputs of mp_pytorch itself, driven through the reference's factories and the
    BlackBoxWrapper.get_trajectory call sequence.  Runs from committed tests/golden/ref_*.npz when a maintainer has
    produced them (`python tools/pin_against_mp_pytorch.py`), else live when the package is importable, else SKIPS --
    and that skip is the statement "parity unpinned" (DESIGN.md section 2).
    """
    import glob
    # (ref_controllers.npz -- the reference's own controller files, no "package" entry -- is not one of these)
    committed = [f for f in glob.glob(os.path.join(GOLD, "ref_*.npz"))
                 if "package" in np.load(f).files and str(np.load(f)["package"]) == "mp_pytorch"]
    if committed:
        r = _run_pin(["--check-only", "--out", GOLD])
    else:
        try:
            import mp_pytorch  # noqa: F401
        except ImportError:
            pytest.skip("mp_pytorch is not importable here and no tests/golden/ref_*.npz from it is committed: the oracle "
                        "stays UNPINNED; run `python tools/pin_against_mp_pytorch.py` where the package is installed")
        r = _run_pin(["--out", str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "PINNED: the oracle with its shipped defaults reproduces the reference on every case" in r.stdout


@pytest.mark.parametrize("switch,value", [(None, None), ("relative_goal_mode", "after_scale"), ("goal_offset_mode", "add"),
                                          ("single_rbf_mode", "refuse"), ("dmp_first_sample", "step")])
def test_pin_script_plumbing_with_the_facade(tmp_path, switch, value):
    """
    The pinning script's own plumbing (constructor kwargs, call sequence, fixture format, --check-only, switch
    detection), exercised with tests/fake_mp_pytorch -- the oracle behind mp_pytorch's interface, which pins NOTHING.
    When the facade exhibits the non-default setting of one switch the script must say so, name that setting and fail.
    """
    beh = {switch: value} if switch else None
    r = _run_pin(["--package", "tests.fake_mp_pytorch", "--out", str(tmp_path)], beh)
    out = r.stdout
    assert os.path.exists(tmp_path / "ref_cfg2_prodmp_boxpushing.npz") and os.path.exists(tmp_path / "ref_probe_single_rbf.npz")
    z = np.load(tmp_path / "ref_cfg2_prodmp_boxpushing.npz")
    assert str(z["package"]) == "tests.fake_mp_pytorch" and z["pos_0"].shape == (2, 100, 7) and len(str(z["generator_sha256"])) == 64
    if switch is None:
        assert r.returncode == 0, out[-2000:] + r.stderr[-1000:]
        assert "PINNED" in out and "NOT pinned" not in out
        again = _run_pin(["--check-only", "--out", str(tmp_path)])          # the fixtures alone reproduce the verdict
        assert again.returncode == 0 and again.stdout.splitlines()[1:] == out.splitlines()[1:]
    else:
        assert r.returncode == 1, out[-2000:] + r.stderr[-1000:]
        line = next(ln for ln in out.splitlines() if ln.startswith(f"[pin] {switch}"))
        assert f"reference behaves as '{value}'" in line and "shipped default" in line
        for other in ("relative_goal_mode", "goal_offset_mode", "single_rbf_mode", "dmp_first_sample"):
            if other != switch:
                ln = next(x for x in out.splitlines() if x.startswith(f"[pin] {other}"))
                assert "shipped default" not in ln, ln


# ---- the configuration constants, pinned to the reference's own files (round 6) -----------------------------------------------
# tests/golden/ref_configs.json is written by tests/golden/make_ref_config_golden.py from /root/reference with `ast`: the literal
# _BB_DEFAULTS, the reference's nested_update FunctionDef compiled alone, the mp_config class attributes of the mp_wrapper.py files and
# the merge order of bb_env_constructor (registry.py:284-292).  Everything below compares what this repository TYPED with it.
def _norm(rec):
    import dataclasses
    pc, bc, tc = rec[:3]
    if tc.goal_offset_mode == "ignore":
        tc = dataclasses.replace(tc, goal_offset=0.0)       # (swallowed by **kwargs: the value plays no part)
    if bc.basis_generator_type != "zero_rbf":
        bc = dataclasses.replace(bc, num_basis_zero_start=0, num_basis_zero_goal=0)      # (zero_rbf only)
    return (pc, bc, tc) + tuple(rec[3:5])


def test_bb_defaults_and_nested_update_equal_the_references():
    from fancy_gym_amd.envs.registry import _BB_DEFAULTS, resolve_mp_config
    from tests import ref_configs as R
    ref = R.load()
    assert R.same(_BB_DEFAULTS, ref["_BB_DEFAULTS"])
    for env_id, e in ref["envs"].items():
        got = resolve_mp_config(e["mp_type"], {e["mp_type"]: e["mp_config"]})
        assert R.same(got, e["config"]), env_id


def test_every_baseline_constant_typed_in_this_repository_equals_the_reference_merge():
    """bench.py's CFG / gains, the CFG1 - CFG5 tuples of the GPU suite, the golden generator's configurations, the learned-phase
    configurations of tests/test_gpu_learned_phase.py and tools/learned_phase_bench.py -- against the merged reference configs"""
    import dataclasses
    import importlib.util
    from tests import ref_configs as R
    from tests.golden.make_golden import CONFIGS as GOLD
    ref = R.load()["envs"]
    rec = {k: R.oracle_records(k, v) for k, v in ref.items()}

    def load_module(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        src = open(path).read()
        # the constants only: everything before the first function definition (no torch / GPU work at import)
        head = src[:src.index("\ndef ")]
        exec(compile(head, path, "exec"), mod.__dict__)
        return mod

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # 1. bench.py (cfg2)
    bench = load_module(os.path.join(root, "bench.py"), "bench_consts")
    pc, bc, tc, dt, dur, (pg, dg), _, _ = rec["fancy_ProDMP/BoxPushingDense-v0"]
    assert bench.CFG == dict(num_dof=tc.action_dim, num_basis=bc.num_basis, dt=dt, duration=dur, tau=pc.tau, alpha_phase=pc.alpha_phase,
                             basis_bandwidth_factor=bc.basis_bandwidth_factor, basis_alpha=bc.alpha)
    assert np.array_equal(bench.P_GAINS, pg) and np.array_equal(bench.D_GAINS, dg)
    assert bench.T_STEPS == ref["fancy_ProDMP/BoxPushingDense-v0"]["max_episode_steps"]
    # 2. CFG1 - CFG5 (tests/test_gpu_trajectory.py; imported lazily: the module needs torch only)
    from tests.test_gpu_trajectory import CFG1, CFG2, CFG3, CFG4, CFG5
    for mine, env_id in ((CFG1, "fancy_ProMP/Reacher5d-v0"), (CFG2, "fancy_ProDMP/BoxPushingDense-v0"), (CFG3, "fancy_DMP/Reacher7d-v0"),
                         (CFG4, "fancy_ProDMP/BoxPushingDenseReplan-v0"), (CFG5, "fancy_ProMP/TableTennis4D-v0")):
        assert _norm(mine) == _norm(rec[env_id]), env_id
    # 3. the golden generator's five BASELINE configurations (+ gains)
    for name, env_id in (("cfg1_promp_reacher5d", "fancy_ProMP/Reacher5d-v0"), ("cfg2_prodmp_boxpushing", "fancy_ProDMP/BoxPushingDense-v0"),
                         ("cfg3_dmp_reacher7d", "fancy_DMP/Reacher7d-v0"), ("cfg4_prodmp_replan", "fancy_ProDMP/BoxPushingDenseReplan-v0"),
                         ("cfg5_promp_tabletennis", "fancy_ProMP/TableTennis4D-v0"), ("tt_prodmp_learn_tau_delay", "fancy_ProDMP/TableTennis4D-v0")):
        g = GOLD[name]
        assert _norm((g["pc"], g["bc"], g["tc"], g["dt"], g["duration"])) == _norm(rec[env_id]), name
        assert np.array_equal(np.broadcast_to(g["gains"][0], rec[env_id][5][0].shape), rec[env_id][5][0]), name
        assert np.array_equal(np.broadcast_to(g["gains"][1], rec[env_id][5][1].shape), rec[env_id][5][1]), name
    # 4. the learned-phase families (tests/test_gpu_learned_phase.py, tools/learned_phase_bench.py)
    from tests.test_gpu_learned_phase import CONFIGS as LP
    for name, env_id in (("tt_prodmp", "fancy_ProDMP/TableTennis4D-v0"), ("tt_prodmp_replan", "fancy_ProDMP/TableTennisGoalSwitchingReplan-v0"),
                         ("beerpong_promp", "fancy_ProMP/BeerPong-v0")):
        pc, bc, tc, dt, dur, (pg, dg), every, mpt = LP[name]
        r = rec[env_id]
        assert _norm((pc, bc, tc, dt, dur)) == _norm(r), name
        assert np.array_equal(pg, r[5][0]) and np.array_equal(dg, r[5][1]), name
        sched = r[6]
        if every is None:
            assert sched is None and (r[7] is None or r[7] == mpt), name
        else:
            assert np.array_equal(sched, np.arange(401) % every == 0) and r[7] == mpt, name
    # cfg4's schedule and planning budget (tests use every = 25, max_planning_times = 4)
    r4 = rec["fancy_ProDMP/BoxPushingDenseReplan-v0"]
    assert np.array_equal(r4[6], np.arange(401) % 25 == 0) and r4[7] == 4
    assert ref["fancy_ProDMP/BoxPushingDenseReplan-v0"]["config"]["black_box_kwargs"]["condition_on_desired"] is True
    # the joint limits of the validity gate (table_tennis_utils.py:3-4)
    from tests.test_gpu_learned_phase import JNT_HIGH, JNT_LOW
    tt = R.load()["table_tennis_utils"]
    assert np.array_equal(JNT_LOW, tt["jnt_pos_low"]) and np.array_equal(JNT_HIGH, tt["jnt_pos_high"])
