"""
mpk_trajectory_phase_vjp (k_phase_vjp) on the device: the vector-Jacobian product of the per-episode-phase trajectory map -- learned tau /
delay, per-episode init_time -- against float64 torch autograd of the restatement in tests/phase_vjp_ref.py (which equals the float64
oracle to 1e-12: tests/test_phase_vjp_host.py).

Bound per output array (phase columns of g_params, its local columns, g_init_pos, g_init_vel): the larger of the project's rule
1e-5 max|ref| + 1e-5 |ref| and 4 x the error of float32 CPU autograd of the same restatement against the float64 value -- the margin
tests/test_gpu_traj_vjp.py gives a float32 sum over T; both maxima are printed before the assertion.

Inputs: tau / delay at least 5 % of their bound's width inside the bounds, except row 0 (above tau_hi) and row 1 (below tau_lo); no step
within 1e-4 of a clip of the phase (phase_vjp_ref.make_inputs advances the seed until that holds, and says which rows it leaves out).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import mp_oracle as O
from tests import phase_vjp_ref as R
from tests.test_gpu_trajectory import RTOL, make_engine
from tests.test_phase_vjp_host import all_configs, init_time_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ["tt_prodmp", "tt_prodmp_replan", "beerpong_promp", "promp_5dof_learn_both", "prodmp_3dof_learn_tau", "promp_16dof_learn_tau",
         "promp_exp_learn_both", "prodmp_after_scale_no_weights", "cfg4_per_episode_init_time"]
GRID = [f"{kind}_d{D}_t{T}" for kind in ("promp", "prodmp") for D in (1, 3, 7) for T in (2, 3, 5, 63, 64, 65)]
BATCHES = (1, 3, 65)
# launch_phase_vjp's grid: workgroups of 4 waves, one episode per wave and trip, at most 8 workgroups per CU (mpk_phase_vjp.hip)
WAVES_PER_WG, WG_PER_CU = 4, 8

_engines, _cases = {}, {}


def dev(x):
    return torch.as_tensor(x, device="cuda")


def engine_of(name):
    if name not in _engines:
        pc, bc, tc, dt, dur, _ = all_configs()[name]
        _engines[name] = make_engine(pc, bc, tc, dt, dur, device=0)
    return _engines[name]


def case(name, B, seed=0):
    """inputs, upstream gradients, the float64 reference and the float32 CPU autograd's error: computed once, shared, never written to"""
    key = (name, B, seed)
    if key not in _cases:
        pc, bc, tc, dt, dur, it_spec = all_configs()[name]
        it = init_time_of(it_spec, B)
        params, ip, iv, used = R.make_inputs(pc, bc, tc, dt, dur, B, it, seed)
        assert R.phase_clip_margin(pc, params, it, dt, dur) >= 1e-4 or tc.trajectory_generator_type != "promp"
        rng = np.random.default_rng(1000 + used)
        T, D = O.num_steps(dur, dt), tc.action_dim
        g_pos, g_vel = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(2))
        c = dict(name=name, B=B, it=it, params=params, ip=ip, iv=iv, g_pos=g_pos, g_vel=g_vel, n_phase=int(pc.learn_tau) + int(pc.learn_delay),
                 cfg=(pc, bc, tc, dt, dur))
        for use in ((True, True), (False, True), (True, False)):
            args = (pc, bc, tc, params, ip, iv, it, dt, dur, g_pos if use[0] else None, g_vel if use[1] else None)
            ref = R.vjp(*args)
            e32 = [np.abs(a - r) for a, r in zip(R.vjp(*args, dtype=torch.float32), ref)]
            c[use] = (ref, e32)
            if B > 3:
                break               # the NULL cases run on the small batches
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def it_arg(c):
    return dev(c["it"]) if isinstance(c["it"], np.ndarray) else c["it"]


def split(c, g_params, g_ip, g_iv):
    n = c["n_phase"]
    return (("g_params[phase]", g_params[:, :n]), ("g_params[local]", g_params[:, n:]), ("g_init_pos", g_ip), ("g_init_vel", g_iv))


def check(c, got, use, label):
    ref, e32 = c[use]
    worst = 0.0
    for (what, g), (_, r), (_, e) in zip(split(c, *[x.cpu().numpy().astype(np.float64) for x in got]), split(c, *ref), split(c, *e32)):
        if r.size == 0:
            continue
        err = np.abs(g - r)
        tol = np.maximum(RTOL * np.abs(r).max() + RTOL * np.abs(r), 4.0 * e.max())
        print(f"[phase_vjp] {c['name']} B={c['B']} {label} {what}: max |gpu - f64| {err.max():.3e}  max |f32 cpu - f64| {e.max():.3e}  "
              f"max|ref| {np.abs(r).max():.3e}")
        assert np.isfinite(g).all() and not (err > tol).any(), f"{what} {label}: max err {err.max():.3e}, {(err > tol).sum()} outside"
        worst = max(worst, err.max())
    return worst


def exact_values(c, got):
    """what no column reads, the held indices and the clamp leave as exact zeros"""
    pc, bc, tc = c["cfg"][:3]
    g_params, g_ip, g_iv = (x.cpu().numpy() for x in got)
    if pc.learn_tau:
        assert g_params[0, 0] == 0.0 and (c["B"] < 2 or g_params[1, 0] == 0.0)
    if tc.trajectory_generator_type == "prodmp":
        if pc.learn_delay:
            assert (g_params[:, int(pc.learn_tau)] == 0.0).all()
    else:
        assert (g_iv == 0.0).all()
        if bc.basis_generator_type != "zero_rbf":
            assert (g_ip == 0.0).all()


def run_case(name, B):
    c = case(name, B)
    eng = engine_of(name)
    params, ip, iv, g_pos, g_vel = (dev(c[k]) for k in ("params", "ip", "iv", "g_pos", "g_vel"))
    it = it_arg(c)
    # the plain launch, then the same call under autograd: same bits, same kernel
    pos0, vel0 = eng.trajectory(params, ip, iv, it)
    k_fwd = eng.last_kernel()
    leaves = [x.clone().requires_grad_(True) for x in (params, ip, iv)]
    pos, vel = eng.trajectory(*leaves, it, phase_gradient="pathwise")
    assert eng.last_kernel() == k_fwd and pos.requires_grad and vel.requires_grad
    assert torch.equal(pos, pos0) and torch.equal(vel, vel0)
    torch.autograd.backward((pos, vel), (g_pos, g_vel))
    assert eng.last_kernel().startswith("k_phase_vjp<"), eng.last_kernel()
    bare = eng.trajectory_phase_vjp(params, ip, iv, g_pos, g_vel, it)
    assert eng.last_kernel().startswith("k_phase_vjp<")
    for leaf, b in zip(leaves, bare):
        assert torch.equal(leaf.grad, b)
    check(c, bare, (True, True), "bare")
    check(c, [leaf.grad for leaf in leaves], (True, True), "backward")
    exact_values(c, bare)
    eng.check_range()


# ---- 1 - 3. parity, exact values, the forward under autograd -------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NAMED)
def test_parity_with_float64_autograd(name, B):
    run_case(name, B)


@pytest.mark.parametrize("name", GRID)
def test_parity_on_the_round_boundaries_of_the_lane_map(name):
    """T in {2, 3, 5, 63, 64, 65}: below, at and one past a round of 64 lanes (and ProMP's differences at the horizon's ends)"""
    for B in BATCHES:
        run_case(name, B)


@pytest.mark.parametrize("name", ["promp_d3_t5", "prodmp_d3_t5"])
def test_batch_wraps_around_the_grid(name):
    """every wave of the capped grid takes at least two episodes, the last trip part full"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * WAVES_PER_WG * WG_PER_CU * cus + 3
    c = case(name, B)
    eng = engine_of(name)
    bare = eng.trajectory_phase_vjp(dev(c["params"]), dev(c["ip"]), dev(c["iv"]), dev(c["g_pos"]), dev(c["g_vel"]), it_arg(c))
    check(c, bare, (True, True), "wrap")
    exact_values(c, bare)


# ---- 4. NULL handling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tt_prodmp", "beerpong_promp", "promp_5dof_learn_both", "cfg4_per_episode_init_time"])
def test_null_gradients_and_outputs(name):
    c = case(name, 3)
    eng = engine_of(name)
    params, ip, iv, g_pos, g_vel = (dev(c[k]) for k in ("params", "ip", "iv", "g_pos", "g_vel"))
    it = it_arg(c)
    full = eng.trajectory_phase_vjp(params, ip, iv, g_pos, g_vel, it)
    check(c, eng.trajectory_phase_vjp(params, ip, iv, None, g_vel, it), (False, True), "g_pos NULL")
    check(c, eng.trajectory_phase_vjp(params, ip, iv, g_pos, None, it), (True, False), "g_vel NULL")
    for i in range(3):
        need = tuple(j != i for j in range(3))
        sentinel = [torch.full_like(x, 7.0) for x in full]
        got = eng.trajectory_phase_vjp(params, ip, iv, g_pos, g_vel, it, need=need, out=[s if n else None for s, n in zip(sentinel, need)])
        torch.cuda.synchronize()
        assert got[i] is None and (sentinel[i] == 7.0).all()
        for j in range(3):
            if j != i:
                assert got[j] is sentinel[j] and torch.equal(got[j], full[j])
    with pytest.raises(ValueError):
        eng.trajectory_phase_vjp(params, ip, iv, None, None, it)


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tt_prodmp", "beerpong_promp", "promp_d7_t65"])
def test_same_bits_run_to_run_and_for_any_alignment(name):
    c = case(name, 3)
    eng = engine_of(name)
    params, ip, iv = (dev(c[k]) for k in ("params", "ip", "iv"))
    it = it_arg(c)
    first = eng.trajectory_phase_vjp(params, ip, iv, dev(c["g_pos"]), dev(c["g_vel"]), it)
    again = eng.trajectory_phase_vjp(params, ip, iv, dev(c["g_pos"]), dev(c["g_vel"]), it)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    n = c["g_pos"].size
    for off in (1, 2, 3):
        views = []
        for g in (c["g_pos"], c["g_vel"]):
            buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
            base = (16 - buf.data_ptr() % 16) % 16 // 4
            view = buf[base + off: base + off + n].view(g.shape)
            view.copy_(dev(g))
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            views.append(view)
        for a, b in zip(first, eng.trajectory_phase_vjp(params, ip, iv, views[0], views[1], it)):
            assert torch.equal(a, b)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = case("tt_prodmp", 3)
    eng = engine_of("tt_prodmp")
    params, ip, iv = (dev(c[k]) for k in ("params", "ip", "iv"))
    p = params.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="shared phase only"):
        eng.trajectory(p, ip, iv)
    with pytest.raises(ValueError, match="phase_gradient"):
        eng.trajectory(p, ip, iv, phase_gradient="finite_difference")
    c4 = case("cfg4_per_episode_init_time", 3)
    eng4 = engine_of("cfg4_per_episode_init_time")
    p4 = dev(c4["params"]).clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="one init_time shared by the batch"):
        eng4.trajectory(p4, dev(c4["ip"]), dev(c4["iv"]), dev(c4["it"]))
    # ... and a shared-phase call with a float init_time keeps mpk_trajectory_vjp's kernels under the option
    pos, vel = eng4.trajectory(p4, dev(c4["ip"]), dev(c4["iv"]), 0.4, phase_gradient="pathwise")
    (pos.sum() + vel.sum()).backward()
    assert eng4.last_kernel().startswith("k_traj_vjp_"), eng4.last_kernel()
    # a DMP that learns tau
    pc = O.PhaseCfg("exp", tau=2.0, alpha_phase=2.0, learn_tau=True, tau_bound=(1.0, 2.0))
    bc, tc = O.BasisCfg("rbf", num_basis=5, basis_bandwidth_factor=3), O.TrajCfg("dmp", action_dim=5, alpha=25.0)
    dmp = make_engine(pc, bc, tc, 0.02, 2.0, device=0)
    pd = torch.ones((2, dmp.num_params), device="cuda", requires_grad=True)
    z = torch.zeros((2, 5), device="cuda")
    with pytest.raises(NotImplementedError, match="DMP"):
        dmp.trajectory(pd, z, z, phase_gradient="pathwise")
    with pytest.raises(NotImplementedError, match="DMP"):
        dmp.trajectory_phase_vjp(pd.detach(), z, z, torch.ones((2, dmp.num_steps, 5), device="cuda"), None)
    with pytest.raises(NotImplementedError, match="shared phase only"):
        dmp.trajectory(pd, z, z)


def _box(name, B, **kw):
    from tests.test_gpu_learned_phase import _bb
    return _bb(name, B, **kw)


def test_black_box_refusals():
    with pytest.raises(ValueError, match="phase_gradient"):
        _box("tt_prodmp", 2, phase_gradient="frozen")
    with pytest.raises(NotImplementedError, match="learn_sub_trajectories"):
        _box("tt_prodmp", 2, phase_gradient="pathwise", learn_sub_trajectories=True)
    box = _box("tt_prodmp", 2)
    box.reset()
    p = torch.ones((2, box.engine.num_params), device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="shared phase only"):
        box.get_trajectory(p)
    with pytest.raises(NotImplementedError):
        _box("tt_prodmp", 2, phase_gradient="pathwise").step(p, differentiable=True)


# ---- 7. BatchedBlackBox ----------------------------------------------------------------------------------------------------------------
def test_black_box_get_trajectory_keeps_the_graph():
    B = 5
    c = case("tt_prodmp", B)
    box = _box("tt_prodmp", B, phase_gradient="pathwise")
    box.reset()
    raw = dev(c["params"]).clone().requires_grad_(True)
    traj = box.get_trajectory(raw)
    assert traj["des_pos"].requires_grad and traj["des_vel"].requires_grad
    g_pos, g_vel = dev(c["g_pos"]), dev(c["g_vel"])
    torch.autograd.backward((traj["des_pos"], traj["des_vel"]), (g_pos, g_vel))
    assert box.engine.last_kernel().startswith("k_phase_vjp<")
    cond_pos = box.condition_pos if box.condition_pos is not None else box.q.float()
    cond_vel = box.condition_vel if box.condition_vel is not None else box.qd.float()
    bare = box.engine.trajectory_phase_vjp(traj["params"].detach(), cond_pos, cond_vel, g_pos, g_vel, 0.0)[0]
    # the box clamps the phase columns itself before the plan (the frozen phase): rows it clipped get exactly 0 there, as in the kernel
    assert torch.equal(raw.grad[:, 2:], bare[:, 2:])
    inside = ((raw[:, :2] >= traj["params"][:, :2]) & (raw[:, :2] <= traj["params"][:, :2])).detach()
    assert torch.equal(raw.grad[:, :2], torch.where(inside, bare[:, :2], torch.zeros_like(bare[:, :2])))
    assert (raw.grad[:2, 0] == 0.0).all() and (raw.grad[:, 1] == 0.0).all() and (raw.grad[2:, 0] != 0.0).any()


# ---- 8. the example's loop ---------------------------------------------------------------------------------------------------------------
def test_the_example_fits_weights_and_tau():
    """examples/batched_timing_fit.py's loop at B = 8 for 50 Adam steps (lr 0.05) on demonstrations from the float64 restatement: the loss
    falls (0.4000 -> 4.6015e-3), and the final loss of the device loop agrees with the same loop on the CPU float32 restatement to 4 x
    the relative gap between the CPU float32 and float64 loops, measured here first.  That gap, measured on the CPU: 4.6e-7 (device against the CPU float32 loop: 1.0e-7)."""
    spec = importlib.util.spec_from_file_location("batched_timing_fit", os.path.join(ROOT, "examples", "batched_timing_fit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    pc = O.PhaseCfg("linear", tau=3.0, learn_tau=True, tau_bound=ex.TAU_BOUND)
    bc = O.BasisCfg("zero_rbf", num_basis=2, num_basis_zero_start=2, num_basis_zero_goal=0, basis_bandwidth_factor=3)
    tc, dt, dur = O.TrajCfg("promp", action_dim=7), 0.01, 3.0
    B, iters, lr = 8, 50, 0.05
    demo, ip = ex.demo_parameters(B, 0)
    with torch.no_grad():
        d64, ip64 = torch.from_numpy(demo.astype(np.float64)), torch.from_numpy(ip.astype(np.float64))
        want = R.trajectory(pc, bc, tc, d64, ip64, torch.zeros_like(ip64), 0.0, dt, dur)

    def cpu_loop(dtype):
        ipt = torch.from_numpy(ip).to(dtype)
        th0 = torch.zeros((B, demo.shape[1]), dtype=dtype)
        th0[:, 0] = ex.TAU_START
        return ex.fit_loop(lambda th: R.trajectory(pc, bc, tc, th, ipt, torch.zeros_like(ipt), 0.0, dt, dur, dtype), th0,
                           want[0].to(dtype), want[1].to(dtype), iters, lr)[1]

    start = np.zeros_like(demo)
    start[:, 0] = ex.TAU_START
    assert R.phase_clip_margin(pc, start, 0.0, dt, dur) >= 1e-4       # (at a step ON the clip torch.clamp passes the gradient, the kernel does not)
    l64, l32 = cpu_loop(torch.float64), cpu_loop(torch.float32)
    gap = abs(l32[-1] - l64[-1]) / l64[-1]
    eng = ex.make_engine()
    ipd = dev(ip)
    th0 = torch.zeros((B, demo.shape[1]), device="cuda")
    th0[:, 0] = ex.TAU_START
    theta, lg = ex.fit_loop(lambda th: eng.trajectory(th, ipd, torch.zeros_like(ipd), phase_gradient="pathwise"), th0,
                            want[0].float().cuda(), want[1].float().cuda(), iters, lr)
    diff = abs(lg[-1] - l32[-1]) / l32[-1]
    print(f"[phase_vjp] example: loss {lg[0]:.6e} -> {lg[-1]:.6e} (cpu f32 {l32[-1]:.6e}, cpu f64 {l64[-1]:.6e}); "
          f"gap f32 / f64 {gap:.3e}, device against cpu f32 {diff:.3e}")
    assert lg[-1] < 0.05 * lg[0]
    assert diff <= 4.0 * gap, (diff, gap)
