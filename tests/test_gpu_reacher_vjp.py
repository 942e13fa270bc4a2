"""
mpk_reacher_rollout_vjp, the autograd wiring of TrajectoryEngine.reacher_rollout and BatchedBlackBox.step(differentiable=True) on the GPU.

Yardstick: torch autograd of the float64 CPU restatement of oracle.reacher_rollout (tests/reacher_vjp_ref.py; it agrees with a
hand-written numpy reverse sweep to delta_ref <= 1e-15, the cases appended later to <= 5.2e-15, tests/test_reacher_vjp_host.py).  Bounds per
output array:
  float64 outputs (g_q0, g_qd0, g_goal)   |gpu - ref| <= 1e-12 max|ref|   -- the project's contract for device against host float64
                                          with cos / sin (README parity row); two to three orders of magnitude above delta_ref
  float32 outputs (g_des_pos, g_des_vel)  |gpu - ref| <= 2^-24 |ref| + 1e-12 max|ref|   -- one rounding of the float64 result
Every comparison prints its maximum before it asserts.
"""
import functools
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch

from . import reacher_vjp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTRL_CASES = R.CTRL_CASES


@functools.lru_cache(maxsize=None)
def engine(D, T, dt):
    from fancy_gym_amd import TrajectoryEngine
    return TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=3, dt=dt,
                            duration=T * dt, tau=T * dt)


def spec_of(c):
    from fancy_gym_amd import RolloutSpec
    return RolloutSpec(c["controller"], c["D"], c["pg"], c["dg"], c["lo"], c["hi"], plant="double_integrator", dt=c["dt"])


def dev(x):
    return torch.tensor(np.asarray(x), device="cuda")


def launch(c, use=(True, True, True), need=(True,) * 5, out=None, des=None):
    """the bare product on the device for a case; ``des``: (des_pos, des_vel) device tensors that replace the case's"""
    eng = engine(c["D"], c["T"], c["dt"])
    dp, dv = des if des is not None else (dev(c["des_pos"]), dev(c["des_vel"]))
    res = eng.reacher_rollout_vjp(spec_of(c), dp, dv, dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]), dev(c["g_r"]) if use[0] else None,
                                  g_q=dev(c["g_q"]) if use[1] else None, g_qd=dev(c["g_qd"]) if use[2] else None,
                                  n_steps=dev(c["n_steps"]), step0=dev(c["step0"]), steps_before_reward=c["sbr"], need=need, out=out)
    return res, eng


def check(name, got, ref):
    """the module docstring's bounds; returns the printed maxima"""
    worst = {}
    for k in R.OUTPUTS:
        g, r = got[k], ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        scale = np.abs(r).max()
        err = np.abs(g.astype(np.float64) - r)
        bound = 1e-12 * scale + (2.0 ** -24 * np.abs(r) if g.dtype == np.float32 else 0.0)
        worst[k] = float(err.max() / scale) if scale > 0 else float(err.max())
        print(f"{name} {k}: max |gpu - ref| / max|ref| = {worst[k]:.3e}  (max excess over the bound {np.max(err - bound):.3e})")
    for k in R.OUTPUTS:
        g, r = got[k], ref[k]
        scale = np.abs(r).max()
        err = np.abs(g.astype(np.float64) - r)
        bound = 1e-12 * scale + (2.0 ** -24 * np.abs(r) if g.dtype == np.float32 else 0.0)
        assert np.all(err <= bound), (name, k, worst[k])
    return worst


@pytest.mark.parametrize("name,controller", CTRL_CASES)
def test_against_the_float64_reference(name, controller):
    c = R.make_case(name, controller)
    res, eng = launch(c)
    assert eng.last_kernel() == R.kernel_name(c)          # <ctrl, 2 | 5 | 7>, or <ctrl> alone: the run-time-D instantiation
    full = {k: v.cpu().numpy() for k, v in zip(R.OUTPUTS, res)}
    n = R.compared(c)
    check(f"{name} {controller}", {k: v[:n] for k, v in full.items()}, R.reference(name, controller))
    # rows behind the executed steps are exact zeros; an episode that executes nothing passes g_q, g_qd through unchanged
    dead = np.arange(c["T"])[None] >= c["n_steps"][:, None]
    assert dead.any() and not full["g_des_pos"][dead].any() and not full["g_des_vel"][dead].any()
    idle = c["n_steps"] == 0
    assert np.array_equal(full["g_q0"][idle], c["g_q"][idle]) and np.array_equal(full["g_qd0"][idle], c["g_qd"][idle])
    if c["B"] > R.SUBSET:
        # several workgroups: the whole launch is the same bits a second time
        again, _ = launch(c)
        for a, b in zip(res, again):
            assert torch.equal(a, b)
        assert idle.any() and np.isfinite(full["g_des_pos"]).all() and np.isfinite(full["g_goal"]).all()


def test_adjoint_identity_against_the_device_forward():
    """<g_des_pos, v> against the central difference of the DEVICE forward's sum g_r r along v, no reference gradient involved.  des_pos
    is put on a 2^-16 grid and v in {-1, 0, 1}, so des_pos +- eps v is exact in float32 for every eps of the sweep.  eps: the LARGEST
    power of two at which the CPU restatement's own central difference agrees with its <g, v> to 1e-6 relative -- there the difference
    is dominated by the truncation term, which device and host share, not by the rounding of either forward (~1e-16 / eps); the device
    must then agree to 10 x what the CPU achieves at that eps."""
    base = R.make_case("b5_t35_d2")
    rng = np.random.default_rng(5)
    dp = (np.round(base["des_pos"].astype(np.float64) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
    c = dict(base, des_pos=dp)
    v = rng.integers(-1, 2, dp.shape).astype(np.float32)
    use = (True, False, False)
    gv_ref = float((R.autograd(c, use)["g_des_pos"] * v).sum())
    eps = err_cpu = None
    for k in range(2, 15):
        e = 2.0 ** -k
        for s in (1.0, -1.0):
            assert np.array_equal((dp + np.float32(s * e) * v).astype(np.float64), dp.astype(np.float64) + s * e * v)
        cd = (R.loss_value(c, dp + np.float32(e) * v, use) - R.loss_value(c, dp - np.float32(e) * v, use)) / (2.0 * e)
        rel = abs(cd - gv_ref) / abs(gv_ref)
        print(f"eps = 2^-{k}: CPU central difference off by {rel:.3e}")
        if rel <= 1e-6:
            eps, err_cpu = e, rel
            break
    assert eps is not None, "no eps of the sweep reaches 1e-6 on the CPU reference"
    eng = engine(c["D"], c["T"], c["dt"])

    def device_loss(pos):
        q, qd = dev(c["q0"]), dev(c["qd0"])
        _, rew = eng.reacher_rollout(spec_of(c), dev(pos), dev(c["des_vel"]), q, qd, dev(c["goal"]), n_steps=dev(c["n_steps"]),
                                     step0=dev(c["step0"]), steps_before_reward=c["sbr"], want_actions=False)
        return float((c["g_r"] * rew.cpu().numpy()).sum())

    cd_gpu = (device_loss(dp + np.float32(eps) * v) - device_loss(dp - np.float32(eps) * v)) / (2.0 * eps)
    res, _ = launch(c, use=use, need=(True, False, False, False, False))
    gv_gpu = float((res[0].cpu().numpy().astype(np.float64) * v).sum())
    rel = abs(cd_gpu - gv_gpu) / abs(gv_gpu)
    print(f"eps = {eps}: CPU {err_cpu:.3e}, device |cd - <g, v>| / |<g, v>| = {rel:.3e} (bound {10 * err_cpu:.3e})")
    assert rel <= 10.0 * err_cpu


def test_null_inputs_and_outputs():
    """every combination of absent upstream gradients and unrequested outputs: what is written is the bits of the full launch with the
    same upstream gradients (and matches the reference), what is not requested stays untouched -- the five outputs lie side by side in
    one NaN-filled arena"""
    c = R.make_case("b7_t33_d7_clipped")
    B, T, D = c["B"], c["T"], c["D"]
    sizes = [B * T * D, B * T * D, 2 * B * D, 2 * B * D, 2 * B * 2]          # in floats (float64 outputs: two each)
    offs = np.concatenate([[4], 4 + np.cumsum([s + 4 for s in sizes])])     # four canary floats around every output
    arena = torch.empty(int(offs[-1]), dtype=torch.float32, device="cuda")
    shapes = [(B, T, D), (B, T, D), (B, D), (B, D), (B, 2)]

    def views():
        out = []
        for i, shape in enumerate(shapes):
            v = arena[int(offs[i]):int(offs[i]) + sizes[i]]
            out.append(v.view(shape) if i < 2 else v.view(torch.float64).view(shape))
        return out

    for use in itertools.product((True, False), repeat=3):
        full, _ = launch(c, use=use)
        full = [x.clone() for x in full]
        if any(use):
            ref = R.autograd(c, use)
            check(f"upstream {use}", {k: v.cpu().numpy() for k, v in zip(R.OUTPUTS, full)}, ref)
        else:
            assert not any(bool(x.any()) for x in full)
        for need in itertools.product((True, False), repeat=5):
            arena.fill_(float("nan"))
            vs = views()
            res, _ = launch(c, use=use, need=need, out=[v if n else None for v, n in zip(vs, need)])
            mask = torch.zeros_like(arena, dtype=torch.bool)
            for i, n in enumerate(need):
                if n:
                    assert res[i] is vs[i] and torch.equal(res[i], full[i]), (use, need, R.OUTPUTS[i])
                    mask[int(offs[i]):int(offs[i]) + sizes[i]] = True
                else:
                    assert res[i] is None
            assert bool(torch.isnan(arena[~mask]).all()), (use, need)


def test_autograd_through_reacher_rollout():
    autograd_through_reacher_rollout("b7_t33_d7_clipped")


def test_autograd_through_reacher_rollout_at_a_run_time_dof_count():
    assert R.kernel_name(R.make_case("b23_t40_d3")) == "k_reacher_rollout_vjp<motor>"
    autograd_through_reacher_rollout("b23_t40_d3")


def autograd_through_reacher_rollout(name):
    c = R.make_case(name)
    eng, spec = engine(c["D"], c["T"], c["dt"]), spec_of(c)
    kw = dict(n_steps=dev(c["n_steps"]), step0=dev(c["step0"]), steps_before_reward=c["sbr"])

    def run(dp, dv, goal, **extra):
        q, qd = dev(c["q0"]), dev(c["qd0"])
        act, rew = eng.reacher_rollout(spec, dp, dv, q, qd, goal, **kw, **extra)
        return act, rew, q, qd

    act0, rew0, q0, qd0 = run(dev(c["des_pos"]), dev(c["des_vel"]), dev(c["goal"]))
    assert rew0.grad_fn is None and not rew0.requires_grad
    dp, dv, goal = dev(c["des_pos"]).requires_grad_(), dev(c["des_vel"]).requires_grad_(), dev(c["goal"]).requires_grad_()
    before = eng.last_kernel()
    act, rew, q, qd = run(dp, dv, goal)
    assert eng.last_kernel() == before                    # the forward launch is the plain call's
    assert rew.grad_fn is not None and torch.equal(rew, rew0) and torch.equal(act, act0) and not act.requires_grad
    assert torch.equal(q, q0) and torch.equal(qd, qd0) and not q.requires_grad and not qd.requires_grad
    g_r = dev(c["g_r"])
    (g_r * rew).sum().backward()
    assert eng.last_kernel() == R.kernel_name(c)
    bare, _ = launch(c, use=(True, False, False))
    assert torch.equal(dp.grad, bare[0]) and torch.equal(dv.grad, bare[1]) and torch.equal(goal.grad, bare[4])
    assert bool(dp.grad.any()) and bool(goal.grad.any())
    # needs_input_grad: only des_pos requires grad
    dp2 = dev(c["des_pos"]).requires_grad_()
    _, rew2, _, _ = run(dp2, dev(c["des_vel"]), dev(c["goal"]), want_actions=False)
    (g_r * rew2).sum().backward()
    assert torch.equal(dp2.grad, bare[0])
    # without requires_grad, and under no_grad: no graph, out= is honoured
    bufs = (torch.empty_like(act0), torch.empty_like(rew0))
    a3, r3, _, _ = run(dev(c["des_pos"]), dev(c["des_vel"]), dev(c["goal"]), out=bufs)
    assert a3 is bufs[0] and r3 is bufs[1] and r3.grad_fn is None and torch.equal(r3, rew0)
    with torch.no_grad():
        bufs = (torch.empty_like(act0), torch.empty_like(rew0))
        a4, r4, _, _ = run(dp, dv, goal, out=bufs)
    assert a4 is bufs[0] and r4 is bufs[1] and r4.grad_fn is None and not r4.requires_grad and torch.equal(r4, rew0)


@pytest.mark.parametrize("id", ["fancy_ProDMP/LongSimpleReacher-v0", "fancy_ProMP/LongSimpleReacher-v0", "fancy_DMP/LongSimpleReacher-v0"])
def test_batched_black_box_differentiable_step(id):
    from fancy_gym_amd import make_batched
    B = 8
    bb, twin, plain = (make_batched(id, B, verbose=2) for _ in range(3))
    for x in (bb, twin, plain):
        x.reset(seed=11)
    gen = torch.Generator(device="cpu").manual_seed(3)
    theta = (0.5 * torch.randn((B, bb.engine.num_params), generator=gen)).cuda()
    params = theta.clone().requires_grad_()
    start = (bb.q.clone(), bb.qd.clone())
    out = bb.step(params, differentiable=True)
    want = twin.step(theta, fuse=False)
    assert out["rewards"].grad_fn is not None and out["step_rewards"].grad_fn is not None
    for k, v in want.items():
        assert torch.equal(out[k].detach(), v), k
        if v.dtype not in (torch.float32, torch.float64):
            assert out[k].dtype == v.dtype
    assert torch.equal(bb.q, twin.q) and torch.equal(bb.qd, twin.qd) and torch.equal(bb.traj_steps, twin.traj_steps)
    w = torch.linspace(0.5, 1.5, B, dtype=torch.float64, device="cuda")
    (w * out["rewards"]).sum().backward()
    assert bb.engine.last_kernel().startswith("k_traj_vjp")          # the second launch of the backward
    # the chain of the two bare products
    seg = out["trajectory_length"]
    t = torch.arange(bb.T, device="cuda").view(1, -1)
    g_rewards = torch.where(t < seg.view(-1, 1), w.view(-1, 1), torch.zeros((), dtype=torch.float64, device="cuda"))
    gp, gv, _, _, _ = bb.engine.reacher_rollout_vjp(bb.spec, out["des_pos"].detach(), out["des_vel"].detach(), start[0], start[1], bb.goal,
                                                    g_rewards, n_steps=seg, step0=bb.traj_steps - seg,
                                                    steps_before_reward=bb.steps_before_reward, need=(True, True, False, False, False))
    chain = bb.engine.trajectory_vjp(gp, gv, 0.0, need=(True, False, False))[0]
    assert torch.equal(params.grad, chain) and bool(params.grad.any())
    # the default step with parameters that require grad: as before, nothing carries a graph
    p2 = theta.clone().requires_grad_()
    res = plain.step(p2)
    assert res["rewards"].grad_fn is None and not res["rewards"].requires_grad
    assert res["step_rewards"].grad_fn is None
    assert torch.equal(res["rewards"], want["rewards"]) and torch.equal(plain.q, twin.q)


def test_batched_black_box_mean_and_last_aggregation_values_and_gradients():
    """the differentiable aggregation is mpk_reward_aggregate's value bit for bit, and its gradient is g / seg (mean) or the last-step
    indicator (last)"""
    c = R.make_case("b7_t33_d7_clipped")
    eng = engine(c["D"], c["T"], c["dt"])
    seg = dev(c["n_steps"])
    for agg in ("sum", "mean", "last"):
        rew = dev(c["g_r"]).clone().requires_grad_()
        ret = eng.reward_aggregate(rew, seg, agg)
        with torch.no_grad():
            assert torch.equal(ret, eng.reward_aggregate(rew.detach(), seg, agg))
        w = torch.arange(1, c["B"] + 1, dtype=torch.float64, device="cuda")
        (w * ret).sum().backward()
        t = np.arange(c["T"])[None]
        n = c["n_steps"][:, None]
        wn = w.cpu().numpy()[:, None]
        exp = {"sum": np.where(t < n, wn, 0.0), "mean": np.where(t < n, wn / np.maximum(n, 1), 0.0),
               "last": np.where(t == n - 1, wn, 0.0)}[agg]
        assert np.array_equal(rew.grad.cpu().numpy(), exp), agg


def test_batched_black_box_refusals():
    from fancy_gym_amd import make_batched
    bb = make_batched("fancy_ProMP/HoleReacher-v0", 4)
    bb.reset(seed=1)
    with pytest.raises(NotImplementedError, match="simple_reacher"):
        bb.step(torch.zeros((4, bb.engine.num_params), device="cuda"), differentiable=True)
    bb = make_batched("fancy_ProDMP/LongSimpleReacher-v0", 4)
    bb.reset(seed=1)
    bb.pos_limits = (np.full(5, -10.0), np.full(5, 10.0))
    with pytest.raises(NotImplementedError, match="pos_limits"):
        bb.step(torch.zeros((4, bb.engine.num_params), device="cuda"), differentiable=True)
    bb.pos_limits = None
    bb._n_phase = 1
    with pytest.raises(NotImplementedError, match="learned tau"):
        bb.step(torch.zeros((4, bb.engine.num_params), device="cuda"), differentiable=True)
    bb._n_phase = 0
    bb.do_replanning, bb._lockstep = True, None
    with pytest.raises(NotImplementedError, match="init_time"):
        bb.step(torch.zeros((4, bb.engine.num_params), device="cuda"), differentiable=True)
    # the C entry point names its limits
    from fancy_gym_amd import RolloutSpec, TrajectoryEngine
    wide = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=17, num_basis=3, dt=0.01,
                            duration=0.04, tau=0.04)
    z = torch.zeros((1, 4, 17), device="cuda")
    s = torch.zeros((1, 17), dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="at most 16"):
        wide.reacher_rollout_vjp(RolloutSpec("motor", 17, plant="double_integrator", dt=0.01), z, z, s, s, torch.zeros((1, 2)), None)
    long = engine(2, 2200, 0.01)
    z = torch.zeros((1, 2200, 2), device="cuda")
    s = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="checkpoints"):
        long.reacher_rollout_vjp(RolloutSpec("motor", 2, plant="double_integrator", dt=0.01), z, z, s, s, torch.zeros((1, 2)), None)


@pytest.mark.parametrize("D", [5, 1])
def test_horizon_limit_is_the_one_the_refusal_names(D):
    """T = 2000 is accepted (the long cases above); T = 2200 is refused, and the refusal names the largest T the checkpoints fit: a
    launch at exactly that T -- the whole LDS of a CU but for less than 1 KB -- returns and matches the reference, T + 1 is refused.
    The limit is taken from the message on purpose: the message, the LDS carve and the launch have to agree."""
    def zeros(T):
        z = torch.zeros((2, T, D), device="cuda")
        s = torch.zeros((2, D), dtype=torch.float64, device="cuda")
        return z, z, s, s, torch.zeros((2, 2), dtype=torch.float64, device="cuda"), None

    from fancy_gym_amd import RolloutSpec
    spec = RolloutSpec("motor", D, np.full(D, 0.6), 0.075 + 0.01 * np.arange(D), -1000.0, 1000.0, plant="double_integrator", dt=0.01)
    with pytest.raises(NotImplementedError, match=r"at most \d+ steps") as info:
        engine(D, 2200, 0.01).reacher_rollout_vjp(spec, *zeros(2200))
    limit = int(re.search(r"at most (\d+) steps", str(info.value)).group(1))
    print(f"D = {D}: the refusal at T = 2200 names at most {limit} steps")
    assert 2000 <= limit < 2200
    c = dict(R.recipe(f"limit_d{D}", (2, limit, D, -1000.0, 1000.0, limit - 10, 0.01), "motor", 4242 + D, 0))
    c["n_steps"] = np.array([limit, 17], np.int32)
    res, eng = launch(c)
    assert eng.last_kernel() == R.kernel_name(c)
    got = {k: v.cpu().numpy() for k, v in zip(R.OUTPUTS, res)}
    assert all(np.isfinite(v).all() for v in got.values())
    check(f"T = {limit} D = {D}", got, R.autograd(c))
    assert not got["g_des_pos"][1, 17:].any() and not got["g_des_vel"][1, 17:].any()
    cond = R.conditions(c)
    assert cond["n_paid"] > 0 and cond["min_dist"] > 1e-3 and cond["saturated"] == 0.0 and cond["bound_gap"] >= 1e-9
    with pytest.raises(NotImplementedError, match=f"at most {limit} steps"):
        engine(D, limit + 1, 0.01).reacher_rollout_vjp(spec, *zeros(limit + 1))


def test_a_paid_step_at_the_goal_contributes_no_distance_term():
    """include/mpk.h: "A paid step with dist = 0 contributes no distance term".  Episode 0 sits on its goal at every step (one link,
    position controller, des_pos = q0 = qd0 = 0, goal = (1, 0): q' = 0, the end effector is (cos 0, sin 0)); episode 1 is an ordinary
    row of the recipe in the same wave (reacher_vjp_ref.at_the_goal).  Reference: numpy_sweep, whose paid weight is 0 where dist == 0
    (autograd divides by dist)."""
    c = R.at_the_goal()               # (what the reference gives here: tests/test_reacher_vjp_host.py)
    ref = R.numpy_sweep(c)
    # the device forward at the same inputs: reward = -dist - a^2, so an exact 0 says dist == 0 there too (printed, not required)
    eng = engine(1, 20, 0.1)
    _, rew = eng.reacher_rollout(spec_of(c), dev(c["des_pos"]), dev(c["des_vel"]), dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]),
                                 n_steps=dev(c["n_steps"]), step0=dev(c["step0"]), steps_before_reward=0, want_actions=False)
    print(f"device forward, episode 0: max |reward| = {float(rew[0].abs().max()):.3e} (0: dist is exactly 0 on the device)")
    res, eng = launch(c)
    assert eng.last_kernel() == "k_reacher_rollout_vjp<position>"
    got = {k: v.cpu().numpy() for k, v in zip(R.OUTPUTS, res)}
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["g_goal"][0], np.zeros(2))
    check("dist = 0", got, ref)
    for e in (0, 1):
        check(f"dist = 0, episode {e}", {k: v[e:e + 1] for k, v in got.items()}, {k: v[e:e + 1] for k, v in ref.items()})


def test_layout_and_determinism():
    """input and output pointers 4 and 8 bytes off a 16-byte boundary: the same bits; two runs: the same bits -- at a compiled-in DoF
    count and at a run-time one with an idle lane and a part-full last wave"""
    for name in ("b5_t35_d5_clipped_all_paid", "b23_t40_d3"):
        layout_and_determinism(R.make_case(name))


def layout_and_determinism(c):
    B, T, D = c["B"], c["T"], c["D"]
    base, _ = launch(c)
    again, _ = launch(c)
    for a, b in zip(base, again):
        assert torch.equal(a, b)
    n = B * T * D
    for shift in (1, 2):                      # floats
        def shifted(x=None):
            buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v = buf[shift:shift + n].view(B, T, D)
            if x is not None:
                v.copy_(dev(x))
            assert v.data_ptr() % 16 == 4 * shift and v.is_contiguous()
            return buf, v
        (_, dp), (_, dv) = shifted(c["des_pos"]), shifted(c["des_vel"])
        (bp, gp), (bv, gv) = shifted(), shifted()
        res, eng = launch(c, des=(dp, dv), out=[gp, gv, None, None, None])
        assert eng.last_kernel() == R.kernel_name(c)
        assert res[0].data_ptr() == gp.data_ptr() and res[1].data_ptr() == gv.data_ptr()
        for a, b in zip(base, res):
            assert torch.equal(a, b), shift
        for buf in (bp, bv):                  # nothing written around the shifted outputs
            assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + n:]).all())


def test_example_improves_the_mean_return():
    path = os.path.join(ROOT, "examples", "batched_reacher_gradient.py")
    spec = importlib.util.spec_from_file_location("batched_reacher_gradient", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.optimise(envs=64, iters=30, seed=0, verbose=False)
    print(f"mean return {first:.4f} -> {last:.4f}")
    assert last > first
