"""
mpk_episode_return_vjp, the autograd wiring of TrajectoryEngine.episode_return(differentiable=True) and BatchedBlackBox.step(params,
differentiable=True) at the default verbosity on the GPU.

Yardstick: the composed float64 reference of tests/episode_vjp_ref.py, linearised at the DEVICE's own float32 plan (mpk_trajectory's
output for the same inputs, so that clip masks are decided on the same numbers); tests/test_episode_return_vjp_host.py measures its
agreement with torch autograd of the whole float64 chain (delta_ref <= 1e-14).  Bounds per output array (episode_vjp_ref.check):
  g_q0, g_qd0, g_goal                 |gpu - ref| <= 1e-12 max|ref|     -- the project's float64 contract
  g_params, g_init_pos, g_init_vel    |gpu - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the reference's float32-einsum error)
                                      -- the rule of tests/test_gpu_traj_vjp.py: the table rows are float32
Every comparison prints its maxima before it asserts.
"""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from . import episode_vjp_ref as E
from . import reacher_vjp_ref as R
from .test_gpu_trajectory import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = E.X_OUTPUTS + E.S_OUTPUTS + ("q_end", "qd_end")
ALL = (True,) * 8


@functools.lru_cache(maxsize=None)
def engine(mp, D, T, tau=1.0):
    pc, bc, tc = E.mp_config(mp, D, tau)
    eng = make_engine(pc, bc, tc, E.DT_PLAN, T * E.DT_PLAN)
    assert eng.num_steps == T
    return eng


def spec_of(c):
    from fancy_gym_amd import RolloutSpec
    return RolloutSpec(c["controller"], c["D"], c["pg"], c["dg"], c["lo"], c["hi"], plant="double_integrator", dt=c["dt"])


def dev(x):
    return torch.tensor(np.asarray(x), device="cuda")


def kernel_name(c):
    mp = "dmp_resp" if c["mp"] == "dmp" else c["mp"]
    return f"k_episode_return_vjp<{mp}, {c['controller']}" + (f", {c['D']}>" if c["D"] in R.COMPILED_D else ">")


def launch(c, agg="sum", use=(True, True, True), need=ALL, out=None, params=None):
    """the bare product on the device for a case -> (dict of the needed outputs, engine)"""
    eng = engine(c["mp"], c["D"], c["T"])
    res = eng.episode_return_vjp(dev(c["params"]) if params is None else params, dev(c["init_pos"]), dev(c["init_vel"]), spec_of(c),
                                 dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]), dev(c["g_ret"]) if use[0] else None,
                                 g_q=dev(c["g_q"]) if use[1] else None, g_qd=dev(c["g_qd"]) if use[2] else None,
                                 n_steps=dev(c["n_steps"]), step0=dev(c["step0"]), steps_before_reward=c["sbr"], aggregation=agg,
                                 need=need, out=out)
    return dict(zip(NAMES, res)), eng


def device_plan(c):
    eng = engine(c["mp"], c["D"], c["T"])
    pos, vel = eng.trajectory(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]))
    return pos, vel


@functools.lru_cache(maxsize=None)
def reference(name, agg="sum", use=(True, True, True)):
    """the composed float64 reference of a case at the device's plan, computed once and shared; read-only"""
    c = E.make_case(name)
    pos, vel = device_plan(c)
    dp, dv = pos.cpu().numpy(), vel.cpu().numpy()
    ref, e32 = E.composed(c, dp, dv, agg, use)
    for v in list(ref.values()) + list(e32.values()):
        v.setflags(write=False)
    return ref, e32, R.conditions(E.rollout_case(c, dp, dv, agg))


def host(res):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


# ---- 1. against the float64 reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.CASES))
def test_against_the_float64_reference(name):
    c = E.make_case(name)
    agg = E.AGGS[list(E.CASES).index(name) % 3]
    res, eng = launch(c, agg)
    assert eng.last_kernel() == kernel_name(c), eng.last_kernel()
    ref, e32, cond = reference(name, agg)
    print(f"{name} {agg}: {cond}")
    assert cond["bound_gap"] >= 1e-9 and cond["n_paid"] > 0 and cond["min_dist"] > 1e-3
    assert (cond["saturated"] > 0.0) == E.CASES[name][5]
    got = host(res)
    E.check(f"{name} {agg}", got, ref, e32)
    # an episode that executes nothing: exact zeros for the parameters, g_q / g_qd passed through, the state where it was
    idle = c["n_steps"] == 0
    for k in E.X_OUTPUTS:
        assert not got[k][idle].any(), k
    assert np.array_equal(got["g_q0"][idle], c["g_q"][idle]) and np.array_equal(got["g_qd0"][idle], c["g_qd"][idle])
    assert np.array_equal(got["q_end"][idle], c["q0"][idle]) and np.array_equal(got["qd_end"][idle], c["qd0"][idle])
    if c["mp"] == "promp":
        assert not got["g_init_vel"].any()                # (no column reads it: exact zeros)
    assert got["g_params"].any()


# ---- 2. against the two existing launches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("agg", E.AGGS)
def test_against_the_two_launches(agg, with_state):
    name = "prodmp_motor_d5_t17_b11_clipped" if with_state else "promp_motor_d7_t33_b8_clipped"
    c = E.make_case(name)
    eng = engine(c["mp"], c["D"], c["T"])
    use = (True, with_state, with_state)
    res, _ = launch(c, agg, use)
    pos, vel = device_plan(c)
    g_r = dev(E.step_reward_grads(c, agg))
    gp, gv, gq0, gqd0, ggoal = eng.reacher_rollout_vjp(spec_of(c), pos, vel, dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]), g_r,
                                                       g_q=dev(c["g_q"]) if with_state else None,
                                                       g_qd=dev(c["g_qd"]) if with_state else None, n_steps=dev(c["n_steps"]),
                                                       step0=dev(c["step0"]), steps_before_reward=c["sbr"])
    gx = eng.trajectory_vjp(gp, gv, 0.0)
    two = {k: v.cpu().numpy().astype(np.float64) for k, v in zip(E.X_OUTPUTS + E.S_OUTPUTS, tuple(gx) + (gq0, gqd0, ggoal))}
    _, e32, _ = reference(name, agg, use)
    E.check(f"{name} {agg} state={with_state} vs two launches", host(res), two, e32)
    for k in E.S_OUTPUTS:                                 # the float64 chain is the same chain
        assert torch.equal(res[k], dict(g_q0=gq0, g_qd0=gqd0, g_goal=ggoal)[k]), k


# ---- 3. the replay is the forward's bits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prodmp_motor_d5_t33_b13", "promp_motor_d7_t33_b8_clipped", "dmp_motor_d3_t33_b20",
                                  "prodmp_velocity_d7_t17_b10_clipped", "promp_position_d3_t17_b22"])
def test_replay_ends_on_the_forwards_state(name):
    c = E.make_case(name)
    eng = engine(c["mp"], c["D"], c["T"])
    q, qd = dev(c["q0"]), dev(c["qd0"])
    fwd = eng.episode_return(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]), spec_of(c), q, qd, n_steps=dev(c["n_steps"]),
                             reward="simple_reacher", goal=dev(c["goal"]), step0=dev(c["step0"]), steps_before_reward=c["sbr"])
    assert eng.last_kernel().startswith("k_episode_return<")
    res, _ = launch(c, need=(False,) * 6 + (True, True))
    assert torch.equal(res["q_end"], q) and torch.equal(res["qd_end"], qd)
    assert not torch.equal(q, dev(c["q0"])) and torch.equal(fwd["seg_len"], dev(c["n_steps"]))


@pytest.mark.parametrize("mp", ["prodmp", "promp", "dmp"])
def test_replay_ends_on_the_forwards_state_under_replanning(mp):
    """every = 16 at T = 33: two consecutive plans, the second with init_time = 16 dt from the state the first one left"""
    c = E.build(f"replan_{mp}", (mp, "motor", 5, 33, 13, False), 900)
    B, D, T = c["B"], c["D"], c["T"]
    eng = engine(mp, D, T)
    q, qd = dev(c["q0"]), dev(c["qd0"])
    ts, ps = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ip, iv = dev(c["init_pos"]), dev(c["init_vel"])
    for plan in range(2):
        start, s0 = (q.clone(), qd.clone()), ts.clone()
        init_time = plan * 16 * E.DT_PLAN
        fwd = eng.episode_return(dev(c["params"]), ip, iv, spec_of(c), q, qd, replan=(ts, ps, done, 16, 2 ** 31 - 1, T),
                                 reward="simple_reacher", goal=dev(c["goal"]), steps_before_reward=c["sbr"], init_time=init_time,
                                 condition=True)
        seg = fwd["seg_len"]
        assert seg.tolist() == [16] * B and ts.tolist() == [16 * (plan + 1)] * B
        res = eng.episode_return_vjp(dev(c["params"]), ip, iv, spec_of(c), start[0], start[1], dev(c["goal"]), dev(c["g_ret"]),
                                     n_steps=seg, step0=s0, steps_before_reward=c["sbr"], init_time=init_time, need=ALL)
        res = dict(zip(NAMES, res))
        assert torch.equal(res["q_end"], q) and torch.equal(res["qd_end"], qd), plan
        assert bool(res["g_params"].any()) and bool(torch.isfinite(res["g_params"]).all())
        ip, iv = fwd["cond_pos"], fwd["cond_vel"]


# ---- 4. NULL outputs and inputs --------------------------------------------------------------------------------------------------
def test_null_inputs_and_outputs():
    name = "prodmp_motor_d5_t17_b11_clipped"
    c = E.make_case(name)
    # NULL g_ret with g_q, g_qd given: the final state's gradient alone
    use = (False, True, True)
    full, _ = launch(c, "sum", use)
    ref, e32, _ = reference(name, "sum", use)
    E.check("no g_ret", host(full), ref, e32)
    assert not bool(full["g_goal"].any()) and bool(full["g_params"].any())
    # no upstream gradient at all: zeros
    none, _ = launch(c, "sum", (False, False, False))
    assert not any(bool(none[k].any()) for k in E.X_OUTPUTS + E.S_OUTPUTS)
    # an output left NULL does not change the others: each one alone, and each one left out
    full, _ = launch(c, "mean")
    for i in range(8):
        for need in (tuple(j == i for j in range(8)), tuple(j != i for j in range(8))):
            res, _ = launch(c, "mean", need=need)
            for k, n in zip(NAMES, need):
                assert (res[k] is None) == (not n)
                if n:
                    assert torch.equal(res[k], full[k]), (need, k)


# ---- 5. layout and determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prodmp_motor_d5_t33_b13", "promp_position_d3_t17_b22"])
def test_layout_and_determinism(name):
    """two runs: the same bits; params and every output 0 .. 3 dwords off a 16-byte boundary: the same bits, and the guard values around
    every output stay"""
    c = E.make_case(name)
    B, D, P = c["B"], c["D"], c["P"]
    base, eng = launch(c, "mean")
    again, _ = launch(c, "mean")
    for k in NAMES:
        assert torch.equal(base[k], again[k]), k
    shapes = [(B, P), (B, D), (B, D), (B, D), (B, D), (B, 2), (B, D), (B, D)]
    for shift in range(4):                    # dwords
        def shifted(shape, dtype, x=None):
            words = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
            buf = torch.full((words + 16,), float("nan"), dtype=torch.float32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            off = shift if dtype == torch.float32 else 2 * (shift % 2)        # (float64 arrays stay 8-byte aligned)
            v = buf[off:off + words]
            v = (v.view(torch.float64) if dtype == torch.float64 else v).view(shape)
            if x is not None:
                v.copy_(dev(x))
            assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
            return buf, v, off, words
        _, prm, _, _ = shifted((B, P), torch.float32, c["params"])
        outs = [shifted(s, torch.float32 if i < 3 else torch.float64) for i, s in enumerate(shapes)]
        res, _ = launch(c, "mean", out=[o[1] for o in outs], params=prm)
        assert eng.last_kernel() == kernel_name(c)
        for k, (buf, v, off, words) in zip(NAMES, outs):
            assert res[k].data_ptr() == v.data_ptr() and torch.equal(res[k], base[k]), (shift, k)
            assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + words:]).all()), (shift, k)


# ---- 6. autograd through episode_return ------------------------------------------------------------------------------------------
def test_autograd_through_episode_return():
    c = E.make_case("prodmp_motor_d5_t33_b13")
    eng, spec = engine(c["mp"], c["D"], c["T"]), spec_of(c)
    kw = dict(n_steps=dev(c["n_steps"]), reward="simple_reacher", step0=dev(c["step0"]), steps_before_reward=c["sbr"], aggregation="mean")

    def run(params, ip, iv, goal, **extra):
        q, qd = dev(c["q0"]), dev(c["qd0"])
        r = eng.episode_return(params, ip, iv, spec, q, qd, goal=goal, **kw, **extra)
        return r, q, qd

    params, ip, iv, goal = (dev(c[k]).requires_grad_() for k in ("params", "init_pos", "init_vel", "goal"))
    plain, q0, qd0 = run(params, ip, iv, goal)            # without the flag: constants, as before
    assert plain["ret"].grad_fn is None and not plain["ret"].requires_grad
    forward_kernel = eng.last_kernel()
    r, q, qd = run(params, ip, iv, goal, differentiable=True)
    assert eng.last_kernel() == forward_kernel            # the forward launch is the plain call's
    assert r["ret"].grad_fn is not None and torch.equal(r["ret"], plain["ret"]) and torch.equal(r["seg_len"], plain["seg_len"])
    assert torch.equal(q, q0) and torch.equal(qd, qd0) and not q.requires_grad
    (dev(c["g_ret"]) * r["ret"]).sum().backward()
    assert eng.last_kernel().startswith("k_episode_return_vjp") and eng.last_kernel() == kernel_name(c)
    bare, _ = launch(c, "mean", (True, False, False))
    for t, k in ((params, "g_params"), (ip, "g_init_pos"), (iv, "g_init_vel"), (goal, "g_goal")):
        assert torch.equal(t.grad, bare[k]) and bool(t.grad.any()), k
    # needs_input_grad: only params requires grad
    p2 = dev(c["params"]).requires_grad_()
    r2, _, _ = run(p2, dev(c["init_pos"]), dev(c["init_vel"]), dev(c["goal"]), differentiable=True)
    (dev(c["g_ret"]) * r2["ret"]).sum().backward()
    assert torch.equal(p2.grad, bare["g_params"])
    # nothing requires grad, or no_grad: the plain call
    r3, _, _ = run(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]), dev(c["goal"]), differentiable=True)
    assert r3["ret"].grad_fn is None and torch.equal(r3["ret"], plain["ret"])
    with torch.no_grad():
        r4, _, _ = run(params, ip, iv, goal, differentiable=True)
    assert r4["ret"].grad_fn is None and not r4["ret"].requires_grad and torch.equal(r4["ret"], plain["ret"])
    with pytest.raises(NotImplementedError, match="simple_reacher"):
        eng.episode_return(params, ip, iv, spec, dev(c["q0"]), dev(c["qd0"]), reward=None, differentiable=True)


# ---- 7. BatchedBlackBox at the default verbosity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["fancy_ProDMP/LongSimpleReacher-v0", "fancy_ProMP/LongSimpleReacher-v0", "fancy_DMP/LongSimpleReacher-v0"])
def test_batched_black_box_differentiable_step_at_the_default_verbosity(id):
    from fancy_gym_amd import make_batched
    B = 8
    bb, twin, sep = make_batched(id, B), make_batched(id, B), make_batched(id, B)
    full = make_batched(id, B, verbose=2)
    assert bb.verbose == 1
    for x in (bb, twin, sep, full):
        x.reset(seed=11)
    gen = torch.Generator(device="cpu").manual_seed(3)
    theta = (0.5 * torch.randn((B, bb.engine.num_params), generator=gen)).cuda()
    params = theta.clone().requires_grad_()
    out = bb.step(params, differentiable=True)
    assert bb.engine.last_kernel().startswith("k_episode_return<")
    want = twin.step(theta)
    assert out["rewards"].grad_fn is not None and set(out) == set(want)
    for k, v in want.items():
        assert torch.equal(out[k].detach(), v), k
        assert out[k].dtype == v.dtype
    assert torch.equal(bb.q, twin.q) and torch.equal(bb.qd, twin.qd) and torch.equal(bb.traj_steps, twin.traj_steps)
    w = torch.linspace(0.5, 1.5, B, dtype=torch.float64, device="cuda")
    (w * out["rewards"]).sum().backward()
    assert bb.engine.last_kernel().startswith("k_episode_return_vjp<"), bb.engine.last_kernel()
    # the verbose = 2 twin: the two-launch gradient.  Bound: the rule of (1) with its float32-einsum term left out (the stricter part)
    p2 = theta.clone().requires_grad_()
    o2 = full.step(p2, differentiable=True)
    (w * o2["rewards"]).sum().backward()
    assert full.engine.last_kernel().startswith("k_traj_vjp")
    g, r = params.grad.double().cpu().numpy(), p2.grad.double().cpu().numpy()
    scale, err = np.abs(r).max(), np.abs(g - r)
    print(f"{id}: max|grad| {scale:.3e}  max |one launch - two launches| {err.max():.3e}  project rule {E.RTOL * scale:.3e}")
    assert scale > 0 and np.all(err <= E.RTOL * scale + E.RTOL * np.abs(r))
    # fuse=False at the default verbosity: the two-launch gradient bit for bit
    p3 = theta.clone().requires_grad_()
    o3 = sep.step(p3, fuse=False, differentiable=True)
    assert "step_rewards" not in o3 and torch.equal(o3["rewards"].detach(), o2["rewards"].detach())
    (w * o3["rewards"]).sum().backward()
    assert sep.engine.last_kernel().startswith("k_traj_vjp") and torch.equal(p3.grad, p2.grad)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_limit():
    from fancy_gym_amd import RolloutSpec, TrajectoryEngine

    def call(eng, D, spec=None, T=None):
        P = eng.num_params
        s = torch.zeros((1, D), dtype=torch.float64, device="cuda")
        spec = spec or RolloutSpec("motor", D, plant="double_integrator", dt=0.01)
        return eng.episode_return_vjp(torch.zeros((1, P), device="cuda"), torch.zeros((1, D), device="cuda"),
                                      torch.zeros((1, D), device="cuda"), spec, s, s, torch.zeros((1, 2), dtype=torch.float64, device="cuda"),
                                      torch.ones(1, dtype=torch.float64, device="cuda"))

    kw = dict(device=0, dt=0.01, duration=0.2)
    with pytest.raises(NotImplementedError, match="learned tau"):
        call(TrajectoryEngine("promp", "linear", "rbf", 2, 3, tau=0.2, learn_tau=True, **kw), 2)
    dmp = TrajectoryEngine("dmp", "exp", "rbf", 2, 3, tau=1.0, **kw)
    dmp.set_option("dmp_response", 0)
    with pytest.raises(NotImplementedError, match="response route"):
        call(dmp, 2)
    with pytest.raises(NotImplementedError, match="17 DoF.*at most 16"):
        call(TrajectoryEngine("promp", "linear", "rbf", 17, 3, tau=0.2, **kw), 17)
    with pytest.raises(NotImplementedError, match="20 contraction columns.*at most 16"):
        call(TrajectoryEngine("promp", "linear", "rbf", 2, 20, tau=0.2, **kw), 2)
    ok = TrajectoryEngine("promp", "linear", "rbf", 2, 3, tau=0.2, **kw)
    with pytest.raises(NotImplementedError, match="double integrator"):
        TrajectoryEngine.episode_return_vjp(ok, torch.zeros((1, ok.num_params)), 0.0, 0.0, RolloutSpec("motor", 2, plant="static"),
                                            0.0, 0.0, torch.zeros((1, 2)), None)
    # the C entry point itself (the engine refuses that plant before the call)
    import ctypes as C
    from fancy_gym_amd import _lib
    static = RolloutSpec("motor", 2, plant="static")
    assert ok._lib.mpk_episode_return_vjp(ok._h, None, None, None, 0.0, C.byref(static.c), *([None] * 5), 0, 0, *([None] * 11), 0,
                                          None) == _lib.MPK_ENOTIMPL
    assert "MPK_PLANT_DOUBLE_INTEGRATOR" in _lib.last_error()
    # episode_return(differentiable=True) refuses BEFORE the forward changes the state
    q = torch.ones((1, 2), dtype=torch.float64, device="cuda")
    long = TrajectoryEngine("promp", "linear", "rbf", 2, 3, tau=24.0, device=0, dt=0.01, duration=24.0)
    with pytest.raises(NotImplementedError, match="checkpoints"):
        long.episode_return(torch.zeros((1, long.num_params), device="cuda", requires_grad=True), 0.0, 0.0,
                            RolloutSpec("motor", 2, plant="double_integrator", dt=0.01), q, q.clone(), reward="simple_reacher",
                            goal=torch.zeros((1, 2)), differentiable=True)
    assert torch.equal(q, torch.ones_like(q))


def test_horizon_limit_is_the_one_the_refusal_names():
    """T = 2400 is refused, and the refusal names the largest T the checkpoints fit: a launch at exactly that T -- the whole LDS of a CU
    but for less than 1 KB -- returns and passes (1), T + 1 is refused.  The limit is taken from the message on purpose: the message, the
    LDS carve and the launch have to agree."""
    from fancy_gym_amd import RolloutSpec
    mp, D = "promp", 2

    def zeros(T):
        eng = engine(mp, D, T, T * E.DT_PLAN)             # (tau = the duration: the linear phase ends at 1)
        s = torch.zeros((2, D), dtype=torch.float64, device="cuda")
        z = torch.zeros((2, D), device="cuda")
        return eng, (torch.zeros((2, eng.num_params), device="cuda"), z, z,
                     RolloutSpec("motor", D, np.full(D, 0.6), 0.075 + 0.01 * np.arange(D), -1000.0, 1000.0, plant="double_integrator",
                                 dt=0.01), s, s, torch.zeros((2, 2), dtype=torch.float64, device="cuda"), None)

    eng, args = zeros(2400)
    with pytest.raises(NotImplementedError, match=r"at most \d+ steps") as info:
        eng.episode_return_vjp(*args)
    limit = int(re.search(r"at most (\d+) steps", str(info.value)).group(1))
    print(f"the refusal at T = 2400 names at most {limit} steps")
    assert 2000 <= limit < 2400
    c = dict(E.build("limit", (mp, "motor", D, limit, 2, False), 4242, tau=limit * E.DT_PLAN))
    c["dt"] = 0.01
    c["sbr"] = limit - 10
    c["n_steps"] = np.array([limit, 17], np.int32)
    eng = engine(mp, D, limit, limit * E.DT_PLAN)
    res = eng.episode_return_vjp(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]), spec_of(c), dev(c["q0"]), dev(c["qd0"]),
                                 dev(c["goal"]), dev(c["g_ret"]), g_q=dev(c["g_q"]), g_qd=dev(c["g_qd"]), n_steps=dev(c["n_steps"]),
                                 step0=dev(c["step0"]), steps_before_reward=c["sbr"], need=ALL)
    assert eng.last_kernel() == "k_episode_return_vjp<promp, motor, 2>"
    pos, vel = eng.trajectory(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]))
    dp, dv = pos.cpu().numpy(), vel.cpu().numpy()
    ref, e32 = E.composed(c, dp, dv, "sum")
    cond = R.conditions(E.rollout_case(c, dp, dv, "sum"))
    print(f"T = {limit}: {cond}")
    assert cond["n_paid"] > 0 and cond["min_dist"] > 1e-3 and cond["saturated"] == 0.0 and cond["bound_gap"] >= 1e-9
    E.check(f"T = {limit}", host(dict(zip(NAMES, res))), ref, e32)
    eng, args = zeros(limit + 1)
    with pytest.raises(NotImplementedError, match=f"at most {limit} steps"):
        eng.episode_return_vjp(*args)


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------
def test_example_improves_the_mean_return_through_the_one_launch_backward():
    path = os.path.join(ROOT, "examples", "batched_reacher_gradient.py")
    spec = importlib.util.spec_from_file_location("batched_reacher_gradient", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.optimise(envs=64, iters=30, seed=0, verbose=False)
    print(f"mean return {first:.4f} -> {last:.4f}")
    assert last > first
