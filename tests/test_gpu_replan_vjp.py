"""
Gradients that cross plan boundaries on the GPU: the three ``_cond`` entry points (mpk_episode_return_vjp_cond,
mpk_reacher_rollout_vjp_cond, mpk_hole_reacher_rollout_vjp_cond), the carrying autograd functions of fancy_gym_amd/engine.py and
``BatchedBlackBox(replan_gradient="episode")``.

Yardsticks (tests/replan_vjp_ref.py, verified against each other in tests/test_replan_vjp_host.py):
  * per launch: ``link`` -- the existing float64 reference of that kernel plus the condition term at row tcond = clamp(n - 1, 0, T - 1),
    compared by the rule the existing test of the kernel applies to the same output (episode_vjp_ref.check; the checks of
    tests/test_gpu_reacher_vjp.py and tests/test_gpu_hole_vjp.py);
  * per episode: ``whole_episode_autograd`` -- ONE torch float64 graph over all plans, linearised at the device's own float32 plans and
    hand-overs.
The horizon is T = 33 with replanning_every = 16: three plans execute 16, 16 and 1 steps -- a full tile, a full tile from a non-zero
step0, and a one-step plan with tcond = 0.  Every comparison prints its maxima before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from . import episode_vjp_ref as E
from . import hole_vjp_ref as H
from . import reacher_vjp_ref as R
from . import replan_vjp_ref as RP
from . import test_gpu_episode_return_vjp as TE
from . import test_gpu_hole_vjp as TH
from . import test_gpu_reacher_vjp as TR

pytestmark = pytest.mark.gpu

dev = TE.dev

# where g_cond_pos, g_cond_vel go in the predecessor's argument list: behind g_qd
COND_AT = {"mpk_episode_return_vjp": 16, "mpk_reacher_rollout_vjp": 13, "mpk_hole_reacher_rollout_vjp": 16}


class _ViaCond:
    """the library with the three old entry points routed through their ``_cond`` successors with NULL, NULL"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in COND_AT:
            cond, i = getattr(self._lib, name + "_cond"), COND_AT[name]
            return lambda *a: cond(*a[:i], None, None, *a[i:])
        return getattr(self._lib, name)


def via_cond(eng, call):
    lib = eng._lib
    eng._lib = _ViaCond(lib)
    try:
        return call()
    finally:
        eng._lib = lib


def cond_grads(c, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((c["B"], c["D"])).astype(np.float32) for _ in range(2))


# ---- 1. the old entry points are the new ones with NULL ------------------------------------------------------------------------------
def test_old_entry_points_unchanged():
    c = E.make_case("prodmp_motor_d5_t33_b13")
    old, eng = TE.launch(c, "mean")
    name = eng.last_kernel()
    new = via_cond(eng, lambda: TE.launch(c, "mean")[0])
    assert eng.last_kernel() == name == TE.kernel_name(c)
    for k in TE.NAMES:
        assert torch.equal(old[k], new[k]), k
    for controller in ("motor", "velocity"):
        c = R.make_case("b7_t33_d7_clipped", controller)
        old, eng = TR.launch(c)
        new = via_cond(eng, lambda: TR.launch(c)[0])
        assert eng.last_kernel() == R.kernel_name(c)
        for k, a, b in zip(R.OUTPUTS, old, new):
            assert torch.equal(a, b), (controller, k)
    for controller, rew in (("motor", "simple"), ("velocity", "vel_acc")):
        c = H.make_case("b7_t33_d5_clipped", controller, rew)
        old, eng = TH.launch(c, g_ret=c["g_ret"], agg="mean")
        new = via_cond(eng, lambda: TH.launch(c, g_ret=c["g_ret"], agg="mean")[0])
        assert eng.last_kernel() == H.kernel_name(c)
        for k, a, b in zip(H.OUTPUTS, old, new):
            assert torch.equal(a, b), (controller, rew, k)


# ---- 2. the link -------------------------------------------------------------------------------------------------------------------------
EPISODE_LINK = ["prodmp_motor_d5_t33_b13", "prodmp_position_d2_t33_b33", "promp_position_d3_t17_b22", "prodmp_velocity_d7_t17_b10_clipped",
                "promp_motor_d7_t33_b8_clipped", "dmp_motor_d3_t33_b20", "promp_velocity_d2_t17_b31", "dmp_velocity_d5_t33_b1"]


@pytest.mark.parametrize("alone", [False, True])
@pytest.mark.parametrize("name", EPISODE_LINK)
def test_episode_link(name, alone):
    """mpk_episode_return_vjp_cond against ``link``: g_cond_* together with g_ret, g_q, g_qd, and alone.  n_steps of the recipe hold T, 0,
    T - 1, 17, 16, 1.  With the velocity / position controller the condition term must pass the controller's guards"""
    c = E.make_case(name)
    agg = E.AGGS[EPISODE_LINK.index(name) % 3]
    use = (False,) * 3 if alone else (True,) * 3
    gcp, gcv = cond_grads(c, 40 + EPISODE_LINK.index(name))
    eng = TE.engine(c["mp"], c["D"], c["T"])
    for given in ((gcp, gcv), (gcp, None), (None, gcv)):
        res = eng.episode_return_vjp(dev(c["params"]), dev(c["init_pos"]), dev(c["init_vel"]), TE.spec_of(c), dev(c["q0"]), dev(c["qd0"]),
                                     dev(c["goal"]), None if alone else dev(c["g_ret"]), g_q=None if alone else dev(c["g_q"]),
                                     g_qd=None if alone else dev(c["g_qd"]), n_steps=dev(c["n_steps"]), step0=dev(c["step0"]),
                                     steps_before_reward=c["sbr"], aggregation=agg, need=TE.ALL,
                                     g_cond_pos=None if given[0] is None else dev(given[0]),
                                     g_cond_vel=None if given[1] is None else dev(given[1]))
        assert eng.last_kernel() == TE.kernel_name(c) + " + cond", eng.last_kernel()
        got = TE.host(dict(zip(TE.NAMES, res)))
        pos, vel = TE.device_plan(c)
        ref, e32 = RP.link("episode", c, pos.cpu().numpy(), vel.cpu().numpy(), agg, use, given[0], given[1])
        E.check(f"{name} {agg} alone={alone} cond=({given[0] is not None}, {given[1] is not None})", got, ref, e32)
        if given[0] is not None and given[1] is not None:
            full = got
    # the condition is a copy of the plan: its term does not reach the plant adjoint or the goal
    base, _ = TE.launch(c, agg, use)
    for k in E.S_OUTPUTS:
        assert np.array_equal(full[k], base[k].cpu().numpy()), k
    if alone:
        assert np.abs(full["g_params"]).max() > 0
        if c["mp"] != "promp":
            # an episode that executed nothing still gets row 0: the plan's first row is not the start state's copy for every column
            idle = c["n_steps"] == 0
            assert not idle.any() or np.abs(full["g_init_pos"][idle]).max() > 0


ROLLOUT_LINK = [("b7_t33_d7_clipped", "motor"), ("b5_t35_d2", "velocity"), ("b23_t40_d3", "position"), ("b19_t33_d4_clipped", "velocity"),
                ("b5_t35_d5_clipped_all_paid", "position")]


def _rows_are_the_condition(c, n, g_des, g_cond, what):
    """the array of the input the controller does not read: row tcond is g_cond rounded once, every other row an exact zero"""
    rows = RP.tcond(n, c["T"])
    want = np.zeros_like(g_des)
    want[np.arange(c["B"]), rows] = g_cond
    assert np.array_equal(g_des, want), what
    assert g_des.any()


@pytest.mark.parametrize("alone", [False, True])
@pytest.mark.parametrize("name,controller", ROLLOUT_LINK)
def test_rollout_link(name, controller, alone):
    c = R.make_case(name, controller)
    use = (False,) * 3 if alone else (True,) * 3
    gcp, gcv = cond_grads(c, 60)
    eng = TR.engine(c["D"], c["T"], c["dt"])
    res = eng.reacher_rollout_vjp(TR.spec_of(c), dev(c["des_pos"]), dev(c["des_vel"]), dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]),
                                  None if alone else dev(c["g_r"]), g_q=None if alone else dev(c["g_q"]),
                                  g_qd=None if alone else dev(c["g_qd"]), n_steps=dev(c["n_steps"]), step0=dev(c["step0"]),
                                  steps_before_reward=c["sbr"], g_cond_pos=dev(gcp), g_cond_vel=dev(gcv))
    assert eng.last_kernel() == R.kernel_name(c) + " + cond"
    got = {k: v.cpu().numpy() for k, v in zip(R.OUTPUTS, res)}
    ref, _ = RP.link("rollout", c, c["des_pos"], c["des_vel"], use=use, g_cond_pos=gcp, g_cond_vel=gcv)
    TR.check(f"{name} {controller} alone={alone}", got, ref)
    assert set(c["n_steps"].tolist()) >= {c["T"], 0, 1} or c["B"] < 6
    if controller == "velocity":
        _rows_are_the_condition(c, c["n_steps"], got["g_des_pos"], gcp, "velocity: g_des_pos")
    if controller == "position":
        _rows_are_the_condition(c, c["n_steps"], got["g_des_vel"], gcv, "position: g_des_vel")
    # one pointer alone: the other half is untouched
    only = TR.launch(c, use)[0]
    half = eng.reacher_rollout_vjp(TR.spec_of(c), dev(c["des_pos"]), dev(c["des_vel"]), dev(c["q0"]), dev(c["qd0"]), dev(c["goal"]),
                                   None if alone else dev(c["g_r"]), g_q=None if alone else dev(c["g_q"]),
                                   g_qd=None if alone else dev(c["g_qd"]), n_steps=dev(c["n_steps"]), step0=dev(c["step0"]),
                                   steps_before_reward=c["sbr"], g_cond_pos=dev(gcp))
    assert torch.equal(half[0], res[0]) and torch.equal(half[1], only[1])
    for i in (2, 3, 4):
        assert torch.equal(half[i], only[i]) and torch.equal(res[i], only[i])


HOLE_LINK = [("b7_t33_d5_clipped", "motor", "simple"), ("b5_t35_d5", "velocity", "vel_acc"), ("b23_t40_d3", "position", "simple"),
             ("b7_t33_d5_clipped", "velocity", "simple")]


@pytest.mark.parametrize("alone", [False, True])
@pytest.mark.parametrize("name,controller,rew", HOLE_LINK)
def test_hole_link(name, controller, rew, alone):
    c = H.make_case(name, controller, rew)
    use = (False,) * 3 if alone else (True,) * 3
    gcp, gcv = cond_grads(c, 80)
    eng = TH.engine(c["D"], c["T"])

    def run(des_pos):
        return eng.hole_reacher_rollout_vjp(
            TH.spec_of(c), des_pos, dev(c["des_vel"]), dev(c["q0"]), dev(c["qd0"]), dev(c["hole"]), n_exec=dev(c["n_exec"]),
            collided=dev(c["collided"]), step0=dev(c["step0"]), g_rewards=None if alone else dev(c["g_r"]),
            g_q=None if alone else dev(c["g_q"]), g_qd=None if alone else dev(c["g_qd"]), rew_fct=rew, collision_penalty=c["penalty"],
            steps_before_reward=c["sbr"], g_cond_pos=dev(gcp), g_cond_vel=dev(gcv))
    res = run(dev(c["des_pos"]))
    assert eng.last_kernel() == H.kernel_name(c) + " + cond"
    got = TH.host(res)
    ref, _ = RP.link("hole", c, c["des_pos"], c["des_vel"], use=use, g_cond_pos=gcp, g_cond_vel=gcv)
    TH.check(f"{name} {controller} {rew} alone={alone}", got, ref)
    if controller == "velocity":
        _rows_are_the_condition(c, c["n_exec"], got["g_des_pos"], gcp, "velocity: g_des_pos")
        # des_pos may still be absent: the new argument changes what the kernel writes, not what it reads
        for a, b in zip(run(None), res):
            assert torch.equal(a, b)
    if controller == "position":
        _rows_are_the_condition(c, c["n_exec"], got["g_des_vel"], gcv, "position: g_des_vel")
    base, _ = TH.launch(c, use)
    for i in (2, 3, 4):
        assert torch.equal(res[i], base[i]), H.OUTPUTS[i]


# ---- the box: three plans of a SimpleReacher episode ---------------------------------------------------------------------------------
# name: (mp, controller, D, T, B, clipped) as episode_vjp_ref.CASES, all at T = 33
BOX_CASES = {
    "prodmp_motor_d5_b13": ("prodmp", "motor", 5, 33, 13, False),
    "prodmp_position_d2_b33": ("prodmp", "position", 2, 33, 33, False),
    "promp_velocity_d3_b22_clipped": ("promp", "velocity", 3, 33, 22, True),
    "promp_motor_d7_b10_clipped": ("promp", "motor", 7, 33, 10, True),
    "dmp_motor_d3_b20": ("dmp", "motor", 3, 33, 20, False),
}
PATHS = ("lean", "two_launch")          # verbose < 2 (_step_lean: one backward launch per plan) | verbose >= 2 (rollout + trajectory)


@functools.lru_cache(maxsize=None)
def box_case(name):
    c = RP.build(name, BOX_CASES[name], 700 + 11 * list(BOX_CASES).index(name))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def make_box(c, agg, condition, path, option="episode"):
    from .test_gpu_fuzz import _batched_from_cfg
    pc, bc, tc = E.mp_config(c["mp"], c["D"], c["tau"])
    bb = _batched_from_cfg(pc, bc, tc, E.DT_PLAN, c["T"] * E.DT_PLAN, c["B"], c["controller"], c["pg"], c["dg"], c["lo"], c["hi"],
                           plant="double_integrator", reward="simple_reacher", reward_aggregation=agg, replanning_every=RP.EVERY,
                           condition_on_desired=condition, steps_before_reward=c["sbr"], verbose=1 if path == "lean" else 2,
                           replan_gradient=option)
    assert bb.T == c["T"] == bb.horizon
    return bb


def run_episode(bb, c, differentiable=True, params=None, fuse=True, reset=True, plans=range(3)):
    """reset and three steps; per plan what the by-hand chain and the references need, recorded BEFORE / AFTER the step"""
    if reset:
        bb.reset(dev(c["q0"]), dev(c["qd0"]), goal=dev(c["goal"]))
        bb.goal.requires_grad_()
    rec = []
    for k in plans:
        p = dev(c["params_k"][k]).requires_grad_() if params is None else params[k]
        r = dict(params=p, start=(bb.q.clone(), bb.qd.clone()), s0=bb.traj_steps.clone(), init_time=float(bb._lockstep * bb.dt))
        r["init"] = ((bb.condition_pos.clone(), bb.condition_vel.clone()) if bb.condition_pos is not None
                     else (bb.q.float(), bb.qd.float()))
        r["out"] = bb.step(p, fuse=fuse, differentiable=differentiable)
        r["seg"] = r["out"]["trajectory_length"].clone()
        r["after"] = (bb.q.clone(), bb.qd.clone())
        if "des_pos" in r["out"]:
            r["plan"] = (r["out"]["des_pos"].detach(), r["out"]["des_vel"].detach())
        else:
            r["plan"] = bb.engine.trajectory(p.detach(), r["init"][0], r["init"][1], r["init_time"])
        rec.append(r)
    return rec


def episode_loss(rec, w_ret, w_q=None, w_qd=None):
    loss = 0.0
    for r, w in zip(rec, w_ret):
        if w is not None:
            loss = loss + (dev(w) * r["out"]["rewards"]).sum()
    if w_q is not None:
        loss = loss + (dev(w_q) * rec[-1]["out"]["end_pos"]).sum() + (dev(w_qd) * rec[-1]["out"]["end_vel"]).sum()
    return loss


def aggregate_backward(g_ret, seg, agg, T):
    """_RewardAggregateFn's backward, operation for operation"""
    seg = seg.view(-1, 1)
    t = torch.arange(T, device=g_ret.device, dtype=seg.dtype).view(1, -1)
    g = g_ret.view(-1, 1)
    if agg == "mean":
        g = g / seg.clamp(min=1).to(g.dtype)
    live = (t == seg - 1) if agg == "last" else (t < seg)
    return torch.where(live, g, torch.zeros((), dtype=g.dtype, device=g.device))


def plan_backward(bb, path, r, g_ret, g_q, g_qd, gcp, gcv):
    """ONE plan's backward with the bare products -> (g_params, g_init_pos, g_init_vel, g_q0, g_qd0, g_task)"""
    eng, agg = bb.engine, bb.reward_aggregation
    if path == "lean":
        res = eng.episode_return_vjp(r["params"].detach(), r["init"][0], r["init"][1], bb.spec, r["start"][0], r["start"][1],
                                     bb.goal.detach(), g_ret, g_q=g_q, g_qd=g_qd, n_steps=r["seg"], step0=r["s0"],
                                     steps_before_reward=bb.steps_before_reward, aggregation=agg, init_time=r["init_time"],
                                     g_cond_pos=gcp, g_cond_vel=gcv)
        return res[:6]
    if path == "two_launch":
        g_r = None if g_ret is None else aggregate_backward(g_ret, r["seg"], agg, bb.T)
        gp, gv, gq0, gqd0, gtask = eng.reacher_rollout_vjp(bb.spec, r["plan"][0], r["plan"][1], r["start"][0], r["start"][1], bb.goal.detach(),
                                                            g_r, g_q=g_q, g_qd=g_qd, n_steps=r["seg"], step0=r["s0"],
                                                            steps_before_reward=bb.steps_before_reward, g_cond_pos=gcp, g_cond_vel=gcv)
    else:
        gp, gv, gq0, gqd0, gtask = eng.hole_reacher_rollout_vjp(
            bb.spec, r["plan"][0], r["plan"][1], r["start"][0], r["start"][1], bb.hole.detach(), n_exec=r["seg"],
            collided=r["out"]["is_collided"].to(torch.uint8), step0=r["s0"], g_ret=g_ret, aggregation=agg, g_q=g_q, g_qd=g_qd,
            rew_fct=bb.rew_fct, collision_penalty=bb.hole_task["collision_penalty"], steps_before_reward=bb.steps_before_reward,
            g_cond_pos=gcp, g_cond_vel=gcv)
    return tuple(eng.trajectory_vjp(gp, gv, r["init_time"])) + (gq0, gqd0, gtask)


def hand_chain(bb, path, rec, w_ret, w_q=None, w_qd=None):
    """the episode's backward by hand, last plan to first, with the hand-overs of DESIGN.md "Gradients across plan boundaries":
      state link      g_q(k - 1) = g_q0(k), g_qd(k - 1) = g_qd0(k)
      condition link  condition_on_desired: g_cond_pos(k - 1) = g_init_pos(k), g_cond_vel(k - 1) = g_init_vel(k), float32 as they are
      cast            otherwise init_pos(k) = q_end(k - 1).float(): g_q(k - 1) += g_init_pos(k).double(), g_qd likewise
    -> (per-plan g_params, the task's gradient accumulated in the order the plans' backwards run)"""
    g_q = None if w_q is None else dev(w_q)
    g_qd = None if w_qd is None else dev(w_qd)
    gcp = gcv = g_task = None
    g_params = [None] * len(rec)
    for k in range(len(rec) - 1, -1, -1):
        g_ret = None if w_ret[k] is None else dev(w_ret[k])
        g_params[k], g_ip, g_iv, g_q, g_qd, gt = plan_backward(bb, path, rec[k], g_ret, g_q, g_qd, gcp, gcv)
        g_task = gt if g_task is None else g_task + gt
        if bb.condition_on_desired:
            gcp, gcv = g_ip, g_iv
        else:
            g_q, g_qd = g_q + g_ip.double(), g_qd + g_iv.double()
    return g_params, g_task


def sim_of(rec, hole=False):
    cpu = lambda t: t.detach().cpu().numpy()          # noqa: E731
    sim = dict(plans32=[(cpu(r["plan"][0]), cpu(r["plan"][1])) for r in rec], inits32=[(cpu(r["init"][0]), cpu(r["init"][1])) for r in rec],
               segs=[cpu(r["seg"]) for r in rec], step0s=[cpu(r["s0"]) for r in rec], init_times=[r["init_time"] for r in rec],
               starts=[(cpu(r["start"][0]), cpu(r["start"][1])) for r in rec])
    if hole:
        sim["collided"] = [cpu(r["out"]["is_collided"]).astype(np.uint8) for r in rec]
    return sim


def against_the_whole_graph(what, c, rec, grads, g_task, w_ret, w_q, w_qd, agg, condition, kind="reacher", jacobian=None):
    """test 4's comparison: every plan's params.grad and the task's gradient against ``whole_episode_autograd`` at the device's own plans,
    each held to the x-output rule with that plan's float32-einsum error (the task: the rule's first part alone)"""
    sim = sim_of(rec, kind == "hole")
    zero = np.zeros(c["B"])
    wr = [zero if w is None else w for w in w_ret]
    wq, wqd = (np.zeros((c["B"], c["D"])) if w is None else w for w in (w_q, w_qd))
    whole = RP.whole_episode_autograd(c, sim, wr, wq, wqd, agg, condition, kind, jacobian)
    chain = RP.chain_of_links(c, sim, wr, wq, wqd, agg, condition, kind, jacobian)
    for k, g in enumerate(grads):
        RP.check_x(f"{what} plan {k} g_params", g.cpu().numpy(), whole["g_params"][k], chain[k][1]["g_params"])
    RP.check_x(f"{what} task", g_task.cpu().numpy(), whole["g_task"])
    return whole


# ---- 3. + 4. the wiring is the hand-made chain, bit for bit; and the float64 graph of the whole episode -------------------------------
@pytest.mark.parametrize("condition", [False, True])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(BOX_CASES))
def test_wiring_equals_the_hand_made_chain_and_the_whole_episode_graph(name, path, condition):
    """The loss is a random-weighted sum of all plans' rewards plus a random-weighted end_pos / end_vel of the last plan.

    Bit for bit against the chain done by hand with the bare products; then against ``whole_episode_autograd`` by the x-output rule of
    episode_vjp_ref.check, 1e-5 max|ref| + 1e-5 |ref| or 4 x that plan's float32-einsum error.  The float64 1e-12 contract is per link
    (test_*_link above): across links every hand-over passes through a float32 (g_init_*, g_cond_*), so the float64 outputs inherit
    2^-24-relative terms -- hence the x rule for every output here, the goal included."""
    c = box_case(name)
    agg = E.AGGS[list(BOX_CASES).index(name) % 3]
    bb = make_box(c, agg, condition, path)
    rec = run_episode(bb, c)
    assert [r["seg"].tolist() for r in rec] == [[16] * c["B"], [16] * c["B"], [1] * c["B"]]
    assert all(r["out"]["rewards"].grad_fn is not None for r in rec)
    episode_loss(rec, c["w_ret"], c["w_q"], c["w_qd"]).backward()
    last = bb.engine.last_kernel()
    assert last.startswith("k_episode_return_vjp<" if path == "lean" else "k_traj_vjp"), last
    if path == "lean" and condition:
        assert last.endswith(" + cond")                   # (plan 0's backward: the condition upstream of plan 1's init_*)
    grads = [r["params"].grad for r in rec]
    assert all(g is not None and bool(g.any()) for g in grads[:2])
    g_goal = bb.goal.grad.clone()
    hand, hand_goal = hand_chain(bb, path, rec, c["w_ret"], c["w_q"], c["w_qd"])
    for k in range(3):
        assert torch.equal(grads[k], hand[k]), (name, path, condition, k)
    assert torch.equal(g_goal, hand_goal)
    cond = R.conditions(dict(c, des_pos=rec[0]["plan"][0].cpu().numpy(), des_vel=rec[0]["plan"][1].cpu().numpy(),
                             n_steps=rec[0]["seg"].cpu().numpy()))
    print(f"{name} {path} condition={condition} {agg}: plan 0 {cond}")
    assert cond["bound_gap"] >= 1e-9
    against_the_whole_graph(f"{name} {path} condition={condition}", c, rec, grads, g_goal, c["w_ret"], c["w_q"], c["w_qd"], agg, condition)


# ---- 5. the test that fails without the feature --------------------------------------------------------------------------------------
@pytest.mark.parametrize("condition", [False, True])
@pytest.mark.parametrize("path", PATHS)
def test_last_plans_reward_reaches_the_first_plans_parameters(path, condition):
    name = "prodmp_motor_d5_b13"
    c = box_case(name)
    w = [None, None, c["w_ret"][2]]
    bb = make_box(c, "sum", condition, path)
    rec = run_episode(bb, c)
    episode_loss(rec, w).backward()
    grads = [r["params"].grad for r in rec]
    assert grads[0] is not None and bool(grads[0].any()) and bool(grads[1].any())
    against_the_whole_graph(f"last reward only, {path} condition={condition}", c, rec, grads, bb.goal.grad, w, None, None, "sum", condition)
    # without the option: the same script leaves the earlier plans alone, and the last plan's gradient is today's value
    plain = make_box(c, "sum", condition, path, option=None)
    rec0 = run_episode(plain, c)
    assert all("end_pos" not in r["out"] and "end_vel" not in r["out"] for r in rec0)
    episode_loss(rec0, w).backward()
    assert rec0[0]["params"].grad is None and rec0[1]["params"].grad is None
    today = plan_backward(plain, path, rec0[2], dev(w[2]), None, None, None, None)
    assert torch.equal(rec0[2]["params"].grad, today[0]) and bool(today[0].any())
    assert torch.equal(plain.goal.grad, today[5])
    # (the last plan's own gradient does not depend on the option: the boundary terms go to the EARLIER plans)
    assert torch.equal(rec0[2]["params"].grad, grads[2])


# ---- 6. the forward is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("condition", [False, True])
@pytest.mark.parametrize("path", PATHS)
def test_forward_untouched(path, condition):
    c = box_case("promp_motor_d7_b10_clipped")
    on, off = make_box(c, "mean", condition, path), make_box(c, "mean", condition, path, option=None)
    keys = ("rewards", "trajectory_length", "done", "terminated", "truncated", "current_pos", "current_vel")
    if path == "two_launch":
        keys += ("des_pos", "des_vel", "step_actions", "step_rewards")
    a, b = run_episode(on, c), run_episode(off, c, differentiable=False)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert set(ra["out"]) == set(rb["out"]) | {"end_pos", "end_vel"}
        for key in keys:
            assert torch.equal(ra["out"][key].detach(), rb["out"][key]), (k, key)
            assert ra["out"][key].dtype == rb["out"][key].dtype
        # end_pos / end_vel: the state right after the step, carrying the graph; the state itself stays graph-free
        assert torch.equal(ra["out"]["end_pos"].detach(), ra["after"][0]) and torch.equal(ra["out"]["end_vel"].detach(), ra["after"][1])
        assert torch.equal(ra["after"][0], rb["after"][0]) and torch.equal(ra["after"][1], rb["after"][1])
        assert ra["out"]["end_pos"].requires_grad and ra["out"]["end_pos"].dtype == torch.float64
        assert not ra["out"]["current_pos"].requires_grad and not on.q.requires_grad
        assert torch.equal(ra["init"][0], rb["init"][0]) and torch.equal(ra["init"][1], rb["init"][1])
    if condition:
        assert torch.equal(on.condition_pos, off.condition_pos) and not on.condition_pos.requires_grad
        assert torch.equal(on._twin["cond_pos"].detach(), on.condition_pos) and on._twin["cond_pos"].requires_grad
    for x in ("traj_steps", "plan_steps", "done"):
        assert torch.equal(getattr(on, x), getattr(off, x)), x
    assert on._lockstep == off._lockstep


def test_option_without_replanning_changes_nothing():
    from fancy_gym_amd import make_batched
    id, B = "fancy_ProDMP/LongSimpleReacher-v0", 8
    on, off = make_batched(id, B, replan_gradient="episode"), make_batched(id, B)
    theta = (0.5 * torch.randn((B, on.engine.num_params), generator=torch.Generator().manual_seed(3))).cuda()
    grads = []
    for bb in (on, off):
        bb.reset(seed=11)
        p = theta.clone().requires_grad_()
        out = bb.step(p, differentiable=True)
        assert "end_pos" not in out and bb._twin is None
        out["rewards"].sum().backward()
        grads.append((p.grad, out["rewards"].detach()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


# ---- 7. HoleReacher with mixed fates -------------------------------------------------------------------------------------------------
HOLE_ID = "fancy_ProMP/HoleReacher-v0"


def hole_case(bb, thetas):
    D = bb.D
    return dict(name=HOLE_ID, controller=bb.spec.controller_type, rew_fct=bb.rew_fct, B=bb.B, T=bb.T, D=D, lo=-TH.LIM32, hi=TH.LIM32,
                dt=bb.dt, penalty=bb.hole_task["collision_penalty"], sbr=bb.steps_before_reward, pg=np.ones(D), dg=np.full(D, 0.1),
                hole=bb.hole.detach().cpu().numpy(), params_k=[t.cpu().numpy() for t in thetas])


@pytest.mark.parametrize("condition", [False, True])
@pytest.mark.parametrize("verbose,rew", [(1, "simple"), (2, "vel_acc")])
def test_hole_reacher_with_mixed_fates(verbose, rew, condition):
    """replanning_every = 50 at T = 200: some episodes collide inside plan 0, some inside plan 1, some never in the three plans.  A
    collided episode executes 0 steps in later plans: its later-plan parameter gradients are exact zeros and the gradient of its end
    state passes through those plans unchanged into the plan it collided in"""
    from fancy_gym_amd import make_batched
    B = 48
    over = {"black_box_kwargs": {"replanning_every": 50, "condition_on_desired": condition}}
    bb = make_batched(HOLE_ID, B, collision_gradient="frozen", replan_gradient="episode", verbose=verbose, mp_config_override=over,
                      rew_fct=rew)
    assert bb.condition_on_desired == condition and bb.rew_fct == rew
    bb.reset(seed=5)
    bb.hole.requires_grad_()
    gen = torch.Generator(device="cpu").manual_seed(9)
    thetas = [(0.6 * torch.randn((B, bb.engine.num_params), generator=gen)).cuda() for _ in range(3)]
    params = [t.clone().requires_grad_() for t in thetas]
    rec = run_episode(bb, None, params=params, reset=False)
    coll = [r["out"]["is_collided"].cpu().numpy() for r in rec]
    segs = [r["seg"].cpu().numpy() for r in rec]
    in0, in1 = coll[0], coll[1] & ~coll[0]
    never = ~(coll[0] | coll[1] | coll[2])
    print(f"{rew} verbose {verbose} condition={condition}: collided in plan 0: {int(in0.sum())}, in plan 1: {int(in1.sum())}, "
          f"never: {int(never.sum())}; executed {[s.tolist() for s in segs]}")
    assert in0.any() and in1.any() and never.any()
    assert not segs[1][in0].any() and not segs[2][in0 | in1].any() and (segs[2][never] == 50).all()
    rng = np.random.default_rng(17)
    w_ret = [rng.uniform(0.5, 1.5, B) for _ in range(3)]
    w_q, w_qd = rng.standard_normal((B, bb.D)), rng.standard_normal((B, bb.D))
    episode_loss(rec, w_ret, w_q, w_qd).backward()
    grads = [p.grad for p in params]
    # collided episodes: exact zeros for the parameters of the plans after the collision
    assert not bool(grads[1][torch.as_tensor(in0)].any()) and not bool(grads[2][torch.as_tensor(in0 | in1)].any())
    assert bool(grads[0][torch.as_tensor(in0)].any()) and bool(grads[1][torch.as_tensor(in1)].any())
    hand, hand_hole = hand_chain(bb, "hole", rec, w_ret, w_q, w_qd)
    for k in range(3):
        assert torch.equal(grads[k], hand[k]), k
    assert torch.equal(bb.hole.grad, hand_hole)
    c = hole_case(bb, thetas)
    against_the_whole_graph(f"hole {rew} verbose {verbose} condition={condition}", c, rec, grads, bb.hole.grad, w_ret, w_q, w_qd,
                            bb.reward_aggregation, condition, "hole", lambda k: TH.jacobian(HOLE_ID, rec[k]["init_time"]))


# ---- 8. cuts and determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_cuts(path):
    """a reset between plans, a plain step between two differentiable ones and get_trajectory on its own each cut the chain: the earlier
    plans' params.grad is what their own rewards give, untouched by later rewards"""
    c = box_case("prodmp_motor_d5_b13")
    w = c["w_ret"]

    def own_gradient_of_plan_0(bb, rec):
        return plan_backward(bb, path, rec[0], dev(w[0]), None, None, None, None)[0]

    for cut in ("plain_step", "get_trajectory", "reset"):
        bb = make_box(c, "sum", True, path)
        rec = run_episode(bb, c, plans=[0])
        assert bb._twin is not None
        if cut == "plain_step":
            bb.step(dev(c["params_k"][1]))
        elif cut == "get_trajectory":
            bb.get_trajectory(dev(c["params_k"][1]))
        else:
            bb.reset(dev(c["q0"]), dev(c["qd0"]), goal=bb.goal)
        assert bb._twin is None
        rec += run_episode(bb, c, reset=False, plans=[1] if cut == "reset" else [2])
        later = rec[1]["params"]
        ((dev(w[0]) * rec[0]["out"]["rewards"]).sum() + (dev(w[1]) * rec[1]["out"]["rewards"]).sum()
         + rec[1]["out"]["end_pos"].sum()).backward()
        assert bool(later.grad.any())
        assert torch.equal(rec[0]["params"].grad, own_gradient_of_plan_0(bb, rec)), cut


@pytest.mark.parametrize("path", PATHS)
def test_two_identical_runs_give_the_same_bits(path):
    c = box_case("promp_velocity_d3_b22_clipped")
    runs = []
    for _ in range(2):
        bb = make_box(c, "last", True, path)
        rec = run_episode(bb, c)
        episode_loss(rec, c["w_ret"], c["w_q"], c["w_qd"]).backward()
        runs.append([r["params"].grad for r in rec] + [bb.goal.grad])
    for a, b in zip(*runs):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
