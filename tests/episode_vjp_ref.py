"""
The float64 reference of mpk_episode_return_vjp, shared by tests/test_episode_return_vjp_host.py and tests/test_gpu_episode_return_vjp.py.

The chain is plan -> rollout -> reward -> aggregation.  Its reference gradient is COMPOSED of the two references the project already has:
  * tests/reacher_vjp_ref.py (``autograd``): the gradient of  L = sum g_r r + sum g_q q_T + sum g_qd qd_T  w.r.t. the desired trajectory,
    the plan-start state and the goal, with g_r[b, t] = g_ret[b] w_t the aggregation's weights (``step_reward_grads``);
  * the oracle's explicit trajectory Jacobian as tests/test_gpu_traj_vjp.py builds it (the plan is affine in one episode's
    x = (params, init_pos, init_vel): column i = f(e_i) - f(0) in float64), contracted with (g_des_pos, g_des_vel) in float64.
The rollout reference is linearised at a GIVEN float32 plan (on the GPU: the device's own mpk_trajectory output, so that clip masks are
decided on the same numbers); ``whole_chain_autograd`` differentiates the entire chain in one torch graph at the same plan, which is what
the host test compares the composition with.
"""
import functools

import numpy as np
import torch

from oracle import mp_oracle as O

from . import reacher_vjp_ref as R

DT_PLAN = 0.02          # the plan's time step; duration = T * DT_PLAN
DT_PLANT = 0.1          # the double integrator's (reacher_vjp_ref's short cases)
SBR = 14                # steps_before_reward: with step0 in {0, 1, 2} the paid steps start in tile 0 (t = 12 .. 14) and go on in tile 1
AGGS = ("sum", "mean", "last")

MPS = {
    # tau = 1: DMP's alpha ds = 25 * 0.02 = 0.5 <= 1, the response route
    "prodmp": lambda D, tau: (O.PhaseCfg("exp", tau=tau, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                         O.TrajCfg("prodmp", action_dim=D)),
    "promp": lambda D, tau: (O.PhaseCfg("linear", tau=tau),
                        O.BasisCfg("zero_rbf", num_basis=5, num_basis_zero_start=1, num_basis_zero_goal=0, basis_bandwidth_factor=3),
                        O.TrajCfg("promp", action_dim=D)),
    "dmp": lambda D, tau: (O.PhaseCfg("exp", tau=tau, alpha_phase=2.0), O.BasisCfg("rbf", num_basis=5, basis_bandwidth_factor=3),
                      O.TrajCfg("dmp", action_dim=D, alpha=25.0)),
}

# name: (mp, controller, D, T, B, clipped).  E = floor(64 / D) episodes per wave: B in {1, E - 1, E + 1} -- one episode, idle lanes, a
# tail wave; D in {2, 5, 7} compiled in, 3 at run time; T in {17, 33}: a partial last tile behind one and two full ones
CASES = {
    "prodmp_motor_d5_t33_b13": ("prodmp", "motor", 5, 33, 13, False),
    "prodmp_motor_d5_t17_b11_clipped": ("prodmp", "motor", 5, 17, 11, True),
    "prodmp_position_d2_t33_b33": ("prodmp", "position", 2, 33, 33, False),
    "prodmp_velocity_d7_t17_b10_clipped": ("prodmp", "velocity", 7, 17, 10, True),
    "prodmp_motor_d2_t33_b1_clipped": ("prodmp", "motor", 2, 33, 1, True),
    "promp_motor_d7_t33_b8_clipped": ("promp", "motor", 7, 33, 8, True),
    "promp_position_d3_t17_b22": ("promp", "position", 3, 17, 22, False),
    "promp_velocity_d2_t17_b31": ("promp", "velocity", 2, 17, 31, False),
    "promp_motor_d5_t17_b13": ("promp", "motor", 5, 17, 13, False),
    "dmp_motor_d3_t33_b20": ("dmp", "motor", 3, 33, 20, False),
    "dmp_velocity_d5_t33_b1": ("dmp", "velocity", 5, 33, 1, False),
    "dmp_position_d7_t17_b1_clipped": ("dmp", "position", 7, 17, 1, True),
}
X_OUTPUTS = ("g_params", "g_init_pos", "g_init_vel")
S_OUTPUTS = ("g_q0", "g_qd0", "g_goal")
RTOL = 1e-5             # tests/test_gpu_trajectory.py


def mp_config(mp, D, tau=1.0):
    return MPS[mp](D, tau)


@functools.lru_cache(maxsize=None)
def jacobian(mp, D, T, init_time=0.0, tau=1.0):
    """float64 (J [2, T, D, n], f0 [2, T, D], P) of ONE episode's plan over its n = P + 2 D inputs: plan(x) = f0 + J x"""
    pc, bc, tc = mp_config(mp, D, tau)
    P = O.num_params(pc, bc, tc)
    n = P + 2 * D
    x = np.zeros((n + 1, n))
    x[1:] = np.eye(n)
    pos, vel = O.get_trajectory(pc, bc, tc, x[:, :P], T * DT_PLAN, DT_PLAN, init_time, x[:, P:P + D], x[:, P + D:], dtype=np.float64)
    assert pos.shape[1] == T, (pos.shape, T)
    J = np.ascontiguousarray(np.moveaxis(np.stack([pos[1:] - pos[0], vel[1:] - vel[0]]), 1, -1))
    f0 = np.stack([pos[0], vel[0]])
    J.setflags(write=False)
    f0.setflags(write=False)
    return J, f0, P


def plan_f64(mp, D, T, x, init_time=0.0):
    """the float64 plan (pos, vel) [B, T, D] of x [B, n]"""
    J, f0, _ = jacobian(mp, D, T, init_time)        # (tau = 1: the cases of this file)
    return tuple(f0[j][None] + np.einsum("tdn,bn->btd", J[j], x) for j in range(2))


def build(name, shape, seed, tau=1.0):
    """the inputs of one case: reacher_vjp_ref's recipe for the rollout side, plus x = (params, init_pos, init_vel) float32 and g_ret"""
    mp, controller, D, T, B, clipped = shape
    lo, hi = (-0.4, 0.6) if clipped else (-1000.0, 1000.0)
    c = dict(R.recipe(name, (B, T, D, lo, hi, SBR, DT_PLANT), controller, seed, 0))
    _, _, P = jacobian(mp, D, T, 0.0, tau)
    rng = np.random.default_rng(seed + 7)
    c["mp"], c["P"], c["tau"] = mp, P, tau
    c["params"] = (0.5 * rng.standard_normal((B, P))).astype(np.float32)
    c["init_pos"] = c["q0"].astype(np.float32)
    c["init_vel"] = c["qd0"].astype(np.float32)
    c["g_ret"] = rng.uniform(0.5, 1.5, B)
    # executed steps: all, none, T - 1, one step into the second tile, one full tile, one step
    c["n_steps"] = np.minimum(np.array([T, 0, T - 1, 17, 16, 1])[np.arange(B) % 6] if B > 1 else np.array([T]), T).astype(np.int32)
    for k in ("des_pos", "des_vel", "g_r"):
        del c[k]
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def make_case(name):
    return build(name, CASES[name], 100 + 13 * list(CASES).index(name))


def x_of(c):
    return np.concatenate([c["params"], c["init_pos"], c["init_vel"]], axis=1).astype(np.float64)


def oracle_plan32(c, init_time=0.0):
    """the float64 oracle plan rounded to float32: the stand-in for the device's plan where there is no device"""
    pos, vel = plan_f64(c["mp"], c["D"], c["T"], x_of(c), init_time)
    return pos.astype(np.float32), vel.astype(np.float32)


def step_reward_grads(c, agg, g_ret=None):
    """g_r [B, T] = g_ret w_t for t < n: w_t = 1 (sum), 1 / n (mean), [t == n - 1] (last) -- _RewardAggregateFn's backward"""
    g = (c["g_ret"] if g_ret is None else g_ret)[:, None]
    t = np.arange(c["T"])[None]
    n = c["n_steps"][:, None]
    if agg == "sum":
        return np.where(t < n, g, 0.0)
    if agg == "mean":
        return np.where(t < n, g / np.maximum(n, 1), 0.0)
    return np.where(t == n - 1, g, 0.0)


def rollout_case(c, des_pos32, des_vel32, agg, use=(True, True, True)):
    """the case as reacher_vjp_ref reads it: the plan as its desired trajectory, the aggregation's g_r"""
    g_r = step_reward_grads(c, agg) if use[0] else np.zeros((c["B"], c["T"]))
    return dict(c, des_pos=des_pos32, des_vel=des_vel32, g_r=g_r)


def composed(c, des_pos32, des_vel32, agg, use=(True, True, True), init_time=0.0):
    """(ref, e32): the composed float64 gradients -- g_params, g_init_pos, g_init_vel, g_q0, g_qd0, g_goal -- linearised at the given
    float32 plan, and per x-output the error of a float32 CPU einsum of the float32-rounded Jacobian with the float32-rounded
    (g_des_pos, g_des_vel) against the float64 value (tests/test_gpu_traj_vjp.py: what any float32 sum over T pays)"""
    rc = rollout_case(c, des_pos32, des_vel32, agg, use)
    g = R.autograd(rc, (True, use[1], use[2]))
    J, _, P = jacobian(c["mp"], c["D"], c["T"], init_time, c["tau"])
    D = c["D"]
    gx = np.zeros((c["B"], J.shape[-1]))
    g32 = torch.zeros(gx.shape, dtype=torch.float32)
    for j, k in enumerate(("g_des_pos", "g_des_vel")):
        gx += np.einsum("tdn,btd->bn", J[j], g[k])
        g32 += torch.einsum("tdn,btd->bn", torch.from_numpy(J[j].astype(np.float32)), torch.from_numpy(g[k].astype(np.float32)))
    e = np.abs(g32.numpy().astype(np.float64) - gx)
    ref = dict(g_params=gx[:, :P], g_init_pos=gx[:, P:P + D], g_init_vel=gx[:, P + D:], g_q0=g["g_q0"], g_qd0=g["g_qd0"], g_goal=g["g_goal"])
    e32 = dict(g_params=e[:, :P], g_init_pos=e[:, P:P + D], g_init_vel=e[:, P + D:])
    return ref, e32


def whole_chain_autograd(c, des_pos32, des_vel32, agg, use=(True, True, True), init_time=0.0):
    """torch autograd through plan (f0 + J x) -> rollout -> reward -> aggregation in ONE float64 graph, evaluated at the given float32
    plan (the plan's value is moved onto it by a constant), for  L = sum g_ret ret + sum g_q q_T + sum g_qd qd_T"""
    J, f0, P = jacobian(c["mp"], c["D"], c["T"], init_time, c["tau"])
    D = c["D"]
    x = torch.tensor(x_of(c), requires_grad=True)
    des = []
    for j, d32 in enumerate((des_pos32, des_vel32)):
        lin = torch.tensor(f0[j])[None] + torch.einsum("tdn,bn->btd", torch.tensor(J[j]), x)
        des.append(lin + (torch.tensor(d32.astype(np.float64)) - lin).detach())
    q0, qd0, goal = (torch.tensor(np.asarray(c[k], dtype=np.float64), requires_grad=True) for k in ("q0", "qd0", "goal"))
    rew, q, qd, _, _ = R.torch_rollout(dict(c), des[0], des[1], q0, qd0, goal)
    n = torch.tensor(c["n_steps"].astype(np.int64))
    if agg == "sum":
        ret = rew.sum(dim=1)
    elif agg == "mean":
        ret = rew.sum(dim=1) / n.clamp(min=1)
    else:
        ret = torch.where(n > 0, rew.gather(1, (n - 1).clamp(min=0)[:, None])[:, 0], torch.zeros(c["B"], dtype=torch.float64))
    loss = ret.sum() * 0.0
    if use[0]:
        loss = loss + (torch.tensor(c["g_ret"]) * ret).sum()
    if use[1]:
        loss = loss + (torch.tensor(c["g_q"]) * q).sum()
    if use[2]:
        loss = loss + (torch.tensor(c["g_qd"]) * qd).sum()
    gx, gq0, gqd0, ggoal = (g.numpy() for g in torch.autograd.grad(loss, [x, q0, qd0, goal]))
    return dict(g_params=gx[:, :P], g_init_pos=gx[:, P:P + D], g_init_vel=gx[:, P + D:], g_q0=gq0, g_qd0=gqd0, g_goal=ggoal)


def check(what, got, ref, e32):
    """g_q0, g_qd0, g_goal: |got - ref| <= 1e-12 max|ref| (the project's float64 contract); g_params, g_init_pos, g_init_vel: the rule
    of tests/test_gpu_traj_vjp.py, |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the reference's float32-einsum error) -- the table
    rows are float32.  ``got`` may leave outputs out.  Prints every maximum, then asserts."""
    bad = []
    for k in X_OUTPUTS + S_OUTPUTS:
        if k not in got or got[k] is None:
            continue
        g, r = np.asarray(got[k], dtype=np.float64), ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        scale = np.abs(r).max() if r.size else 0.0
        err = np.abs(g - r)
        if k in S_OUTPUTS:
            tol = np.full(r.shape, 1e-12 * scale)
            note = f"bound {1e-12 * scale:.3e}"
        else:
            e = e32[k].max() if e32[k].size else 0.0
            tol = np.maximum(RTOL * scale + RTOL * np.abs(r), 4.0 * e)
            note = f"f32-einsum err {e:.3e}  project rule {RTOL * scale:.3e}"
        print(f"[episode vjp] {what} {k}: max|ref| {scale:.3e}  max err {err.max() if err.size else 0.0:.3e}  {note}")
        if not np.isfinite(g).all() or (err > tol).any():
            bad.append((k, float(err.max())))
    assert not bad, (what, bad)
