"""
The float64 references of the gradients that cross plan boundaries (``BatchedBlackBox(replan_gradient="episode")`` and the three ``_cond``
entry points), shared by tests/test_replan_vjp_host.py and tests/test_gpu_replan_vjp.py.  Built from what exists:

``link``                    ONE plan's backward with an upstream gradient of the condition output: episode_vjp_ref.composed /
                            reacher_vjp_ref.autograd / hole_vjp_ref.autograd plus the condition term where it belongs --
                            g_des_*[b, tcond] += g_cond_* for the rollout products, g_x += J[0][tcond]^T g_cond_pos + J[1][tcond]^T
                            g_cond_vel for the episode product (J: episode_vjp_ref.jacobian at the plan's init_time), with
                            tcond = clamp(n - 1, 0, T - 1).
``chain_of_links``          the links of an episode's plans, last to first, handing g_q0 / g_qd0 / g_init_* back as DESIGN.md ("Gradients
                            across plan boundaries") says -- in float64, no rounding at the hand-overs.
``whole_episode_autograd``  ONE torch float64 graph over all plans: plan (f0 + J x at that plan's init_time) -> rollout -> reward ->
                            aggregation, plan after plan, the next plan's init_pos / init_vel taken from the state or from row tcond.
                            Every plan's value is moved onto the given float32 plan with ``lin + (d32 - lin).detach()`` (the device of
                            episode_vjp_ref.whole_chain_autograd: clip masks are decided on the given numbers), and the float32 cast of
                            the state hand-over is pinned to the given float32 values the same way.
``simulate``                the forward of an episode on the CPU (oracle plans rounded to float32, reacher_vjp_ref's rollout): the plans,
                            hand-overs and plan-start states the two references above are linearised at where there is no device.
"""
import numpy as np
import torch

from . import episode_vjp_ref as E
from . import hole_vjp_ref as H
from . import reacher_vjp_ref as R

EVERY = 16              # replanning_every: at T = 33 three plans execute 16, 16 and 1 steps
T_EPISODE = 33


def tcond(n, T):
    """the row the forward copies into cond_pos / cond_vel: the last executed step, row 0 for an episode that executed nothing"""
    return np.clip(np.asarray(n, dtype=np.int64) - 1, 0, T - 1)


def schedule(T=T_EPISODE, every=EVERY):
    """[(step0, n_steps)] of the plans of a lockstep episode with horizon T: t % every == 0 replans"""
    return [(s, min(every, T - s)) for s in range(0, T, every)]


def _add_rows(g, rows, g_cond):
    out = g.copy()
    if g_cond is not None:
        out[np.arange(out.shape[0]), rows] += np.asarray(g_cond, dtype=np.float64)
    return out


def link(kind, c, des_pos32, des_vel32, agg="sum", use=(True, True, True), g_cond_pos=None, g_cond_vel=None, init_time=0.0):
    """(ref, e32) of one plan's backward.  ``kind`` "episode": ``c`` as episode_vjp_ref.build gives it (g_ret, g_q, g_qd, n_steps);
    "rollout": as reacher_vjp_ref (g_r); "hole": as hole_vjp_ref (g_r, n_exec, collided).  e32: episode_vjp_ref.composed's
    float32-einsum error ("episode"), else None"""
    T = c["T"]
    if kind == "episode":
        ref, e32 = E.composed(c, des_pos32, des_vel32, agg, use, init_time)
        J, _, P = E.jacobian(c["mp"], c["D"], T, init_time, c["tau"])
        D, rows = c["D"], tcond(c["n_steps"], T)
        gx = np.zeros((c["B"], J.shape[-1]))
        for j, g in enumerate((g_cond_pos, g_cond_vel)):
            if g is not None:
                gx += np.einsum("bdn,bd->bn", J[j][rows], np.asarray(g, dtype=np.float64))       # J[j][tcond]^T g_cond
        ref = dict(ref, g_params=ref["g_params"] + gx[:, :P], g_init_pos=ref["g_init_pos"] + gx[:, P:P + D],
                   g_init_vel=ref["g_init_vel"] + gx[:, P + D:])
        return ref, e32
    mod, nkey = (R, "n_steps") if kind == "rollout" else (H, "n_exec")
    g = mod.autograd(dict(c, des_pos=des_pos32, des_vel=des_vel32), use)
    rows = tcond(c[nkey], T)
    return dict(g, g_des_pos=_add_rows(g["g_des_pos"], rows, g_cond_pos), g_des_vel=_add_rows(g["g_des_vel"], rows, g_cond_vel)), None


def plan_case(c, k, step0, n_steps, g_ret, g_q=None, g_qd=None, start=None):
    """the case of plan k of an episode as episode_vjp_ref / reacher_vjp_ref read it"""
    B, D = c["B"], c["D"]
    z = np.zeros((B, D))
    out = dict(c, params=c["params_k"][k], n_steps=np.asarray(n_steps, np.int32), step0=np.asarray(step0, np.int32),
               g_ret=np.asarray(g_ret, np.float64), g_q=z if g_q is None else g_q, g_qd=z if g_qd is None else g_qd)
    if start is not None:
        out.update(q0=start[0], qd0=start[1])
    return out


def _hole_link(c, k, sim, w_ret, g_q, g_qd, agg, gcp, gcv, jacobian):
    """``link("hole")`` of plan k contracted with the plan's explicit Jacobian, as episode_vjp_ref.composed does it for the reacher:
    (ref, e32) with composed's keys (g_goal: the hole's gradient)"""
    B, D = c["B"], c["D"]
    ck = dict(c, n_exec=np.asarray(sim["segs"][k], np.int32), step0=np.asarray(sim["step0s"][k], np.int32),
              collided=np.asarray(sim["collided"][k], np.uint8), q0=sim["starts"][k][0], qd0=sim["starts"][k][1], g_q=g_q, g_qd=g_qd)
    ck["g_r"] = H.expand_g_ret(ck, agg, np.asarray(w_ret[k], dtype=np.float64))
    g, _ = link("hole", ck, *sim["plans32"][k], g_cond_pos=gcp, g_cond_vel=gcv)
    J, _, P = jacobian(k)
    gx = np.zeros((B, J.shape[-1]))
    g32 = torch.zeros(gx.shape, dtype=torch.float32)
    for j, key in enumerate(("g_des_pos", "g_des_vel")):
        gx += np.einsum("tdn,btd->bn", J[j], g[key])
        g32 += torch.einsum("tdn,btd->bn", torch.from_numpy(J[j].astype(np.float32)), torch.from_numpy(g[key].astype(np.float32)))
    e = np.abs(g32.numpy().astype(np.float64) - gx)
    ref = dict(g_params=gx[:, :P], g_init_pos=gx[:, P:P + D], g_init_vel=gx[:, P + D:], g_q0=g["g_q0"], g_qd0=g["g_qd0"], g_goal=g["g_hole"])
    return ref, dict(g_params=e[:, :P], g_init_pos=e[:, P:P + D], g_init_vel=e[:, P + D:])


def chain_of_links(c, sim, w_ret, w_q, w_qd, agg, condition, kind="reacher", jacobian=None):
    """the episode's gradient as a chain of ``link`` references, last plan to first: per plan (ref, e32) with the keys of
    episode_vjp_ref.composed; the goal's (kind "hole": the hole's) gradient is the sum of the plans' g_goal.  Hand-overs (float64 here, no
    rounding): state link g_q(k - 1) = g_q0(k), g_qd(k - 1) = g_qd0(k); condition link g_cond_*(k - 1) = g_init_*(k); without
    condition_on_desired the cast q.float() is the identity: g_q(k - 1) += g_init_pos(k), g_qd(k - 1) += g_init_vel(k)"""
    n = len(sim["segs"])
    g_q, g_qd, gcp, gcv = np.asarray(w_q, dtype=np.float64), np.asarray(w_qd, dtype=np.float64), None, None
    out = [None] * n
    for k in range(n - 1, -1, -1):
        if kind == "hole":
            ref, e32 = _hole_link(c, k, sim, w_ret, g_q, g_qd, agg, gcp, gcv, jacobian)
        else:
            ck = plan_case(c, k, sim["step0s"][k], sim["segs"][k], w_ret[k], g_q, g_qd, sim["starts"][k])
            ck.update(init_pos=sim["inits32"][k][0], init_vel=sim["inits32"][k][1])
            ref, e32 = link("episode", ck, *sim["plans32"][k], agg, g_cond_pos=gcp, g_cond_vel=gcv, init_time=sim["init_times"][k])
        out[k] = (ref, e32)
        g_q, g_qd = ref["g_q0"], ref["g_qd0"]
        if condition:
            gcp, gcv = ref["g_init_pos"], ref["g_init_vel"]
        else:
            g_q, g_qd = g_q + ref["g_init_pos"], g_qd + ref["g_init_vel"]
    return out


def _aggregate(rew, n, agg):
    nt = torch.as_tensor(np.asarray(n, dtype=np.int64))
    if agg == "sum":
        return rew.sum(dim=1)
    if agg == "mean":
        return torch.where(nt > 0, rew.sum(dim=1) / nt.clamp(min=1), torch.zeros(rew.shape[0], dtype=torch.float64))
    return torch.where(nt > 0, rew.gather(1, (nt - 1).clamp(min=0)[:, None])[:, 0], torch.zeros(rew.shape[0], dtype=torch.float64))


def whole_episode_autograd(c, sim, w_ret, w_q, w_qd, agg, condition, kind="reacher", jacobian=None):
    """the gradients of  L = sum_k sum_b w_ret[k][b] ret_k[b] + sum w_q q_end + sum w_qd qd_end  w.r.t. every plan's params and the goal /
    hole, by ONE torch float64 graph over all plans, at the given float32 plans and hand-overs (``sim``: plans32, inits32, segs, step0s,
    init_times, starts[0]; kind "hole": also collided per plan).  ``jacobian(k)`` -> (J, f0, P) of plan k (default:
    episode_vjp_ref.jacobian at the plan's init_time).  Returns dict(g_params=[per plan], g_task=...)"""
    B, D, T = c["B"], c["D"], c["T"]
    n_plans = len(sim["segs"])
    task_key = "goal" if kind == "reacher" else "hole"
    task = torch.tensor(np.asarray(c[task_key], dtype=np.float64), requires_grad=True)
    q, qd = (torch.tensor(np.asarray(s, dtype=np.float64)) for s in sim["starts"][0])
    ip, iv = (torch.tensor(np.asarray(a, dtype=np.float64)) for a in sim["inits32"][0])       # (the reset state: not differentiated)
    params, loss = [], torch.zeros((), dtype=torch.float64)
    rows_b = torch.arange(B)
    for k in range(n_plans):
        J, f0, P = jacobian(k) if jacobian is not None else E.jacobian(c["mp"], D, T, sim["init_times"][k], c["tau"])
        p = torch.tensor(c["params_k"][k].astype(np.float64), requires_grad=True)
        params.append(p)
        x = torch.cat([p, ip, iv], dim=1)
        des = []
        for j, d32 in enumerate(sim["plans32"][k]):
            lin = torch.tensor(f0[j])[None] + torch.einsum("tdn,bn->btd", torch.tensor(J[j]), x)
            des.append(lin + (torch.tensor(np.asarray(d32, dtype=np.float64)) - lin).detach())
        n_k = np.asarray(sim["segs"][k], np.int32)
        if kind == "reacher":
            ck = dict(c, n_steps=n_k, step0=np.asarray(sim["step0s"][k], np.int32))
            rew, q, qd = R.torch_rollout(ck, des[0], des[1], q, qd, task)[:3]
        else:
            ck = dict(c, n_exec=n_k, step0=np.asarray(sim["step0s"][k], np.int32), collided=np.asarray(sim["collided"][k], np.uint8))
            rew, q, qd = H.torch_rollout(ck, des[0], des[1], q, qd, task)[:3]
        loss = loss + (torch.tensor(np.asarray(w_ret[k], dtype=np.float64)) * _aggregate(rew, n_k, agg)).sum()
        if k + 1 < n_plans:
            if condition:
                rows = torch.as_tensor(tcond(n_k, T))
                ip, iv = des[0][rows_b, rows], des[1][rows_b, rows]      # (float32 values already: the plan is pinned to them)
            else:
                # the float32 cast of the hand-over, pinned to the given float32 values: the identity for the derivative
                ip, iv = (s + (torch.tensor(np.asarray(v32, dtype=np.float64)) - s).detach() for s, v32 in zip((q, qd), sim["inits32"][k + 1]))
    loss = loss + (torch.tensor(np.asarray(w_q, dtype=np.float64)) * q).sum() + (torch.tensor(np.asarray(w_qd, dtype=np.float64)) * qd).sum()
    grads = torch.autograd.grad(loss, params + [task], allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, params + [task])]
    return dict(g_params=[g.numpy() for g in grads[:-1]], g_task=grads[-1].numpy())


def build(name, shape, seed, n_plans=3):
    """episode_vjp_ref.build with the plant on the plan's clock (a BatchedBlackBox has one dt), an episode's worth of parameters
    ``params_k`` [n_plans][B, P], the start state at rest on its float32 image, and the weights of the loss"""
    c = dict(E.build(name, shape, seed))
    rng = np.random.default_rng(seed + 31)
    B, D, P = c["B"], c["D"], c["P"]
    c["dt"] = E.DT_PLAN
    c["params_k"] = [(0.5 * rng.standard_normal((B, P))).astype(np.float32) for _ in range(n_plans)]
    c["q0"] = c["q0"].astype(np.float32).astype(np.float64)
    c["qd0"] = c["qd0"].astype(np.float32).astype(np.float64)
    c["init_pos"], c["init_vel"] = c["q0"].astype(np.float32), c["qd0"].astype(np.float32)
    c["w_ret"] = [rng.uniform(0.5, 1.5, B) for _ in range(n_plans)]
    c["w_q"], c["w_qd"] = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    c["step0"] = np.zeros(B, np.int32)
    return c


def simulate(c, condition, T=T_EPISODE, every=EVERY):
    """the forward of a lockstep episode on the CPU: per plan the oracle's float64 plan rounded to float32, rolled out by
    reacher_vjp_ref from the state the plan before left; the next plan's (init_pos, init_vel) float32 from row tcond or from the state"""
    B = c["B"]
    q, qd = c["q0"], c["qd0"]
    ip, iv = c["init_pos"], c["init_vel"]
    sim = dict(plans32=[], inits32=[], segs=[], step0s=[], init_times=[], starts=[])
    for k, (s0, n) in enumerate(schedule(T, every)):
        it = s0 * E.DT_PLAN
        x = np.concatenate([c["params_k"][k], ip, iv], axis=1).astype(np.float64)
        pos, vel = (a.astype(np.float32) for a in E.plan_f64(c["mp"], c["D"], c["T"], x, it))
        seg, step0 = np.full(B, n, np.int32), np.full(B, s0, np.int32)
        sim["plans32"].append((pos, vel)); sim["inits32"].append((ip, iv)); sim["segs"].append(seg); sim["step0s"].append(step0)
        sim["init_times"].append(it); sim["starts"].append((q, qd))
        _, q, qd, _, _ = R.forward(dict(c, des_pos=pos, des_vel=vel, q0=q, qd0=qd, n_steps=seg, step0=step0))
        if condition:
            rows = tcond(seg, c["T"])
            ip, iv = pos[np.arange(B), rows], vel[np.arange(B), rows]
        else:
            ip, iv = q.astype(np.float32), qd.astype(np.float32)
    return sim


def check_x(what, got, ref, e32=None):
    """the x-output rule of episode_vjp_ref.check for one array: |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the float32-einsum
    error).  Prints the maxima, then asserts"""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    scale = np.abs(r).max() if r.size else 0.0
    e = float(np.max(e32)) if e32 is not None and np.size(e32) else 0.0
    err = np.abs(g - r)
    tol = np.maximum(E.RTOL * scale + E.RTOL * np.abs(r), 4.0 * e)
    print(f"[replan vjp] {what}: max|ref| {scale:.3e}  max err {err.max() if err.size else 0.0:.3e}  f32-einsum err {e:.3e}  "
          f"project rule {E.RTOL * scale:.3e}")
    assert np.isfinite(g).all() and not (err > tol).any(), (what, float(err.max()))
