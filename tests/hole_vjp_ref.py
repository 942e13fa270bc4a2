"""
References for mpk_hole_reacher_rollout_vjp, shared by tests/test_hole_vjp_host.py and tests/test_gpu_hole_vjp.py.

Two independent float64 gradients of the same scalar  L = sum g_r r + sum g_q q_T + sum g_qd qd_T  of the HoleReacher rollout with the
executed steps ``n_exec`` and the collision verdict ``collided`` GIVEN (frozen):
  * ``autograd``: torch autograd through ``torch_rollout``, a torch restatement of the host HoleReacherEnv step loop under
    BlackBoxWrapper.step (controller, np.clip, direct-velocity plant, reward).  Every float32 operation of the numpy flow -- the float32
    action of the velocity / position controllers, acc, its square sum, dt * qd with the float32 dt -- is written as straight-through
    rounding ``x + (x.float().double() - x).detach()``: the forward values equal the host env's bit for bit
    (tests/test_hole_vjp_host.py), the backward is the float64 derivative of the unrounded operations; torch.clamp for the clip (its
    derivative is 1 at a bound);
  * ``numpy_sweep``: the reverse sweep of include/mpk.h (mpk_hole_reacher_rollout_vjp) written out by hand, its forward pass in numpy's
    own float32 / float64 operations.
Inputs follow one recipe (``make_case``); ``conditions`` measures what the tests require of them.
"""
import functools

import numpy as np
import torch

TWO_PI = 2.0 * np.pi
PENALTY = 100.0          # fancy/HoleReacher-v0's collision_penalty
# (B, T, D, act bound, steps_before_reward of rew_fct "simple", rotation of the executed-step counts)
CASES = {
    "b5_t35_d5": (5, 35, 5, TWO_PI, 20, 0),
    "b7_t33_d5_clipped": (7, 33, 5, 0.4, 18, 1),
    "b3_t200_d5_registered": (3, 200, 5, TWO_PI, 199, 0),
    "b23_t40_d3": (23, 40, 3, TWO_PI, 30, 2),
    "b7_t19_d16": (7, 19, 16, TWO_PI, 10, 3),
    "b70_t48_d1": (70, 48, 1, TWO_PI, 40, 4),
    "b7_t16_d6": (7, 16, 6, TWO_PI, 10, 5),
    "b7_t1_d3": (7, 1, 3, TWO_PI, 0, 0),
    "b1000_t200_d5": (1000, 200, 5, TWO_PI, 199, 1),
}
CLIPPED = ("b7_t33_d5_clipped",)
BOTH_REWARDS = ("b5_t35_d5", "b7_t33_d5_clipped", "b3_t200_d5_registered")
CONTROLLERS = ("motor", "velocity", "position")
# every case with the three controllers; the first three with both reward functions
CTRL_CASES = [(n, k, r) for n in CASES for k in CONTROLLERS for r in (("simple", "vel_acc") if n in BOTH_REWARDS else ("simple",))]
DT = 0.01            # HoleReacherEnv.dt: float32(0.01) != 0.01, so the two dtype rules of a step use different constants
SUBSET = 64          # rows of the large case that are compared with the reference
OUTPUTS = ("g_des_pos", "g_des_vel", "g_q0", "g_qd0", "g_hole")
_PER_EPISODE = ("des_pos", "des_vel", "q0", "qd0", "hole", "g_r", "g_q", "g_qd", "n_exec", "collided", "step0")


@functools.lru_cache(maxsize=None)
def make_case(name, controller="motor", rew_fct="simple"):
    """the inputs of one case as a dict of read-only numpy arrays (des_pos / des_vel float32, the rest float64 / int32 / uint8)"""
    index = list(CASES).index(name)
    seed = 100 * index + 10 * CONTROLLERS.index(controller) + ("simple", "vel_acc").index(rew_fct)
    return recipe(name, CASES[name], controller, rew_fct, seed)


def recipe(name, shape, controller, rew_fct, rng_seed):
    """the one recipe of every case: ``shape`` as a CASES entry"""
    B, T, D, bound, sbr, rot = shape
    rng = np.random.default_rng(rng_seed)
    t = np.arange(T)[None, :, None] * DT

    def sinusoid(amp):
        return (rng.uniform(-amp, amp, (B, 1, D)) * np.sin(rng.uniform(0.2, 3.0, (B, 1, D)) * TWO_PI * t
                                                           + rng.uniform(0.0, 7.0, (B, 1, D)))).astype(np.float32)
    q0 = rng.uniform(-0.3, 0.3, (B, D))
    q0[:, 0] = rng.uniform(np.pi / 4, 3 * np.pi / 4, B)
    w = rng.uniform(0.15, 0.5, B)
    c = dict(
        name=name, controller=controller, rew_fct=rew_fct, B=B, T=T, D=D, lo=-bound, hi=bound, dt=DT, penalty=PENALTY,
        sbr=199 if rew_fct == "vel_acc" else sbr,
        pg=1.0 - 0.02 * np.arange(D), dg=0.1 + 0.01 * np.arange(D),           # (the ProDMP id: 1.0 and 0.1)
        des_pos=sinusoid(1.5), des_vel=sinusoid(1.5),
        q0=q0, qd0=rng.uniform(-0.2, 0.2, (B, D)),
        hole=np.stack([rng.choice([-1, 1], B) * rng.uniform(w / 2, 3.5), w, np.ones(B)], axis=1),
        g_r=rng.uniform(0.5, 1.5, (B, T)), g_ret=rng.uniform(0.5, 1.5, B), g_q=rng.standard_normal((B, D)),
        g_qd=rng.standard_normal((B, D)),
    )
    # executed steps T, T - 1, 17, 16, 1, 0 in one batch (rotated per case); the step offsets 0, 1, 2: an episode with offset 0 takes
    # the float64 rule on its first step, the others the float32 rule throughout
    lens = np.minimum(np.array([T, T - 1, 17, 16, 1, 0]), T).clip(min=0)
    n = np.roll(lens, rot)[np.arange(B) % 6].astype(np.int32)
    c["n_exec"] = n
    c["step0"] = (np.arange(B) % 3).astype(np.int32)
    # collided: every other episode that ended early, and the first one that ran the whole plan
    coll = (np.arange(B) % 2 == 0) & (n > 0) & (n < T)
    full = np.flatnonzero(n == T)
    if T > 1 and len(full):
        coll[full[0]] = True
    c["collided"] = coll.astype(np.uint8)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def compared(c):
    """the leading rows of a case that the references cover: all of them up to 256 episodes, SUBSET of a larger case"""
    return SUBSET if c["B"] > 256 else c["B"]


def rows(c, idx):
    """the case restricted to the episodes ``idx`` (episodes are independent)"""
    out = dict(c)
    for k in _PER_EPISODE + ("g_ret",):
        out[k] = c[k][idx]
    out["B"] = len(idx)
    return out


def rnd(x):
    """a float32 rounding of the numpy flow, straight through: the value is rounded, the derivative is the identity"""
    return x + (x.float().double() - x).detach()


def _np_sum(x, add):
    """np.sum of every row of x [B, n] in the order numpy adds a contiguous vector (oracle/mp_oracle.py: np_sum_rows): in index order
    below 8 entries; from 8 on eight accumulators over the whole blocks of eight, combined pairwise, then the remainder in order"""
    n = x.shape[1]
    if n < 8:
        s = x[:, 0]
        for d in range(1, n):
            s = add(s, x[:, d])
        return s
    r = [x[:, j] for j in range(8)]
    i = 8
    while i + 8 <= n:
        r = [add(r[j], x[:, i + j]) for j in range(8)]
        i += 8
    s = add(add(add(r[0], r[1]), add(r[2], r[3])), add(add(r[4], r[5]), add(r[6], r[7])))
    for d in range(i, n):
        s = add(s, x[:, d])
    return s


def _sum32(x):
    """np.sum of a float32 row, every addition rounded to float32"""
    return _np_sum(x, lambda a, b: rnd(a + b))


def _sum64(x):
    return _np_sum(x, lambda a, b: a + b)


def torch_rollout(c, des_pos, des_vel, q0, qd0, hole):
    """the host step loop restated in torch (module docstring): rewards [B, T], final q, qd, and per step the applied actions, the
    controller output u and the distance (for the host comparison and the input conditions)"""
    B, T, D, dt = c["B"], c["T"], c["D"], c["dt"]
    dt32 = float(np.float32(dt))
    motor, vel_acc = c["controller"] == "motor", c["rew_fct"] == "vel_acc"
    pg, dg = torch.tensor(c["pg"]), torch.tensor(c["dg"])
    n, s0 = torch.tensor(c["n_exec"].astype(np.int64)), torch.tensor(c["step0"].astype(np.int64))
    coll = torch.tensor(c["collided"].astype(bool))
    q, qd = q0, qd0
    rewards, acts, us, dists = [], [], [], []
    zero = torch.zeros(B, dtype=torch.float64)
    for t in range(T):
        live, s = t < n, s0 + t
        if motor:
            u = pg * (des_pos[:, t] - q) + dg * (des_vel[:, t] - qd)
        elif c["controller"] == "position":
            u = des_pos[:, t]
        else:
            u = des_vel[:, t]
        a = torch.clamp(u, c["lo"], c["hi"])
        if motor:
            acc = (a - qd) / dt
            qd_n = a
            q_n = q + dt * qd_n
            acc_cost, vel_cost = _sum64(acc * acc), _sum64(qd_n * qd_n)
        else:
            # the float32 action becomes qd: from the episode's second env step on acc is a float32 operation, dt * qd always is
            f32 = s > 0
            a32 = rnd(a)
            acc32 = rnd(rnd(a32 - rnd(qd)) / dt32)
            acc64 = (a - qd) / dt
            acc = torch.where(f32[:, None], acc32, acc64)
            qd_n = torch.where(f32[:, None], a32, a)
            q_n = q + rnd(dt32 * a32)
            acc_cost = torch.where(f32, _sum32(rnd(acc32 * acc32)), _sum64(acc64 * acc64))
            v32 = rnd(qd_n)
            vel_cost = _sum32(rnd(v32 * v32))
            a = a32
        ang = torch.cumsum(q_n, dim=1)
        ex = torch.cumsum(torch.cos(ang), dim=1)[:, -1]
        ey = torch.cumsum(torch.sin(ang), dim=1)[:, -1]
        dx, dy = ex - hole[:, 0], ey - (0.0 - hole[:, 2])
        dist = torch.sqrt(dx * dx + dy * dy)
        last = coll & (t == n - 1)
        lastf = last.double()
        if vel_acc:
            paid = s == 199
            dist_cost = torch.where(paid, dist ** 2, zero)
            r = ((dist_cost * -1.0 + vel_cost * -1e-4) + acc_cost * -1e-6) + (lastf * dist_cost) * -c["penalty"]
        else:
            paid = (s == c["sbr"]) | last
            dist_cost = torch.where(paid, dist ** 2, zero)
            r = (dist_cost * -1.0 + acc_cost * -5e-8) + lastf * -c["penalty"]
        rewards.append(torch.where(live, r, zero))
        acts.append(torch.where(live[:, None], a, torch.zeros_like(a)))
        qd = torch.where(live[:, None], qd_n, qd)
        q = torch.where(live[:, None], q_n, q)
        us.append(u)
        dists.append(dist)
    return torch.stack(rewards, dim=1), q, qd, torch.stack(acts, dim=1), torch.stack(us, dim=1), torch.stack(dists, dim=1)


def _leaves(c, grad):
    return [torch.tensor(np.asarray(c[k], dtype=np.float64), requires_grad=grad) for k in ("des_pos", "des_vel", "q0", "qd0", "hole")]


def forward(c):
    """(rewards, q, qd, actions, u, dist) of the restatement as numpy arrays"""
    with torch.no_grad():
        return tuple(x.numpy() for x in torch_rollout(c, *_leaves(c, False)))


def loss_value(c, des_pos=None, use=(True, True, True)):
    """L in float64 for the case's upstream gradients (``des_pos``: a float32 array that replaces the case's)"""
    cc = dict(c) if des_pos is None else dict(c, des_pos=des_pos)
    rew, q, qd = forward(cc)[:3]
    return float((c["g_r"] * rew).sum() * use[0] + (c["g_q"] * q).sum() * use[1] + (c["g_qd"] * qd).sum() * use[2])


def expand_g_ret(c, agg, g_ret=None):
    """the step-reward gradients an aggregate's gradient stands for: g_ret w_t for t < n_exec, w_t = 1 (sum), 1 / n_exec (mean: g_ret /
    n_exec) or [t == n_exec - 1] (last)"""
    g = (c["g_ret"] if g_ret is None else g_ret)[:, None]
    t, n = np.arange(c["T"])[None], c["n_exec"][:, None]
    if agg == "mean":
        g = g / np.maximum(n, 1).astype(np.float64)
    return np.where((t == n - 1) if agg == "last" else (t < n), g, 0.0)


def autograd(c, use=(True, True, True)):
    """dict of the five gradients by torch autograd; ``use[i]`` False: upstream gradient i (g_r, g_q, g_qd) is absent (0)"""
    leaves = _leaves(c, True)
    rew, q, qd = torch_rollout(c, *leaves)[:3]
    loss = rew.sum() * 0.0
    if use[0]:
        loss = loss + (torch.tensor(c["g_r"]) * rew).sum()
    if use[1]:
        loss = loss + (torch.tensor(c["g_q"]) * q).sum()
    if use[2]:
        loss = loss + (torch.tensor(c["g_qd"]) * qd).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return {k: (np.zeros_like(l.detach().numpy()) if g is None else g.numpy()) for k, g, l in zip(OUTPUTS, grads, leaves)}


def numpy_sweep(c, use=(True, True, True)):
    """the reverse sweep of include/mpk.h written out: forward pass in numpy's own dtypes keeping (acc, m, q', qd', delta) of every
    step, then t = n - 1 .. 0"""
    B, T, D, dt, lo, hi = c["B"], c["T"], c["D"], c["dt"], c["lo"], c["hi"]
    dt32 = np.float32(dt)
    motor, vel_acc = c["controller"] == "motor", c["rew_fct"] == "vel_acc"
    pg, dg, n, s0, coll = c["pg"], c["dg"], c["n_exec"], c["step0"], c["collided"].astype(bool)
    dp, dv = c["des_pos"].astype(np.float64), c["des_vel"].astype(np.float64)
    q, qd = c["q0"].copy(), c["qd0"].copy()
    ACC, M, QN, VN, DEL = (np.zeros((T, B, D)) for _ in range(5))
    for t in range(T):
        live = (t < n)[:, None]
        u = pg * (dp[:, t] - q) + dg * (dv[:, t] - qd) if motor else (dp[:, t] if c["controller"] == "position" else dv[:, t])
        a = np.clip(u, lo, hi)
        if motor:
            acc, qd_n = (a - qd) / dt, a
            q_n = q + dt * qd_n
            vn, delta = qd_n, np.full((B, 1), dt)
        else:
            f32 = (s0 + t > 0)[:, None]
            a32 = a.astype(np.float32)
            acc = np.where(f32, ((a32 - qd.astype(np.float32)) / dt32).astype(np.float64), (a - qd) / dt)
            qd_n = np.where(f32, a32.astype(np.float64), a)
            q_n = q + (dt32 * a32).astype(np.float64)
            vn, delta = qd_n.astype(np.float32).astype(np.float64), np.where(f32, np.float64(dt32), dt)
        ACC[t], M[t], QN[t], VN[t], DEL[t] = acc, (lo <= u) & (u <= hi), q_n, vn, delta
        qd, q = np.where(live, qd_n, qd), np.where(live, q_n, q)
    deltap = dt if motor else np.float64(dt32)
    c_acc = -1e-6 if vel_acc else -5e-8
    g_r = c["g_r"] if use[0] else np.zeros((B, T))
    lq = c["g_q"].copy() if use[1] else np.zeros((B, D))
    lqd = c["g_qd"].copy() if use[2] else np.zeros((B, D))
    g_pos, g_vel, g_hole = np.zeros((B, T, D)), np.zeros((B, T, D)), np.zeros((B, 3))
    for t in range(T - 1, -1, -1):
        live = t < n
        last = coll & (t == n - 1)
        gr = np.where(live, g_r[:, t], 0.0)
        if vel_acc:
            W = (s0 + t == 199) * (1.0 + c["penalty"] * last)
        else:
            W = ((s0 + t == c["sbr"]) | last).astype(np.float64)
        W = np.where(live, W, 0.0)
        ang = np.cumsum(QN[t], axis=1)
        sn, cs = np.sin(ang), np.cos(ang)
        diff = np.stack([cs.sum(1) - c["hole"][:, 0], sn.sum(1) + c["hole"][:, 2]], axis=1)
        sx = np.cumsum((-sn)[:, ::-1], axis=1)[:, ::-1]           # sum_{l >= j} -sin c_l
        sy = np.cumsum(cs[:, ::-1], axis=1)[:, ::-1]
        k2 = 2.0 * gr * W
        lq = lq - k2[:, None] * (diff[:, :1] * sx + diff[:, 1:] * sy)
        g_hole[:, 0] += k2 * diff[:, 0]
        g_hole[:, 2] -= k2 * diff[:, 1]
        lqd_n = lqd + (-2e-4 * gr)[:, None] * VN[t] if vel_acc else lqd
        lacc = 2.0 * c_acc * gr[:, None] * ACC[t]
        la = deltap * lq + lqd_n + lacc / DEL[t]
        lu = np.where(live[:, None] & (M[t] > 0), la, 0.0)
        lqd = np.where(live[:, None], -lacc / DEL[t], lqd)
        if motor:
            g_pos[:, t], g_vel[:, t] = pg * lu, dg * lu
            lq, lqd = lq - pg * lu, lqd - dg * lu
        elif c["controller"] == "position":
            g_pos[:, t] = lu
        else:
            g_vel[:, t] = lu
    return dict(g_des_pos=g_pos, g_des_vel=g_vel, g_q0=lq, g_qd0=lqd, g_hole=g_hole)


def paid_steps(c):
    """[B, T] bool: the executed steps that pay a distance term"""
    t = np.arange(c["T"])[None]
    n, s = c["n_exec"][:, None], c["step0"][:, None] + t
    live = t < n
    if c["rew_fct"] == "vel_acc":
        return live & (s == 199)
    return live & ((s == c["sbr"]) | (c["collided"].astype(bool)[:, None] & (t == n - 1)))


def conditions(c):
    """what the tests require of the inputs: min |u - bound| and the saturated fraction over the live (t, d), min dist over the paid steps"""
    u, dist = forward(c)[4:6]
    live = np.arange(c["T"])[None] < c["n_exec"][:, None]
    paid = paid_steps(c)
    ul = u[live]
    return dict(bound_gap=float(np.minimum(np.abs(ul - c["lo"]), np.abs(ul - c["hi"])).min()),
                saturated=float(((ul < c["lo"]) | (ul > c["hi"])).mean()),
                min_dist=float(dist[paid].min()) if paid.any() else np.inf, n_paid=int(paid.sum()))


def kernel_name(c):
    """the instantiation mpk_last_kernel must name for a case: D = 5 is compiled in, every other D runs the run-time-D instantiation"""
    tail = ", 5>" if c["D"] == 5 else ">"
    return f"k_hole_rollout_vjp<{c['controller']}, {c['rew_fct']}{tail}"


@functools.lru_cache(maxsize=None)
def reference(name, controller="motor", rew_fct="simple", use=(True, True, True)):
    """the autograd gradients of a case (the large case: of its first SUBSET rows), computed once and shared; read-only"""
    c = make_case(name, controller, rew_fct)
    if compared(c) < c["B"]:
        c = rows(c, np.arange(compared(c)))
    ref = autograd(c, use)
    for v in ref.values():
        v.setflags(write=False)
    return ref
