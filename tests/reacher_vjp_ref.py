"""
References for mpk_reacher_rollout_vjp, shared by tests/test_reacher_vjp_host.py and tests/test_gpu_reacher_vjp.py.

Two independent float64 gradients of the same scalar  L = sum g_r r + sum g_q q_T + sum g_qd qd_T  of oracle.reacher_rollout:
  * ``autograd``: torch autograd through ``torch_rollout``, a float64 CPU restatement of oracle.reacher_rollout with torch.clamp (its
    derivative is 1 at a bound); the leaves are float64 tensors that hold the fp32 values of the desired trajectory;
  * ``numpy_sweep``: the reverse sweep of include/mpk.h (mpk_reacher_rollout_vjp) written out by hand in numpy.
Inputs follow one recipe (``make_case``); ``conditions`` measures what the tests require of them (distance of every controller output
to a clip bound, distance to the goal at paid steps, the saturated fraction).
"""
import functools

import numpy as np
import torch

# (B, T, D, act_low, act_high, steps_before_reward, dt)
CASES = {
    "b5_t35_d2": (5, 35, 2, -1000.0, 1000.0, 30, 0.1),
    "b5_t35_d5_clipped_all_paid": (5, 35, 5, -0.4, 0.6, 0, 0.1),
    "b3_t200_d5_registered": (3, 200, 5, -1000.0, 1000.0, 199, 0.01),
    "b7_t33_d7_clipped": (7, 33, 7, -0.3, 0.45, 20, 0.1),
    "b1000_t200_d5": (1000, 200, 5, -1000.0, 1000.0, 199, 0.01),
    # appended (the seed and the n_steps rotation depend on a case's index): the DoF counts that are not compiled in -- the run-time-D
    # instantiations, idle lanes at D = 3 and 6, 64 and 4 episodes per wave at D = 1 and 16 --, a part-full last wave behind a full one
    # (70 = 64 + 6, 23 = 21 + 2, 19 = 16 + 3), T on a tile boundary, a single tile, a single step (n_steps of 17 above T), and two
    # horizons whose checkpoints take the launch above 64 KB of LDS
    "b70_t48_d1": (70, 48, 1, -1000.0, 1000.0, 40, 0.1),
    "b23_t40_d3": (23, 40, 3, -1000.0, 1000.0, 30, 0.1),
    "b19_t33_d4_clipped": (19, 33, 4, -0.4, 0.6, 20, 0.1),
    "b9_t32_d8": (9, 32, 8, -1000.0, 1000.0, 25, 0.1),
    "b7_t19_d16": (7, 19, 16, -1000.0, 1000.0, 10, 0.1),
    "b7_t16_d6": (7, 16, 6, -1000.0, 1000.0, 10, 0.1),
    "b7_t1_d3": (7, 1, 3, -1000.0, 1000.0, 0, 0.1),
    "b4_t2000_d5_long": (4, 2000, 5, -1000.0, 1000.0, 1990, 0.01),
    "b4_t2000_d1_long": (4, 2000, 1, -1000.0, 1000.0, 1990, 0.01),
}
CLIPPED = ("b5_t35_d5_clipped_all_paid", "b7_t33_d7_clipped", "b19_t33_d4_clipped")
ORIGINAL = tuple(CASES)[:5]                                   # the references of these agree to 1e-15
LONG = ("b4_t2000_d5_long", "b4_t2000_d1_long")               # seconds of autograd each: the motor controller only
# every case with the motor controller; the first two and the appended short ones with the other two as well
CTRL_CASES = [(n, "motor") for n in CASES] + \
             [(n, k) for n in CASES if n in ORIGINAL[:2] or (n not in ORIGINAL and n not in LONG) for k in ("position", "velocity")]
COMPILED_D = (2, 5, 7)                                        # k_reacher_rollout_vjp<ctrl, D>; every other D: <ctrl>
SUBSET = 64          # rows of the large case that are compared with the reference
OUTPUTS = ("g_des_pos", "g_des_vel", "g_q0", "g_qd0", "g_goal")


@functools.lru_cache(maxsize=None)
def make_case(name, controller="motor", seed=0):
    """the inputs of one case as a dict of read-only numpy arrays (des_pos / des_vel float32, the rest float64 / int32)"""
    index = list(CASES).index(name)
    return recipe(name, CASES[name], controller, 1000 * seed + 17 * index + {"motor": 0, "position": 1, "velocity": 2}[controller], index)


def recipe(name, shape, controller, rng_seed, rot):
    """the one recipe of every case: ``shape`` as a CASES entry, ``rot`` rotates the executed-step counts"""
    B, T, D, lo, hi, sbr, dt = shape
    rng = np.random.default_rng(rng_seed)
    t = np.arange(T)[None, :, None] / T
    amp = rng.uniform(-1.0, 1.0, (B, 1, D))
    freq = rng.uniform(0.5, 2.0, (B, 1, D))
    ph = rng.uniform(0.0, 2.0 * np.pi, (B, 1, D))
    c = dict(
        name=name, controller=controller, B=B, T=T, D=D, lo=lo, hi=hi, sbr=sbr, dt=dt,
        pg=np.full(D, 0.6), dg=0.075 + 0.01 * np.arange(D),
        des_pos=(amp * np.sin(2.0 * np.pi * freq * t + ph)).astype(np.float32),
        des_vel=rng.uniform(-1.0, 1.0, (B, T, D)).astype(np.float32),
        q0=rng.uniform(-0.5, 0.5, (B, D)), qd0=rng.uniform(-0.2, 0.2, (B, D)),
        goal=rng.uniform(-D / 2.0, D / 2.0, (B, 2)),
        g_r=rng.uniform(0.5, 1.5, (B, T)), g_q=rng.standard_normal((B, D)), g_qd=rng.standard_normal((B, D)),
    )
    # executed steps T, T - 1, 17, 16, 1, 0 in one batch (rotated per case so that the five-episode cases see all of them between
    # them); a different step offset per episode
    lens = np.array([T, T - 1, 17, 16, 1, 0])
    c["n_steps"] = np.roll(lens, rot)[np.arange(B) % 6].astype(np.int32)
    c["step0"] = (np.arange(B) % 3).astype(np.int32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def at_the_goal():
    """two one-link episodes under the position controller, every step paid: episode 0 sits on its goal throughout (des_pos = q0 = qd0 =
    0, goal = (1, 0): q' = 0 and the end effector is (cos 0, sin 0), dist exactly 0) with non-zero upstream gradients, episode 1 is an
    ordinary row of the recipe"""
    base = recipe("at_the_goal", (2, 20, 1, -1000.0, 1000.0, 0, 0.1), "position", 777, 0)
    c = dict(base)
    for k in ("des_pos", "q0", "qd0", "goal"):
        c[k] = base[k].copy()
        c[k][0] = 0.0
    c["goal"][0] = (1.0, 0.0)
    c["n_steps"], c["step0"] = np.array([20, 20], np.int32), np.array([0, 0], np.int32)
    return c


def compared(c):
    """the leading rows of a case that the references cover: all of them up to 256 episodes, SUBSET of a larger case"""
    return SUBSET if c["B"] > 256 else c["B"]


def rows(c, idx):
    """the case restricted to the episodes ``idx`` (episodes are independent)"""
    out = dict(c)
    for k in ("des_pos", "des_vel", "q0", "qd0", "goal", "g_r", "g_q", "g_qd", "n_steps", "step0"):
        out[k] = c[k][idx]
    out["B"] = len(idx)
    return out


def _np_sum(x):
    """np.sum of every row of x [B, n] in the order numpy adds a contiguous vector (oracle.np_sum_rows, in torch): in index order
    below 8 entries; from 8 on eight accumulators over the whole blocks of eight, combined pairwise, then the remainder in order"""
    n = x.shape[1]
    if n < 8:
        s = x[:, 0]
        for d in range(1, n):
            s = s + x[:, d]
        return s
    r = [x[:, j] for j in range(8)]
    i = 8
    while i + 8 <= n:
        r = [r[j] + x[:, i + j] for j in range(8)]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for d in range(i, n):
        s = s + x[:, d]
    return s


def torch_rollout(c, des_pos, des_vel, q0, qd0, goal):
    """oracle.reacher_rollout restated in float64 torch ops (same operations in the same order): rewards [B, T], final q, qd, and the
    per-step controller output u and distance (for the input conditions)"""
    B, T, D, dt = c["B"], c["T"], c["D"], c["dt"]
    pg, dg = torch.tensor(c["pg"]), torch.tensor(c["dg"])
    n, s0 = torch.tensor(c["n_steps"].astype(np.int64)), torch.tensor(c["step0"].astype(np.int64))
    q, qd = q0, qd0
    rewards, us, dists = [], [], []
    for t in range(T):
        live = t < n
        if c["controller"] == "motor":
            u = pg * (des_pos[:, t] - q) + dg * (des_vel[:, t] - qd)
        elif c["controller"] == "position":
            u = des_pos[:, t]
        else:
            u = des_vel[:, t]
        a = torch.clamp(u, c["lo"], c["hi"])
        qd_n = qd + dt * a
        q_n = q + dt * qd_n
        ang = torch.cumsum(q_n, dim=1)
        ex = torch.cumsum(torch.cos(ang), dim=1)[:, -1]
        ey = torch.cumsum(torch.sin(ang), dim=1)[:, -1]
        dx, dy = ex - goal[:, 0], ey - goal[:, 1]
        dist = torch.sqrt(dx * dx + dy * dy)
        ctrl = _np_sum(a * a)
        r = torch.where(s0 + t >= c["sbr"], 0.0 - dist, torch.zeros_like(dist)) - ctrl
        rewards.append(torch.where(live, r, torch.zeros_like(r)))
        qd = torch.where(live[:, None], qd_n, qd)
        q = torch.where(live[:, None], q_n, q)
        us.append(u)
        dists.append(dist)
    return torch.stack(rewards, dim=1), q, qd, torch.stack(us, dim=1), torch.stack(dists, dim=1)


def _leaves(c, grad):
    return [torch.tensor(np.asarray(c[k], dtype=np.float64), requires_grad=grad) for k in ("des_pos", "des_vel", "q0", "qd0", "goal")]


def forward(c):
    """(rewards, q, qd, u, dist) of the restatement as numpy arrays"""
    with torch.no_grad():
        return tuple(x.numpy() for x in torch_rollout(c, *_leaves(c, False)))


def loss_value(c, des_pos=None, use=(True, True, True)):
    """L in float64 for the case's upstream gradients (``des_pos``: a float32 array that replaces the case's)"""
    cc = dict(c) if des_pos is None else dict(c, des_pos=des_pos)
    rew, q, qd, _, _ = forward(cc)
    return float((c["g_r"] * rew).sum() * use[0] + (c["g_q"] * q).sum() * use[1] + (c["g_qd"] * qd).sum() * use[2])


def autograd(c, use=(True, True, True)):
    """dict of the five gradients by torch autograd; ``use[i]`` False: upstream gradient i (g_r, g_q, g_qd) is absent (0)"""
    leaves = _leaves(c, True)
    rew, q, qd, _, _ = torch_rollout(c, *leaves)
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
    """the reverse sweep of include/mpk.h written out: forward pass keeping (a, m, q') of every step, then t = n - 1 .. 0"""
    B, T, D, dt, lo, hi = c["B"], c["T"], c["D"], c["dt"], c["lo"], c["hi"]
    pg, dg, n, s0 = c["pg"], c["dg"], c["n_steps"], c["step0"]
    dp, dv = c["des_pos"].astype(np.float64), c["des_vel"].astype(np.float64)
    q, qd = c["q0"].copy(), c["qd0"].copy()
    A, M, QN = np.zeros((T, B, D)), np.zeros((T, B, D), bool), np.zeros((T, B, D))
    for t in range(T):
        live = (t < n)[:, None]
        u = pg * (dp[:, t] - q) + dg * (dv[:, t] - qd) if c["controller"] == "motor" else (dp[:, t] if c["controller"] == "position" else dv[:, t])
        a = np.clip(u, lo, hi)
        qd_n = qd + dt * a
        q_n = q + dt * qd_n
        A[t], M[t], QN[t] = a, (lo <= u) & (u <= hi), q_n
        qd, q = np.where(live, qd_n, qd), np.where(live, q_n, q)
    g_r = c["g_r"] if use[0] else np.zeros((B, T))
    lq = c["g_q"].copy() if use[1] else np.zeros((B, D))
    lqd = c["g_qd"].copy() if use[2] else np.zeros((B, D))
    g_pos, g_vel, g_goal = np.zeros((B, T, D)), np.zeros((B, T, D)), np.zeros((B, 2))
    for t in range(T - 1, -1, -1):
        live = t < n
        paid = live & (s0 + t >= c["sbr"])
        gr = np.where(live, g_r[:, t], 0.0)
        ang = np.cumsum(QN[t], axis=1)
        sn, cs = np.sin(ang), np.cos(ang)
        diff = np.stack([cs.sum(1), sn.sum(1)], axis=1) - c["goal"]
        dist = np.sqrt((diff * diff).sum(1))
        sx = np.cumsum((-sn)[:, ::-1], axis=1)[:, ::-1]           # sum_{l >= j} -sin c_l
        sy = np.cumsum(cs[:, ::-1], axis=1)[:, ::-1]
        w = np.where(paid & (dist > 0.0), gr / np.where(dist > 0.0, dist, 1.0), 0.0)   # (mpk.h: dist = 0 contributes no distance term)
        lq = lq - w[:, None] * (diff[:, :1] * sx + diff[:, 1:] * sy)
        g_goal = g_goal + w[:, None] * diff
        lqd_n = lqd + dt * lq
        la = dt * lqd_n - 2.0 * A[t] * gr[:, None]
        lu = np.where(live[:, None] & M[t], la, 0.0)
        lqd = np.where(live[:, None], lqd_n, lqd)
        if c["controller"] == "motor":
            g_pos[:, t], g_vel[:, t] = pg * lu, dg * lu
            lq, lqd = lq - pg * lu, lqd - dg * lu
        elif c["controller"] == "position":
            g_pos[:, t] = lu
        else:
            g_vel[:, t] = lu
    return dict(g_des_pos=g_pos, g_des_vel=g_vel, g_q0=lq, g_qd0=lqd, g_goal=g_goal)


def conditions(c):
    """what the tests require of the inputs: min |u - bound| and the saturated fraction over the live (t, d), min dist over the paid steps"""
    _, _, _, u, dist = forward(c)
    t = np.arange(c["T"])[None]
    live = t < c["n_steps"][:, None]
    paid = live & (c["step0"][:, None] + t >= c["sbr"])
    ul = u[live]
    return dict(bound_gap=float(np.minimum(np.abs(ul - c["lo"]), np.abs(ul - c["hi"])).min()),
                saturated=float(((ul < c["lo"]) | (ul > c["hi"])).mean()),
                min_dist=float(dist[paid].min()) if paid.any() else np.inf, n_paid=int(paid.sum()))


def kernel_name(c):
    """the instantiation mpk_last_kernel must name for a case"""
    return f"k_reacher_rollout_vjp<{c['controller']}, {c['D']}>" if c["D"] in COMPILED_D else f"k_reacher_rollout_vjp<{c['controller']}>"


@functools.lru_cache(maxsize=None)
def reference(name, controller="motor", use=(True, True, True)):
    """the autograd gradients of a case (the large case: of its first SUBSET rows), computed once and shared; read-only"""
    c = make_case(name, controller)
    if compared(c) < c["B"]:
        c = rows(c, np.arange(compared(c)))
    ref = autograd(c, use)
    for v in ref.values():
        v.setflags(write=False)
    return ref
