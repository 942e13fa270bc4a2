#!/usr/bin/env python3
"""
Reference-generated fixture for HoleReacher (build container only: reads /root/reference).

The reference package cannot be imported here (gymnasium / matplotlib are absent), so -- as make_ref_validity_golden.py does --
the FunctionDefs the step loop runs are taken from their files with `ast` and compiled ALONE, then bound to a plain class:
BaseReacherDirectEnv.step, BaseReacherEnv._update_joints / _check_self_collision, HoleReacherEnv._get_reward / _get_line_points /
check_wall_collision / _check_collisions / _terminate, HolereacherReward.__init__ / reset / get_reward, and ccw / intersect of
utils.py.  No reference text is stored.  The driver is the loop of BlackBoxWrapper.step (black_box_wrapper.py:175-203): controller,
np.clip to the float32 action bounds, env.step, break on terminated / truncated (TimeLimit 200).

Output: tests/golden/ref_hole_reacher.npz, one row per episode (n_links = 5, T = 200):
  ctrl int [E] (0 motor, 1 velocity), q0 / qd0 float64 [E, D] state at plan start, step0 int [E], n_steps int [E] (steps the plan may
  run: 200 - step0), hole float64 [E, 3], penalty float64 [E], allow_self / allow_wall bool [E], des_pos / des_vel float32 [E, T, D],
  actions float32 [E, T, D] / rewards float64 [E, T] (0 after the break), q / qd float64 [E, D] after the plan, n_exec int [E],
  collided / success bool [E], kind int [E] (0 none, 1 joint limit, 2 links crossing, 3 wall), margin float64 [E] (the smallest
  distance of a deciding comparison to its threshold over the executed steps), family str [E];
  mp_config (json of the merged mp_config of the four ids), meta (numpy version, sha256 of this file and of every reference file).

    python tests/golden/make_ref_hole_reacher_golden.py [--check]
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np

REF = "/root/reference/fancy_gym/envs/classic_control"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_hole_reacher.npz")
D, T, DT = 5, 200, 0.01
F32 = np.float32

_read = {}


def src(name):
    with open(os.path.join(REF, name), "rb") as f:
        data = f.read()
    _read[name] = hashlib.sha256(data).hexdigest()
    return data.decode()


def functions(name, wanted, cls=None):
    """the FunctionDefs `wanted` of file `name` (inside class `cls` if given), each compiled alone"""
    tree = ast.parse(src(name), filename=name)
    scope = tree.body
    if cls is not None:
        scope = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    out = {}
    for node in scope:
        if isinstance(node, ast.FunctionDef) and node.name in wanted:
            node.decorator_list = []
            out[node.name] = compile(ast.Module(body=[node], type_ignores=[]), f"{name}:{node.name}", "exec")
    assert sorted(out) == sorted(wanted), (name, sorted(out))
    return out


def build_classes():
    ns = {"np": np}
    for c in functions("utils.py", ["ccw", "intersect"]).values():
        exec(c, ns)
    pieces = [("base_reacher/base_reacher_direct.py", ["step"], "BaseReacherDirectEnv"),
              ("base_reacher/base_reacher.py", ["_update_joints", "_check_self_collision"], "BaseReacherEnv"),
              ("hole_reacher/hole_reacher.py", ["_get_reward", "_get_line_points", "check_wall_collision", "_check_collisions",
                                                "_terminate"], "HoleReacherEnv")]
    env_methods = {}
    for name, wanted, cls in pieces:
        for fn, c in functions(name, wanted, cls).items():
            exec(c, ns)
            env_methods[fn] = ns[fn]
    rew_methods = {}
    for fn, c in functions("hole_reacher/hr_simple_reward.py", ["__init__", "reset", "get_reward"], "HolereacherReward").items():
        exec(c, ns)
        rew_methods[fn] = ns[fn]
    Reward = type("HolereacherReward", (), rew_methods)

    class Env:
        dt = DT

        def __init__(self, q0, qd0, steps, hole, penalty, allow_self, allow_wall):
            self.n_links = D
            self.link_lengths = np.ones(D)
            self.j_min, self.j_max = -np.pi * np.ones(D), np.pi * np.ones(D)
            self.allow_self_collision = allow_self
            self._joints = np.zeros((D + 1, 2))
            self._joint_angles, self._angle_velocity, self._steps = q0, qd0, steps
            self._tmp_x, self._tmp_width, self._tmp_depth = hole
            self._goal = np.hstack([self._tmp_x, -self._tmp_depth])
            self.reward_function = Reward(allow_self, allow_wall, penalty)
            self.reward_function.reset()
            self._update_joints()

        @property
        def end_effector(self):            # BaseReacherEnv.end_effector (base_reacher.py:141-143)
            return self._joints[self.n_links].T

        def _get_obs(self):
            return np.zeros(1)

    for fn, f in env_methods.items():
        setattr(Env, fn, f)
    return Env


def mp_configs():
    """the merged mp_config of fancy_ProMP / fancy_DMP / fancy_ProDMP/HoleReacher-v0 (defaults <- the wrapper's mp_config)"""
    tree = ast.parse(src("hole_reacher/mp_wrapper.py"))
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MPWrapper")
    node = next(n for n in cls.body if isinstance(n, ast.Assign) and n.targets[0].id == "mp_config")
    cfg = ast.literal_eval(node.value)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from fancy_gym_amd.envs.registry import resolve_mp_config
    return {mp: resolve_mp_config(mp, cfg) for mp in ("ProMP", "DMP", "ProDMP")}


def margins(env):
    """smallest distance of the comparisons that decide this step's collision flags to their thresholds"""
    m = np.inf
    if not env.allow_self_collision:
        q = env._joint_angles
        m = min(m, float(np.min(np.abs(np.pi - np.abs(q)))))
        j = env._joints
        for i in range(D):
            for k in range(i + 2, D):
                A, B, C, E = j[i], j[i + 1], j[k], j[k + 1]
                for a, b, c in ((A, C, E), (B, C, E), (A, B, C), (A, B, E)):
                    v = (c[1] - a[1]) * (b[0] - a[0]) - (b[1] - a[1]) * (c[0] - a[0])
                    m = min(m, abs(v - 1e-12))
    if not env.reward_function.allow_wall_collision:
        p = env._get_line_points(num_points_per_link=100)
        px, py = p[..., 0], p[..., 1]
        hl, hr = env._tmp_x - env._tmp_width / 2, env._tmp_x + env._tmp_width / 2
        # (the first point of the first link is the origin, exactly, in every implementation: not a deciding comparison)
        px, py = px.ravel()[1:], py.ravel()[1:]
        # a region holds a point iff min over the points of the largest signed distance to its bounds is < 0
        for region in (np.maximum(px - hl, py), np.maximum(hr - px, py),
                       np.maximum(np.maximum(hl - px, px - hr), py + env._tmp_depth)):
            m = min(m, abs(float(np.min(region))))
    return m


def run_plan(Env, ctrl, q0, qd0, step0, hole, penalty, allow_self, allow_wall, dpos, dvel):
    env = Env(q0.copy(), qd0.copy() if isinstance(qd0, np.ndarray) else qd0, step0, hole, penalty, allow_self, allow_wall)
    low, high = -np.ones(D, F32) * F32(2 * np.pi), np.ones(D, F32) * F32(2 * np.pi)
    acts, rews = np.zeros((T, D), F32), np.zeros(T)
    n_steps = T - step0
    collided = success = False
    kind, margin, n = 0, np.inf, 0
    for t in range(n_steps):
        if ctrl == 1:
            a = dvel[t]
        else:
            a = 1.0 * (dpos[t] - env._joint_angles) + 0.1 * (dvel[t] - env._angle_velocity)
        a = np.clip(a, low, high)
        _, r, terminated, truncated, info = env.step(a)
        truncated = env._steps >= 200
        acts[t], rews[t] = a, r
        n = t + 1
        margin = min(margin, margins(env))
        if env._steps - 1 == 199 or info["is_collided"]:
            margin = min(margin, abs(float(np.linalg.norm(env.end_effector - env._goal)) - 0.005))
        success = bool(info["is_success"])
        if terminated:
            collided = True
            if not allow_self and (np.any(env._joint_angles > env.j_max) or np.any(env._joint_angles < env.j_min)):
                kind = 1
            elif env._check_self_collision():
                kind = 2
            else:
                kind = 3
        if terminated or truncated:
            break
    return dict(actions=acts, rewards=rews, q=np.asarray(env._joint_angles, np.float64),
                qd=np.asarray(env._angle_velocity, np.float64), n_exec=n, collided=collided, success=success, kind=kind,
                margin=margin, n_steps=n_steps, env=env)


def smooth(rng, amp, n=T):
    """a float32 velocity profile: a few random sinusoids, on a grid of 2^-8 rad/s (the fixture compresses)"""
    t = np.arange(n)[:, None] * DT
    out = np.zeros((n, D))
    for _ in range(3):
        out += rng.uniform(-amp, amp, D) * np.sin(rng.uniform(0.2, 3.0, D) * t * 2 * np.pi + rng.uniform(0, 2 * np.pi, D))
    return grid(out)


def grid(x, bits=8):
    """float32 values on a grid of 2^-bits"""
    return (np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F32)


def draw_hole(rng):
    width = rng.uniform(0.15, 0.5)
    x = rng.choice([-1, 1]) * rng.uniform(width / 2, 3.5)
    return np.array([x, width, 1.0])


def generate():
    Env = build_classes()
    rows = []
    rng = np.random.default_rng(20261015)

    def add(family, ctrl, q0, qd0, step0, hole, penalty, allow_self, allow_wall, dpos, dvel):
        r = run_plan(Env, ctrl, q0, qd0, step0, hole, penalty, allow_self, allow_wall, dpos, dvel)
        r.pop("env")
        qd_in = np.asarray(qd0, np.float64) if isinstance(qd0, np.ndarray) else np.zeros(D)
        rows.append(dict(r, family=family, ctrl=ctrl, q0=q0.astype(np.float64), qd0=qd_in, step0=step0, hole=np.asarray(hole, np.float64),
                         penalty=float(penalty), allow_self=allow_self, allow_wall=allow_wall, des_pos=dpos, des_vel=dvel))
        return r

    def start(rng):
        q = np.zeros(D)
        q[0] = rng.uniform(np.pi / 4, 3 * np.pi / 4)
        return q

    zeros = np.zeros((T, D), F32)
    # seeded plans, velocity controller: random starts, sampled holes
    for _ in range(40):
        hole = draw_hole(rng)
        add("velocity", 1, start(rng), np.zeros(D), 0, hole, 100, False, False, zeros, smooth(rng, rng.choice([0.5, 1.5, 3.0])))
    # seeded plans, motor controller: desired positions integrate the desired velocities
    for _ in range(16):
        hole, q0 = draw_hole(rng), start(rng)
        dv = smooth(rng, rng.choice([0.5, 1.5, 3.0]))
        dp = grid(q0 + np.cumsum(dv.astype(np.float64) * DT, axis=0), 12)
        add("motor", 0, q0, np.zeros(D), 0, hole, 100, False, False, dp, dv)
    # scripted hits of each kind
    up = np.array([np.pi / 2, 0, 0, 0, 0])
    v = np.zeros((T, D), F32); v[:, 0] = 3.0
    add("script_wall_left", 1, up, np.zeros(D), 0, [2.0, 0.3, 1.0], 100, False, False, zeros, v)
    v = np.zeros((T, D), F32); v[:, 0] = -3.0
    add("script_wall_right", 1, up, np.zeros(D), 0, [-2.0, 0.3, 1.0], 100, False, False, zeros, v)
    add("script_hole_floor", 1, np.array([-np.pi / 2, 0, 0, 0, 0]), np.zeros(D), 0, [0.0, 0.5, 1.0], 100, False, False, zeros, zeros)
    # the arm curls into a pentagon standing on the origin (first link at 0.63 rad, all above the floor) until the last link
    # crosses the first
    v = np.zeros((T, D), F32); v[:, 1:] = 2.0
    add("script_links_cross", 1, np.array([0.63, 0, 0, 0, 0]), np.zeros(D), 0, [3.4, 0.2, 1.0], 100, False, False, zeros, v)
    v = np.zeros((T, D), F32); v[:, 2] = 4.0; v[:, 3] = -4.0
    add("script_joint_limit", 1, up, np.zeros(D), 0, [3.4, 0.2, 1.0], 100, False, False, zeros, v)
    # a survivor that reaches into the hole: the straight arm hanging down in a wide hole, no motion (pays at step 199)
    # a survivor: four links just above the floor to the left, the last one hanging into the hole, 4 mm from the goal at step 199
    add("script_survivor", 1, np.array([np.pi - 1e-3, 0, 0, 0, np.pi / 2 + 1e-3]), np.zeros(D), 0, [-3.999998, 0.4, 1.0], 1000,
        False, False, zeros, zeros)
    # plans that start mid-episode: a prefix of step0 steps under the same controller (velocity: qd is float32 afterwards),
    # then the recorded plan from step0
    n_mid = 0
    while n_mid < 12:
        hole, q0 = draw_hole(rng), start(rng)
        step0 = int(rng.integers(1, 190))
        ctrl = int(rng.integers(0, 2))
        dv = smooth(rng, 0.5)
        dp = grid(q0 + np.cumsum(dv.astype(np.float64) * DT, axis=0), 12)
        pre = run_plan(Env, ctrl, q0, np.zeros(D), 0, hole, 100, False, False, dp, dv)
        if pre["n_exec"] < step0:
            continue
        env = Env(q0.copy(), np.zeros(D), 0, hole, 100, False, False)
        for t in range(step0):
            a = dv[t] if ctrl == 1 else 1.0 * (dp[t] - env._joint_angles) + 0.1 * (dv[t] - env._angle_velocity)
            env.step(np.clip(a, -F32(2 * np.pi), F32(2 * np.pi)))
        assert env._angle_velocity.dtype == (np.float32 if ctrl == 1 else np.float64)
        dv2 = smooth(rng, rng.choice([0.5, 2.0]))
        dp2 = grid(env._joint_angles + np.cumsum(dv2.astype(np.float64) * DT, axis=0), 12) if ctrl == 0 else zeros
        add("mid_episode", ctrl, np.asarray(env._joint_angles, np.float64), np.asarray(env._angle_velocity), step0, hole, 100,
            False, False, dp2, dv2)
        n_mid += 1
    # the allow_* toggles and both penalties
    for allow_self, allow_wall in ((True, False), (False, True), (True, True)):
        for penalty in (100, 1000):
            for _ in range(2):
                hole = draw_hole(rng)
                add(f"allow_{int(allow_self)}{int(allow_wall)}", 1, start(rng), np.zeros(D), 0, hole, penalty, allow_self, allow_wall,
                    zeros, smooth(rng, 3.0))
    for _ in range(4):
        add("penalty_1000", 1, start(rng), np.zeros(D), 0, draw_hole(rng), 1000, False, False, zeros, smooth(rng, 3.0))

    out = {}
    for key in ("ctrl", "step0", "n_steps", "n_exec", "kind"):
        out[key] = np.array([r[key] for r in rows], np.int32)
    for key in ("collided", "success", "allow_self", "allow_wall"):
        out[key] = np.array([r[key] for r in rows], bool)
    for key in ("penalty", "margin"):
        out[key] = np.array([r[key] for r in rows], np.float64)
    for key in ("q0", "qd0", "hole", "q", "qd", "rewards"):
        out[key] = np.stack([r[key] for r in rows]).astype(np.float64)
    for key in ("des_pos", "des_vel", "actions"):
        out[key] = np.stack([r[key] for r in rows]).astype(F32)
    out["family"] = np.array([r["family"] for r in rows])
    out["mp_config"] = np.array(json.dumps(mp_configs(), sort_keys=True))
    with open(os.path.abspath(__file__), "rb") as f:
        gen = hashlib.sha256(f.read()).hexdigest()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "generator": gen, "reference_files": _read}, sort_keys=True))
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in out.items():
            if k == "meta":
                continue
            assert np.array_equal(old[k], v), k
        print("ok: matches", OUT)
        return
    np.savez_compressed(OUT, **out)
    fam, n = np.unique(out["family"], return_counts=True)
    print(OUT, os.path.getsize(OUT), "bytes;", dict(zip(fam.tolist(), n.tolist())))
    print("collided", int(out["collided"].sum()), "kinds", np.bincount(out["kind"], minlength=4).tolist(), "success",
          int(out["success"].sum()), "margin < 1e-9:", int((out["margin"] < 1e-9).sum()))


if __name__ == "__main__":
    main()
