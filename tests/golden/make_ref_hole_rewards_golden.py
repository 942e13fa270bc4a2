#!/usr/bin/env python3
"""
Reference-generated fixture for HoleReacher's three reward functions (reads the reference sources where make_ref_hole_reacher_golden.py
reads them).

As make_ref_hole_reacher_golden.py does (its helpers are imported, the file is not changed), the FunctionDefs the step loop runs are
taken from their files with `ast` and compiled ALONE, then bound to a plain class: BaseReacherDirectEnv.step, BaseReacherEnv.
_update_joints / _check_self_collision, HoleReacherEnv._get_reward / _get_line_points / check_wall_collision / _check_collisions /
_terminate, ccw / intersect of utils.py, and HolereacherReward.__init__ / reset / get_reward of each of hr_simple_reward.py,
hr_dist_vel_acc_reward.py and hr_unbounded_reward.py, built as HoleReacherEnv.__init__ builds them (hole_reacher.py:48-58).  No
reference text is stored.  The driver is the loop of BlackBoxWrapper.step (black_box_wrapper.py:175-203) over WHOLE episodes
(steps 0 .. 199): controller, np.clip to the float32 action bounds, env.step, break on terminated / truncated (TimeLimit 200).

Output: tests/golden/ref_hole_rewards.npz; n_links = 5, T = 200, E episodes, R = 3 reward functions in the order of `rew_fct`:
  rew_fct str [R] ("simple", "vel_acc", "unbounded"); family str [E]; ctrl int [E] (0 motor, 1 velocity); q0 float64 [E, D] (qd = 0
  at reset); hole float64 [E, 3]; penalty float64 [E]; allow_self / allow_wall bool [E]; des_pos / des_vel float32 [E, T, D];
  actions float32 [E, T, D] (0 after the break), n_exec int [E], collided bool [E], q / qd float64 [E, D] after the episode -- the
  same for every reward function (the generator asserts it): the collision test and the plant do not depend on the reward;
  rewards float64 [R, E, T] (0 after the break), success bool [R, E] (is_success of the last executed step);
  ee_stored float64 [E, 2]: unbounded's end_eff_pos after the episode (the end effector of step 180 or of the colliding step; NaN
  if the episode ended before either);
  kind int [E] (0 none, 1 joint limit, 2 links crossing, 3 wall);
  margin float64 [E]: the smallest distance of a deciding collision comparison to its threshold over the executed steps;
  margin_success float64 [R, E]: |dist - 0.005| at the step that decides is_success by distance (simple: step 199 or the collision;
  vel_acc: step 199; unbounded: none, inf);  margin_ee_y float64 [E]: |end effector y| at a non-colliding step 199 (unbounded's
  `env.end_effector[1] > 0`; inf otherwise);
  mp_config (json of the merged mp_config of the four ids), meta (numpy version, sha256 of this file and of every reference file).

    python tests/golden/make_ref_hole_rewards_golden.py [--check]
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_hole_reacher_golden as base  # noqa: E402  (its helpers: src / functions / margins / smooth / grid / draw_hole)

OUT = os.path.join(HERE, "ref_hole_rewards.npz")
D, T, DT = base.D, base.T, base.DT
F32 = np.float32
REW_FCTS = ("simple", "vel_acc", "unbounded")
REW_FILES = {"simple": "hole_reacher/hr_simple_reward.py", "vel_acc": "hole_reacher/hr_dist_vel_acc_reward.py",
             "unbounded": "hole_reacher/hr_unbounded_reward.py"}


def build_classes():
    """{rew_fct: Env class}: the env methods shared, the reward class of each file"""
    ns = {"np": np}
    for c in base.functions("utils.py", ["ccw", "intersect"]).values():
        exec(c, ns)
    pieces = [("base_reacher/base_reacher_direct.py", ["step"], "BaseReacherDirectEnv"),
              ("base_reacher/base_reacher.py", ["_update_joints", "_check_self_collision"], "BaseReacherEnv"),
              ("hole_reacher/hole_reacher.py", ["_get_reward", "_get_line_points", "check_wall_collision", "_check_collisions",
                                                "_terminate"], "HoleReacherEnv")]
    env_methods = {}
    for name, wanted, cls in pieces:
        for fn, c in base.functions(name, wanted, cls).items():
            exec(c, ns)
            env_methods[fn] = ns[fn]
    classes = {}
    for rew_fct in REW_FCTS:
        rns = {"np": np}
        for fn, c in base.functions(REW_FILES[rew_fct], ["__init__", "reset", "get_reward"], "HolereacherReward").items():
            exec(c, rns)
        reward_cls = type("HolereacherReward", (), {fn: rns[fn] for fn in ("__init__", "reset", "get_reward")})

        class Env:
            dt = DT
            REW = rew_fct
            Reward = reward_cls

            def __init__(self, q0, hole, penalty, allow_self, allow_wall):
                self.n_links = D
                self.link_lengths = np.ones(D)
                self.j_min, self.j_max = -np.pi * np.ones(D), np.pi * np.ones(D)
                self.allow_self_collision = allow_self
                self._joints = np.zeros((D + 1, 2))
                self._joint_angles, self._angle_velocity, self._steps = q0, np.zeros(D), 0
                self._tmp_x, self._tmp_width, self._tmp_depth = hole
                self._goal = np.hstack([self._tmp_x, -self._tmp_depth])
                # hole_reacher.py:48-58: unbounded takes no collision penalty
                self.reward_function = (self.Reward(allow_self, allow_wall) if self.REW == "unbounded"
                                        else self.Reward(allow_self, allow_wall, penalty))
                self.reward_function.reset()
                self._update_joints()

            @property
            def end_effector(self):            # BaseReacherEnv.end_effector (base_reacher.py:137-139)
                return self._joints[self.n_links].T

            @property
            def current_pos(self):             # BaseReacherEnv.current_pos (base_reacher.py:65-67)
                return self._joint_angles.copy()

            def _get_obs(self):
                return np.zeros(1)

        for fn, f in env_methods.items():
            setattr(Env, fn, f)
        classes[rew_fct] = Env
    return classes


def run_episode(Env, ctrl, q0, hole, penalty, allow_self, allow_wall, dpos, dvel):
    env = Env(q0.copy(), hole, penalty, allow_self, allow_wall)
    low, high = -np.ones(D, F32) * F32(2 * np.pi), np.ones(D, F32) * F32(2 * np.pi)
    acts, rews = np.zeros((T, D), F32), np.zeros(T)
    collided = success = False
    kind, n = 0, 0
    m_coll = m_succ = m_y = np.inf
    for t in range(T):
        if ctrl == 1:
            a = dvel[t]
        else:
            a = 1.0 * (dpos[t] - env._joint_angles) + 0.1 * (dvel[t] - env._angle_velocity)
        a = np.clip(a, low, high)
        _, r, terminated, truncated, info = env.step(a)
        truncated = env._steps >= T
        acts[t], rews[t] = a, r
        n = t + 1
        m_coll = min(m_coll, base.margins(env))
        dist = float(np.linalg.norm(env.end_effector - env._goal))
        if (Env.REW == "simple" and (t == 199 or info["is_collided"])) or (Env.REW == "vel_acc" and t == 199):
            m_succ = min(m_succ, abs(dist - 0.005))
        if Env.REW == "unbounded" and t == 199 and not info["is_collided"]:
            m_y = min(m_y, abs(float(env.end_effector[1])))
        success = bool(info["is_success"])
        if terminated:
            collided = True
            if not allow_self and (np.any(env._joint_angles > env.j_max) or np.any(env._joint_angles < env.j_min)):
                kind = 1
            elif not allow_self and env._check_self_collision():
                kind = 2
            else:
                kind = 3
        if terminated or truncated:
            break
    ee = getattr(env.reward_function, "end_eff_pos", None)
    return dict(actions=acts, rewards=rews, q=np.asarray(env._joint_angles, np.float64),
                qd=np.asarray(env._angle_velocity, np.float64), n_exec=n, collided=collided, success=success, kind=kind,
                margin=m_coll, margin_success=m_succ, margin_ee_y=m_y,
                ee_stored=np.full(2, np.nan) if ee is None else np.asarray(ee, np.float64))


def generate():
    classes = build_classes()
    rows = []
    rng = np.random.default_rng(20261016)
    zeros = np.zeros((T, D), F32)

    def add(family, ctrl, q0, hole, penalty, allow_self, allow_wall, dpos, dvel):
        per = {f: run_episode(classes[f], ctrl, q0, np.asarray(hole, np.float64), penalty, allow_self, allow_wall, dpos, dvel)
               for f in REW_FCTS}
        s = per["simple"]
        for f in REW_FCTS[1:]:
            for k in ("actions", "q", "qd"):
                assert np.array_equal(per[f][k], s[k]), (family, f, k)
            assert per[f]["n_exec"] == s["n_exec"] and per[f]["collided"] == s["collided"], (family, f)
        rows.append(dict(family=family, ctrl=ctrl, q0=np.asarray(q0, np.float64), hole=np.asarray(hole, np.float64),
                         penalty=float(penalty), allow_self=allow_self, allow_wall=allow_wall, des_pos=dpos, des_vel=dvel,
                         actions=s["actions"], n_exec=s["n_exec"], collided=s["collided"], q=s["q"], qd=s["qd"], kind=s["kind"],
                         margin=s["margin"], ee_stored=per["unbounded"]["ee_stored"], margin_ee_y=per["unbounded"]["margin_ee_y"],
                         rewards=np.stack([per[f]["rewards"] for f in REW_FCTS]),
                         success=np.array([per[f]["success"] for f in REW_FCTS]),
                         margin_success=np.array([per[f]["margin_success"] for f in REW_FCTS])))
        return s

    def start(rng):
        q = np.zeros(D)
        q[0] = rng.uniform(np.pi / 4, 3 * np.pi / 4)
        return q

    # random plans, velocity controller: random starts, sampled holes, gentle to wild
    for amp in (0.5, 1.5, 3.0):
        for _ in range(7):
            add(f"velocity_{amp}", 1, start(rng), base.draw_hole(rng), 100, False, False, zeros, base.smooth(rng, amp))
    # random plans, motor controller: desired positions integrate the desired velocities
    for _ in range(9):
        hole, q0 = base.draw_hole(rng), start(rng)
        dv = base.smooth(rng, rng.choice([0.5, 1.5, 3.0]))
        dp = base.grid(q0 + np.cumsum(dv.astype(np.float64) * DT, axis=0), 12)
        add("motor", 0, q0, hole, 100, False, False, dp, dv)
    # a wall hit at an exact step k: the arm curves gently just above the floor, right of a far hole, at rest until joint 0 turns it
    # down at step k (k = 180 stores and pays at once, 199 pays on the last step, 181 .. 198 pay on the ee of the collision)
    flat = np.array([1e-3, 0.02, 0.02, 0.02, 0.02])
    for k in (40, 120, 179, 180, 181, 185, 190, 198, 199):
        v = np.zeros((T, D), F32); v[k:, 0] = -6.0
        add(f"wall_at_{k}", 1, flat, [-2.0, 0.3, 1.0], 100, False, False, zeros, v)
    # the same under the motor controller (the desired position steps down at k)
    for k in (60, 180, 192):
        dp = np.tile(flat.astype(F32), (T, 1)); dp[k:, 0] = -0.5
        add(f"motor_wall_at_{k}", 0, flat, [-2.0, 0.3, 1.0], 100, False, False, dp, zeros)
    # a joint limit at an exact step: the last joint folds back to 0.03 below pi on a bent, upright arm, until it turns past pi at k
    for k in (100, 180, 195):
        v = np.zeros((T, D), F32); v[k:, 4] = 6.0
        add(f"joint_limit_at_{k}", 1, np.array([np.pi / 2, 0.1, 0.1, 0.1, np.pi - 0.03]), [3.4, 0.2, 1.0], 100, False, False, zeros, v)
    # links crossing: the arm curls into a pentagon over the origin until the last link crosses the first
    for speed in (2.0, 1.0):
        v = np.zeros((T, D), F32); v[:, 1:] = speed
        add(f"links_cross_{speed}", 1, np.array([0.63, 0, 0, 0, 0]), [3.4, 0.2, 1.0], 100, False, False, zeros, v)
    # survivors that end inside the hole (end effector y < 0 at step 199): four links just above the floor to the left, the last
    # hanging straight down into the hole, `off` above the goal (simple / vel_acc succeed below 0.005)
    reach = np.array([np.pi - 0.03, 0.01, 0.01, 0.01, np.pi / 2])
    ang = np.cumsum(reach)
    ee = np.array([np.sum(np.cos(ang)), np.sum(np.sin(ang))])
    for off, dx, drift in ((0.002, 0.0, 0.0), (0.004, 1e-3, 0.0), (0.02, 0.0, 0.0), (0.002, 0.0, 2 ** -8)):
        v = np.zeros((T, D), F32); v[:, 4] = drift
        add("survivor_in_hole", 1, reach, [ee[0] + dx, 0.4, off - ee[1]], 1000, False, False, zeros, v)
    # ... and one whose last link swings out of the hole (through the wall: allowed) from step 170: y < 0 at step 180, > 0 at 199
    v = np.zeros((T, D), F32); v[170:, 4] = -6.0
    add("leaves_hole", 1, reach, [ee[0], 0.4, 0.01 - ee[1]], 1000, True, True, zeros, v)
    # the allow_* toggles and both penalties
    for allow_self, allow_wall in ((True, False), (False, True), (True, True)):
        for penalty in (100, 1000):
            add(f"allow_{int(allow_self)}{int(allow_wall)}", 1, start(rng), base.draw_hole(rng), penalty, allow_self, allow_wall,
                zeros, base.smooth(rng, 3.0))
    for _ in range(3):
        add("penalty_1000", 1, start(rng), base.draw_hole(rng), 1000, False, False, zeros, base.smooth(rng, 3.0))

    out = {"rew_fct": np.array(REW_FCTS)}
    for key in ("ctrl", "n_exec", "kind"):
        out[key] = np.array([r[key] for r in rows], np.int32)
    for key in ("collided", "allow_self", "allow_wall"):
        out[key] = np.array([r[key] for r in rows], bool)
    for key in ("penalty", "margin", "margin_ee_y"):
        out[key] = np.array([r[key] for r in rows], np.float64)
    for key in ("q0", "hole", "q", "qd", "ee_stored"):
        out[key] = np.stack([r[key] for r in rows]).astype(np.float64)
    for key in ("des_pos", "des_vel", "actions"):
        out[key] = np.stack([r[key] for r in rows]).astype(F32)
    out["rewards"] = np.stack([r["rewards"] for r in rows], axis=1).astype(np.float64)
    out["success"] = np.stack([r["success"] for r in rows], axis=1).astype(bool)
    out["margin_success"] = np.stack([r["margin_success"] for r in rows], axis=1).astype(np.float64)
    out["family"] = np.array([r["family"] for r in rows])
    out["mp_config"] = np.array(json.dumps(base.mp_configs(), sort_keys=True))
    with open(os.path.abspath(__file__), "rb") as f:
        gen = hashlib.sha256(f.read()).hexdigest()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "generator": gen, "reference_files": base._read}, sort_keys=True))
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in out.items():
            if k == "meta":
                continue
            assert np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("ok: matches", OUT)
        return
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out["family"]), "episodes")
    n = out["n_exec"]
    print("collided", int(out["collided"].sum()), "kinds", np.bincount(out["kind"], minlength=4).tolist(),
          "collision steps", sorted((n[out["collided"]] - 1).tolist()))
    print("success per rew_fct", dict(zip(REW_FCTS, out["success"].sum(axis=1).tolist())))
    ok = ~out["collided"]
    print("survivors: ee y < 0 at 199:", int((out["ee_stored"][ok, 1] < 0).sum()), "margin < 1e-9:", int((out["margin"] < 1e-9).sum()),
          "margin_success < 1e-9:", int((out["margin_success"] < 1e-9).sum()), "margin_ee_y < 1e-9:",
          int((out["margin_ee_y"] < 1e-9).sum()))


if __name__ == "__main__":
    main()
