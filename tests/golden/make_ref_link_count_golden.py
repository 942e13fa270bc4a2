#!/usr/bin/env python3
"""
Reference-generated fixture for the reacher envs at link counts other than 2 and 5 (build container only: reads the reference checkout).

Every other reference fixture of the reacher envs has n_links 2 or 5.  From 8 entries on np.sum of a vector no longer adds in index
order (eight accumulators, see oracle/mp_oracle.py: np_sum_rows), and the reference's rewards are such sums over the links:
sum(acc ** 2), sum(vel ** 2), sum(action ** 2).  Link counts here: 1 (no non-adjacent link pair), 3 (a plain run-time count), 7 (the
last in-order sum), 8 (eight accumulators, no remainder), 9 (remainder 1), 15 (remainder 7), 16 (two rounds).

The envs are the classes make_ref_step_env_golden.py: build_classes() compiles from the reference's FunctionDefs (taken with `ast`,
compiled ALONE; its helpers are imported, the file is not changed).  No reference text is stored.  Restated here: the loop of
BlackBoxWrapper.step (black_box_wrapper.py:175-203: controller, np.clip to the float32 action bounds, env.step, break on terminated /
truncated at TimeLimit 200) as make_ref_hole_reacher_golden.py: run_plan restates it for five links, and the registered kwargs of
fancy/HoleReacher-v0 (envs/__init__.py:72-88).

Output: tests/golden/ref_reacher_links.npz, three groups.  DM = 16: rows of fewer links are padded (0 for plans / actions, NaN for states).

(a) HoleReacher black-box plans, one row per episode, key "plan__<field>", R = 3 reward functions in the order of `rew_fct`:
  D / T / ctrl (0 motor, 1 velocity) / step0 / n_steps (steps the plan may run: min(T, 200 - step0)) int32 [E]; family str [E];
  q0 / qd0 float64 [E, DM] (state at plan start; a plan with step0 = 176 starts after 176 reference steps under the same controller,
  so qd0 holds float32 values under the velocity controller); hole float64 [E, 3]; des_pos / des_vel float32 [E, 25, DM];
  actions float32 [E, 25, DM], q / qd float64 [E, DM] after the plan, n_exec int32 [E], collided bool [E], kind int8 [E] (0 none,
  1 joint limit, 2 links crossing, 3 wall) -- the same for every reward function (asserted);
  rewards float64 [R, E, 25] (0 behind the break), success bool [R, E], margin float64 [E] (the smallest distance of a deciding
  comparison to its threshold over the executed steps: collision predicates, joint limits, the 0.005 success radius, the sign of the
  end effector's height at a non-colliding step 199).
(b) step-based vector-env traces (run_env of make_ref_step_env_golden.py: seeded reset, float32 actions on the 2^-8 grid, TimeLimit
  200, same-step autoreset), `traces` (json) lists them; for trace <name>, key "<name>__<field>", the fields of ref_step_envs.npz.
  A HoleReacher trace holds all three reward functions: reward float64 [R, S, N] and is_success bool [R, S, N]; every other field
  is the same for the three (asserted) and stored once.
(c) seeded resets, key "reset__<field>": kind (0 SimpleReacher, 1 HoleReacher) / n_links int32 [E], seed uint64 [E], NR = 4 resets
  per row (reset(seed=seed), then reset() x 3): q0 float64 [E, NR, DM], task float64 [E, NR, 3], rng uint64 [E, NR, 5] (the words of
  mpk_nprng_state), obs float32 [E, NR, 3 DM + 4];
  observation rows of stored states, key "obs__<field>": kind / n_links / steps int32 [E], q / qd float64 [E, DM], task float64
  [E, 3], obs float32 [E, 3 DM + 4] (_get_obs of the env put into that state).
Every margin is asserted >= 1e-9 here; a drawn row that misses is redrawn.  meta: numpy version, sha256 of this file and of every
reference file read.

    python tests/golden/make_ref_link_count_golden.py [--check]
"""
import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_step_env_golden as SE  # noqa: E402  (build_classes / run_env / hole_margin / collision_kind / rng_words / grid / smooth)

OUT = os.path.join(HERE, "ref_reacher_links.npz")
LINKS = (1, 3, 7, 8, 9, 15, 16)
LONG = (8, 9, 16)                    # link counts whose step traces run past the step limit
# HoleReacher cannot STEP with one link in the reference: check_wall_collision indexes the [n_links, points, 2] array of
# _get_line_points, whose np.squeeze drops the link axis when n_links is 1 (hole_reacher.py:143,152: IndexError).  Its reset and its
# observation do not go there, so group (c) keeps one link for both envs; groups (a) and (b) hold HoleReacher from three links on.
HOLE_LINKS = LINKS[1:]
DM, TM, DT, LIMIT = 16, 25, 0.01, 200
HORIZONS = ((12, 0), (25, 176))      # (T, step0): the second holds the steps 180 and 199
F32 = np.float32
REW_FCTS = ("simple", "vel_acc", "unbounded")
REG = dict(random_start=True, allow_self_collision=False, allow_wall_collision=False, hole_width=None, hole_depth=1, hole_x=None,
           collision_penalty=100)      # fancy/HoleReacher-v0 (envs/__init__.py:72-88)
MARGIN = 1e-9


def grid12(x):
    return SE.grid(x, 12)


# ---- (a) black-box plans --------------------------------------------------------------------------------------------------------------
def place(env, q, qd, steps, hole3):
    """the env in a given state (what reset() sets, base_reacher.py:81-91 / hole_reacher.py:97-100, with these values)"""
    D = env.n_links
    env._tmp_x, env._tmp_width, env._tmp_depth = (np.float64(v) for v in hole3)
    env._goal = np.hstack([env._tmp_x, -env._tmp_depth])
    env.reward_function.reset()
    env._joint_angles, env._angle_velocity = q.copy(), qd.copy()
    env._joints = np.zeros((D + 1, 2))
    env._update_joints()
    env._steps = int(steps)
    env._is_collided = False


def control(env, ctrl, dpos, dvel, t):
    """the tracking controller (pd_controller.py / vel_controller.py) and the clip of black_box_wrapper.py:176-179"""
    D = env.n_links
    bound = np.ones(D, F32) * F32(2 * np.pi)
    if ctrl == 1:
        a = dvel[t]
    else:
        a = 1.0 * (dpos[t] - env._joint_angles) + 0.1 * (dvel[t] - env._angle_velocity)
    return np.clip(a, -bound, bound)


def run_plan(env, ctrl, dpos, dvel, T, with_margin=True):
    D = env.n_links
    acts, rews = np.zeros((T, D), F32), np.zeros(T)
    n, kind, margin, collided, success = 0, 0, np.inf, False, False
    for t in range(min(T, LIMIT - env._steps)):
        a = control(env, ctrl, dpos, dvel, t)
        before = env._steps
        _, r, terminated, _, info = env.step(a)
        truncated = env._steps >= LIMIT
        acts[t], rews[t] = a, r
        n = t + 1
        hit = bool(info["is_collided"])
        assert bool(terminated) == hit
        if with_margin:
            margin = min(margin, SE.hole_margin(env, before == 199 or hit))
            if before == 199 and not hit:
                margin = min(margin, abs(float(env.end_effector[1])))      # hr_unbounded_reward.py: `env.end_effector[1] > 0`
        success = bool(info["is_success"])
        if hit:
            collided, kind = True, SE.collision_kind(env)
        if terminated or truncated:
            break
    return dict(actions=acts, rewards=rews, q=np.asarray(env._joint_angles, np.float64), qd=np.asarray(env._angle_velocity, np.float64),
                n_exec=n, collided=collided, success=success, kind=kind, margin=margin)


def draw_hole(rng):
    width = rng.uniform(0.15, 0.5)
    return np.array([rng.choice([-1, 1]) * rng.uniform(width / 2, 3.5), width, 1.0])


def candidate(rng, family, D, ctrl, T):
    """(start pose, drive) of one episode: `drive` is a velocity per joint (velocity controller) / an offset of the desired position
    (motor controller) on top of a small smooth motion of every joint, so that every link's acceleration enters the reward sums"""
    q = np.zeros(D)
    bends = rng.choice([-1.0, 1.0], D) * rng.uniform(0.03, 0.12, D) * min(1.0, 5.0 / D)
    drive = np.zeros(D)
    fast = 6.0 if ctrl == 1 else 5.0
    if family == "survive":
        q[:] = bends
        q[0] = rng.uniform(np.pi / 2 - 0.3, np.pi / 2 + 0.3)
    elif family == "wall":                # low over the floor, curling upwards, then the first joint sweeps the arm down
        side = rng.choice([-1.0, 1.0])
        q[:] = np.abs(bends) * side * 0.5
        low = rng.uniform(0.25, 0.45)
        q[0] = low if side > 0 else np.pi - low
        drive[0] = -side * fast
    elif family == "limit":               # the last joint folded back to just below pi, then turned past it
        side = rng.choice([-1.0, 1.0])
        q[:] = bends
        q[0] = rng.uniform(np.pi / 2 - 0.2, np.pi / 2 + 0.2)
        gap = rng.uniform(0.08, 0.2)
        if D == 1:
            q[0] = np.pi - gap
            side = 1.0
        else:
            q[D - 1] = side * (np.pi - gap)
        drive[D - 1] = side * fast
    elif family == "cross":               # the last three links nearly close a triangle at the tip; the last joint closes it
        q[:] = bends
        q[0] = rng.uniform(np.pi / 2 - 0.4, np.pi / 2 - 0.1)
        q[D - 2] = 1.9 + rng.uniform(-0.08, 0.08)
        q[D - 1] = 2.48 - rng.uniform(0.12, 0.3)
        drive[D - 1] = fast
    else:
        raise ValueError(family)
    return q, drive


def plan_inputs(rng, q, drive, D, ctrl, T, amp):
    """des_pos / des_vel float32 [T, D] for a plan that starts at q"""
    # (a jitter of every joint in every step: slow profiles on the grid give accelerations of a few grid units, whose squares add up
    # without rounding in any order -- such rows could not tell numpy's order of additions from another)
    dv = SE.grid(SE.smooth(rng, amp, T, D).astype(np.float64) + rng.integers(-2, 3, (T, D)) * 0.125)
    if ctrl == 1:
        dv = SE.grid(dv.astype(np.float64) + drive)
        return np.zeros((T, D), F32), dv
    dp = grid12(q + drive + np.cumsum(dv.astype(np.float64) * DT, axis=0))
    return dp, dv


def plans(hole_cls):
    rows = []
    quota = {"survive": 2, "wall": 1, "limit": 1, "cross": 1}
    for D in HOLE_LINKS:
        envs = {f: hole_cls(D, **dict(REG, rew_fct=f)) for f in REW_FCTS}
        for ctrl in (0, 1):
            for T, step0 in HORIZONS:
                rng = np.random.default_rng(20261019 + 1000 * D + 100 * ctrl + T)
                for family, want in quota.items():
                    if family == "cross" and D < 3:
                        continue
                    want_kind = {"survive": 0, "limit": 1, "cross": 2, "wall": 3}[family]
                    got = 0
                    for attempt in range(200):
                        if got == want:
                            break
                        hole3 = draw_hole(rng)
                        q, drive = candidate(rng, family, D, ctrl, T)
                        qd = np.zeros(D)
                        amp = 0.3 * min(1.0, 5.0 / D)
                        env = envs["simple"]
                        if step0:
                            # the prefix: `step0` reference steps of a gentle motion under the same controller
                            pp, pv = plan_inputs(rng, q, np.zeros(D), D, ctrl, step0, 0.02)
                            place(env, q, qd, 0, hole3)
                            pre = run_plan(env, ctrl, pp, pv, step0, with_margin=False)
                            if pre["collided"]:
                                continue
                            q, qd = pre["q"], np.asarray(env._angle_velocity)
                            assert qd.dtype == (np.float32 if ctrl == 1 else np.float64) and env._steps == step0
                        dp, dv = plan_inputs(rng, q, drive, D, ctrl, T, amp)
                        per = {}
                        for f in REW_FCTS:
                            place(envs[f], q, qd, step0, hole3)
                            per[f] = run_plan(envs[f], ctrl, dp, dv, T, with_margin=f == "simple")
                        s = per["simple"]
                        for f in REW_FCTS[1:]:
                            for k in ("actions", "q", "qd"):
                                assert np.array_equal(per[f][k], s[k]), (D, family, f, k)
                            assert per[f]["n_exec"] == s["n_exec"] and per[f]["collided"] == s["collided"]
                        if s["margin"] < MARGIN or s["kind"] != want_kind:
                            continue
                        if family == "survive" and s["n_exec"] != min(T, LIMIT - step0):
                            continue
                        got += 1
                        rows.append(dict(D=D, T=T, ctrl=ctrl, step0=step0, n_steps=min(T, LIMIT - step0), family=family,
                                         q0=np.asarray(q, np.float64), qd0=np.asarray(qd, np.float64), hole=hole3, des_pos=dp, des_vel=dv,
                                         actions=s["actions"], q=s["q"], qd=s["qd"], n_exec=s["n_exec"], collided=s["collided"],
                                         kind=s["kind"], margin=s["margin"], rewards=np.stack([per[f]["rewards"] for f in REW_FCTS]),
                                         success=np.array([per[f]["success"] for f in REW_FCTS])))
                    assert got == want, (D, ctrl, T, family, got)
    out = {}

    def padded(key, width, fill, dtype):
        arr = np.full((len(rows),) + width, fill, dtype)
        for i, r in enumerate(rows):
            v = np.asarray(r[key])
            arr[(i,) + tuple(slice(0, n) for n in v.shape)] = v
        return arr

    for key in ("D", "T", "ctrl", "step0", "n_steps", "n_exec"):
        out[key] = np.array([r[key] for r in rows], np.int32)
    out["kind"] = np.array([r["kind"] for r in rows], np.int8)
    out["collided"] = np.array([r["collided"] for r in rows], bool)
    out["margin"] = np.array([r["margin"] for r in rows], np.float64)
    out["family"] = np.array([r["family"] for r in rows])
    out["hole"] = np.stack([r["hole"] for r in rows]).astype(np.float64)
    for key in ("q0", "qd0", "q", "qd"):
        out[key] = padded(key, (DM,), np.nan, np.float64)
    for key in ("des_pos", "des_vel", "actions"):
        out[key] = padded(key, (TM, DM), 0.0, F32)
    out["rewards"] = np.ascontiguousarray(padded("rewards", (3, TM), 0.0, np.float64).transpose(1, 0, 2))
    out["success"] = np.stack([r["success"] for r in rows], axis=1).astype(bool)
    return {"plan__" + k: v for k, v in out.items()}


# ---- (b) step-based traces ------------------------------------------------------------------------------------------------------------
def trace_builders(rng, env, D, S):
    """per-env action builders (seed -> float32 [S, D] on the 2^-8 grid)"""
    if env == "simple_reacher":
        def big(s):
            a = SE.smooth(rng, 40.0, S, D)
            a[5::37] = SE.grid(rng.choice([-1.0, 1.0], (len(a[5::37]), D)) * rng.uniform(1000.5, 2500.0, (len(a[5::37]), D)))
            return a
        # (torques of hundreds of grid units: their squares need more than float32's 24 bits, so the order of additions shows)
        return [lambda s: SE.smooth(rng, 300.0, S, D), big]
    # A reset leaves the arm straight, and collinear links have ccw = 0: 1e-12 from the threshold of the crossing test.  So every
    # joint turns steadily from the first step on: a bias of 20 .. 60 grid units, all different, of either sign, under a ripple and a jitter of
    # at most 13 units -- no joint angle returns to 0, and no neighbour starts out at -2 x the angle next to it (three joints in
    # a line).  What still comes within 1e-9 of a threshold is redrawn (step_traces).
    def bends():
        while True:
            m = rng.permutation(np.arange(20, 61))[:D].astype(np.float64)
            if not np.any((m[1:] == 2 * m[:-1]) | (m[:-1] == 2 * m[1:])):
                return rng.choice([-1.0, 1.0], D) * m * 2.0 ** -8

    def jitter():                         # up to 8 units either way in every step: accelerations whose squares do not add up exactly
        return rng.integers(-8, 9, (S, D)) * 2.0 ** -8

    def gentle(s):
        return SE.grid(SE.smooth(rng, 5.0 / 3 * 2.0 ** -8, S, D).astype(np.float64) + bends() + jitter())

    def sweep(s):
        # The first joint sweeps the arm into the floor, episode after episode, and the other joints turn fast, each in its own
        # direction, by 200 .. 390 units drawn anew in every step: accelerations of hundreds of units, whose squares need more than
        # float32's 24 bits -- slow profiles on the grid have sums of squares that are exact in ANY order and could not tell numpy's
        # order of additions from another.  All magnitudes within a factor of 2: no angle is -2 x its neighbour's.
        sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0) * rng.choice([-1.0, 1.0])
        a = sign * rng.integers(200, 391, (S, D)) * 2.0 ** -8
        a[:, 0] = rng.choice([-1.0, 1.0]) * rng.uniform(2.0, 7.0)
        return SE.grid(a)

    return [gentle, sweep]


def trace_list(simple, hole):
    out = []
    for D in LINKS:
        S = 205 if D in LONG else 40
        out.append((f"simple{D}", "simple_reacher", D, S, {}))
        if D in HOLE_LINKS:
            out.append((f"hole{D}", "hole_reacher", D, S, dict(REG)))
    return out


def step_traces(simple, hole):
    out, index = {}, []
    for ti, (name, env, D, S, kw) in enumerate(trace_list(simple, hole)):
        is_hole = env == "hole_reacher"
        rng = np.random.default_rng(20261020 + ti)
        seed = 5000 * (ti + 1)
        fcts = REW_FCTS if is_hole else (None,)
        for attempt in range(40):
            builders = trace_builders(rng, env, D, S)
            acts = [np.ascontiguousarray(b(seed + i), F32) for i, b in enumerate(builders)]
            runs = {}
            for f in fcts:
                make = (lambda f=f: hole(D, **dict(kw, rew_fct=f))) if is_hole else (lambda: simple(D))
                runs[f] = []
                for i, a in enumerate(acts):
                    runs[f].append(SE.run_env(make, seed + i, a, is_hole))
                    if runs[f][-1] is None:
                        break
                if runs[f][-1] is None:
                    break
            if any(r is None for rs in runs.values() for r in rs):
                continue
            if trace_ok(runs[fcts[0]], is_hole, S, D):
                break
        else:
            raise AssertionError((name, "no draw met the coverage in 40"))
        envs = runs[fcts[0]]
        N = len(envs)
        put = lambda k, v: out.__setitem__(f"{name}__{k}", v)      # noqa: E731
        put("actions", np.stack(acts, axis=1))
        for k, dt_ in (("obs0", F32), ("q0", np.float64), ("qd0", np.float64), ("task0", np.float64), ("rng0", np.uint64)):
            put(k, np.stack([e[k] for e in envs]).astype(dt_))
        kinds = dict(final_obs=F32, terminated=bool, truncated=bool, q=np.float64, qd=np.float64, steps=np.int32, task=np.float64,
                     rng=np.uint64)
        if is_hole:
            kinds.update(is_collided=bool, kind=np.int8, margin=np.float64)
        stack = lambda es, k, dt_: np.stack([np.stack([np.asarray(v) for v in e["rows"][k]]) for e in es], axis=1).astype(dt_)  # noqa: E731
        for k, dt_ in kinds.items():
            put(k, stack(envs, k, dt_))
            for f in fcts[1:]:
                if k != "margin":
                    assert np.array_equal(stack(runs[f], k, dt_), out[f"{name}__{k}"]), (name, f, k)
        if is_hole:
            put("reward", np.stack([stack(runs[f], "reward", np.float64) for f in fcts]))
            put("is_success", np.stack([stack(runs[f], "is_success", bool) for f in fcts]))
            put("margin", np.min(np.stack([stack(runs[f], "margin", np.float64) for f in fcts]), axis=0))
        else:
            put("reward", stack(envs, "reward", np.float64))
        at = sorted((t, b) for b, e in enumerate(envs) for t, _ in e["resets"])
        obs_of = {(t, b): o for b, e in enumerate(envs) for t, o in e["resets"]}
        n = envs[0]["obs0"].shape[0]
        put("reset_at", np.array(at, np.int32).reshape(-1, 2))
        put("reset_obs", np.stack([obs_of[k] for k in at]).astype(F32) if at else np.zeros((0, n), F32))
        if is_hole:
            # a survivor's step 199 under "unbounded" decides on the sign of the end effector's height (not part of hole_margin)
            fo, tr = out[f"{name}__final_obs"], out[f"{name}__truncated"] & ~out[f"{name}__is_collided"]
            ee_y = fo[..., 3 * D + 2].astype(np.float64) - 1.0          # the row holds ee - goal, goal y = -depth = -1
            assert not tr.any() or np.abs(ee_y[tr]).min() > 1e-6, name
            assert out[f"{name}__margin"].min() >= MARGIN, name
        index.append(dict(name=name, env=env, n_links=D, kwargs=kw, seed=seed, N=N, S=S))
    out["traces"] = np.array(json.dumps(index, sort_keys=True))
    return out


def trace_ok(envs, is_hole, S, D):
    """what a trace must show"""
    trunc = np.array([e["rows"]["truncated"] for e in envs])
    if not is_hole:
        return S <= 200 or bool(trunc.any(axis=1).all())
    coll = np.array([e["rows"]["is_collided"] for e in envs])
    if S > 200:
        # a survivor that is paid at step 199 and truncated, and an env that collides
        return bool((trunc.any(axis=1) & ~coll.any(axis=1)).any() and coll.any())
    return bool(coll.any() and (~coll.any(axis=1)).any())


# ---- (c) resets and observation rows --------------------------------------------------------------------------------------------------
def resets_and_rows(simple, hole):
    NR, NC = 4, 3 * DM + 4
    res, obs = [], []
    for kind, cls in ((0, simple), (1, hole)):
        for D in LINKS:
            make = (lambda: simple(D)) if kind == 0 else (lambda: hole(D, **REG))
            rng = np.random.default_rng(9000 + 100 * kind + D)
            seeds = [0, 2 ** 64 - 1] + [int(s) for s in rng.integers(0, 2 ** 64, size=2, dtype=np.uint64)]
            for seed in seeds:
                env = make()
                row = dict(kind=kind, n_links=D, seed=seed, q0=np.full((NR, DM), np.nan), task=np.full((NR, 3), np.nan),
                           rng=np.zeros((NR, 5), np.uint64), obs=np.full((NR, NC), np.nan, F32))
                for k in range(NR):
                    o, _ = env.reset(seed=seed if k == 0 else None)
                    row["q0"][k, :D] = env._joint_angles
                    t = SE.task_row(env, kind == 1)
                    row["task"][k, :len(t)] = t
                    row["rng"][k] = SE.rng_words(env)
                    row["obs"][k, :len(o)] = o
                res.append(row)
            # stored states: random and edge angles, zero / large velocities (float32 ones for HoleReacher), steps 0, 1, 199, 200, ...
            env = make()
            env.reset(seed=1)
            edge_q = [np.pi, -np.pi, np.nextafter(np.pi, 4.0), np.pi / 2, 3.5, -7.25, 0.0, 40.0]
            for i in range(6):
                q = rng.uniform(-4.0, 4.0, D)
                if i % 2 == 1:
                    q[rng.integers(D)] = edge_q[i % len(edge_q)]
                qd = [np.zeros(D), rng.standard_normal(D), rng.standard_normal(D) * 1e3, rng.uniform(-5e4, 5e4, D)][i % 4]
                if kind == 1 and i % 2 == 1:
                    qd = qd.astype(F32)
                steps = [0, 1, 199, 200][i % 4] if i < 4 else int(rng.integers(0, 201))
                if kind == 0:
                    while True:
                        g = rng.uniform(-D, D, 2)
                        if np.linalg.norm(g) < D:
                            break
                    task = np.array([g[0], g[1], np.nan])
                    env._goal = task[:2].copy()
                else:
                    width = rng.uniform(0.15, 0.5)
                    task = np.array([rng.choice([-1, 1]) * rng.uniform(width / 2, 3.5), width, 1.0])
                    env._tmp_x, env._tmp_width, env._tmp_depth = task
                    env._goal = np.hstack([env._tmp_x, -env._tmp_depth])
                env._joint_angles, env._angle_velocity, env._steps = q, qd, steps
                env._update_joints()
                o = env._get_obs()
                assert o.dtype == F32
                row = dict(kind=kind, n_links=D, steps=steps, q=np.full(DM, np.nan), qd=np.full(DM, np.nan), task=task,
                           obs=np.full(NC, np.nan, F32))
                row["q"][:D], row["qd"][:D], row["obs"][:len(o)] = q, qd, o
                obs.append(row)
    out = {}
    for prefix, rows, ints in (("reset", res, ("kind", "n_links")), ("obs", obs, ("kind", "n_links", "steps"))):
        for key in rows[0]:
            if key in ints:
                out[f"{prefix}__{key}"] = np.array([r[key] for r in rows], np.int32)
            elif key == "seed":
                out[f"{prefix}__{key}"] = np.array([r[key] for r in rows], np.uint64)
            else:
                out[f"{prefix}__{key}"] = np.stack([r[key] for r in rows])
    return out


def generate():
    simple, hole = SE.build_classes()
    out = {"rew_fct": np.array(REW_FCTS)}
    out.update(plans(hole))
    out.update(step_traces(simple, hole))
    out.update(resets_and_rows(simple, hole))
    with open(os.path.abspath(__file__), "rb") as f:
        gen = hashlib.sha256(f.read()).hexdigest()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "generator": gen, "reference_files": SE._read}, sort_keys=True))
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), sorted(set(old.files) ^ set(out))
        for k, v in out.items():
            if k == "meta":
                continue
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("ok: matches", OUT)
        return
    # an .npz is a zip of .npy members: LZMA members (np.load reads them through zipfile) take a sixth less room than
    # np.savez_compressed's deflate on these float64 states
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_LZMA)
    print(OUT, os.path.getsize(OUT), "bytes")
    p = lambda k: out["plan__" + k]      # noqa: E731
    for D in HOLE_LINKS:
        m = p("D") == D
        print(f"  plans D {D}: {int(m.sum())} episodes, kinds {np.bincount(p('kind')[m], minlength=4).tolist()}, survivors "
              f"{int((~p('collided')[m]).sum())}, success {p('success')[:, m].sum(axis=1).tolist()}, min margin {p('margin')[m].min():.2e}")
    for tr in json.loads(str(out["traces"])):
        g = lambda k: out[f"{tr['name']}__{k}"]      # noqa: E731
        extra = ""
        if tr["env"] == "hole_reacher":
            extra = f" collided {int(g('is_collided').sum())} kinds {np.bincount(g('kind').ravel(), minlength=4).tolist()} " \
                    f"min margin {g('margin').min():.2e}"
        print(f"  {tr['name']}: N {tr['N']} S {tr['S']} resets {len(g('reset_at'))} truncated {int(g('truncated').sum())}{extra}")


if __name__ == "__main__":
    main()
