#!/usr/bin/env python3
"""
Reference-generated fixture for the STEP-BASED reacher ids as vector envs (build container only: reads the reference checkout).

The reference package cannot be imported here (gymnasium / matplotlib are absent), so -- as make_ref_reset_golden.py does -- the
FunctionDefs an env.reset() / env.step(action) runs are taken from their files with `ast` and compiled ALONE, each group inside a
class of its own name on top of a stand-in for gymnasium.Env (so that `super()` resolves as in the reference):
  BaseReacherEnv         reset, _update_joints, _check_self_collision, dt, current_pos, end_effector
  BaseReacherTorqueEnv   step            (compiled ITSELF: the float32 flow of `self.dt * action` is the point)
  BaseReacherDirectEnv   step
  SimpleReacherEnv       reset, _get_reward, _terminate, _get_obs, _generate_goal, _check_collisions
  HoleReacherEnv         reset, _get_reward, _terminate, _generate_hole, _get_obs, _get_line_points, _check_collisions,
                         check_wall_collision
  HolereacherReward      __init__, reset, get_reward of hr_simple_reward.py, hr_dist_vel_acc_reward.py, hr_unbounded_reward.py
  ccw, intersect         utils.py
No reference text is stored.  Restated here: the attributes the constructors set (base_reacher.py:16-58, simple_reacher.py:20-31,
hole_reacher.py:20-58), gymnasium.Env.reset(seed=s) (np.random.Generator(np.random.PCG64(np.random.SeedSequence(s)))), and in the
driver gymnasium's TimeLimit (truncated = elapsed steps >= 200, the registered max_episode_steps) and the vector env's same-step
autoreset: episode b is seeded with seed + b, and an env whose step ended its episode is reset() at once, without a seed.

Output: tests/golden/ref_step_envs.npz.  `traces` (json) lists the traces with their constants; for trace <name>, N envs, S steps,
D links, n = 3 D + 3 (SimpleReacher) / 3 D + 4 (HoleReacher) observation columns, every array under the key "<name>__<field>":
  actions float32 [S, N, D] (on a grid of 2^-8, not clipped, also beyond the action space); obs0 float32 [N, n], q0 / qd0 float64
  [N, D], task0 float64 [N, 2 | 3], rng0 uint64 [N, 5] after the seeded reset (rng: PCG64 state high / low, inc high / low,
  has_uint32 | uinteger << 32 -- the words of mpk_nprng_state);
  after each step: final_obs float32 [S, N, n], reward float64 [S, N], terminated / truncated bool [S, N], q / qd float64 [S, N, D],
  steps int32 [S, N], task float64 [S, N, 2 | 3], rng uint64 [S, N, 5] (all AFTER the autoreset of that step), HoleReacher also
  is_collided / is_success bool [S, N], kind int8 [S, N] (0 none, 1 joint limit, 2 links crossing, 3 wall) and margin float64 [S, N]
  (the smallest distance of a deciding comparison of that step to its threshold);
  reset_at int32 [R, 2] (step, env) and reset_obs float32 [R, n]: the vector env's obs is final_obs, with these rows replaced.
Every margin is asserted >= 1e-9 here; a drawn row that misses is redrawn.  meta: numpy version, sha256 of this file and of every
reference file read.

    python tests/golden/make_ref_step_env_golden.py [--check]
"""
import ast
import hashlib
import json
import os
import sys
from typing import Any, Dict, Iterable, Optional, Tuple, Union

import numpy as np

REF = "/root/reference/fancy_gym/envs/classic_control"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_step_envs.npz")
DT, LIMIT = 0.01, 200
F32 = np.float32
M64 = (1 << 64) - 1

_read = {}


def src(name):
    with open(os.path.join(REF, name), "rb") as f:
        data = f.read()
    _read[name] = hashlib.sha256(data).hexdigest()
    return data.decode()


def klass(name, cls, wanted, base, ns):
    """class `cls`(`base`) holding only the FunctionDefs `wanted` of class `cls` in file `name`, compiled and run in `ns`"""
    tree = ast.parse(src(name), filename=name)
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    defs = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(d.name for d in defs) == sorted(wanted), (name, cls, sorted(d.name for d in defs))
    node = ast.ClassDef(name=cls, bases=[ast.Name(id=base, ctx=ast.Load())], keywords=[], body=defs, decorator_list=[],
                        type_params=[])
    mod = ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[]))
    exec(compile(mod, f"{name}:{cls}", "exec"), ns)
    return ns[cls]


class GymEnv:
    """the part of gymnasium.Env a reset touches (gymnasium/core.py: Env.reset, Env.np_random; utils/seeding.py: np_random)"""
    _np_random = None

    def reset(self, *, seed=None, options=None):
        if seed is not None:
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))

    @property
    def np_random(self):
        if self._np_random is None:
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence()))
        return self._np_random


def build_classes():
    gym = type("gym", (), {"Env": GymEnv})
    ns = {"np": np, "gym": gym, "GymEnv": GymEnv, "Optional": Optional, "Dict": Dict, "Any": Any, "Tuple": Tuple, "Union": Union,
          "Iterable": Iterable, "ObsType": Any}
    tree = ast.parse(src("utils.py"), filename="utils.py")
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("ccw", "intersect"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), "utils.py:" + node.name, "exec"), ns)
    klass("base_reacher/base_reacher.py", "BaseReacherEnv",
          ["reset", "_update_joints", "_check_self_collision", "dt", "current_pos", "end_effector"], "GymEnv", ns)
    klass("base_reacher/base_reacher_torque.py", "BaseReacherTorqueEnv", ["step"], "BaseReacherEnv", ns)
    klass("base_reacher/base_reacher_direct.py", "BaseReacherDirectEnv", ["step"], "BaseReacherEnv", ns)
    simple = klass("simple_reacher/simple_reacher.py", "SimpleReacherEnv",
                   ["reset", "_get_reward", "_terminate", "_get_obs", "_generate_goal", "_check_collisions"], "BaseReacherTorqueEnv", ns)
    hole = klass("hole_reacher/hole_reacher.py", "HoleReacherEnv",
                 ["reset", "_get_reward", "_terminate", "_generate_hole", "_get_obs", "_get_line_points", "_check_collisions",
                  "check_wall_collision"], "BaseReacherDirectEnv", ns)
    rewards = {}
    for rew, fname in (("simple", "hr_simple_reward.py"), ("vel_acc", "hr_dist_vel_acc_reward.py"),
                       ("unbounded", "hr_unbounded_reward.py")):
        rewards[rew] = klass("hole_reacher/" + fname, "HolereacherReward", ["__init__", "reset", "get_reward"], "object", {"np": np})

    def common(self, n_links, random_start, allow_self_collision):
        # BaseReacherEnv.__init__ (base_reacher.py:16-58): the attributes reset and step read
        self.link_lengths = np.ones(n_links)
        self.n_links = n_links
        self._dt = 0.01
        self.random_start = random_start
        self.allow_self_collision = allow_self_collision
        self._joints = self._joint_angles = self._angle_velocity = self._acc = None
        self._start_pos = np.hstack([[np.pi / 2], np.zeros(n_links - 1)])
        self._start_vel = np.zeros(n_links)
        self.j_min = -np.pi * np.ones(n_links)
        self.j_max = np.pi * np.ones(n_links)
        self.steps_before_reward = 199
        self._steps = 0

    def simple_init(self, n_links, target=None, random_start=True, allow_self_collision=False):
        common(self, n_links, random_start, allow_self_collision)
        self.inital_target = target                  # simple_reacher.py:23 (sic)
        self._goal = None
        self._start_pos = np.zeros(n_links)          # simple_reacher.py:29
        self.steps_before_reward = 199

    def hole_init(self, n_links, hole_x=None, hole_depth=None, hole_width=1., random_start=False, allow_self_collision=False,
                  allow_wall_collision=False, collision_penalty=1000, rew_fct="simple"):
        common(self, n_links, random_start, allow_self_collision)
        self.initial_x, self.initial_width, self.initial_depth = hole_x, hole_width, hole_depth
        self._tmp_x = self._tmp_width = self._tmp_depth = self._goal = None
        if rew_fct == "unbounded":                   # hole_reacher.py:48-58
            self.reward_function = rewards[rew_fct](allow_self_collision, allow_wall_collision)
        else:
            self.reward_function = rewards[rew_fct](allow_self_collision, allow_wall_collision, collision_penalty)

    simple.__init__ = simple_init
    hole.__init__ = hole_init
    hole._set_patches = lambda self: None
    return simple, hole


def rng_words(env):
    st = env.np_random.bit_generator.state
    s, i = st["state"]["state"], st["state"]["inc"]
    return np.array([s >> 64, s & M64, i >> 64, i & M64, (st["has_uint32"] & 0xFFFFFFFF) | (st["uinteger"] << 32)], dtype=np.uint64)


def task_row(env, hole):
    if hole:
        return np.array([env._tmp_x, env._tmp_width, env._tmp_depth], np.float64)
    return np.asarray(env._goal, np.float64)


def hole_margin(env, paid):
    """smallest distance of the comparisons that decide this step's flags to their thresholds (make_ref_hole_reacher_golden.py)"""
    m = np.inf
    D = env.n_links
    if not env.allow_self_collision:
        m = min(m, float(np.min(np.abs(np.pi - np.abs(env._joint_angles)))))
        j = env._joints
        for i in range(D):
            for k in range(i + 2, D):
                A, B, C, E = j[i], j[i + 1], j[k], j[k + 1]
                for a, b, c in ((A, C, E), (B, C, E), (A, B, C), (A, B, E)):
                    v = (c[1] - a[1]) * (b[0] - a[0]) - (b[1] - a[1]) * (c[0] - a[0])
                    m = min(m, abs(v - 1e-12))
    if not env.reward_function.allow_wall_collision:
        p = env._get_line_points(num_points_per_link=100)
        px, py = p[..., 0].ravel()[1:], p[..., 1].ravel()[1:]     # (the first point is the origin, exactly, everywhere)
        hl, hr = env._tmp_x - env._tmp_width / 2, env._tmp_x + env._tmp_width / 2
        for region in (np.maximum(px - hl, py), np.maximum(hr - px, py),
                       np.maximum(np.maximum(hl - px, px - hr), py + env._tmp_depth)):
            m = min(m, abs(float(np.min(region))))
    if paid:
        m = min(m, abs(float(np.linalg.norm(env.end_effector - env._goal)) - 0.005))
    return m


def collision_kind(env):
    if not env.allow_self_collision:
        if np.any(env._joint_angles > env.j_max) or np.any(env._joint_angles < env.j_min):
            return 1
        if env._check_self_collision():
            return 2
    return 3


def run_env(make, seed, actions, hole):
    """one sub-env of the vector env over all steps; None when a margin misses 1e-9"""
    env = make()
    obs0, _ = env.reset(seed=int(seed))
    S = actions.shape[0]
    r = dict(obs0=obs0, q0=np.array(env._joint_angles, np.float64), qd0=np.array(env._angle_velocity, np.float64),
             task0=task_row(env, hole), rng0=rng_words(env))
    rows = {k: [] for k in ("final_obs", "reward", "terminated", "truncated", "q", "qd", "steps", "task", "rng", "is_collided",
                            "is_success", "kind", "margin")}
    resets = []
    elapsed = 0
    for t in range(S):
        step_before = env._steps
        obs, reward, terminated, truncated, info = env.step(actions[t])
        assert obs.dtype == F32 and actions[t].dtype == F32
        elapsed += 1
        truncated = elapsed >= LIMIT                              # gymnasium.wrappers.TimeLimit
        if hole:
            collided = bool(info["is_collided"])
            assert bool(terminated) == collided
            paid = step_before == 199 or collided
            m = hole_margin(env, paid)
            if m < 1e-9:
                return None
            rows["is_collided"].append(collided)
            rows["is_success"].append(bool(info["is_success"]))
            rows["kind"].append(collision_kind(env) if collided else 0)
            rows["margin"].append(m)
        else:
            assert not terminated
        rows["final_obs"].append(obs)
        rows["reward"].append(float(reward))
        rows["terminated"].append(bool(terminated))
        rows["truncated"].append(bool(truncated))
        if terminated or truncated:                               # same-step autoreset: reset() without a seed
            obs, _ = env.reset()
            elapsed = 0
            resets.append((t, obs))
        rows["q"].append(np.array(env._joint_angles, np.float64))
        rows["qd"].append(np.array(env._angle_velocity, np.float64))
        rows["steps"].append(env._steps)
        rows["task"].append(task_row(env, hole))
        rows["rng"].append(rng_words(env))
    r.update(rows=rows, resets=resets)
    return r


def grid(x, bits=8):
    """float32 values on a grid of 2^-bits"""
    return (np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F32)


def smooth(rng, amp, S, D):
    """a float32 profile: a few random sinusoids, on a grid of 2^-8 (the fixture compresses)"""
    t = np.arange(S)[:, None] * DT
    out = np.zeros((S, D))
    for _ in range(3):
        out += rng.uniform(-amp, amp, D) * np.sin(rng.uniform(0.2, 3.0, D) * t * 2 * np.pi + rng.uniform(0, 2 * np.pi, D))
    return grid(out)


BEND = dict(j1=0.3125, j2=-0.203125, j3=0.15625, j4=0.265625)      # no symmetry: no chord parallel to a link


def const(S, D, **cols):
    """constant velocities.  Five links: every joint the caller leaves out bends slowly (BEND), so that no two links are ever
    collinear -- the straight arm of a reset has ccw = 0, a margin of 1e-12 to its threshold"""
    a = np.zeros((S, D), F32)
    for k, v in (dict(BEND, **cols) if D == 5 else cols).items():
        a[:, int(k[1:])] = v
    return a


def servo(make, seed, S, D, target, vmax=3.0):
    """float32 grid actions that drive the first HoleReacher episode's joints to `target`, the first joint last, then hold; the steps
    behind that episode bend the arm slowly (BEND).  Planned on a scratch env with the same seed, so the start is the episode's own"""
    env = make()
    env.reset(seed=int(seed))
    acts = const(S, D)
    for t in range(S):
        err = (target - env._joint_angles) / DT
        move = np.abs(err) >= 2.0 ** -9
        if move[1:].any():
            move[0] = False                                       # the first joint sweeps the arm down once the others are in place
        acts[t] = grid(np.where(move, np.clip(err, -vmax, vmax), 0.0))
        _, _, terminated, _, _ = env.step(acts[t])
        if terminated or env._steps >= LIMIT:
            break
    return acts


def traces(simple, hole):
    """(name, constants, make, seed, [per-env action builder])"""
    out = []
    S_LONG, S_SHORT = 403, 120

    def simple_trace(name, n_links, S, **kw):
        def rows(rng):
            D = n_links
            big = smooth(rng, 40.0, S, D)
            big[5::37] = grid(rng.choice([-1.0, 1.0], (len(big[5::37]), D)) * rng.uniform(1000.5, 2500.0, (len(big[5::37]), D)))
            return [lambda s: smooth(rng, 5.0, S, D), lambda s: big]
        out.append((name, dict(env="simple_reacher", n_links=n_links, kwargs=kw), lambda: simple(n_links, **kw), rows))

    simple_trace("simple2", 2, S_LONG)
    simple_trace("simple5", 5, S_LONG)
    simple_trace("simple2_fixed", 2, 210, target=(0.5, -1.25), random_start=False)

    reg = dict(random_start=True, allow_self_collision=False, allow_wall_collision=False, hole_width=None, hole_depth=1, hole_x=None,
               collision_penalty=100)      # fancy/HoleReacher-v0 (envs/__init__.py:72-88)

    def hole_trace(name, S, rows, **kw):
        k = dict(reg, **kw)
        out.append((name, dict(env="hole_reacher", n_links=5, kwargs=k), lambda: hole(5, **k), rows))

    D = 5
    for rew in ("simple", "vel_acc", "unbounded"):
        # survivors: run into truncation at step 200 and pay the step-199 distance, also with actions beyond +-2 pi
        def long_rows(rng, S=S_LONG):
            def wild(s):
                w = smooth(rng, 0.2, S, D) + const(S, D)
                w[::2, 1] += 7.0
                w[1::2, 1] -= 7.0
                return grid(w)
            return [lambda s: smooth(rng, 0.3, S, D), wild, lambda s: const(S, D)]
        hole_trace(f"hole_{rew}_long", S_LONG, long_rows, rew_fct=rew)

        # collisions of each kind, again and again: every hit starts the next episode in the same step
        def short_rows(rng, S=S_SHORT):
            return [lambda s: const(S, D, j0=3.0), lambda s: const(S, D, j0=-7.5), lambda s: const(S, D, j2=4.0, j3=-4.0),
                    lambda s: const(S, D, j1=9.0), lambda s: smooth(rng, 3.0, S, D), lambda s: smooth(rng, 6.0, S, D)]
        hole_trace(f"hole_{rew}_short", S_SHORT, short_rows, rew_fct=rew)
        # the links cross where the wall is switched off
        hole_trace(f"hole_{rew}_cross", 100, lambda rng: [lambda s: const(100, D, j1=2.0, j2=2.0, j3=2.0, j4=2.0),
                                                          lambda s: const(100, D, j2=2.5, j3=2.5, j4=2.5)],
                   rew_fct=rew, allow_wall_collision=True)
        # a fixed hole the arm reaches into: success at step 199.  Four links to the left, each rising a little less than the one
        # before (cumulative angles pi - a_i: above the floor, never collinear), the last one hanging into the hole: |ee - goal| =
        # sum(sin a_i) = 0.0039 < 0.005
        rise = np.array([0.0016, 0.0007, 0.0012, 0.0004])
        cum = np.append(np.pi - rise, 1.5 * np.pi)
        target = np.diff(cum, prepend=0.0)
        hx = round(float(np.sum(np.cos(cum))), 6)
        fixed = dict(reg, rew_fct=rew, hole_x=hx, hole_width=0.4, hole_depth=1.0)

        def reach_rows(rng, fixed=fixed, target=target):
            mk = lambda: hole(5, **fixed)      # noqa: E731
            return [lambda s: servo(mk, s, 205, D, target), lambda s: servo(mk, s, 205, D, target, vmax=3.5)]
        hole_trace(f"hole_{rew}_reach", 205, reach_rows, rew_fct=rew, hole_x=hx, hole_width=0.4, hole_depth=1.0)
    # the allow_* toggles, both penalties, random_start=False with a fixed width
    for i, (a_self, a_wall) in enumerate(((True, False), (False, True), (True, True))):
        def toggle_rows(rng, S=90):
            return [lambda s: const(S, D, j0=3.0), lambda s: const(S, D, j2=4.0, j3=-4.0), lambda s: smooth(rng, 6.0, S, D)]
        hole_trace(f"hole_allow_{int(a_self)}{int(a_wall)}", 90, toggle_rows, allow_self_collision=a_self, allow_wall_collision=a_wall,
                   collision_penalty=(100, 1000, 100)[i], rew_fct=("simple", "vel_acc", "unbounded")[i])
    hole_trace("hole_penalty_1000_still_start", 90, lambda rng: [lambda s: const(90, D, j0=-3.0), lambda s: smooth(rng, 6.0, 90, D)],
               collision_penalty=1000, random_start=False, hole_width=0.3)
    return out


def generate():
    simple, hole = build_classes()
    out, index = {}, []
    for ti, (name, consts, make, rows_of) in enumerate(traces(simple, hole)):
        is_hole = consts["env"] == "hole_reacher"
        rng = np.random.default_rng(20261016 + ti)
        seed = 1000 * (ti + 1)
        builders = rows_of(rng)
        envs, acts = [], []
        for b, build in enumerate(builders):
            for attempt in range(20):
                a = np.ascontiguousarray(build(seed + b), F32)
                r = run_env(make, seed + b, a, is_hole)
                if r is not None:
                    break
            assert r is not None, (name, b, "margin < 1e-9 in 20 draws")
            envs.append(r)
            acts.append(a)
        N, S = len(envs), acts[0].shape[0]
        put = lambda k, v: out.__setitem__(f"{name}__{k}", v)      # noqa: E731
        put("actions", np.stack(acts, axis=1))
        for k, dt_ in (("obs0", F32), ("q0", np.float64), ("qd0", np.float64), ("task0", np.float64), ("rng0", np.uint64)):
            put(k, np.stack([e[k] for e in envs]).astype(dt_))
        kinds = dict(final_obs=F32, reward=np.float64, terminated=bool, truncated=bool, q=np.float64, qd=np.float64, steps=np.int32,
                     task=np.float64, rng=np.uint64)
        if is_hole:
            kinds.update(is_collided=bool, is_success=bool, kind=np.int8, margin=np.float64)
        for k, dt_ in kinds.items():
            put(k, np.stack([np.stack([np.asarray(v) for v in e["rows"][k]]) for e in envs], axis=1).astype(dt_))
        at = sorted((t, b) for b, e in enumerate(envs) for t, _ in e["resets"])
        obs_of = {(t, b): o for b, e in enumerate(envs) for t, o in e["resets"]}
        n = envs[0]["obs0"].shape[0]
        put("reset_at", np.array(at, np.int32).reshape(-1, 2))
        put("reset_obs", np.stack([obs_of[k] for k in at]).astype(F32) if at else np.zeros((0, n), F32))
        kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in consts["kwargs"].items()}
        index.append(dict(name=name, env=consts["env"], n_links=consts["n_links"], kwargs=kw, seed=seed, N=N, S=S))
    out["traces"] = np.array(json.dumps(index, sort_keys=True))
    coverage(out, index)
    with open(os.path.abspath(__file__), "rb") as f:
        gen = hashlib.sha256(f.read()).hexdigest()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "generator": gen, "reference_files": _read}, sort_keys=True))
    return out


def coverage(out, index):
    """what the traces must show"""
    for tr in index:
        g = lambda k: out[f"{tr['name']}__{k}"]      # noqa: E731
        name = tr["name"]
        if tr["env"] == "simple_reacher":
            assert not g("terminated").any()
            assert g("truncated").sum(axis=0).min() >= (2 if tr["S"] >= 400 else 1), name
            if "fixed" not in name:
                assert np.abs(g("actions")).max() > 1000.0, name
            continue
        assert g("margin").min() >= 1e-9, name
        rew = tr["kwargs"].get("rew_fct", "simple")
        if name.endswith("_long"):
            assert g("truncated").sum(axis=0).min() >= 2 and not g("terminated").any(), name
            assert np.abs(g("actions")).max() > 2 * np.pi, name
        if name.endswith("_short"):
            kinds = set(np.unique(g("kind")).tolist())
            assert {1, 3} <= kinds, (name, kinds)
            assert np.abs(g("actions")).max() > 2 * np.pi, name
            assert (g("is_collided").sum(axis=0) >= 1).sum() >= 4, name
        if name.endswith("_cross"):
            assert 2 in np.unique(g("kind")).tolist(), name
        if name.endswith("_reach"):
            # the success is paid at step 199: the step that truncates
            ok = g("is_success") & g("truncated")
            assert ok.any(axis=0).all(), (name, rew)


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
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for tr in json.loads(str(out["traces"])):
        g = lambda k: out[f"{tr['name']}__{k}"]      # noqa: E731
        extra = ""
        if tr["env"] == "hole_reacher":
            extra = f" collided {int(g('is_collided').sum())} kinds {np.bincount(g('kind').ravel(), minlength=4).tolist()} " \
                    f"success {int(g('is_success').sum())} min margin {g('margin').min():.2e}"
        print(f"  {tr['name']}: N {tr['N']} S {tr['S']} resets {len(g('reset_at'))} truncated {int(g('truncated').sum())}{extra}")


if __name__ == "__main__":
    main()
