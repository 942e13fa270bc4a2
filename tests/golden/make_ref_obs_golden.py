#!/usr/bin/env python3
"""
Reference-generated fixture for the observations of SimpleReacher and HoleReacher (build container only: reads the reference checkout).

As make_ref_reset_golden.py does, the FunctionDefs an observation runs are taken from their files with `ast` and compiled ALONE, each
inside a class of its own name: BaseReacherEnv._update_joints / end_effector, SimpleReacherEnv._get_obs, HoleReacherEnv._get_obs, both
MPWrapper.context_mask, TimeAwareObservation.observation, BlackBoxWrapper.observation / _get_observation_space, and the `state_bound`
statement of SimpleReacherEnv.__init__ / HoleReacherEnv.__init__ (the env's observation bounds).  They run on a SimpleNamespace-like
self holding stored states.  The float64 row before the cast comes from the same _get_obs with its final `.astype(np.float32)` taken
off the returned expression (an AST edit of the compiled copy).  No reference text is stored.

Restated here, because gymnasium is not installed: spaces.Box(low, high, shape=None, dtype=np.float32) keeps low / high cast to the
dtype; TimeAwareObservation's space appends [0, 1] to the bounds (utils/wrappers.py:33-38).

Output: tests/golden/ref_reacher_obs.npz, one row per stored state, NC = 3 * 5 + 4 columns (NaN / False beyond the row):
  kind int [E] (0 SimpleReacher, 1 HoleReacher), n_links int [E], random_start bool [E], width_given bool [E] (HoleReacher hole_width
  not None), q float64 [E, 5], qd float64 [E, 5], qd_f32 bool [E] (qd held as float32, HoleReacher's dtype rule), task float64 [E, 3]
  (SimpleReacher: goal x, y, NaN; HoleReacher: x, width, depth), steps int [E];
  obs32 float32 [E, NC] (_get_obs), obs64 float64 [E, NC] (its row before the cast), context_mask bool [E, NC],
  ctx32 float32 [E, NC] (BlackBoxWrapper.observation without replanning: the context row), ta32 float32 [E, NC + 1] / ta64 float64
  (with replanning: TimeAwareObservation then BlackBoxWrapper.observation, max_episode_steps = 200; ta64 before the cast),
  ctx_low / ctx_high float32 [E, NC], ta_low / ta_high float32 [E, NC + 1] (the wrapper's observation_space bounds); meta (numpy
  version, sha256 of this file and of every reference file).

    python tests/golden/make_ref_obs_golden.py [--check]
"""
import ast
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

REF = "/root/reference/fancy_gym"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_reacher_obs.npz")
DMAX = 5
NC = 3 * DMAX + 4
MAX_STEPS = 200

_read = {}


def src(name):
    with open(os.path.join(REF, name), "rb") as f:
        data = f.read()
    _read[name] = hashlib.sha256(data).hexdigest()
    return data.decode()


def class_defs(name, cls, wanted):
    tree = ast.parse(src(name), filename=name)
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    defs = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(d.name for d in defs) == sorted(wanted), (name, cls)
    return defs


def klass(name, cls, wanted, ns, edit=None):
    """class `cls` holding only the FunctionDefs `wanted` of class `cls` in file `name` (after `edit`), compiled in `ns`"""
    defs = class_defs(name, cls, wanted)
    if edit:
        defs = [edit(d) for d in defs]
    node = ast.ClassDef(name=cls, bases=[], keywords=[], body=defs, decorator_list=[], type_params=[])
    mod = ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[]))
    exec(compile(mod, f"{name}:{cls}", "exec"), ns)
    return ns[cls]


def strip_astype(fn):
    """the _get_obs FunctionDef with `return X.astype(...)` turned into `return X` (the float64 row before the cast)"""
    fn = ast.parse(ast.unparse(fn)).body[0]
    ret = fn.body[-1]
    assert isinstance(ret, ast.Return) and isinstance(ret.value, ast.Call) and ret.value.func.attr == "astype"
    ret.value = ret.value.func.value
    return fn


def state_bound(name, cls, n_links):
    """the `state_bound = np.hstack(...)` statement of cls.__init__, run with self.n_links = n_links"""
    init = class_defs(name, cls, ["__init__"])[0]
    stmt = [s for s in init.body if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", None) == "state_bound"]
    assert len(stmt) == 1, (name, cls)
    ns = {"np": np, "self": SimpleNamespace(n_links=n_links)}
    exec(compile(ast.fix_missing_locations(ast.Module(body=stmt, type_ignores=[])), f"{name}:{cls}.__init__", "exec"), ns)
    return ns["state_bound"]


class Box:
    """the part of gymnasium.spaces.Box these functions read"""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.low = np.asarray(low).astype(self.dtype)
        self.high = np.asarray(high).astype(self.dtype)
        self.shape = self.low.shape


def build():
    ns = {"np": np, "property": property}
    cr = "envs/classic_control/"
    base = klass(cr + "base_reacher/base_reacher.py", "BaseReacherEnv", ["_update_joints", "end_effector"], ns)
    simple = klass(cr + "simple_reacher/simple_reacher.py", "SimpleReacherEnv", ["_get_obs"], ns)
    hole = klass(cr + "hole_reacher/hole_reacher.py", "HoleReacherEnv", ["_get_obs"], ns)
    simple64 = klass(cr + "simple_reacher/simple_reacher.py", "SimpleReacherEnv", ["_get_obs"], dict(ns), strip_astype)
    hole64 = klass(cr + "hole_reacher/hole_reacher.py", "HoleReacherEnv", ["_get_obs"], dict(ns), strip_astype)
    smask = klass(cr + "simple_reacher/mp_wrapper.py", "MPWrapper", ["context_mask"], dict(ns))
    hmask = klass(cr + "hole_reacher/mp_wrapper.py", "MPWrapper", ["context_mask"], dict(ns))
    tns = dict(ns, Box=Box, OldBox=None)
    ta = klass("utils/wrappers.py", "TimeAwareObservation", ["observation"], tns)
    bns = dict(ns, spaces=SimpleNamespace(Box=Box))
    bb = klass("black_box/black_box_wrapper.py", "BlackBoxWrapper", ["observation", "_get_observation_space"], bns)
    return dict(base=base, obs={0: simple, 1: hole}, obs64={0: simple64, 1: hole64}, mask={0: smask, 1: hmask}, ta=ta, bb=bb)


class Env:
    """the reacher env's state as _get_obs reads it; methods are bound from the compiled classes"""


def make_env(f, kind, n, random_start, width_given, q, qd, task, steps):
    e = Env()
    e.n_links, e.link_lengths, e.random_start = n, np.ones(n), random_start
    e._joint_angles, e._angle_velocity, e._steps = q, qd, steps
    e._joints = np.zeros((n + 1, 2))
    if kind == 0:
        e._goal = task[:2].copy()
    else:
        e._tmp_x, e._tmp_width, e._tmp_depth = task
        e._goal = np.hstack([e._tmp_x, -e._tmp_depth])          # hole_reacher.py:101
        e.initial_width = task[1] if width_given else None
    f["base"]._update_joints(e)
    return e


def observe(f, kind, e, n):
    """(obs32, obs64, mask, ctx32, ta32, ta64, ctx space, ta space) of one state"""
    Env.end_effector = f["base"].end_effector
    obs32 = f["obs"][kind]._get_obs(e)
    obs64 = f["obs64"][kind]._get_obs(e)
    w = SimpleNamespace(env=e)
    mask = f["mask"][kind].context_mask.fget(w)
    name = "envs/classic_control/" + ("simple_reacher/simple_reacher.py" if kind == 0 else "hole_reacher/hole_reacher.py")
    bound = state_bound(name, "SimpleReacherEnv" if kind == 0 else "HoleReacherEnv", n)
    env_space = Box(low=-bound, high=bound, shape=bound.shape)
    # BlackBoxWrapper without replanning: the context row, the masked space
    ctx_env = SimpleNamespace(context_mask=mask, observation_space=env_space)
    wrap = SimpleNamespace(env=ctx_env, return_context_observation=True)
    ctx_space = f["bb"]._get_observation_space(wrap)
    wrap.observation_space = ctx_space
    ctx32 = f["bb"].observation(wrap, obs32.copy())
    # with replanning: TimeAwareObservation (t = the env's step counter), then the wrapper returns the full row
    ta_space = Box(np.append(env_space.low, 0.0), np.append(env_space.high, 1.0), dtype=env_space.dtype)
    taw = SimpleNamespace(t=e._steps, env=SimpleNamespace(spec=SimpleNamespace(max_episode_steps=MAX_STEPS)), observation_space=ta_space)
    ta64 = f["ta"].observation(taw, obs32.copy())
    wrap2 = SimpleNamespace(env=SimpleNamespace(context_mask=mask, observation_space=ta_space), return_context_observation=False)
    full_space = f["bb"]._get_observation_space(wrap2)
    wrap2.observation_space = full_space
    ta32 = f["bb"].observation(wrap2, ta64)
    assert ta32.dtype == np.float32 and ctx32.dtype == np.float32 and obs32.dtype == np.float32
    assert np.array_equal(obs64.astype(np.float32), obs32)
    return obs32, obs64, np.asarray(mask, bool), ctx32, ta32, np.asarray(ta64, np.float64), ctx_space, full_space


def states(rng, kind, n, width_given, k):
    """k stored states: random and edge angles, zero / large velocities (float32 ones for HoleReacher), goals / holes from the
    device reset's ranges, steps 0, 1, 199, 200 and random ones"""
    out = []
    edge_q = [np.pi, -np.pi, np.nextafter(np.pi, 4.0), np.nextafter(-np.pi, -4.0), np.pi / 2, 3.5, -7.25, 0.0, 1e-300, 40.0]
    for i in range(k):
        q = rng.uniform(-4.0, 4.0, n)
        if i % 3 == 1:
            q[rng.integers(n)] = edge_q[i % len(edge_q)]
        if i % 7 == 2:
            q = np.zeros(n)
            q[0] = rng.uniform(np.pi / 4, 3 * np.pi / 4)
        qd = [np.zeros(n), rng.standard_normal(n), rng.standard_normal(n) * 1e3, rng.uniform(-5e4, 5e4, n)][i % 4]
        f32 = kind == 1 and i % 2 == 1
        if f32:
            qd = qd.astype(np.float32)
        if kind == 0:
            L = float(n)
            while True:
                g = rng.uniform(-L, L, 2)
                if np.linalg.norm(g) < L:
                    break
            task = np.array([g[0], g[1], np.nan])
        else:
            width = 0.3 if width_given else rng.uniform(0.15, 0.5)
            x = rng.choice([-1, 1]) * rng.uniform(width / 2, 3.5)
            task = np.array([x, width, 1.0])
        steps = [0, 1, 199, 200][i % 4] if i < 8 else int(rng.integers(0, 201))
        out.append((q, qd, f32, task, steps))
    return out


def pad(x, width, fill, dtype):
    out = np.full(width, fill, dtype)
    out[:len(x)] = x
    return out


def generate():
    f = build()
    rows = []
    ci = 0
    for kind in (0, 1):
        for n in (2, 5):
            for rs in (True, False):
                for wg in ((False,) if kind == 0 else (False, True)):
                    rng = np.random.default_rng(7000 + ci)
                    ci += 1
                    for q, qd, f32, task, steps in states(rng, kind, n, wg, 40):
                        e = make_env(f, kind, n, rs, wg, q, qd, task, steps)
                        obs32, obs64, mask, ctx32, ta32, ta64, cs, ts = observe(f, kind, e, n)
                        rows.append(dict(
                            kind=kind, n_links=n, random_start=rs, width_given=wg, q=pad(q, DMAX, np.nan, np.float64),
                            qd=pad(np.asarray(qd, np.float64), DMAX, np.nan, np.float64), qd_f32=f32, task=task, steps=steps,
                            obs32=pad(obs32, NC, np.nan, np.float32), obs64=pad(obs64, NC, np.nan, np.float64),
                            context_mask=pad(mask, NC, False, bool), ctx32=pad(ctx32, NC, np.nan, np.float32),
                            ta32=pad(ta32, NC + 1, np.nan, np.float32), ta64=pad(ta64, NC + 1, np.nan, np.float64),
                            ctx_low=pad(cs.low, NC, np.nan, np.float32), ctx_high=pad(cs.high, NC, np.nan, np.float32),
                            ta_low=pad(ts.low, NC + 1, np.nan, np.float32), ta_high=pad(ts.high, NC + 1, np.nan, np.float32)))
    out = {}
    types = dict(kind=np.int32, n_links=np.int32, random_start=bool, width_given=bool, qd_f32=bool, steps=np.int32)
    for key in rows[0]:
        out[key] = np.array([r[key] for r in rows], types[key]) if key in types else np.stack([r[key] for r in rows])
    with open(os.path.abspath(__file__), "rb") as fh:
        gen = hashlib.sha256(fh.read()).hexdigest()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "generator": gen, "reference_files": _read}, sort_keys=True))
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for k, v in out.items():
            if k == "meta":
                continue
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("ok: matches", OUT)
        return
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out["kind"]), "states,", int((out["kind"] == 0).sum()), "SimpleReacher")


if __name__ == "__main__":
    main()
