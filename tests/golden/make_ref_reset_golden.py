#!/usr/bin/env python3
"""
Reference-generated fixture for the resets of SimpleReacher and HoleReacher (build container only: reads the reference checkout).

The reference package cannot be imported here (gymnasium / matplotlib are absent), so -- as make_ref_hole_reacher_golden.py does --
the FunctionDefs a reset runs are taken from their files with `ast` and compiled ALONE: BaseReacherEnv.reset, SimpleReacherEnv.reset
/ _generate_goal and HoleReacherEnv.reset / _generate_hole.  Each group is compiled inside a class of its own name (so that `super()`
resolves as in the reference) on top of a stand-in for gymnasium.Env.  Stubbed out: _set_patches, the reward function's reset,
_update_joints and _get_obs (none of them draws).  No reference text is stored.

Restated here, because gymnasium is not installed: gymnasium.Env.reset(seed=s) seeds the env with gymnasium.utils.seeding.np_random(s),
which is np.random.Generator(np.random.PCG64(np.random.SeedSequence(s))); Env.np_random returns that generator.

Output: tests/golden/ref_reacher_resets.npz, one row per episode, NR = 4 resets per episode (reset(seed=seed), then reset() x 3):
  kind int [E] (0 SimpleReacher, 1 HoleReacher), n_links int [E], random_start bool [E], target float64 [E, 2], hole_width / hole_x /
  hole_depth float64 [E] (the env's kwargs; NaN = None, i.e. drawn), seed uint64 [E];
  q0 float64 [E, NR, 5] (joint angles after each reset, NaN beyond n_links), task float64 [E, NR, 3] (SimpleReacher: goal x, y, NaN;
  HoleReacher: x, width, depth), state uint64 [E, NR, 4] (PCG64 state high / low, inc high / low after each reset), has_uint32 uint8
  [E, NR], uinteger uint32 [E, NR]; meta (numpy version, sha256 of this file and of every reference file).

    python tests/golden/make_ref_reset_golden.py [--check]
"""
import ast
import hashlib
import json
import os
import sys
from typing import Any, Dict, Optional, Tuple

import numpy as np

REF = "/root/reference/fancy_gym/envs/classic_control"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_reacher_resets.npz")
NR, DMAX = 4, 5
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
    assert sorted(d.name for d in defs) == sorted(wanted), (name, cls)
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


class _Stub:
    def reset(self):
        pass


def build_classes():
    gym = type("gym", (), {"Env": GymEnv})
    ns = {"np": np, "gym": gym, "GymEnv": GymEnv, "Optional": Optional, "Dict": Dict, "Any": Any, "Tuple": Tuple,
          "ObsType": Any}
    base = klass("base_reacher/base_reacher.py", "BaseReacherEnv", ["reset"], "GymEnv", ns)
    simple = klass("simple_reacher/simple_reacher.py", "SimpleReacherEnv", ["reset", "_generate_goal"], "BaseReacherEnv", ns)
    hole = klass("hole_reacher/hole_reacher.py", "HoleReacherEnv", ["reset", "_generate_hole"], "BaseReacherEnv", ns)

    def common(self, n_links, random_start):
        # BaseReacherEnv.__init__ (base_reacher.py:16-35): the attributes a reset reads
        self.n_links = n_links
        self.link_lengths = np.ones(n_links)
        self.random_start = random_start
        self._start_pos = np.hstack([[np.pi / 2], np.zeros(n_links - 1)])
        self._start_vel = np.zeros(n_links)
        self._steps = 0

    def simple_init(self, n_links, target, random_start):
        common(self, n_links, random_start)
        self.inital_target = target                  # simple_reacher.py:23 (sic)
        self._start_pos = np.zeros(n_links)          # simple_reacher.py:29

    def hole_init(self, n_links, hole_x, hole_depth, hole_width, random_start):
        common(self, n_links, random_start)
        self.initial_x, self.initial_width, self.initial_depth = hole_x, hole_width, hole_depth
        self.reward_function = _Stub()

    for c, init in ((simple, simple_init), (hole, hole_init)):
        c.__init__ = init
        c._update_joints = lambda self: None
        c._get_obs = lambda self: np.zeros(1)
        c._set_patches = lambda self: None
    assert base.reset is not GymEnv.reset
    return simple, hole


def configs():
    """(kind, n_links, random_start, target, hole_width, hole_x, hole_depth, n_random_seeds); None = drawn"""
    out = []
    for n in (2, 5):
        for rs in (True, False):
            for target in (None, (0.5, -1.25)):
                default = rs and target is None
                out.append((0, n, rs, target, None, None, None, 300 if default else 24))
            for width in (None, 0.3):
                for x in (None, 1.75):
                    for depth in (None, 1.0):
                        default = rs and width is None and x is None and depth == 1.0
                        out.append((1, n, rs, None, width, x, depth, 300 if default else 24))
    return out


EDGE_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]


def generate():
    simple, hole = build_classes()
    rows = []
    for ci, (kind, n, rs, target, width, x, depth, n_rand) in enumerate(configs()):
        rand = np.random.default_rng(1000 + ci).integers(0, 2 ** 64, size=n_rand, dtype=np.uint64, endpoint=False)
        for seed in EDGE_SEEDS + [int(s) for s in rand]:
            env = simple(n, None if target is None else np.array(target), rs) if kind == 0 else hole(n, x, depth, width, rs)
            q0 = np.full((NR, DMAX), np.nan)
            task = np.full((NR, 3), np.nan)
            state = np.zeros((NR, 4), np.uint64)
            has32 = np.zeros(NR, np.uint8)
            u32 = np.zeros(NR, np.uint32)
            for k in range(NR):
                env.reset(seed=seed if k == 0 else None)
                q0[k, :n] = env._joint_angles
                if kind == 0:
                    task[k, :2] = env._goal
                else:
                    task[k] = (env._tmp_x, env._tmp_width, env._tmp_depth)
                st = env.np_random.bit_generator.state
                s, inc = st["state"]["state"], st["state"]["inc"]
                state[k] = (s >> 64, s & M64, inc >> 64, inc & M64)
                has32[k], u32[k] = st["has_uint32"], st["uinteger"]
            nan = float("nan")
            rows.append(dict(kind=kind, n_links=n, random_start=rs, target=target if target is not None else (nan, nan),
                             hole_width=nan if width is None else width, hole_x=nan if x is None else x,
                             hole_depth=nan if depth is None else depth, seed=seed, q0=q0, task=task, state=state,
                             has_uint32=has32, uinteger=u32))
    out = {"kind": np.array([r["kind"] for r in rows], np.int32), "n_links": np.array([r["n_links"] for r in rows], np.int32),
           "random_start": np.array([r["random_start"] for r in rows], bool),
           "target": np.array([r["target"] for r in rows], np.float64), "seed": np.array([r["seed"] for r in rows], np.uint64)}
    for key in ("hole_width", "hole_x", "hole_depth"):
        out[key] = np.array([r[key] for r in rows], np.float64)
    for key in ("q0", "task", "state", "has_uint32", "uinteger"):
        out[key] = np.stack([r[key] for r in rows])
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
            assert np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("ok: matches", OUT)
        return
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out["kind"]), "episodes,", int((out["kind"] == 0).sum()), "SimpleReacher")


if __name__ == "__main__":
    main()
