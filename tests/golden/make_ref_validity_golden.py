#!/usr/bin/env python3
"""
Reference-generated fixture for the VALIDITY GATE of TableTennis (build container only: reads /root/reference).

TableTennisEnv.check_traj_validity and TableTennisEnv._get_traj_invalid_penalty (fancy_gym/envs/mujoco/table_tennis/
table_tennis_env.py:282-309) are pure numpy over the module globals `jnt_pos_low` / `jnt_pos_high` (table_tennis_utils.py:3-4).  The
package cannot be imported here (gymnasium / mujoco are absent), so -- as make_ref_config_golden.py does for nested_update -- the two
FunctionDefs are taken from the file with `ast`, stripped of their decorators and compiled ALONE; nothing is imported from the
package and no reference text is stored.  Each case execs them with a namespace of `np` plus that case's jnt_pos_low / jnt_pos_high;
the real limits and the tau / delay bounds come from table_tennis_utils.py by `ast.literal_eval` of the np.array(...) arguments.

Output: tests/golden/ref_validity.npz.  Per case c (names in `cases`):
  c_pos      float32 [B, T, D]   positions as get_trajectory returns them (float32; the reference compares them in float64)
  c_action   float32 [B, 2]      the RAW action[0] (tau) and action[1] (delay) the policy produced
  c_lo/c_hi  float64 [D]         joint limits;  c_tb / c_db float64 [2] tau / delay bounds
  c_valid    bool [B]            check_traj_validity(...)[0]
  c_penalty  float64 [B]         _get_traj_invalid_penalty(...) -- for EVERY row (the reference calls it for invalid rows only)
plus `meta` (numpy version, generator sha256, sha256 of every reference file read).

    python tests/golden/make_ref_validity_golden.py [--check]   (--check: regenerate in memory and compare with the committed file)
"""
import ast
import hashlib
import os
import sys

import numpy as np

REF = "/root/reference/fancy_gym/envs/mujoco/table_tennis"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_validity.npz")
F32 = np.float32

_read = {}


def src(name):
    with open(os.path.join(REF, name), "rb") as f:
        data = f.read()
    _read[name] = hashlib.sha256(data).hexdigest()
    return data.decode()


def reference_functions():
    """the two FunctionDefs of table_tennis_env.py, each compiled alone (decorators dropped: the staticmethod wrapper is all)"""
    code = {}
    for node in ast.walk(ast.parse(src("table_tennis_env.py"), filename="table_tennis_env.py")):
        if isinstance(node, ast.FunctionDef) and node.name in ("check_traj_validity", "_get_traj_invalid_penalty"):
            node.decorator_list = []
            code[node.name] = compile(ast.Module(body=[node], type_ignores=[]), "table_tennis_env.py:" + node.name, "exec")
    assert sorted(code) == ["_get_traj_invalid_penalty", "check_traj_validity"], sorted(code)

    def run(lo, hi, action, pos):
        ns = {"np": np, "jnt_pos_low": np.asarray(lo, np.float64), "jnt_pos_high": np.asarray(hi, np.float64)}
        for c in code.values():
            exec(c, ns)
        valid = ns["check_traj_validity"](action, pos, None, TB, DB)[0]
        pen = ns["_get_traj_invalid_penalty"](None, action, pos, TB, DB)
        return bool(valid), float(pen)
    return run


def utils_constants():
    """jnt_pos_low / jnt_pos_high / tau_bound / delay_bound of table_tennis_utils.py: literal_eval of the np.array argument"""
    out = {}
    for node in ast.parse(src("table_tennis_utils.py")).body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            name, v = node.targets[0].id, node.value
            if name in ("jnt_pos_low", "jnt_pos_high"):
                assert isinstance(v, ast.Call) and v.func.attr == "array" and len(v.args) == 1
                out[name] = np.array(ast.literal_eval(v.args[0]), np.float64)
            elif name in ("tau_bound", "delay_bound"):
                out[name] = np.array(ast.literal_eval(v), np.float64)
    return out


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def dn(x):
    return np.nextafter(F32(x), F32(-np.inf))


def f32_at_most(x):
    """the largest float32 <= x (float64)"""
    f = F32(x)
    return dn(f) if float(f) > x else f


def f32_at_least(x):
    f = F32(x)
    return up(f) if float(f) < x else f


def rows_for(lo, hi, T, D, rng, cfg5_quirk=False):
    """(pos [T, D] float32, action [2] float32) variants of one shape: inside, over / under, exactly on the limits, non-finite"""
    flo = np.where(np.abs(lo) < 1e30, lo, -1.0)           # (NaN and the +-1e39 limits: positions drawn in [-1, 1])
    fhi = np.where(np.abs(hi) < 1e30, hi, 1.0)
    span = np.where(fhi > flo, fhi - flo, 1.0)
    ok_act = np.array([0.5 * (TB[0] + TB[1]), 0.5 * (DB[0] + DB[1])], F32)

    def inside():
        # on a grid of 2^-10 (the fixture compresses), strictly inside
        return np.round((flo + span * rng.uniform(0.1, 0.9, (T, D))) * 1024.0).astype(F32) / F32(1024.0)

    rows = []

    def add(p, a=ok_act):
        rows.append((np.asarray(p, F32), np.asarray(a, F32)))

    t1, d1 = int(rng.integers(T)), int(rng.integers(D))
    t2, d2 = int(rng.integers(T)), (d1 + 1) % D
    add(inside())                                              # all inside
    p = inside(); p[t1, d1] = fhi[d1] + 0.01 * span[d1]; add(p)                  # one over
    p = inside(); p[t1, d1] = flo[d1] - 0.01 * span[d1]; add(p)                  # one under
    p = inside(); p[t1, d1] = fhi[d1] + 0.3; p[t2, d2] = flo[d2] - 0.7; add(p)    # over and under
    p = inside(); p[:, d1] = fhi[d1] + 0.2; add(p)                              # a whole DoF over
    for d in sorted({0, d1, D - 1}):
        # exactly on a limit: the float32 nearest to it and its two neighbours, for the high and the low limit
        for lim in (hi[d], lo[d]):
            if not abs(lim) < 1e30:
                continue
            for v in (F32(lim), up(lim), dn(lim), f32_at_most(lim), f32_at_least(lim)):
                p = inside(); p[t1, d] = v; add(p)
            p = inside(); p[:, d] = F32(lim); add(p)
    # non-finite positions, alone and beside a violation elsewhere
    for v in (np.nan, np.inf, -np.inf):
        p = inside(); p[t1, d1] = v; add(p)
        p = inside(); p[t1, d1] = v; p[t2, d2] = fhi[d2] + 0.5; add(p)
        p = inside(); p[:, d1] = v; add(p)
    p = inside(); p[t1, d1] = np.inf; p[t2, d2] = -np.inf; add(p)
    p = inside(); p[t1, d1] = np.nan; p[t2, d2] = np.inf; add(p)
    # raw tau / delay: non-finite, on the bounds, just outside, beside a position violation
    p_bad = inside(); p_bad[t2, d2] = flo[d2] - 0.25
    for a in ((np.nan, ok_act[1]), (ok_act[0], np.nan), (np.inf, ok_act[1]), (-np.inf, ok_act[1]), (ok_act[0], np.inf),
              (ok_act[0], -np.inf), (np.nan, np.nan)):
        add(inside(), a)
        add(p_bad, a)
    for a in ((TB[0], DB[0]), (TB[1], DB[1]), (TB[0], DB[1]), (TB[1], DB[0]), (up(TB[1]), ok_act[1]), (dn(TB[0]), ok_act[1]),
              (ok_act[0], up(DB[1])), (ok_act[0], dn(DB[0])), (f32_at_most(DB[1]), f32_at_least(DB[0])), (2.0, 0.3)):
        add(inside(), a)
    add(p_bad, (2.0, -0.1))
    if cfg5_quirk:
        # TableTennis4D with ProMP: action[0] / action[1] are the first two WEIGHTS, the reference still holds them to the tau / delay
        # bounds (table_tennis_env.py:305-306)
        for a in ((0.3, -0.2), (0.7, 0.1), (1.2, 0.06), (-0.4, 0.9)):
            add(inside(), a)
            add(p_bad, a)
    return rows


def build():
    run = reference_functions()
    K = utils_constants()
    global TB, DB
    TB, DB = K["tau_bound"], K["delay_bound"]
    low, high = K["jnt_pos_low"], K["jnt_pos_high"]
    cases = []                                  # (name, lo, hi, T, cfg5 quirk)
    for T in (1, 15, 16, 17, 350):
        cases.append((f"tt7_T{T}", low, high, T, T == 350))
    for D, T, s in ((1, 16, 0.37), (3, 17, 1.3), (16, 15, 0.71), (17, 33, 1.0), (3, 1, 2.0)):
        cases.append((f"scaled{D}_T{T}", np.resize(low, D) * s, np.resize(high, D) * s, T, False))
    lo, hi = low.copy(), high.copy(); lo[2] = np.nan
    cases.append(("nan_lo_T17", lo, hi, 17, False))
    lo, hi = low.copy(), high.copy(); hi[5] = np.nan
    cases.append(("nan_hi_T16", lo, hi, 16, False))
    lo, hi = low.copy(), high.copy(); lo[1], hi[1] = 0.5, -0.5
    cases.append(("lo_gt_hi_T15", lo, hi, 15, False))
    lo, hi = low.copy(), high.copy(); lo[0], hi[0], hi[4] = -1e39, 1e39, 1e39
    cases.append(("huge_T17", lo, hi, 17, False))
    out = {}
    for k, (name, lo, hi, T, quirk) in enumerate(cases):
        rng = np.random.default_rng(9000 + k)
        D = lo.shape[0]
        rows = rows_for(lo, hi, T, D, rng, quirk)
        if name.startswith("huge"):
            p = rows[0][0].copy(); p[0, 0] = np.finfo(F32).max; p[1, 4] = -np.finfo(F32).max; rows.append((p, rows[0][1]))
        pos = np.stack([r[0] for r in rows]); act = np.stack([r[1] for r in rows])
        valid, pen = np.empty(len(rows), bool), np.empty(len(rows))
        with np.errstate(invalid="ignore"):
            for b in range(len(rows)):
                # the reference sees float64 positions (np.float32 trajectories compared with float64 limits promote) and the raw action
                valid[b], pen[b] = run(lo, hi, act[b].astype(np.float64), pos[b].astype(np.float64))
        out.update({f"{name}_pos": pos, f"{name}_action": act, f"{name}_lo": lo, f"{name}_hi": hi, f"{name}_tb": TB, f"{name}_db": DB,
                    f"{name}_valid": valid, f"{name}_penalty": pen})
    out["cases"] = np.array([c[0] for c in cases])
    meta = ("generated by tests/golden/make_ref_validity_golden.py from /root/reference table_tennis_env.py (check_traj_validity and "
            "_get_traj_invalid_penalty compiled alone with ast) and table_tennis_utils.py (literal_eval); "
            f"numpy {np.__version__}; generator sha256 "
            + hashlib.sha256(open(os.path.abspath(__file__), "rb").read()).hexdigest() + "; "
            + "; ".join(f"{f} sha256 {h}" for f, h in sorted(_read.items())))
    out["meta"] = np.array(meta)
    return out


def main():
    out = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "committed fixture has other arrays"
        for k, v in out.items():
            if k == "meta":
                continue
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        assert str(old["meta"]) == str(out["meta"]), "meta differs (generator or reference file changed)"
        print("ref_validity.npz matches the reference")
        return
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
