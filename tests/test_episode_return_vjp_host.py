"""mpk_episode_return_vjp without a GPU: the composed float64 reference of tests/episode_vjp_ref.py (reacher_vjp_ref's rollout gradient
contracted with the oracle's explicit trajectory Jacobian) agrees with torch autograd of the whole float64 chain -- plan, rollout,
reward, aggregation -- for all three aggregations; the inputs of the GPU suite meet the conditions it relies on; and the entry point, its
unit and the Python surface exist."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from fancy_gym_amd import _lib

from . import episode_vjp_ref as E
from . import reacher_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fancy_gym_amd", "csrc")
# delta_ref: the disagreement of the composed reference and the whole-chain autograd, relative to each array's maximum.  Both are float64
# sums of a few hundred terms of one sign pattern; the largest value measured over every case and aggregation is printed by the test and
# is below 1e-14.  The GPU bounds -- 1e-12 for the float64 outputs, 1e-5 for the float32 ones -- sit two and nine orders above.
DELTA_REF = 1e-14


@pytest.mark.parametrize("agg", E.AGGS)
@pytest.mark.parametrize("name", list(E.CASES))
def test_composed_reference_equals_autograd_of_the_whole_chain(name, agg):
    c = E.make_case(name)
    dp, dv = E.oracle_plan32(c)
    ref, e32 = E.composed(c, dp, dv, agg)
    whole = E.whole_chain_autograd(c, dp, dv, agg)
    worst = 0.0
    for k in E.X_OUTPUTS + E.S_OUTPUTS:
        scale = np.abs(whole[k]).max()
        if scale == 0.0:                # (promp: init_vel is read by no column; position / velocity: one of the two plan gradients)
            assert not ref[k].any(), k
            continue
        delta = np.abs(ref[k] - whole[k]).max() / scale
        worst = max(worst, delta)
        print(f"{name} {agg} {k}: delta_ref = {delta:.2e}")
        assert delta <= DELTA_REF, (k, delta)
    # the GPU bounds sit well above delta_ref
    assert worst <= 1e-12 / 50
    # an episode that executes nothing: zero parameter gradients, g_q / g_qd passed through
    idle = c["n_steps"] == 0
    for k in E.X_OUTPUTS:
        assert not ref[k][idle].any()
    assert np.array_equal(ref["g_q0"][idle], c["g_q"][idle]) and np.array_equal(ref["g_qd0"][idle], c["g_qd"][idle])
    assert ref["g_params"].any()


@pytest.mark.parametrize("use", [(False, True, True), (True, False, False)])
def test_composed_reference_with_absent_upstream_gradients(use):
    c = E.make_case("prodmp_motor_d5_t17_b11_clipped")
    dp, dv = E.oracle_plan32(c)
    ref, _ = E.composed(c, dp, dv, "mean", use)
    whole = E.whole_chain_autograd(c, dp, dv, "mean", use)
    for k in E.X_OUTPUTS + E.S_OUTPUTS:
        scale = np.abs(whole[k]).max()
        assert np.abs(ref[k] - whole[k]).max() <= DELTA_REF * scale, k


@pytest.mark.parametrize("name", list(E.CASES))
def test_input_conditions_on_the_oracle_plan(name):
    """what the GPU suite asserts again on the device's plan: no controller output within 1e-9 of a clip bound, paid distances above
    1e-3, saturated steps in the clipped cases and none in the others, paid steps in two tiles"""
    c = E.make_case(name)
    dp, dv = E.oracle_plan32(c)
    cond = R.conditions(E.rollout_case(c, dp, dv, "sum"))
    print(f"{name}: {cond}")
    assert cond["bound_gap"] >= 1e-9 and cond["n_paid"] > 0 and cond["min_dist"] > 1e-3
    clipped = E.CASES[name][5]
    assert (cond["saturated"] > 0.0) == clipped
    t = np.arange(c["T"])[None]
    paid = (t < c["n_steps"][:, None]) & (c["step0"][:, None] + t >= c["sbr"])
    assert paid[:, :16].any() and paid[:, 16:].any()
    assert c["n_steps"].max() == c["T"] and (c["B"] == 1 or c["n_steps"].min() == 0)


def test_cases_cover_what_the_kernel_branches_on():
    shapes = list(E.CASES.values())
    assert {s[0] for s in shapes} == {"prodmp", "promp", "dmp"} and {s[1] for s in shapes} == {"motor", "position", "velocity"}
    assert {s[2] for s in shapes} == {2, 3, 5, 7} and {s[3] for s in shapes} == {17, 33}
    for mp, _, D, _, B, _ in shapes:
        assert B in (1, 64 // D - 1, 64 // D + 1), (D, B)
    for mp in ("prodmp", "promp", "dmp"):
        assert {B == 1 for m, _, D, _, B, _ in shapes if m == mp} >= {False}
    assert {s[5] for s in shapes} == {True, False}


# ---- fails without the feature -------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mpk.h")).read()
    m = re.search(r"int mpk_episode_return_vjp\(([^;]*)\);", hdr)
    assert m, "include/mpk.h does not declare mpk_episode_return_vjp"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["h", "params", "init_pos", "init_vel", "init_time_shared", "rc", "q0", "qd0", "n_steps", "step0", "goal",
                    "steps_before_reward", "agg", "g_ret", "g_q", "g_qd", "g_params", "g_init_pos", "g_init_vel", "g_q0", "g_qd0", "g_goal",
                    "q_end", "qd_end", "B", "stream"]
    res, argtypes = _lib.SIGNATURES["mpk_episode_return_vjp"]
    assert res is C.c_int and len(argtypes) == len(args) == 26
    assert argtypes[4] is C.c_double and argtypes[11] is C.c_int32 and argtypes[12] is C.c_int32 and argtypes[24] is C.c_int32
    # appended behind every earlier prototype; the version does not move
    assert hdr.rindex("int mpk_episode_return_vjp(") > hdr.rindex("int mpk_reacher_rollout_vjp(")
    assert re.search(r"#define\s+MPK_ABI_VERSION\s+4\b", hdr) and _lib.MPK_ABI_VERSION == 4
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4 and hasattr(lib, "mpk_episode_return_vjp")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_episode_return_vjp$", out, re.M), "libmpk.so does not export mpk_episode_return_vjp"
    doc = hdr[hdr.rindex("/*", 0, hdr.rindex("int mpk_episode_return_vjp(")):]
    for phrase in ("mpk_trajectory", "mpk_reacher_rollout_vjp", "mpk_trajectory_vjp", "MPK_AGG_MEAN", "q_end", "MPK_ENOTIMPL"):
        assert phrase in doc, phrase


def test_unit_is_built_hashed_and_amalgamated():
    hashed = {os.path.basename(p) for p in _lib.SOURCE_FILES}
    assert "mpk_episode_vjp.hip" in _lib.KERNEL_UNITS and "mpk_episode_vjp.hip" in hashed
    assert "mpk_vjp_row.h" in _lib.KERNEL_HEADERS and "mpk_vjp_row.h" in hashed
    assert '#include "mpk_episode_vjp.hip"' in open(os.path.join(CSRC, "mpk_kernels.hip")).read()
    # one definition of the transpose's rows, included by both units
    for unit in ("mpk_traj_vjp.hip", "mpk_episode_vjp.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert '#include "mpk_vjp_row.h"' in text and "float vjp_row(" not in text, unit
    assert _lib.embedded_source_hash() == _lib.source_hash()


def test_null_handle_is_refused():
    lib = _lib.load()
    assert lib.mpk_episode_return_vjp(None, None, None, None, 0.0, *([None] * 6), 0, 0, *([None] * 11), 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()


def test_python_surface_exists():
    from fancy_gym_amd import RolloutSpec, TrajectoryEngine
    from fancy_gym_amd.batched import BatchedBlackBox
    import torch
    sig = inspect.signature(TrajectoryEngine.episode_return_vjp).parameters
    assert list(sig)[1:9] == ["params", "init_pos", "init_vel", "spec", "q0", "qd0", "goal", "g_ret"]
    for k in ("g_q", "g_qd", "n_steps", "step0", "steps_before_reward", "aggregation", "init_time", "need", "out"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["steps_before_reward"].default == 199 and len(sig["need"].default) == 8
    assert inspect.signature(TrajectoryEngine.episode_return).parameters["differentiable"].default is False
    assert inspect.signature(BatchedBlackBox._step_lean).parameters["differentiable"].default is False
    z = torch.zeros((1, 4))
    s = torch.zeros((1, 2), dtype=torch.float64)
    for spec in (RolloutSpec("metaworld", 2, plant="static"), RolloutSpec("motor", 2, plant="static")):
        with pytest.raises(NotImplementedError, match="double integrator"):
            TrajectoryEngine.episode_return_vjp(None, z, z, z, spec, s, s, s, None)
