"""mpk_reacher_rollout_vjp without a GPU: the two float64 references of tests/reacher_vjp_ref.py agree with the oracle and with each
other, the inputs of the GPU suite meet the conditions it relies on, and the entry point, its unit, the opt-in of
``BatchedBlackBox.step`` and the refusals that need no device exist."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from fancy_gym_amd import _lib
from oracle import mp_oracle as O

from . import reacher_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fancy_gym_amd", "csrc")
SMALL = [n for n in R.CASES if R.CASES[n][0] <= R.SUBSET]
CTRL_CASES = R.CTRL_CASES
# delta_ref of the appended cases: the largest value measured over them is 1.3e-15 (b9_t32_d8 position, g_des_pos and g_qd0; every
# other one <= 6.4e-16); the bound is 4 x that, two orders below the GPU suite's 1e-12.  The original cases keep 1e-15.
DELTA_REF_APPENDED = 4 * 1.3e-15
assert DELTA_REF_APPENDED <= 1e-14


def small(name, controller="motor"):
    c = R.make_case(name, controller)
    return R.rows(c, np.arange(R.compared(c))) if R.compared(c) < c["B"] else c


@pytest.mark.parametrize("name,controller", CTRL_CASES)
def test_restatement_equals_the_oracle(name, controller):
    c = small(name, controller)
    rew, q, qd, _, _ = R.forward(c)
    _, rr, rq, rqd = O.reacher_rollout(c["des_pos"], c["des_vel"], controller, c["pg"], c["dg"], c["lo"], c["hi"], c["dt"], c["q0"],
                                       c["qd0"], c["goal"], n_steps=c["n_steps"], step0=c["step0"], steps_before_reward=c["sbr"])
    print(f"{name} {controller}: max |rewards - oracle| = {np.abs(rew - rr).max():.3e}")
    assert np.abs(rew - rr).max() <= 1e-14
    assert np.array_equal(q, rq) and np.array_equal(qd, rqd)


@pytest.mark.parametrize("name,controller", CTRL_CASES)
def test_autograd_and_the_numpy_sweep_agree(name, controller):
    """delta_ref, the disagreement of the two references relative to each array's maximum: the GPU suite's 1e-12 leaves three orders
    of magnitude above it"""
    c = small(name, controller)
    a, s = R.reference(name, controller), R.numpy_sweep(c)        # (the shared autograd result: the long cases take seconds)
    bound = 1e-15 if name in R.ORIGINAL else DELTA_REF_APPENDED
    for k in R.OUTPUTS:
        scale = np.abs(a[k]).max()
        if scale == 0.0:                # (position: g_des_vel, velocity: g_des_pos)
            assert not s[k].any(), k
            continue
        delta = np.abs(a[k] - s[k]).max() / scale
        print(f"{name} {controller} {k}: delta_ref = {delta:.2e}")
        assert delta <= bound, (k, delta)
    # rows behind the executed steps are exact zeros; an episode that executes nothing passes g_q, g_qd through
    dead = np.arange(c["T"])[None] >= c["n_steps"][:, None]
    assert not a["g_des_pos"][dead].any() and not a["g_des_vel"][dead].any()
    idle = c["n_steps"] == 0
    assert np.array_equal(a["g_q0"][idle], c["g_q"][idle]) and np.array_equal(a["g_qd0"][idle], c["g_qd"][idle])


def test_numpy_sweep_with_a_paid_step_at_the_goal():
    """include/mpk.h: a paid step with dist = 0 contributes no distance term.  The sweep is the reference of that case: finite, no
    gradient to the goal, the other outputs of the episode not trivially zero; the ordinary episode beside it still equals autograd
    (which divides by dist and is not defined for episode 0)"""
    c = R.at_the_goal()
    assert c["g_q"][0].all() and c["g_qd"][0].all() and c["g_r"][0].all()
    dist = R.forward(c)[4]
    assert not dist[0].any() and dist[1].min() > 1e-3           # exactly 0 at every step of episode 0
    s = R.numpy_sweep(c)
    assert all(np.isfinite(v).all() for v in s.values())
    assert not s["g_goal"][0].any() and s["g_goal"][1].all()
    assert s["g_des_pos"][0].all() and s["g_q0"][0].all() and s["g_qd0"][0].all() and not s["g_des_vel"].any()
    a = R.autograd(R.rows(c, np.array([1])))
    for k in R.OUTPUTS:
        scale = np.abs(a[k]).max()
        delta = np.abs(a[k] - s[k][1:]).max() / scale if scale > 0.0 else np.abs(s[k][1:]).max()
        print(f"at the goal, episode 1 {k}: delta_ref = {delta:.2e}")
        assert delta <= DELTA_REF_APPENDED, (k, delta)


@pytest.mark.parametrize("use", [(True, False, False), (False, True, True), (False, False, True)])
def test_references_agree_with_absent_upstream_gradients(use):
    c = small("b7_t33_d7_clipped")
    a, s = R.autograd(c, use), R.numpy_sweep(c, use)
    for k in R.OUTPUTS:
        scale = np.abs(a[k]).max()
        assert np.abs(a[k] - s[k]).max() <= 1e-15 * scale, k


@pytest.mark.parametrize("name,controller", CTRL_CASES)
def test_input_conditions(name, controller):
    """conditions of the GPU comparisons, met by the references alone: no controller output within 1e-9 of a clip bound (the
    derivative of clip is then the same for every implementation), the goal at least 1e-3 from the end effector wherever the
    distance is paid, a meaningful share of saturated steps in the clipped motor cases, no output that is all zeros"""
    c = R.make_case(name, controller)
    cond = R.conditions(c)
    print(f"{name} {controller}: {cond}")
    assert cond["bound_gap"] >= 1e-9
    assert cond["n_paid"] > 0 and cond["min_dist"] > 1e-3
    if name in R.CLIPPED and controller == "motor":
        assert 0.02 <= cond["saturated"] <= 0.50
    elif name not in R.CLIPPED:
        assert cond["saturated"] == 0.0
    ref = R.reference(name, controller)
    zero_by_construction = {"position": "g_des_vel", "velocity": "g_des_pos"}.get(controller)
    for k in R.OUTPUTS:
        if k == zero_by_construction:
            continue
        assert ref[k].any(), k
    lens = set(R.make_case(name)["n_steps"].tolist())
    T = c["T"]
    if c["B"] >= 6:
        assert {T, T - 1, 17, 16, 1, 0} <= lens
    assert len(set(c["step0"].tolist())) > 1


def test_every_length_of_the_recipe_occurs_in_the_small_cases():
    seen = set()
    for name in SMALL:
        c = R.make_case(name)
        seen |= {int(n) if n in (17, 16, 1, 0) else ("T" if n == c["T"] else "T-1") for n in c["n_steps"]}
    assert seen == {"T", "T-1", 17, 16, 1, 0}


# ---- fails without the feature -------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mpk.h")).read()
    m = re.search(r"int mpk_reacher_rollout_vjp\(([^;]*)\);", hdr)
    assert m, "include/mpk.h does not declare mpk_reacher_rollout_vjp"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["h", "rc", "des_pos", "des_vel", "q0", "qd0", "n_steps", "step0", "goal", "steps_before_reward", "g_rewards", "g_q",
                    "g_qd", "g_des_pos", "g_des_vel", "g_q0", "g_qd0", "g_goal", "B", "T", "stream"]
    res, argtypes = _lib.SIGNATURES["mpk_reacher_rollout_vjp"]
    assert res is C.c_int and len(argtypes) == len(args) == 21
    assert argtypes[9] is C.c_int32 and argtypes[18] is C.c_int32 and argtypes[19] is C.c_int32
    # appended behind every earlier prototype; the version does not move
    assert hdr.rindex("int mpk_reacher_rollout_vjp(") > hdr.rindex("int mpk_trajectory_vjp(")
    assert re.search(r"#define\s+MPK_ABI_VERSION\s+4\b", hdr) and _lib.MPK_ABI_VERSION == 4
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4 and hasattr(lib, "mpk_reacher_rollout_vjp")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_reacher_rollout_vjp$", out, re.M), "libmpk.so does not export mpk_reacher_rollout_vjp"
    # the header carries the formulas and cites the forward it transposes
    doc = hdr[hdr.rindex("/*", 0, hdr.rindex("int mpk_reacher_rollout_vjp(")):]
    for phrase in ("mpk_reacher_rollout", "lqd += dt lq", "la = dt lqd - 2 a g_r", "torch.clamp", "MPK_ENOTIMPL"):
        assert phrase in doc, phrase


def test_unit_is_built_hashed_and_amalgamated():
    assert "mpk_rollout_vjp.hip" in _lib.KERNEL_UNITS
    assert "mpk_rollout_vjp.hip" in {os.path.basename(p) for p in _lib.SOURCE_FILES}
    assert '#include "mpk_rollout_vjp.hip"' in open(os.path.join(CSRC, "mpk_kernels.hip")).read()
    assert _lib.embedded_source_hash() == _lib.source_hash()


def test_null_handle_is_refused():
    lib = _lib.load()
    assert lib.mpk_reacher_rollout_vjp(*([None] * 9), 0, *([None] * 8), 1, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()


def test_step_accepts_differentiable_and_python_surface_exists():
    from fancy_gym_amd import TrajectoryEngine
    from fancy_gym_amd.batched import BatchedBlackBox
    p = inspect.signature(BatchedBlackBox.step).parameters
    assert list(p)[1:] == ["params", "fuse", "differentiable"] and p["differentiable"].default is False and p["fuse"].default is True
    sig = inspect.signature(TrajectoryEngine.reacher_rollout_vjp).parameters
    assert list(sig)[1:8] == ["spec", "des_pos", "des_vel", "q0", "qd0", "goal", "g_rewards"]
    for k in ("g_q", "g_qd", "n_steps", "step0", "steps_before_reward", "need"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["steps_before_reward"].default == 199


def _bb(**kw):
    """the attributes ``_refuse_differentiable`` reads, without an engine (it decides on the host)"""
    base = dict(reward="simple_reacher", pos_limits=None, _n_phase=0, do_replanning=False, _lockstep=0)
    return types.SimpleNamespace(**{**base, **kw})


def test_refusals_decided_on_the_host():
    import torch

    from fancy_gym_amd import RolloutSpec, TrajectoryEngine
    from fancy_gym_amd.batched import BatchedBlackBox
    refuse = BatchedBlackBox._refuse_differentiable
    refuse(_bb())
    refuse(_bb(do_replanning=True, _lockstep=25))
    for kw, word in ((dict(reward="hole_reacher"), "simple_reacher"), (dict(reward=None), "simple_reacher"),
                     (dict(pos_limits=([0.0], [1.0])), "pos_limits"), (dict(_n_phase=1), "learned tau"),
                     (dict(do_replanning=True, _lockstep=None), "init_time")):
        with pytest.raises(NotImplementedError, match=word):
            refuse(_bb(**kw))
    z = torch.zeros((1, 4, 2))
    s = torch.zeros((1, 2), dtype=torch.float64)
    for spec in (RolloutSpec("metaworld", 2, plant="static"), RolloutSpec("motor", 2, plant="static"),
                 RolloutSpec("velocity", 2, plant="velocity_direct", dt=0.01)):
        with pytest.raises(NotImplementedError, match="double integrator"):
            TrajectoryEngine.reacher_rollout_vjp(None, spec, z, z, s, s, s, None)
