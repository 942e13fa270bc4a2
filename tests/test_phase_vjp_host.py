"""
The surface of mpk_trajectory_phase_vjp and its reference (CPU; the device side: tests/test_gpu_phase_vjp.py): the entry point in the
header, the ctypes table and the built library; the torch restatement of tests/phase_vjp_ref.py against the float64 oracle on every
configuration the device tests use; the exact zeros its autograd gives (ProDMP's delay, clipped tau rows).  Every comparison prints its
maximum before it asserts.
"""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import mp_oracle as O

from . import phase_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_configs():
    """name -> (pc, bc, tc, dt, duration, init_time of B episodes or 0.0): every configuration of tests/test_gpu_phase_vjp.py"""
    from tests.test_gpu_learned_phase import CONFIGS, CONFIGS_ALL
    out = {}
    for name in CONFIGS:
        out[name] = CONFIGS[name][:5] + (("cycle" if name == "tt_prodmp_replan" else 0.0),)
    out["cfg4_per_episode_init_time"] = CONFIGS_ALL["cfg4_prodmp_replan"][:5] + ("cycle",)
    for name, cfg in R.EXTRA.items():
        out[name] = cfg + (0.0,)
    for kind in ("promp", "prodmp"):
        for D in (1, 3, 7):
            for T in (2, 3, 5, 63, 64, 65):
                out[f"{kind}_d{D}_t{T}"] = R.grid_config(kind, D, T) + (0.0,)
    return out


def init_time_of(spec, B):
    return np.array([0.0, 0.4, 0.8], np.float32)[np.arange(B) % 3] if isinstance(spec, str) else spec


def test_surface():
    from fancy_gym_amd import BatchedBlackBox, TrajectoryEngine, _lib, make_batched
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    proto = ("int mpk_trajectory_phase_vjp(mpk_handle h, const float* params, const float* init_pos, const float* init_vel, "
             "const float* init_time, double init_time_shared, const float* g_pos, const float* g_vel, float* g_params, "
             "float* g_init_pos, float* g_init_vel, int32_t B, void* stream);")
    assert proto in header
    # appended last, behind mpk_hole_reacher_rollout_vjp; the ABI stays 4
    protos = re.findall(r"\bint (mpk_\w+)\(", raw)
    assert protos[-2:] == ["mpk_hole_reacher_rollout_vjp", "mpk_trajectory_phase_vjp"]
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4
    for word in ("held indices", "torch.clamp", "g_delay = 0.0 exactly"):
        assert word in header, word
    assert list(_lib.SIGNATURES)[-1] == "mpk_trajectory_phase_vjp"
    res, args = _lib.SIGNATURES["mpk_trajectory_phase_vjp"]
    assert len(args) == 13
    # the unit is built, hashed and amalgamated
    unit = os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_phase_vjp.hip")
    assert "mpk_phase_vjp.hip" in _lib.KERNEL_UNITS and os.path.exists(unit) and unit in _lib.SOURCE_FILES
    with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_kernels.hip")) as f:
        assert '#include "mpk_phase_vjp.hip"' in f.read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_trajectory_phase_vjp$", syms, re.M)
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4
    assert lib.mpk_trajectory_phase_vjp(None, None, None, None, None, 0.0, None, None, None, None, None, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    # python: opt-in everywhere
    p = inspect.signature(TrajectoryEngine.trajectory).parameters
    assert p["phase_gradient"].default is None
    p = inspect.signature(TrajectoryEngine.trajectory_phase_vjp).parameters
    assert list(p)[:7] == ["self", "params", "init_pos", "init_vel", "g_pos", "g_vel", "init_time"] and p["init_time"].default == 0.0
    assert p["need"].kind is p["need"].KEYWORD_ONLY and p["need"].default == (True, True, True) and p["out"].default is None
    assert inspect.signature(BatchedBlackBox.__init__).parameters["phase_gradient"].default is None
    assert inspect.signature(make_batched).parameters["phase_gradient"].default is None


@pytest.mark.parametrize("name", list(all_configs()))
def test_the_float64_restatement_equals_the_float64_oracle(name):
    pc, bc, tc, dt, dur, it_spec = all_configs()[name]
    B = 5
    it = init_time_of(it_spec, B)
    params, ip, iv, _ = R.make_inputs(pc, bc, tc, dt, dur, B, it, seed=3)
    ref_pos, ref_vel = O.get_trajectory(pc, bc, tc, params, dur, dt, it, ip, iv, dtype=np.float64)
    with torch.no_grad():
        pos, vel = R.trajectory(pc, bc, tc, *(torch.from_numpy(a.astype(np.float64)) for a in (params, ip, iv)), it, dt, dur)
    for what, got, ref in (("pos", pos.numpy(), ref_pos), ("vel", vel.numpy(), ref_vel)):
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
        print(f"{name} {what}: max |restatement - oracle| / max|oracle| = {err:.3e}")
        assert err <= 1e-12, (name, what, err)
    # the float32 restatement follows the float32 oracle as two float32 formulations do
    with torch.no_grad():
        pos32, _ = R.trajectory(pc, bc, tc, *(torch.from_numpy(a) for a in (params, ip, iv)), it, dt, dur, dtype=torch.float32)
    err32 = np.abs(pos32.numpy() - ref_pos).max() / np.abs(ref_pos).max()
    print(f"{name} pos float32: {err32:.3e}")
    assert pos32.dtype == torch.float32 and err32 <= 1e-4


@pytest.mark.parametrize("name", ["tt_prodmp", "tt_prodmp_replan", "prodmp_3dof_learn_tau", "prodmp_after_scale_no_weights", "prodmp_d3_t5",
                                  "beerpong_promp", "promp_5dof_learn_both", "promp_exp_learn_both", "promp_d3_t5"])
def test_exact_zeros_of_the_reference_gradient(name):
    """ProDMP: the delay reaches the trajectory through integer indices only -- autograd gives exactly 0; both families: rows whose tau was
    clipped (row 0 above tau_hi, row 1 below tau_lo) get exactly 0 in g_tau, rows inside do not"""
    pc, bc, tc, dt, dur, it_spec = all_configs()[name]
    B = 6
    it = init_time_of(it_spec, B)
    params, ip, iv, _ = R.make_inputs(pc, bc, tc, dt, dur, B, it, seed=5)
    lo, hi = pc.tau_bound
    assert params[0, 0] > hi and params[1, 0] < lo and ((params[2:, 0] > lo) & (params[2:, 0] < hi)).all()
    rng = np.random.default_rng(11)
    T = O.num_steps(dur, dt)
    g_pos, g_vel = (rng.standard_normal((B, T, tc.action_dim)).astype(np.float32) for _ in range(2))
    gp, gip, giv = R.vjp(pc, bc, tc, params, ip, iv, it, dt, dur, g_pos, g_vel)
    assert (gp[:2, 0] == 0.0).all() and (gp[2:, 0] != 0.0).any()
    if tc.trajectory_generator_type == "prodmp" and pc.learn_delay:
        assert (gp[:, 1] == 0.0).all()
    if tc.trajectory_generator_type == "promp":
        assert (giv == 0.0).all()
        if pc.learn_delay:
            assert (gp[:, 1] != 0.0).any()
        if bc.basis_generator_type != "zero_rbf":
            assert (gip == 0.0).all()
