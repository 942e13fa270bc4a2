"""
The closed-form trajectory fit without a GPU: the NumPy reference of tests/trajectory_fit_ref.py is a fit, the public surface exists, and
fit_trajectory / learn_mp_params_from_trajs refuse bad arguments before anything touches a device.
"""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fancy_gym_amd import BatchedBlackBox, TrajectoryEngine, _lib
from fancy_gym_amd.black_box.factory import get_basis_generator, get_phase_generator, get_trajectory_generator
from oracle import mp_oracle as O
from tests import trajectory_fit_ref as R
from tests.test_gpu_trajectory import CFG1, CFG2, CFG3, CFG4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cfg1": CFG1 + (0.0,), "cfg2": CFG2 + (0.0,), "cfg3": CFG3 + (0.0,), "cfg4": CFG4 + (0.5,)}
REG = 1e-9


def design(name):
    pc, bc, tc, dt, duration, it = CASES[name]
    return R.Design(pc, bc, tc, dt, duration, it)


# ---- 1. the helper is a fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_reference_is_the_regularised_least_squares_fit(name):
    ds = design(name)
    y, ip, iv, _ = R.demonstrations(ds, 4, 3)
    c = ds.offset(ip, iv)
    p = R.fit64(ds, y, c, REG)
    r = y.astype(np.float64) - c
    for d in range(ds.D):
        Psi = ds.Psi[d]
        # the gradient of the objective vanishes: Psi^T (Psi p - r) + reg p = 0, to 1e-9 of |Psi^T r|
        grad = (Psi.T @ (Psi @ p[:, d].T - r[:, :, d].T)) + REG * p[:, d].T
        scale = np.linalg.norm(Psi.T @ r[:, :, d].T, axis=0)
        assert (np.linalg.norm(grad, axis=0) <= 1e-9 * scale).all(), (name, d)
        # ... and p is numpy's least-squares solution of the augmented system [Psi; sqrt(reg) I] p = [r; 0]
        aug = np.vstack([Psi, np.sqrt(REG) * np.eye(ds.Kloc)])
        rhs = np.vstack([r[:, :, d].T, np.zeros((ds.Kloc, r.shape[0]))])
        q = np.linalg.lstsq(aug, rhs, rcond=None)[0].T
        rec = Psi @ p[:, d].T
        assert np.abs(Psi @ q.T - rec).max() <= 1e-9 * np.abs(r).max(), (name, d)
    # the float32 fit is a float32 fit
    assert R.fit32(ds, y, c, REG).dtype == np.float32


@pytest.mark.parametrize("name", ["cfg1", "cfg4"])
def test_exact_demonstrations_give_their_parameters_back(name):
    """y = Psi p0 + c exactly (float64): the fit returns (G + reg I)^-1 G p0, which misses p0 by at most reg / (lambda_min + reg) |p0|
    per DoF (the regulariser's own bias) plus the solve's rounding, cond(G) eps |p0|.  (cfg1's smallest Gram eigenvalue is 3.6; cfg4's,
    at init_time 0.5, is 5e-8, so its bias in the weakest direction is 2 % -- the bound says so, the reconstruction does not notice)"""
    ds = design(name)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((3, ds.D, ds.Kloc))
    ip, iv = rng.uniform(-1, 1, (3, ds.D)), rng.uniform(-1, 1, (3, ds.D))
    c = ds.offset(ip, iv)
    y = ds.reconstruct(p0) + c
    assert np.abs(ds.forward(ds.pack(p0), ip, iv) - y).max() <= 1e-12 * np.abs(y).max()     # the map is affine
    p = R.fit64(ds, y, c, REG)
    for d in range(ds.D):
        ev = np.linalg.eigvalsh(ds.Psi[d].T @ ds.Psi[d])
        bound = (REG / (ev[0] + REG) + 100 * ev[-1] / ev[0] * np.finfo(np.float64).eps) * np.linalg.norm(p0[:, d], axis=1)
        assert (np.linalg.norm(p[:, d] - p0[:, d], axis=1) <= bound).all(), (name, d, ev[0])
    # the reconstruction: direction i of G misses by sqrt(lambda_i) reg / (lambda_i + reg) <= sqrt(reg) / 2 of its coefficient
    miss = np.linalg.norm(ds.reconstruct(p) - ds.reconstruct(p0), axis=1)               # [B, D], 2-norm over time
    assert (miss <= (0.5 * np.sqrt(REG) + 1e-12) * np.linalg.norm(p0, axis=2)).all(), name


# ---- 2. the surface ---------------------------------------------------------------------------------------------------------------------
def test_surface():
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    for proto in ("int mpk_trajectory_fit(mpk_handle h, const float* pos, const float* init_pos, const float* init_vel, const float* init_time, "
                  "double init_time_shared, double reg, float* params, int32_t B, void* stream);",
                  "int mpk_trajectory_phase_fit(mpk_handle h, const float* pos, const float* phase_params, const float* init_pos, "
                  "const float* init_vel, const float* init_time, double init_time_shared, double reg, float* params, int32_t B, "
                  "void* stream);",
                  "int mpk_fit_status(mpk_handle h, int32_t* not_positive_definite, void* stream);"):
        assert proto in header, proto
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4
    for word in ("learn_mp_params_from_trajs", "argmin_p", "reg I", "unpinned"):
        assert word in header, word
    assert len(_lib.SIGNATURES["mpk_trajectory_fit"][1]) == 10 and len(_lib.SIGNATURES["mpk_trajectory_phase_fit"][1]) == 11
    unit = os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_traj_fit.hip")
    assert "mpk_traj_fit.hip" in _lib.KERNEL_UNITS and unit in _lib.SOURCE_FILES and "mpk_run_stage.h" in _lib.KERNEL_HEADERS
    with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_kernels.hip")) as f:
        assert '#include "mpk_traj_fit.hip"' in f.read()
    # one staging routine, included by both kernels
    for u in ("mpk_traj_vjp.hip", "mpk_traj_fit.hip"):
        with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", u)) as f:
            text = f.read()
        assert '#include "mpk_run_stage.h"' in text and "stage_run(" in text, u
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mpk_trajectory_fit", "mpk_trajectory_phase_fit", "mpk_fit_status"):
        assert re.search(rf" T {name}$", syms, re.M), name
    lib = _lib.load()
    assert lib.mpk_trajectory_fit(None, None, None, None, None, 0.0, 1e-9, None, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    assert lib.mpk_trajectory_phase_fit(None, None, None, None, None, None, 0.0, 1e-9, None, 1, None) == _lib.MPK_EINVAL
    p = inspect.signature(TrajectoryEngine.fit_trajectory).parameters
    assert list(p) == ["self", "pos", "init_pos", "init_vel", "init_time", "reg", "phase_params", "out"]
    assert p["init_pos"].default is None and p["init_time"].default == 0.0 and p["reg"].default == 1e-9
    assert p["reg"].kind is p["reg"].KEYWORD_ONLY and p["phase_params"].default is None and p["out"].default is None
    p = inspect.signature(BatchedBlackBox.fit_trajectory).parameters
    assert list(p) == ["self", "pos", "phase_params", "reg"] and p["reg"].default == 1e-9


# ---- 3. refusals that need no device ------------------------------------------------------------------------------------------------------
class StubEngine(TrajectoryEngine):
    """the attributes fit_trajectory's checks read, and no handle: a call that got past the checks would fail on the NULL handle"""

    def __init__(self, mp_type, D, T, P, learn_tau=False, learn_delay=False):
        self.config = _lib.mpk_config()
        self.config.learn_tau, self.config.learn_delay = int(learn_tau), int(learn_delay)
        self.mp_type, self.num_dof, self.num_params, self._T = mp_type, D, P, T
        self.device = torch.device("cuda", 0)

    num_steps = property(lambda self: self._T)

    def close(self):
        pass


def test_fit_trajectory_refuses_before_any_device_work():
    eng = StubEngine("prodmp", 7, 100, 42)
    y, z = np.zeros((3, 100, 7), np.float32), np.zeros((3, 7), np.float32)
    for reg in (0.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reg must be a positive finite number"):
            eng.fit_trajectory(y, z, z, reg=reg)
    for bad in (np.zeros((3, 99, 7)), np.zeros((3, 100, 6)), np.zeros((100, 7))):
        with pytest.raises(ValueError, match=r"pos must be \[B, 100, 7\]"):
            eng.fit_trajectory(bad, z, z)
    with pytest.raises(ValueError, match=r"init_vel must be \[3, 7\]"):
        eng.fit_trajectory(y, z, np.zeros((2, 7)))
    with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
        eng.fit_trajectory(y, None, None)
    with pytest.raises(ValueError, match="phase_params given, but this handle has a shared phase"):
        eng.fit_trajectory(y, z, z, phase_params=np.ones((3, 1)))
    with pytest.raises(ValueError, match=r"out must be a contiguous float32 tensor of shape \(3, 42\)"):
        eng.fit_trajectory(y, z, z, out=torch.zeros((3, 41)))
    learned = StubEngine("prodmp", 7, 100, 44, learn_tau=True, learn_delay=True)
    with pytest.raises(ValueError, match=r"learns tau and delay: pass each episode's values as phase_params \[3, 2\]"):
        learned.fit_trajectory(y, z, z)
    with pytest.raises(ValueError, match=r"phase_params must be \[3, 2\]"):
        learned.fit_trajectory(y, z, z, phase_params=np.ones((3, 1)))
    with pytest.raises(NotImplementedError, match="DMP with a per-episode phase"):
        StubEngine("dmp", 7, 100, 43, learn_tau=True).fit_trajectory(y, z, z, phase_params=np.ones((3, 1)))


def make_mp(mp="prodmp", D=3, learn_tau=False):
    pg = get_phase_generator("exp", tau=1.0, alpha_phase=3.0, learn_tau=learn_tau)
    bg = get_basis_generator("prodmp" if mp == "prodmp" else "rbf", pg, num_basis=4)
    gen = get_trajectory_generator(mp, D, bg)
    gen.set_duration(1.0, 0.02)
    return gen


def test_learn_mp_params_from_trajs_refuses_before_any_device_work():
    gen = make_mp()
    assert inspect.signature(gen.learn_mp_params_from_trajs).parameters["reg"].default == 1e-9
    grid = O.make_times(1.0, 0.02, 0.0)
    T = grid.shape[0]
    trajs = np.zeros((2, T, 3), np.float32)
    times = np.broadcast_to(grid, (2, T))
    given = dict(init_time=0.0, init_pos=np.zeros((2, 3)), init_vel=np.zeros((2, 3)))
    for reg in (0.0, -1.0):
        with pytest.raises(ValueError, match="reg must be a positive finite number"):
            gen.learn_mp_params_from_trajs(times, trajs, reg=reg, **given)
    with pytest.raises(ValueError, match=r"trajs must be \[..., T, 3\]"):
        gen.learn_mp_params_from_trajs(times, np.zeros((2, T, 4), np.float32), **given)
    with pytest.raises(ValueError, match=r"trajs must be \[..., T, 3\]"):
        gen.learn_mp_params_from_trajs(times[:, :-1], trajs, **given)
    with pytest.raises(ValueError, match="time grid has 50 steps.*needs 50 samples, got 49"):
        gen.learn_mp_params_from_trajs(times[:, :-1], trajs[:, :-1], **given)
    with pytest.raises(ValueError, match="first sample is the initial condition and trajs needs 51 samples, got 50"):
        gen.learn_mp_params_from_trajs(times, trajs)
    with pytest.raises(ValueError, match="one init_time is shared by the batch"):
        gen.learn_mp_params_from_trajs(times, trajs, init_time=np.array([0.0, 0.1]), init_pos=np.zeros((2, 3)), init_vel=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="not the handle's own grid"):      # a foreign grid: twice the spacing
        gen.learn_mp_params_from_trajs(2.0 * times, trajs, **given)
    with pytest.raises(ValueError, match="not the handle's own grid"):      # ... or shifted against the given init_time
        gen.learn_mp_params_from_trajs(times + 0.1, trajs, **given)
    with pytest.raises(ValueError, match="learns tau / delay"):
        make_mp(learn_tau=True).learn_mp_params_from_trajs(times, trajs, **given)
    fresh = get_trajectory_generator("prodmp", 3, get_basis_generator("prodmp", get_phase_generator("exp"), num_basis=4))
    with pytest.raises(RuntimeError, match="set_duration"):
        fresh.learn_mp_params_from_trajs(times, trajs, **given)
