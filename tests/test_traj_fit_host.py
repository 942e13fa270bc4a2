"""
The closed-form trajectory fit without a GPU: the NumPy reference of tests/trajectory_fit_ref.py is a fit, the public surface exists, and
fit_trajectory / learn_mp_params_from_trajs refuse bad arguments before anything touches a device.  The per-episode-phase table
of tests/test_gpu_traj_fit.py: the instantiations of k_phase_fit it reaches, its CPU fits, and the kernel's Cholesky order emulated in
float64 for the rank-deficient batch.
"""
import dataclasses
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


# ---- 4. the per-episode-phase table (tests/test_gpu_traj_fit.py) without a device -----------------------------------------------------------
def test_the_phase_table_reaches_every_instantiation_and_slot_count():
    """k_phase_fit<MP, KQ> has five instantiations; a lane owns up to four entries of Psi^T (y - c), 64 a slot: the rows of the device
    table take the KQ the table states (phase_fit_limits' rule), cover all five, and fill two, three and four slots"""
    from tests import test_gpu_traj_fit as F
    cfgs = F.phase_configs()
    assert set(cfgs) == set(F.PHASE_KQ) and set(F.PHASE_TABLE) <= set(cfgs)
    pairs, sizes = set(), []
    for name in F.PHASE_TABLE:
        pc, bc, tc = cfgs[name][:3]
        kq = F.phase_fit_kq(bc, tc)
        assert kq == F.PHASE_KQ[name], (name, kq)
        n_rhs, P = tc.action_dim * 4 * kq, O.num_params(pc, bc, tc)
        assert tc.action_dim <= 16 and n_rhs <= 256 and P <= 320, (name, n_rhs, P)      # the launcher's limits
        pairs.add((tc.trajectory_generator_type, kq))
        sizes.append(n_rhs)
    for name in set(cfgs) - set(F.PHASE_TABLE):
        assert F.phase_fit_kq(*cfgs[name][1:3]) == F.PHASE_KQ[name] == 2, name           # the round-boundary grid
    assert pairs == {("promp", 1), ("promp", 2), ("promp", 4), ("prodmp", 2), ("prodmp", 4)}
    for lo, hi in ((64, 128), (128, 192), (192, 256)):
        assert any(lo < n <= hi for n in sizes), (lo, hi, sorted(sizes))
    assert 64 in sizes and 256 in sizes                                                  # a slot exactly full, all four full
    assert O.num_params(*cfgs["promp_16_basis_16_dof"][:3]) == 258
    # the two switch rows take the branches their names say
    assert cfgs["prodmp_4_basis_12_dof_goal_offset_add"][2].goal_offset_mode == "add"
    assert cfgs["tt_prodmp_replan"][2].goal_offset_mode == "ignore" and cfgs["tt_prodmp_replan"][2].goal_offset == 1.0


def test_the_cpu_fits_of_every_phase_row_are_finite():
    """both CPU fits of every row (3 episodes: timing outside, inside and on the bounds), and the horizon each round-boundary row names"""
    from tests import test_gpu_traj_fit as F
    for name in F.PHASE_KQ:
        cs = F.phase_case(name, 3)
        for e in cs["eps"]:
            assert np.isfinite(e["p64"]).all() and np.isfinite(e["p32"]).all() and np.isfinite(e["y"]).all(), name
            assert e["p32"].dtype == np.float32
        if "_round_t" in name:
            assert cs["eps"][0]["ds"].T == int(name.split("_t")[1].split("_")[0]), name


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    from fractions import Fraction
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def emulated_pivots(rows32, reg):
    """k_phase_fit's order in float64 on float32 rows [T, K]: a Gram entry is the fma chain over ascending steps, reg joins the
    diagonal, then the column Cholesky with fma(-L[i][k], L[j][k], s) over ascending k and a division by sqrt(pivot).  Returns the
    pivots; NaN behind the first that is not positive"""
    T, K = rows32.shape
    e = rows32.astype(np.float64)
    M = np.zeros((K, K))
    for i in range(K):
        for j in range(i + 1):
            acc = 0.0
            for s in range(T):
                acc = fma(e[s, i], e[s, j], acc)
            M[i, j] = acc + reg if i == j else acc
    pivots = []
    for j in range(K):
        col = np.zeros(K)
        for i in range(j, K):
            s = M[i, j]
            for k in range(j):
                s = fma(-M[i, k], M[j, k], s)
            col[i] = s
        pivots.append(col[j])
        ljj = np.sqrt(col[j]) if col[j] > 0.0 else float("nan")
        M[j, j] = 1.0 / ljj
        M[j + 1:, j] = col[j + 1:] / ljj
    return np.array(pivots)


def test_the_rank_one_gram_matrix_loses_a_pivot():
    """the mixed batch of test_an_episode_without_a_factor_is_flagged_and_stays_alone, in the kernel's order on the CPU: an ordinary
    episode keeps eight pivots above its smallest eigenvalue; an episode whose phase is clipped at every step has equal rows, a Gram
    matrix of rank 1, and loses a pivot to rounding (here the third: -1.8e-48 after 1.2e-63 and 2.2e-62).  With 5 steps the ordinary
    episodes would lose one too (8 columns, rank 5: pivot 3 = -1.2e-9), hence 12 steps"""
    from tests import test_gpu_traj_fit as F
    pc, bc, tc, dt, duration = F.npd_config()
    reg = F.NPD_REG
    assert np.float64(1.0) + reg == 1.0
    ordinary = R.Design(pc, bc, tc, dt, duration, 0.0)
    with np.errstate(all="ignore"):                      # (the float32 grid collapses at 1e6: the oracle's velocity divides by zero)
        clipped = R.Design(pc, bc, tc, dt, duration, 1e6)
    assert ordinary.T == 12 and ordinary.Kloc == 8
    piv = emulated_pivots(ordinary.Psi[0].astype(np.float32), reg)
    ev = np.linalg.eigvalsh(ordinary.Psi[0].T @ ordinary.Psi[0])
    print(f"ordinary: pivots {piv.min():.3e} .. {piv.max():.3e}, eigenvalues {ev[0]:.3e} .. {ev[-1]:.3e}")
    assert (piv >= 0.999 * ev[0]).all() and ev[0] > 1e-2
    rows = clipped.Psi[0].astype(np.float32)
    assert (rows == rows[0]).all() and (rows[0] > 0).all()
    piv = emulated_pivots(rows, reg)
    lost = np.flatnonzero(~(piv > 0.0))
    print("rank 1: pivots " + " ".join(f"{p:.3e}" for p in piv))
    assert piv[0] > 0.0 and lost.size and lost[0] >= 1
    diag = 12.0 * rows[0].astype(np.float64) ** 2
    assert (np.abs(piv[1:lost[0] + 1]) <= 1e-12 * diag[1:lost[0] + 1]).all()      # residue, not signal
    # ... and five steps against eight columns leave the ordinary episodes without a factor as well
    short = R.Design(dataclasses.replace(pc, tau=0.05), bc, tc, dt, 0.05, 0.0)
    assert short.T == 5 and not (emulated_pivots(short.Psi[0].astype(np.float32), reg) > 0.0).all()
