"""
Conditioning a Gaussian over the MP parameters on whole demonstrations, without a GPU: the public surface exists; the information form the
kernel evaluates (include/mpk.h: the reverse Cholesky M = K^T K, L' = tril(L) K^-1), restated in float64 numpy, is the dense batch formula
of the reference on every case of the GPU test, with a lower-triangular factor of positive diagonal; the float32-table floor cannot make a
bound of the GPU tests vacuous; the edge semantics hold on the restatement; and every refusal is raised before anything touches a device.
"""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fancy_gym_amd import TrajectoryEngine, _lib
from fancy_gym_amd.batched import BatchedBlackBox
from fancy_gym_amd.mp.traj import MPInterface
from tests import demonstration_condition_ref as CR

from .test_traj_condition_host import Recorder, StubEngine, make_mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_surface():
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    proto = ("int mpk_demonstration_condition(mpk_handle h, const float* params, const float* params_L, const float* init_pos, "
             "const float* init_vel, double init_time_shared, const float* pos, const float* obs_std, float* params_out, "
             "float* params_L_out, int32_t B, void* stream);")
    assert proto in header, proto
    assert "int mpk_demonstration_condition_plan(mpk_handle h, int32_t B, int32_t* blocks, int32_t* waves, int32_t* lds_bytes);" in header
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4
    for word in ("M = I + tril(L)^T G tril(L) = K^T K", "L' = tril(L) K^-1", "mu' = mu + L' (K^-T v)", "diag L'_ii = L_ii / K_ii",
                 "k_demo_condition<promp | prodmp>", "may be params_L", "strict upper triangle of params_L is never read",
                 "sigma == 0 cannot be expressed", "comes back bit for bit", "exactly zero column",
                 "Not built: gradients through the posterior"):
        assert word in header, word
    assert len(_lib.SIGNATURES["mpk_demonstration_condition"][1]) == 12          # the prototype's twelve parameters, handle to stream
    csrc = os.path.join(ROOT, "fancy_gym_amd", "csrc")
    assert "mpk_demo_condition.hip" in _lib.KERNEL_UNITS and os.path.join(csrc, "mpk_demo_condition.hip") in _lib.SOURCE_FILES
    assert "mpk_demo_gram.h" in _lib.KERNEL_HEADERS and os.path.join(csrc, "mpk_demo_gram.h") in _lib.SOURCE_FILES
    with open(os.path.join(csrc, "mpk_kernels.hip")) as f:
        assert '#include "mpk_demo_condition.hip"' in f.read()
    for unit in ("mpk_demo_condition.hip", "mpk_demo_log_prob.hip"):                # both kernels compile the same accumulation
        with open(os.path.join(csrc, unit)) as f:
            text = f.read()
        assert '#include "mpk_demo_gram.h"' in text and "demo_accumulate<MP" in text and "demo_build_M<NS>" in text, unit
    with open(os.path.join(csrc, "mpk_internal.h")) as f:
        text = f.read()
        assert "launch_demo_condition(" in text and "demo_condition_launch_plan(" in text
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_demonstration_condition$", syms, re.M) and re.search(r" T mpk_demonstration_condition_plan$", syms, re.M)
    lib = _lib.load()
    assert lib.mpk_demonstration_condition(None, None, None, None, None, 0.0, None, None, None, None, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    assert lib.mpk_demonstration_condition_plan(None, 1, None, None, None) == _lib.MPK_EINVAL and "NULL handle" in _lib.last_error()
    p = inspect.signature(TrajectoryEngine.condition_on_demonstration).parameters
    assert list(p) == ["self", "params", "params_L", "pos", "obs_std", "init_pos", "init_vel", "init_time", "out"]
    assert p["init_pos"].default is None and p["init_vel"].default is None and p["init_time"].default == 0.0
    assert p["out"].kind is p["out"].KEYWORD_ONLY and p["out"].default is None
    assert list(inspect.signature(MPInterface.condition_on_trajectories).parameters) == ["self", "pos", "std"]
    q = inspect.signature(BatchedBlackBox.condition_on_demonstration).parameters
    assert list(q) == ["self", "params", "params_L", "pos", "obs_std", "out"] and q["out"].kind is q["out"].KEYWORD_ONLY


# ---- 2. the information form is the dense formula; the floor cannot make a bound vacuous -------------------------------------------------
@pytest.mark.parametrize("name,B,sigma,missing", CR.gpu_cases())
def test_the_information_form_is_the_dense_formula_and_the_floor_stays_below_the_cap(name, B, sigma, missing):
    """Measured on the CPU before the kernel was written: within 4.5e-8 of max|ref| at worst over cfg2_prodmp, cfg1_promp_zero_padded and
    prodmp_12_columns_16_dof (Pl = 160); asserted at 1e-6 of max|ref|.  Floor cap: 4 x floor <= 1e-2 max|ref| (2.4e-5 measured)"""
    cs = CR.case(name, B, sigma, missing)
    T, D = cs["pos"].shape[1:]
    P = cs["mu"].shape[1]
    assert np.isnan(cs["L"][:, np.triu(np.ones((P, P), bool), 1)]).all()
    assert ((cs["n"] < T * D).all() and (cs["n"] > 0.5 * T * D).all()) if missing else (cs["n"] == T * D).all()
    assert np.isfinite(cs["ref_mu"]).all() and np.isfinite(cs["ref_Sigma"]).all()
    L64 = CR.tril64(cs["L"])
    for b in range(B):
        ob = CR.kept(name, b, cs["c"], cs["pos"], cs["sd"])
        assert len(ob) == cs["n"][b]
        mu, Lp = CR.information_form(cs["mu"][b].astype(np.float64), L64[b], ob)
        e_mu = np.abs(mu - cs["ref_mu"][b]).max() / np.abs(cs["ref_mu"][b]).max()
        e_S = np.abs(Lp @ Lp.T - cs["ref_Sigma"][b]).max() / np.abs(cs["ref_Sigma"][b]).max()
        print(f"[demo-cond] {name} b={b} n={len(ob)} sigma={sigma}: information form vs dense, mean {e_mu:.2e}  covariance {e_S:.2e}")
        assert e_mu <= 1e-6 and e_S <= 1e-6
        assert (np.triu(Lp, 1) == 0.0).all() and (np.diag(Lp) > 0.0).all()
    for label, r, fl in (("mean", cs["ref_mu"], cs["floor_mu"]), ("covariance", cs["ref_Sigma"], cs["floor_Sigma"])):
        cap = 4.0 * fl.max() / np.abs(r).max()
        print(f"[demo-cond] {name} B={B} sigma={sigma} {label}: 4 x floor / max|ref| = {cap:.2e}")
        assert cap <= 1e-2, (label, cap)


def test_the_cases_are_the_ones_stated():
    cases = CR.gpu_cases()
    assert len(cases) == len(set(cases)) == 54 and all(CR.jacobian(c[0])[3] <= 200 for c in cases)    # (200: cfg1's own horizon)
    assert CR.jacobian("prodmp_12_columns_16_dof")[1] == 160 and CR.jacobian("cfg2_prodmp_97_steps")[3] == 97
    assert {c[2:] for c in cases} == set(CR.SIGMAS)


def test_the_reverse_cholesky_and_the_inverse_are_what_they_say():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((23, 23))
    M = np.eye(23) + A @ A.T
    K = CR.reverse_cholesky(M)
    assert (np.triu(K, 1) == 0.0).all() and np.abs(K.T @ K - M).max() <= 1e-13 * np.abs(M).max()
    Ki = CR.lower_inverse(K)
    assert (np.triu(Ki, 1) == 0.0).all() and np.abs(Ki @ K - np.eye(23)).max() <= 1e-12
    assert np.array_equal(np.diag(Ki), 1.0 / np.diag(K))


# ---- 3. edge semantics on the restatement ---------------------------------------------------------------------------------------------------
def test_edges_of_the_restatement():
    name = "cfg2_prodmp"
    cs = CR.case(name, 3, 0.1, True)
    mu, L64 = cs["mu"][0].astype(np.float64), CR.tril64(cs["L"])[0].copy()
    ob = CR.kept(name, 0, cs["c"], cs["pos"], cs["sd"])
    # nothing kept: the prior
    m0, L0 = CR.information_form(mu, L64, [])
    assert np.array_equal(m0, mu) and np.array_equal(L0, L64)
    # an exactly zero column of tril(L): row and column j of M are e_j, so column j of L' is exactly zero
    Lz = L64.copy()
    Lz[:, 5] = 0.0
    mz, Lpz = CR.information_form(mu, Lz, ob)
    assert (Lpz[:, 5] == 0.0).all() and np.abs(Lpz).max() > 0
    ref = CR.R.batch(mu, Lz, ob)
    assert np.abs(mz - ref[0]).max() <= 1e-6 * np.abs(ref[0]).max() and np.abs(Lpz @ Lpz.T - ref[1]).max() <= 1e-6 * np.abs(ref[1]).max()
    # an all-zero L: M = I, the mean unchanged bit for bit
    ma, La = CR.information_form(mu, np.zeros_like(L64), ob)
    assert np.array_equal(ma, mu) and (La == 0.0).all()
    # sigma == 0 has no place in this form
    with pytest.raises(AssertionError, match="sigma == 0"):
        CR.information_form(mu, L64, [ob[0][:3] + (0.0,) + ob[0][4:]])
    # a kept entry count: a removed entry (sigma = inf) carries the garbage value 1e6 and is not among the observations
    assert cs["n"][0] == len(ob) < cs["sd"][0].size and all(abs(x[2]) < 1e5 for x in ob)


# ---- 4. refusals, before anything touches a device -----------------------------------------------------------------------------------------
def test_refusals_before_any_device_work():
    eng = StubEngine("prodmp", 7, 100, 42)
    mu, L, y, z = np.zeros((3, 42), np.float32), np.zeros((3, 42, 42), np.float32), np.zeros((3, 100, 7), np.float32), np.zeros((3, 7))
    call = eng.condition_on_demonstration
    with pytest.raises(ValueError, match=r"params must be \[B, 42\]"):
        call(mu[:, :41], L, y, 0.1, z, z)
    with pytest.raises(ValueError, match=r"params_L must be \[3, 42, 42\]"):
        call(mu, L[:2], y, 0.1, z, z)
    for bad in (y[:, :99], y[:2], y[:, :, :6], y[0], np.zeros((3, 2, 7), np.float32)):
        with pytest.raises(ValueError, match=r"pos must be \[3, 100, 7\]"):
            call(mu, L, bad, 0.1, z, z)
    with pytest.raises(ValueError, match="pos and obs_std are both required"):
        call(mu, L, y, None, z, z)
    with pytest.raises(ValueError, match="pos and obs_std are both required"):
        call(mu, L, None, 0.1, z, z)
    with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
        call(mu, L, y, 0.1)
    with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
        call(mu, L, y, 0.1, z)
    # out=, exactly as condition validates it
    with pytest.raises(ValueError, match="out must be a pair"):
        call(mu, L, y, 0.1, z, z, out=(torch.zeros(3, 42),))
    for out in ((torch.zeros(3, 42), torch.zeros(3, 42, 41)), (torch.zeros(3, 42, dtype=torch.float64), torch.zeros(3, 42, 42)),
                (np.zeros((3, 42), np.float32), torch.zeros(3, 42, 42)), (torch.zeros(42, 3).t(), torch.zeros(3, 42, 42)),
                (torch.zeros(3, 42), torch.zeros(3, 42, 42))):                  # (the last pair: right shapes, but on the CPU)
        with pytest.raises(ValueError, match=r"out\[[01]\] must be a contiguous float32 tensor of shape"):
            call(mu, L, y, 0.1, z, z, out=out)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        StubEngine("prodmp", 7, 100, 43, learn_tau=True).condition_on_demonstration(mu, L, y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        StubEngine("prodmp", 7, 100, 43, learn_delay=True).condition_on_demonstration(mu, L, y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        StubEngine("dmp", 7, 100, 42).condition_on_demonstration(mu, L, y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="at most 16 DoF"):
        StubEngine("prodmp", 20, 25, 100).condition_on_demonstration(np.zeros((3, 100)), np.zeros((3, 100, 100)), np.zeros((3, 25, 20)),
                                                                     0.1, np.zeros((3, 20)), np.zeros((3, 20)))


class DemoCondRecorder(Recorder):
    def condition_on_demonstration(self, params, params_L, pos, obs_std, init_pos, init_vel, init_time):
        self.calls.append(dict(pos=pos, std=obs_std, init_time=init_time, init_pos=init_pos, init_vel=init_vel, params=params,
                               params_L=params_L))
        return torch.as_tensor(params) + 1.0, torch.as_tensor(params_L) * 0.5


def test_condition_on_trajectories_hands_the_stored_gaussian_over_and_changes_nothing():
    for mp, Pl in (("prodmp", 15), ("promp", 12)):
        gen = make_mp(mp)
        rec = DemoCondRecorder()
        gen.engine = lambda rec=rec: rec
        gen.set_params(np.arange(Pl, dtype=np.float32))
        with pytest.raises(RuntimeError, match="set_mp_params_variances"):
            gen.condition_on_trajectories(np.zeros((50, 3)), 0.1)
        gen.set_mp_params_variances(np.eye(Pl, dtype=np.float32))
        gen.set_initial_conditions(0.1, np.ones(3), np.zeros(3))
        pos = np.arange(2 * 50 * 3, dtype=np.float32).reshape(2, 50, 3)
        std = np.full((50, 3), 0.5, np.float32)
        std[20:] = np.inf                                                       # a prefix of 40 %
        mean, L = gen.condition_on_trajectories(torch.from_numpy(pos), std)
        call = rec.calls[-1]
        assert isinstance(mean, torch.Tensor) and mean.shape == (2, Pl) and L.shape == (2, Pl, Pl) and mean.dtype == L.dtype == torch.float32
        assert np.array_equal(mean[1].numpy(), np.arange(Pl) + 1.0) and np.array_equal(L[0].numpy(), 0.5 * np.eye(Pl))
        assert np.array_equal(call["pos"], pos) and np.array_equal(call["std"], std) and call["init_time"] == pytest.approx(0.1)
        assert call["params"].shape == (2, Pl) and np.array_equal(call["params"][1], np.arange(Pl))
        assert call["params_L"].shape == (2, Pl, Pl) and np.array_equal(call["init_pos"], np.ones((2, 3)))
        assert gen.condition_on_trajectories(pos[0], 0.1)[0].shape == (1, Pl) and rec.calls[-1]["pos"].shape == (1, 50, 3)
        assert np.array_equal(gen.params.reshape(-1), np.arange(Pl)) and np.array_equal(gen.params_L, np.eye(Pl))   # the prior stays
        n = len(rec.calls)
        with pytest.raises(ValueError, match=r"pos must be \[N, T, 3\]"):
            gen.condition_on_trajectories(np.zeros((50, 2)), 0.1)
        assert len(rec.calls) == n
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        make_mp("dmp").condition_on_trajectories(np.zeros((50, 3)), 0.1)
