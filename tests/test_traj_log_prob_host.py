"""
The log-likelihood of observed points under a Gaussian over the MP parameters, without a GPU: the public surface exists; the reference
helper (tests/trajectory_log_prob_ref.py) is right by a route independent of its formula -- the product of the one-step predictive
densities along conditioning's sequential update -- and its autograd gradient is the closed form include/mpk.h states; the float32-table
floor cannot make a bound of the GPU tests vacuous; and every refusal is raised before anything touches a device.
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
from tests import trajectory_condition_ref as R
from tests import trajectory_log_prob_ref as LP

from .test_traj_condition_host import Recorder, StubEngine, make_mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = [(n, s, v) for n in ("cfg1_promp_zero_padded", "cfg2_prodmp") for s in (0.1, 1e-3) for v in (False, True)] + \
        [(n, s, False) for n in ("promp_16_columns_3_dof", "prodmp_1_dof", "prodmp_relative_goal") for s in (0.1, 1e-3)]


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_surface():
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    common = ("(mpk_handle h, const float* params, const float* params_L, const float* init_pos, const float* init_vel, "
              "double init_time_shared, const int32_t* obs_steps, int32_t M, const float* obs_pos, const float* obs_pos_std, "
              "const float* obs_vel, const float* obs_vel_std, ")
    for proto in ("int mpk_trajectory_log_prob" + common + "double* log_prob, int32_t B, void* stream);",
                  "int mpk_trajectory_log_prob_vjp" + common + "const double* g, float* g_params, float* g_params_L, int32_t B, "
                  "void* stream);"):
        assert proto in header, proto
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4
    assert re.search(r"#define MPK_LOGPROB_MAX_OBS 64\b", raw) and _lib.MPK_LOGPROB_MAX_OBS == 64
    for word in ("never through L L^T", "exactly 0.0", "not > 0", "g tril(H^T (alpha alpha^T - S^-1) A)", "strict upper triangle of "
                 "params_L is never read", "k_traj_log_prob<promp | prodmp>", "recomputes A, S and C from the inputs",
                 "Pl = 160 with 64 observations runs", "different kernel: not built"):
        assert word in header, word
    assert len(_lib.SIGNATURES["mpk_trajectory_log_prob"][1]) == 15 and len(_lib.SIGNATURES["mpk_trajectory_log_prob_vjp"][1]) == 17
    csrc = os.path.join(ROOT, "fancy_gym_amd", "csrc")
    assert "mpk_traj_log_prob.hip" in _lib.KERNEL_UNITS and os.path.join(csrc, "mpk_traj_log_prob.hip") in _lib.SOURCE_FILES
    assert "mpk_cond_rows.h" in _lib.KERNEL_HEADERS and os.path.join(csrc, "mpk_cond_rows.h") in _lib.SOURCE_FILES
    with open(os.path.join(csrc, "mpk_kernels.hip")) as f:
        assert '#include "mpk_traj_log_prob.hip"' in f.read()
    with open(os.path.join(csrc, "mpk_internal.h")) as f:
        text = f.read()
        assert "launch_traj_log_prob(" in text and "traj_log_prob_limits(" in text
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_trajectory_log_prob$", syms, re.M) and re.search(r" T mpk_trajectory_log_prob_vjp$", syms, re.M)
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4
    assert lib.mpk_trajectory_log_prob(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    assert lib.mpk_trajectory_log_prob_vjp(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, None, None, 1,
                                           None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    p = inspect.signature(TrajectoryEngine.trajectory_log_prob).parameters
    assert list(p) == ["self", "params", "params_L", "obs_steps", "obs_pos", "obs_std", "init_pos", "init_vel", "init_time", "obs_vel",
                       "obs_vel_std"]
    assert all(p[k].kind is p[k].KEYWORD_ONLY for k in ("obs_vel", "obs_vel_std"))
    assert all(p[k].default is None for k in ("obs_pos", "obs_std", "init_pos", "init_vel", "obs_vel", "obs_vel_std"))
    assert p["init_time"].default == 0.0
    q = inspect.signature(TrajectoryEngine.trajectory_log_prob_vjp).parameters
    assert list(q)[:2] == ["self", "g"] and list(q)[2:12] == list(p)[1:]
    assert list(inspect.signature(MPInterface.log_prob_of_observations).parameters) == ["self", "times", "pos", "std", "vel", "vel_std"]
    assert list(inspect.signature(BatchedBlackBox.trajectory_log_prob).parameters)[:6] == ["self", "params", "params_L", "obs_steps",
                                                                                           "obs_pos", "obs_std"]


# ---- 2. the reference is right, by a route independent of its formula ----------------------------------------------------------------
def predictive_sum(mu, L, ob):
    """sum_i log N(r_i; 0, s_i) along conditioning's sequential update: s_i = sigma_i^2 + |L^T h_i|^2 and r_i from the running posterior"""
    total = 0.0
    for x in ob:
        h, c, y, sigma, _ = x
        v = L.T @ h
        s = sigma * sigma + v @ v
        r = y - c - h @ mu
        total += -0.5 * r * r / s - 0.5 * np.log(2.0 * np.pi * s)
        mu, L = R.sequential(mu, L, [x])
    return total


@pytest.mark.parametrize("name,sigma,vel", SMALL)
def test_the_reference_is_the_product_of_the_predictive_densities(name, sigma, vel):
    """... and consequently log p(y1, y2) = log p(y1) + log p(y2 | y1).  Measured: <= 2e-10 absolute; asserted at 1e-8 (|ref| + n)"""
    cs = LP.case(name, 3, 2, sigma, seed=LP.SEED, vel=vel)
    L64 = R.tril64(cs["L"])
    worst = 0.0
    for b in range(3):
        ob = R.observations(name, b, cs["steps"], cs["c"], (cs["pos"], cs["vel"]))
        mu = cs["mu"][b].astype(np.float64)
        ref = cs["ref_lp"][b]
        tol = 1e-8 * (abs(ref) + len(ob))
        seq = predictive_sum(mu, L64[b], ob)
        k = len([x for x in ob if x[4][1] == 0])                            # the first step's observations
        mid = R.sequential(mu, L64[b], ob[:k])
        two = LP.log_prob(mu, L64[b], ob[:k]) + LP.log_prob(mid[0], mid[1], ob[k:])
        worst = max(worst, abs(seq - ref), abs(two - ref))
        assert abs(seq - ref) <= tol and abs(two - ref) <= tol, (b, ref, seq, two)
    print(f"[logp] {name} sigma={sigma} vel={vel}: predictive product and chain rule vs the formula, worst {worst:.2e} absolute")


# ---- 3. the closed-form gradient of mpk.h is autograd's --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sigma,vel", SMALL)
def test_the_closed_form_gradient_is_autograd(name, sigma, vel):
    cs = LP.case(name, 3, 2, sigma, seed=LP.SEED, vel=vel)
    L64 = R.tril64(cs["L"])
    for b in range(3):
        ob = R.observations(name, b, cs["steps"], cs["c"], (cs["pos"], cs["vel"]))
        gm, gL = LP.closed_form(cs["mu"][b].astype(np.float64), L64[b], ob, cs["g"][b])
        e_m = np.abs(gm - cs["ref_gmu"][b]).max() / np.abs(cs["ref_gmu"][b]).max()
        e_L = np.abs(gL - cs["ref_gL"][b]).max() / np.abs(cs["ref_gL"][b]).max()
        print(f"[logp] {name} sigma={sigma} vel={vel} b={b}: closed form vs autograd, g_params {e_m:.2e}  g_params_L {e_L:.2e}")
        assert e_m <= 1e-7 and e_L <= 1e-7
        assert (np.triu(cs["ref_gL"][b], 1) == 0.0).all()


# ---- 4. the floor cannot make a bound vacuous ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vel,B,M,sigma", LP.gpu_cases())
def test_the_float32_table_floor_stays_below_the_cap(name, vel, B, M, sigma):
    cs = LP.case(name, B, M, sigma, seed=LP.SEED, vel=vel)
    assert np.isfinite(cs["ref_lp"]).all() and (cs["n"] == M * R.jacobian(name)[2] * (2 if vel else 1)).all() and (cs["n"] <= 64).all()
    LP.floor_cap(cs, f"{name} B={B} M={M} sigma={sigma} vel={vel}")


# ---- 5. refusals, before anything touches a device -----------------------------------------------------------------------------------------
def test_refusals_before_any_device_work():
    eng = StubEngine("prodmp", 7, 100, 42)
    mu, L, y, z = np.zeros((3, 42), np.float32), np.zeros((3, 42, 42), np.float32), np.zeros((3, 2, 7), np.float32), np.zeros((3, 7))
    g = np.zeros(3)
    for call in (eng.trajectory_log_prob, lambda *a, **k: eng.trajectory_log_prob_vjp(g, *a, **k)):
        with pytest.raises(ValueError, match=r"params must be \[B, 42\]"):
            call(mu[:, :41], L, [1, 2], y, 0.1, z, z)
        with pytest.raises(ValueError, match=r"params_L must be \[3, 42, 42\]"):
            call(mu, L[:2], [1, 2], y, 0.1, z, z)
        with pytest.raises(ValueError, match="sequence of ints"):
            call(mu, L, [1.5, 2.0], y, 0.1, z, z)
        with pytest.raises(ValueError, match="M must be 1..32"):
            call(mu, L, [], np.zeros((3, 0, 7), np.float32), 0.1, z, z)
        for steps in ([2, 1], [3, 3], [-1, 4], [5, 100]):
            with pytest.raises(ValueError, match="strictly increasing step indices"):
                call(mu, L, steps, y, 0.1, z, z)
        with pytest.raises(ValueError, match="nothing is observed"):
            call(mu, L, [1, 2], None, None, z, z)
        with pytest.raises(ValueError, match="obs_pos and obs_std come in pairs"):
            call(mu, L, [1, 2], y, None, z, z)
        with pytest.raises(ValueError, match="obs_vel and obs_vel_std come in pairs"):
            call(mu, L, [1, 2], y, 0.1, z, z, obs_vel_std=0.1)
        with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
            call(mu, L, [1, 2], y, 0.1)
        # 5 steps x 7 DoF x 2 arrays = 70 > 64; 10 steps x 7 DoF = 70 > 64
        y5 = np.zeros((3, 5, 7), np.float32)
        with pytest.raises(NotImplementedError, match="at most 64 scalar observations"):
            call(mu, L, [1, 2, 3, 4, 5], y5, 0.1, z, z, obs_vel=y5, obs_vel_std=0.1)
        with pytest.raises(NotImplementedError, match="at most 64 scalar observations"):
            call(mu, L, list(range(10)), np.zeros((3, 10, 7), np.float32), 0.1, z, z)
        for bad in ("init_pos", "init_vel", "obs_pos", "obs_std"):
            t = {"init_pos": torch.zeros(3, 7), "init_vel": torch.zeros(3, 7), "obs_pos": torch.zeros(3, 2, 7), "obs_std": torch.ones(1)}
            t[bad].requires_grad_(True)
            with pytest.raises(NotImplementedError, match=f"{bad} requires grad"):
                call(mu, L, [1, 2], t["obs_pos"], t["obs_std"], t["init_pos"], t["init_vel"])
        yv = torch.zeros(3, 2, 7, requires_grad=True)
        with pytest.raises(NotImplementedError, match="obs_vel requires grad"):
            call(mu, L, [1, 2], y, 0.1, z, z, obs_vel=yv, obs_vel_std=0.1)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        StubEngine("prodmp", 7, 100, 43, learn_tau=True).trajectory_log_prob(mu, L, [1, 2], y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        StubEngine("prodmp", 7, 100, 43, learn_delay=True).trajectory_log_prob_vjp(g, mu, L, [1, 2], y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        StubEngine("dmp", 7, 100, 42).trajectory_log_prob(mu, L, [1, 2], y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="at most 16 DoF"):
        StubEngine("prodmp", 20, 25, 100).trajectory_log_prob(np.zeros((3, 100)), np.zeros((3, 100, 100)), [1], np.zeros((3, 1, 20)),
                                                              0.1, np.zeros((3, 20)), np.zeros((3, 20)))


class LogProbRecorder(Recorder):
    def trajectory_log_prob(self, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time, *, obs_vel, obs_vel_std):
        self.calls.append(dict(steps=list(obs_steps), pos=obs_pos, std=obs_std, vel=obs_vel, vel_std=obs_vel_std, init_time=init_time,
                               init_pos=init_pos, params=params, params_L=params_L))
        return torch.tensor([-1.25], dtype=torch.float64)


def test_log_prob_of_observations_maps_times_to_steps_and_changes_nothing():
    for mp, Pl in (("prodmp", 15), ("promp", 12)):
        gen = make_mp(mp)
        rec = LogProbRecorder()
        gen.engine = lambda rec=rec: rec
        gen.set_params(np.zeros(gen.num_params, np.float32))
        with pytest.raises(RuntimeError, match="set_mp_params_variances"):
            gen.log_prob_of_observations([0.5], np.zeros((1, 3)), 0.1)
        gen.set_mp_params_variances(np.eye(Pl, dtype=np.float32))
        gen.set_initial_conditions(0.1, np.ones(3), np.zeros(3))
        pos = np.arange(6, dtype=np.float32).reshape(2, 3)
        lp = gen.log_prob_of_observations(torch.tensor([1.1, 0.6]), pos, [0.5, np.inf])
        call = rec.calls[-1]
        assert lp == -1.25 and isinstance(lp, float)
        assert call["steps"] == [24, 49] and np.array_equal(call["pos"], pos[::-1][None])
        assert np.array_equal(call["std"], np.array([[np.inf] * 3, [0.5] * 3], np.float32)[None])
        assert call["vel"] is None and call["init_time"] == pytest.approx(0.1) and call["params_L"].shape == (1, Pl, Pl)
        assert np.array_equal(gen.params.reshape(-1), np.zeros(Pl, np.float32)) and np.array_equal(gen.params_L, np.eye(Pl))
        n = len(rec.calls)
        with pytest.raises(ValueError, match="log_prob_of_observations: time .* is no step of the grid"):
            gen.log_prob_of_observations([0.61], np.zeros((1, 3)), 0.1)
        with pytest.raises(ValueError, match="come in pairs"):
            gen.log_prob_of_observations([0.6], np.zeros((1, 3)), None)
        assert len(rec.calls) == n
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        make_mp("dmp").log_prob_of_observations([0.5], np.zeros((1, 3)), 0.1)
