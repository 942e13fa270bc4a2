"""
Conditioning a Gaussian over the MP parameters on observed points, without a GPU: the public surface exists; the reference helper
(tests/trajectory_condition_ref.py) is what it says -- the sequential square-root update the kernel uses equals the batch formula, keeps
the factor lower triangular with a non-negative diagonal, and does not care how the observations are split over calls; and
condition_on_observations maps times to steps and refuses bad arguments before anything touches a device.
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
from fancy_gym_amd.black_box.factory import get_basis_generator, get_phase_generator, get_trajectory_generator
from tests import trajectory_condition_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMAS = (0.1, 1e-3, 0.0)
CASES = [(n, s) for n in ("cfg1_promp_zero_padded", "cfg2_prodmp", "promp_16_columns_3_dof", "cfg4_prodmp_init_time", "prodmp_1_dof")
         for s in SIGMAS] + [("prodmp_relative_goal", s) for s in SIGMAS[:2]]


# ---- 0. the surface -----------------------------------------------------------------------------------------------------------------------
def test_surface():
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    proto = ("int mpk_trajectory_condition(mpk_handle h, const float* params, const float* params_L, const float* init_pos, "
             "const float* init_vel, double init_time_shared, const int32_t* obs_steps, int32_t M, const float* obs_pos, "
             "const float* obs_pos_std, const float* obs_vel, const float* obs_vel_std, float* params_out, float* params_L_out, "
             "int32_t B, void* stream);")
    assert proto in header, proto
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4
    for word in ("Carlson", "FACTOR", "unpinned one of mpk_trajectory_std", "strict upper triangle is never read", "+inf, NaN",
                 "exact conditioning", "unspecified (it never faults)", "k_traj_condition<promp | prodmp>", "Pl = 256 does not"):
        assert word in header, word
    assert len(_lib.SIGNATURES["mpk_trajectory_condition"][1]) == 16
    unit = os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_traj_condition.hip")
    assert "mpk_traj_condition.hip" in _lib.KERNEL_UNITS and unit in _lib.SOURCE_FILES
    with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_kernels.hip")) as f:
        assert '#include "mpk_traj_condition.hip"' in f.read()
    with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_internal.h")) as f:
        text = f.read()
        assert "launch_traj_condition(" in text and "traj_cond_limits(" in text
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_trajectory_condition$", syms, re.M)
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4
    assert lib.mpk_trajectory_condition(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, None, 1,
                                        None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
    p = inspect.signature(TrajectoryEngine.condition).parameters
    assert list(p) == ["self", "params", "params_L", "obs_steps", "obs_pos", "obs_std", "init_pos", "init_vel", "init_time", "obs_vel",
                       "obs_vel_std", "out"]
    assert all(p[k].kind is p[k].KEYWORD_ONLY for k in ("obs_vel", "obs_vel_std", "out"))
    assert all(p[k].default is None for k in ("obs_pos", "obs_std", "init_pos", "init_vel", "obs_vel", "obs_vel_std", "out"))
    assert p["init_time"].default == 0.0
    assert list(inspect.signature(BatchedBlackBox.condition).parameters)[:6] == ["self", "params", "params_L", "obs_steps", "obs_pos",
                                                                                 "obs_std"]


# ---- 1. the sequential restatement is the batch formula ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sigma", CASES)
def test_the_sequential_update_is_the_batch_formula(name, sigma):
    """mean within 1e-6 max|ref|, L' L'^T within 1e-6 max|Sigma'| (measured: <= 8e-10), L' lower triangular with a non-negative
    diagonal.  The covariance is compared, never the factor (the helper's docstring says why)."""
    ref = R.case(name, 2, 3, sigma, seed=3, vel=name in ("cfg2_prodmp", "cfg1_promp_zero_padded") and sigma > 0)
    L64 = R.tril64(ref["L"])
    worst = [0.0, 0.0]
    for b in range(2):
        ob = R.observations(name, b, ref["steps"], ref["c"], (ref["pos"], ref["vel"]))
        mu, L = R.sequential(ref["mu"][b].astype(np.float64), L64[b], ob)
        assert np.isfinite(mu).all() and np.isfinite(L).all()
        assert (np.triu(L, 1) == 0.0).all() and (np.diag(L) >= 0.0).all()
        e_mu = np.abs(mu - ref["ref_mu"][b]).max() / np.abs(ref["ref_mu"][b]).max()
        e_S = np.abs(L @ L.T - ref["ref_Sigma"][b]).max() / np.abs(ref["ref_Sigma"][b]).max()
        worst = [max(worst[0], e_mu), max(worst[1], e_S)]
    print(f"[cond] {name} sigma={sigma}: sequential vs batch, mean {worst[0]:.2e} of max|ref|, covariance {worst[1]:.2e} of max|Sigma'|")
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6


# ---- 2. two calls are one call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sigma", [("cfg2_prodmp", 0.1), ("cfg2_prodmp", 0.0), ("cfg1_promp_zero_padded", 1e-3)])
def test_splitting_the_observations_over_two_calls_is_one_call(name, sigma):
    ref = R.case(name, 2, 3, sigma, seed=3, vel=sigma > 0)
    L64 = R.tril64(ref["L"])
    for b in range(2):
        ob = R.observations(name, b, ref["steps"], ref["c"], (ref["pos"], ref["vel"]))
        one_mu, one_L = R.sequential(ref["mu"][b].astype(np.float64), L64[b], ob)
        k = len([x for x in ob if x[4][1] == 0])                            # the first step's observations, then the other two steps'
        mid_mu, mid_L = R.sequential(ref["mu"][b].astype(np.float64), L64[b], ob[:k])
        two_mu, two_L = R.sequential(mid_mu, mid_L, ob[k:])
        assert np.array_equal(one_mu, two_mu) and np.array_equal(one_L, two_L)       # the same arithmetic in the same order
        # ... and the batch formula applied twice, which is another arithmetic
        a_mu, a_S = R.batch(ref["mu"][b].astype(np.float64), L64[b], ob[:k])
        S = 0.5 * (a_S + a_S.T)
        evals, evecs = np.linalg.eigh(S)
        half = evecs * np.sqrt(np.maximum(evals, 0.0))                              # any square root of the intermediate covariance
        b_mu, b_S = R.batch(a_mu, half, ob[k:])
        assert np.abs(b_mu - one_mu).max() <= 1e-6 * np.abs(one_mu).max()
        assert np.abs(b_S - one_L @ one_L.T).max() <= 1e-6 * np.abs(b_S).max()


# ---- 3. skipped observations -------------------------------------------------------------------------------------------------------------
def test_skipped_observations_change_nothing():
    name = "cfg2_prodmp"
    ref = R.case(name, 2, 3, 0.1, seed=3)
    L64 = R.tril64(ref["L"])
    mu0 = ref["mu"][0].astype(np.float64)
    y, sd = ref["pos"]
    for bad in (np.inf, np.nan, -1.0):
        sd2 = sd.copy()
        sd2[0, 1, ::2] = bad
        assert len(R.observations(name, 0, ref["steps"], ref["c"], ((y, sd2), None))) == sd[0].size - len(sd2[0, 1, ::2])
        h = R.jacobian(name)[0][0][5, 0, :mu0.size]
        mu, L = R.sequential(mu0, L64[0], [(h, 0.0, 1.0, bad, (0, 0, 0))])
        assert np.array_equal(mu, mu0) and np.array_equal(L, L64[0])
    mu, L = R.sequential(mu0, np.zeros_like(L64[0]), [(h, 0.0, 1.0, 0.0, (0, 0, 0))])      # s == 0
    assert np.array_equal(mu, mu0) and not L.any()


# ---- 4. condition_on_observations: the host side -------------------------------------------------------------------------------------------
def make_mp(mp="prodmp", D=3):
    pg = get_phase_generator("exp", tau=1.0, alpha_phase=3.0)
    bg = get_basis_generator("prodmp" if mp == "prodmp" else "rbf", pg, num_basis=4)
    gen = get_trajectory_generator(mp, D, bg)
    gen.set_duration(1.0, 0.02)
    return gen


class Recorder:
    """stands in for the engine: keeps what condition was called with and returns the prior"""

    def __init__(self):
        self.calls = []

    def condition(self, params, params_L, obs_steps, obs_pos, obs_std, init_pos, init_vel, init_time, *, obs_vel, obs_vel_std):
        self.calls.append(dict(steps=list(obs_steps), pos=obs_pos, std=obs_std, vel=obs_vel, vel_std=obs_vel_std, init_time=init_time,
                               init_pos=init_pos))
        return torch.as_tensor(params) + 1.0, torch.as_tensor(params_L) * 0.5


def test_condition_on_observations_maps_times_to_steps_and_stores_the_posterior():
    for mp, Pl in (("prodmp", 15), ("promp", 12)):
        gen = make_mp(mp)
        rec = Recorder()
        gen.engine = lambda rec=rec: rec
        gen.set_params(np.zeros(gen.num_params, np.float32))
        with pytest.raises(RuntimeError, match="set_mp_params_variances"):
            gen.condition_on_observations([0.5], np.zeros((1, 3)), 0.1)
        assert not rec.calls
        gen.set_mp_params_variances(np.eye(Pl, dtype=np.float32))
        gen.set_initial_conditions(0.1, np.ones(3), np.zeros(3))
        # the grid is init_time + 0.02, ..., init_time + 1.0: step t sits at init_time + (t + 1) dt; times in any order
        pos = np.arange(6, dtype=np.float32).reshape(2, 3)
        params, L = gen.condition_on_observations(torch.tensor([1.1, 0.6]), pos, [0.0, np.inf])
        call = rec.calls[-1]
        assert call["steps"] == [24, 49] and all(type(s) is int for s in call["steps"])
        assert np.array_equal(call["pos"], pos[::-1][None]) and call["pos"].dtype == np.float32
        assert np.array_equal(call["std"], np.array([[np.inf] * 3, [0.0] * 3], np.float32)[None])
        assert call["vel"] is None and call["vel_std"] is None and call["init_time"] == pytest.approx(0.1)
        assert np.array_equal(call["init_pos"], np.ones((1, 3), np.float32))
        assert params is gen.params and L is gen.params_L and gen._pos is None and gen._pos_std is None
        assert np.array_equal(gen.params.reshape(-1), np.ones(Pl, np.float32)) and np.array_equal(gen.params_L, 0.5 * np.eye(Pl))
        gen.condition_on_observations([0.12], None, None, vel=np.zeros((1, 3)), vel_std=np.full((1, 3), 0.5))
        call = rec.calls[-1]
        assert call["steps"] == [0] and call["pos"] is None and call["std"] is None and call["vel_std"].shape == (1, 1, 3)
        n = len(rec.calls)
        for times in ([0.61], [0.1], [1.13], [0.6, 2.0]):                  # between two steps, the initial time itself, past the end
            with pytest.raises(ValueError, match="is no step of the grid"):
                gen.condition_on_observations(times, np.zeros((len(times), 3)), 0.1)
        with pytest.raises(ValueError, match="same time"):
            gen.condition_on_observations([0.6, 0.6], np.zeros((2, 3)), 0.1)
        with pytest.raises(ValueError, match=r"pos must be \[2, 3\]"):
            gen.condition_on_observations([0.6, 0.7], np.zeros((2, 4)), 0.1)
        with pytest.raises(ValueError, match="std does not broadcast"):
            gen.condition_on_observations([0.6, 0.7], np.zeros((2, 3)), np.zeros(5))
        with pytest.raises(ValueError, match="come in pairs"):
            gen.condition_on_observations([0.6], np.zeros((1, 3)), None)
        with pytest.raises(ValueError, match="nothing is observed"):
            gen.condition_on_observations([0.6], None, None)
        assert len(rec.calls) == n
        gen.reset()
        gen.set_params(np.zeros(gen.num_params, np.float32))
        with pytest.raises(RuntimeError, match="set_mp_params_variances"):
            gen.condition_on_observations([0.5], np.zeros((1, 3)), 0.1)
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        make_mp("dmp").condition_on_observations([0.5], np.zeros((1, 3)), 0.1)


# ---- 5. refusals of TrajectoryEngine.condition that need no device -----------------------------------------------------------------------
class StubEngine(TrajectoryEngine):
    """the attributes the checks read, and no handle: a call that got past the checks would fail on the NULL handle"""

    def __init__(self, mp_type, D, T, P, learn_tau=False, learn_delay=False):
        self.config = _lib.mpk_config()
        self.config.learn_tau, self.config.learn_delay = int(learn_tau), int(learn_delay)
        self.mp_type, self.num_dof, self.num_params, self._T = mp_type, D, P, T
        self.device = torch.device("cuda", 0)

    num_steps = property(lambda self: self._T)

    def close(self):
        pass


def test_condition_refuses_before_any_device_work():
    eng = StubEngine("prodmp", 7, 100, 42)
    mu, L, y, z = np.zeros((3, 42), np.float32), np.zeros((3, 42, 42), np.float32), np.zeros((3, 2, 7), np.float32), np.zeros((3, 7))
    with pytest.raises(ValueError, match=r"params must be \[B, 42\]"):
        eng.condition(mu[:, :41], L, [1, 2], y, 0.1, z, z)
    with pytest.raises(ValueError, match=r"params_L must be \[3, 42, 42\]"):
        eng.condition(mu, L[:2], [1, 2], y, 0.1, z, z)
    with pytest.raises(ValueError, match="sequence of ints"):
        eng.condition(mu, L, [1.5, 2.0], y, 0.1, z, z)
    with pytest.raises(ValueError, match="nothing is observed"):
        eng.condition(mu, L, [1, 2], None, None, z, z)
    with pytest.raises(ValueError, match="obs_pos and obs_std come in pairs"):
        eng.condition(mu, L, [1, 2], y, None, z, z)
    with pytest.raises(ValueError, match="obs_vel and obs_vel_std come in pairs"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z, obs_vel_std=0.1)
    with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
        eng.condition(mu, L, [1, 2], y, 0.1)
    with pytest.raises(ValueError, match="out must be a pair"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z, out=(torch.zeros(3, 42),))
    with pytest.raises(ValueError, match=r"out\[0\] must be a contiguous float32 tensor of shape \(3, 42\)"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z, out=(torch.zeros(3, 41), torch.zeros(3, 42, 42)))
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        StubEngine("prodmp", 7, 100, 43, learn_tau=True).condition(mu, L, [1, 2], y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        StubEngine("dmp", 7, 100, 42).condition(mu, L, [1, 2], y, 0.1, z, z)
    with pytest.raises(NotImplementedError, match="at most 16 DoF"):
        StubEngine("prodmp", 20, 25, 100).condition(np.zeros((3, 100)), np.zeros((3, 100, 100)), [1], np.zeros((3, 1, 20)), 0.1,
                                                    np.zeros((3, 20)), np.zeros((3, 20)))
