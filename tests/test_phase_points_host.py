"""
Host-side tests of the point-wise entry points with a per-episode phase (mpk_trajectory_phase_condition / _log_prob / _log_prob_vjp /
_std; TrajectoryEngine.condition_given_timing, trajectory_log_prob_given_timing, trajectory_log_prob_vjp_given_timing,
trajectory_std_given_timing): no GPU.

  1. the surface: the four prototypes of include/mpk.h, each with a ctypes signature that equals it; the sibling methods of the three
     Python layers, next to the shared-phase ones whose parameter lists stay as they are
  2. on every case of tests/test_gpu_phase_points.py's parity test: the floor cap 4 x floor <= 1e-2 x scale for every output array --
     posterior, likelihood and gradients, and the std's float32 floor -- and the dense batch formula against the sequential
     restatement of the kernel's update (tests/trajectory_condition_ref.sequential) on the per-episode rows
  3. the two families' references agree: the point likelihood at steps S is tests/demonstration_phase_ref's dense likelihood of a
     demonstration whose sigma is inf off S (positions only); the std reference is sqrt(diag(J Sigma J^T))
  4. the refusals of the Python layer with a stub engine: nothing touches a device
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fancy_gym_amd import _lib
from fancy_gym_amd.batched import BatchedBlackBox
from fancy_gym_amd.engine import TrajectoryEngine
from fancy_gym_amd.mp.traj import MPInterface

from . import demonstration_phase_ref as DP
from . import phase_points_ref as PP
from . import trajectory_condition_ref as R
from . import trajectory_log_prob_ref as LP
from . import trajectory_std_ref as SR
from .test_demo_phase_host import ctype_of
from .test_traj_condition_host import StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = {"mpk_trajectory_phase_condition": "mpk_trajectory_condition", "mpk_trajectory_phase_log_prob": "mpk_trajectory_log_prob",
          "mpk_trajectory_phase_log_prob_vjp": "mpk_trajectory_log_prob_vjp"}


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_every_new_signature_equals_its_prototype():
    with open(os.path.join(ROOT, "include", "mpk.h")) as f:
        raw = f.read()
    header = re.sub(r"\s+", " ", raw)
    assert re.search(r"#define MPK_ABI_VERSION 4\b", raw) and _lib.MPK_ABI_VERSION == 4, "append-only: no ABI bump"
    for name in tuple(SHARED) + ("mpk_trajectory_phase_std",):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name}: no prototype in include/mpk.h"
        want = [C.POINTER(C.c_int32) if "obs_steps" in d else ctype_of(d, False) for d in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, (name, args, want)
    for name, old in SHARED.items():                                             # the arguments are those of the shared-phase entries
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[old], name
    for word in ("k_traj_condition<promp | prodmp, phase>", "k_traj_log_prob<promp | prodmp, phase[, grad]>",
                 "k_traj_phase_std<promp | prodmp>", "the phase columns of g_params", "unclipped",
                 "Not built: gradients w.r.t. tau / delay, a per-episode init_time, DMP, correlated noise"):
        assert word in header, word
    assert "mpk_traj_phase_std.hip" in _lib.KERNEL_UNITS
    with open(os.path.join(ROOT, "fancy_gym_amd", "csrc", "mpk_kernels.hip")) as f:
        assert '#include "mpk_traj_phase_std.hip"' in f.read()
    lib = _lib.load()
    assert lib.mpk_trajectory_phase_condition(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, None, 1,
                                              None) == _lib.MPK_EINVAL
    assert lib.mpk_trajectory_phase_log_prob(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, 1, None) == _lib.MPK_EINVAL
    assert lib.mpk_trajectory_phase_log_prob_vjp(None, None, None, None, None, 0.0, None, 1, None, None, None, None, None, None, None, 1,
                                                 None) == _lib.MPK_EINVAL
    assert lib.mpk_trajectory_phase_std(None, None, None, 0.0, None, None, 1, None) == _lib.MPK_EINVAL and "NULL handle" in _lib.last_error()


def test_the_python_surface():
    for new, old in (("condition_given_timing", "condition"), ("trajectory_log_prob_given_timing", "trajectory_log_prob"),
                     ("trajectory_log_prob_vjp_given_timing", "trajectory_log_prob_vjp")):
        assert str(inspect.signature(getattr(TrajectoryEngine, new))) == str(inspect.signature(getattr(TrajectoryEngine, old))), new
        assert "exact zeros" in getattr(TrajectoryEngine, new).__doc__ or "unclipped" in getattr(TrajectoryEngine, new).__doc__
    assert list(inspect.signature(TrajectoryEngine.trajectory_std_given_timing).parameters) == \
        ["self", "params", "params_L", "init_time", "pos", "vel", "out"]
    assert list(inspect.signature(TrajectoryEngine.trajectory_std).parameters) == ["self", "params_L", "init_time", "pos", "vel", "out"]
    for new in ("condition_on_observations_given_timing", "log_prob_of_observations_given_timing"):
        assert list(inspect.signature(getattr(MPInterface, new)).parameters) == \
            ["self", "times", "pos", "std", "vel", "vel_std", "phase_params"]
    for new in ("get_traj_pos_std_given_timing", "get_traj_vel_std_given_timing"):
        assert list(inspect.signature(getattr(MPInterface, new)).parameters) == ["self", "phase_params"]
    for new, old in (("condition_given_timing", "condition"), ("trajectory_log_prob_given_timing", "trajectory_log_prob")):
        assert str(inspect.signature(getattr(BatchedBlackBox, new))) == str(inspect.signature(getattr(BatchedBlackBox, old))), new


# ---- 2. the floor cannot make a bound vacuous; the dense formula is the sequential update --------------------------------------------------
def test_the_cases_are_the_ones_stated():
    cases = PP.gpu_cases()
    assert len(cases) == len(set(cases))
    shapes = {name: PP.shape(name) for name in PP.CONFIGS}
    assert [shapes[n][1] for n in PP.NS_NAMES] == [21, 110, 160]                 # NS = 1, 2, 3 rows per lane
    assert {c[1] for c in cases} == {1, 3, 9} and {c[0] for c in cases} == set(PP.CONFIGS)
    assert {c[2] for c in cases if c[0] == "tt_prodmp_70_steps"} == {1, 3, 32}
    assert {shapes[n][4] for n in PP.CONFIGS} >= {6, 70, 350}                    # one partial round, two rounds, six rounds of 64 steps
    assert (PP.LIMIT, 3, 5, 1e-3, False) in cases                                # Pl = 160 at M = 5 (conditioning)
    assert (PP.LIMIT, 3, 4, 1e-3, False) in cases and PP.n_obs(PP.LIMIT, 4, False) == 64      # Pl = 160 at n = 64 (likelihood)
    Kloc = shapes[PP.FREE][1] // shapes[PP.FREE][3]
    assert Kloc >= 9                                                             # the composition tests observe 4 exact values per DoF


@pytest.mark.parametrize("name,B,M,sigma,vel", PP.gpu_cases())
def test_the_floor_stays_below_the_cap_and_dense_is_sequential(name, B, M, sigma, vel):
    cs = PP.case(name, B, M, sigma, vel)
    what = f"{name} B={B} M={M} sigma={sigma} vel={vel}"
    PP.condition_floor_cap(cs, what)
    if cs["has_lp"]:
        LP.floor_cap(cs, what)
    PP.std_floor_cap(cs["ref_std"], cs["e32_std"], what)
    off = cs["off"]
    L64 = PP.tril64(cs["L"])
    for b in range(B):
        ob = PP.observations(cs["H"], cs["c"], b, cs["steps"], (cs["pos"], cs["vel"]))
        assert len(ob) == PP.n_obs(name, M, vel)
        assert [x[4] for x in ob] == sorted((x[4] for x in ob), key=lambda k: (k[1], k[0], k[2]))      # step, array, DoF
        mu_s, L_s = R.sequential(cs["mu"][b, off:].astype(np.float64), L64[b], ob)
        ref = dict(ref_mu=cs["ref_mu"][b:b + 1], ref_Sigma=cs["ref_Sigma"][b:b + 1], floor_mu=cs["floor_mu"][b:b + 1],
                   floor_Sigma=cs["floor_Sigma"][b:b + 1])
        # the float64 restatement against the dense formula: the bound of the GPU test on the episode's own arrays
        for g, r, fl in ((mu_s[None], ref["ref_mu"], ref["floor_mu"]), ((L_s @ L_s.T)[None], ref["ref_Sigma"], ref["floor_Sigma"])):
            assert not (np.abs(g - r) > R.bound(r, fl)).any(), what


# ---- 3. the two families' references agree -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PP.TIMING_NAMES + (PP.FREE,))
def test_the_point_likelihood_is_the_demonstration_likelihood_with_the_rest_at_infinity(name):
    cs = PP.case(name, 3, 3, 1e-3, False)
    P, Pl, off, D, T = PP.shape(name)
    B = cs["mu"].shape[0]
    Hd, cd = DP.rows(name, cs["mu"][:, :off], cs["ip"], cs["iv"])
    assert np.array_equal(Hd, cs["H"][0]) and np.array_equal(cd, cs["c"][0])     # Design's rows are the position Jacobian's
    pos = np.full((B, T, D), 1e6, np.float32)
    sd = np.full((B, T, D), np.inf, np.float32)
    pos[:, list(cs["steps"])] = cs["pos"][0]
    sd[:, list(cs["steps"])] = cs["pos"][1]
    demo = DP.log_prob_references(dict(H=Hd, c=cd, g=cs["g"], off=off, mu=cs["mu"], L=cs["L"], pos=pos, sd=sd))
    for k in ("ref_lp", "ref_gmu", "ref_gL", "n"):
        assert np.array_equal(demo[k], cs[k]), k                                 # the same observations in the same order: the same bits


@pytest.mark.parametrize("name", PP.NS_NAMES)
def test_the_std_reference_is_the_root_of_the_quadratic_form(name):
    cs = PP.case(name, 3, 3, 1e-3, True)
    L64 = PP.tril64(cs["L"])
    Sigma = np.einsum("bpj,bqj->bpq", L64, L64)
    for o in range(2):
        quad = np.einsum("btdp,bpq,btdq->btd", cs["H"][o], Sigma, cs["H"][o])
        assert np.allclose(np.sqrt(quad), cs["ref_std"][o], rtol=1e-9, atol=1e-12 * np.abs(cs["ref_std"][o]).max())
        assert (cs["ref_std"][o] >= 0).all()
    SR.check(cs["ref_std"], cs["ref_std"], cs["e32_std"], name)


# ---- 4. refusals that need no device ----------------------------------------------------------------------------------------------------------
def stub(mp_type="promp", learn_tau=True, learn_delay=False, D=2, P=7, T=10):
    return StubEngine(mp_type, D, T, P, learn_tau=learn_tau, learn_delay=learn_delay)


def test_the_new_methods_refuse_before_the_library_is_touched():
    eng = stub()
    mu, L = np.zeros((2, 7), np.float32), np.zeros((2, 6, 6), np.float32)
    y = np.zeros((2, 1, 2), np.float32)
    with pytest.raises(ValueError, match="condition_given_timing: .*learns neither tau nor delay"):
        stub(learn_tau=False).condition_given_timing(mu, L, [1], y, 0.1)
    with pytest.raises(ValueError, match="trajectory_std_given_timing: .*learns neither tau nor delay"):
        stub(learn_tau=False).trajectory_std_given_timing(mu, L)
    with pytest.raises(NotImplementedError, match="trajectory_log_prob_given_timing: a DMP"):
        stub(mp_type="dmp").trajectory_log_prob_given_timing(mu, L, [1], y, 0.1)
    with pytest.raises(ValueError, match=r"condition_given_timing: params_L must be \[2, Pl, Pl\] with Pl = 6"):
        eng.condition_given_timing(mu, np.zeros((2, 7, 7), np.float32), [1], y, 0.1)
    with pytest.raises(ValueError, match="trajectory_log_prob_vjp_given_timing: obs_pos and obs_std come in pairs"):
        eng.trajectory_log_prob_vjp_given_timing(np.ones(2), mu, L, [1], y, None)
    with pytest.raises(ValueError, match="trajectory_std_given_timing: pos and vel are both False"):
        eng.trajectory_std_given_timing(mu, L, pos=False, vel=False)
    with pytest.raises(ValueError, match="condition_given_timing: init_pos / init_vel may be None only for a ProMP"):
        stub(mp_type="prodmp").condition_given_timing(mu, L, [1], y, 0.1)
    # the plain methods keep refusing a learned-phase handle, in their present words
    with pytest.raises(NotImplementedError, match="condition: a learned tau / delay gives every episode its own phase"):
        eng.condition(np.zeros((2, 7), np.float32), np.zeros((2, 7, 7), np.float32), [1], y, 0.1)
    with pytest.raises(NotImplementedError, match="trajectory_std: a learned tau / delay"):
        eng.trajectory_std(np.zeros((2, 7, 7), np.float32))
