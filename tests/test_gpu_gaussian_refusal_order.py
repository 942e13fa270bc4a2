"""
Which refusal wins when a call of the probabilistic C entries (include/mpk.h: mpk_trajectory_std, mpk_trajectory_condition,
mpk_trajectory_log_prob / _vjp, mpk_demonstration_log_prob / _vjp, mpk_demonstration_condition / _plan and the mpk_demonstration_phase_*
four) is wrong in two ways, and under which entry's name it is refused.  The entries share their checks; the order the checks fire in
and the name each message starts with are part of what a caller sees.  Nothing here launches a kernel: every call is refused, and
``last_kernel()`` is what it was.  The smallest handles: D = 2, two basis functions, T = 4.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

STD = "mpk_trajectory_std"
COND = "mpk_trajectory_condition"
LP = "mpk_trajectory_log_prob"
LP_VJP = "mpk_trajectory_log_prob_vjp"
DLP = "mpk_demonstration_log_prob"
DLP_VJP = "mpk_demonstration_log_prob_vjp"
DCOND = "mpk_demonstration_condition"
DPLAN = "mpk_demonstration_condition_plan"
PLP = "mpk_demonstration_phase_log_prob"
PLP_VJP = "mpk_demonstration_phase_log_prob_vjp"
PCOND = "mpk_demonstration_phase_condition"
PPLAN = "mpk_demonstration_phase_plan"

POINTS = (COND, LP, LP_VJP)                                       # point observations at M shared steps
SHARED_DEMOS = (DLP, DLP_VJP, DCOND)                              # whole demonstrations, the handle's phase
PHASE_DEMOS = (PLP, PLP_VJP, PCOND)                               # whole demonstrations, a per-episode phase
VJPS = (LP_VJP, DLP_VJP, PLP_VJP)
SHARED = (STD,) + POINTS + SHARED_DEMOS + (DPLAN,)
# the word of the learned-phase refusal, by family
KERNEL_WORD = {STD: "a standard-deviation kernel", COND: "a conditioning kernel", LP: "a likelihood kernel", LP_VJP: "a likelihood kernel",
               DLP: "a likelihood kernel", DLP_VJP: "a likelihood kernel", DCOND: "a conditioning kernel", DPLAN: "a conditioning kernel"}
# the name the shape limits (a DMP, the DoF and column limits) refuse under: the gradient entries of the shared-phase routes and the
# shared-phase plan borrow their sibling's
LIMITS_NAME = {LP_VJP: LP, DLP_VJP: DLP, DPLAN: DCOND}


@pytest.fixture(scope="module")
def handles():
    from fancy_gym_amd import TrajectoryEngine
    kw = dict(dt=0.25, duration=1.0, tau=1.0)
    learned = dict(learn_tau=True, tau_bound=(0.5, 1.0))
    engs = dict(promp=TrajectoryEngine("promp", "linear", "rbf", 2, 2, **kw),
                prodmp=TrajectoryEngine("prodmp", "exp", "prodmp", 2, 2, **kw),
                prodmp_tau=TrajectoryEngine("prodmp", "exp", "prodmp", 2, 2, **kw, **learned),
                dmp=TrajectoryEngine("dmp", "exp", "rbf", 2, 2, **kw),
                dmp_tau=TrajectoryEngine("dmp", "exp", "rbf", 2, 2, **kw, **learned))
    assert all(e.num_steps == 4 and e.num_dof == 2 for e in engs.values())
    # every pointer a call passes is this buffer: a refusal that went missing would launch on memory that is there
    engs["buf"] = torch.zeros(1 << 18, device="cuda")
    return engs


def steps_of(values):
    return (C.c_int32 * len(values))(*values)


def raw(eng, buf, which, **kw):
    """the C entry ``which`` with every pointer valid, B = 1 and the steps (0, 1) observed in position, but for ``kw``"""
    ptr = buf.data_ptr()
    a = dict(params=ptr, L=ptr, ip=ptr, iv=ptr, steps=steps_of((0, 1)), M=2, obs_pos=ptr, obs_pos_std=ptr, obs_vel=None, obs_vel_std=None,
             pos=ptr, sd=ptr, out=ptr, out2=ptr, g=ptr, B=1)
    a.update(kw)
    stream = torch.cuda.current_stream().cuda_stream
    entry = getattr(eng._lib, which)
    head = (eng._h, a["params"], a["L"], a["ip"], a["iv"], 0.0)
    points = head + (a["steps"], a["M"], a["obs_pos"], a["obs_pos_std"], a["obs_vel"], a["obs_vel_std"])
    demos = head + (a["pos"], a["sd"])
    if which == STD:
        return entry(eng._h, a["L"], 0.0, a["out"], a["out2"], a["B"], stream)
    if which in (DPLAN, PPLAN):
        return entry(eng._h, a["B"], None, None, None)
    if which == COND:
        return entry(*points, a["out"], a["out2"], a["B"], stream)
    if which == LP:
        return entry(*points, a["out"], a["B"], stream)
    if which == LP_VJP:
        return entry(*points, a["g"], a["out"], a["out2"], a["B"], stream)
    if which in (DLP, PLP):
        return entry(*demos, a["out"], a["B"], stream)
    if which in (DLP_VJP, PLP_VJP):
        return entry(*demos, a["g"], a["out"], a["out2"], a["B"], stream)
    assert which in (DCOND, PCOND), which
    return entry(*demos, a["out"], a["out2"], a["B"], stream)


def refused(handles, key, which, code, word, name=None, **kw):
    """the call is refused with ``code``, the message starts with the entry's name (``name``: the sibling's it borrows) and holds
    ``word``, and nothing was launched"""
    from fancy_gym_amd import _lib
    eng = handles[key]
    before = eng.last_kernel()
    rc = raw(eng, handles["buf"], which, **kw)
    msg = _lib.last_error()
    assert rc == code, (which, key, kw, rc, msg)
    assert msg.startswith((name or which) + ": "), (which, key, kw, msg)
    assert word in msg, (which, key, kw, msg)
    assert eng.last_kernel() == before, (which, key, kw)


def handle_of(which):
    return "prodmp_tau" if which in PHASE_DEMOS + (PPLAN,) else "prodmp"


@pytest.mark.parametrize("which", (STD,) + POINTS + SHARED_DEMOS + PHASE_DEMOS)
def test_null_params_win_over_an_empty_batch(handles, which):
    from fancy_gym_amd import _lib
    word = {STD: "NULL params_L", COND: "NULL params, params_L, params_out or params_L_out", DCOND: "NULL params or params_L, in or out",
            PCOND: "NULL params or params_L, in or out"}.get(which, "NULL params or params_L")
    for key in ("promp", handle_of(which)) if which not in PHASE_DEMOS else (handle_of(which),):
        refused(handles, key, which, _lib.MPK_EINVAL, which + ": " + word, params=None, L=None, B=0)


@pytest.mark.parametrize("which", SHARED + PHASE_DEMOS + (PPLAN,))
def test_an_empty_batch_wins_over_no_observed_steps(handles, which):
    from fancy_gym_amd import _lib
    refused(handles, handle_of(which), which, _lib.MPK_EINVAL, "B must be >= 1", B=0, M=0, steps=None)


@pytest.mark.parametrize("which", POINTS)
def test_the_step_count_and_the_steps_win_over_what_is_observed(handles, which):
    from fancy_gym_amd import _lib
    for key in ("promp", "prodmp"):
        refused(handles, key, which, _lib.MPK_EINVAL, "M must be 1..32", M=33, steps=steps_of(range(33)), obs_pos_std=None)
        refused(handles, key, which, _lib.MPK_EINVAL, "strictly increasing", steps=steps_of((1, 1)), obs_pos=None, obs_pos_std=None)


@pytest.mark.parametrize("which", POINTS)
def test_values_without_standard_deviations_win_over_a_learned_phase(handles, which):
    from fancy_gym_amd import _lib
    refused(handles, "prodmp_tau", which, _lib.MPK_EINVAL, "in pairs", obs_pos_std=None)


@pytest.mark.parametrize("which", SHARED)
def test_a_learned_phase_wins_over_a_dmp(handles, which):
    from fancy_gym_amd import _lib
    refused(handles, "dmp_tau", which, _lib.MPK_ENOTIMPL, "only shared-phase handles have " + KERNEL_WORD[which])


@pytest.mark.parametrize("which", SHARED + PHASE_DEMOS + (PPLAN,))
def test_a_dmp_wins_over_a_missing_start(handles, which):
    from fancy_gym_amd import _lib
    key = "dmp_tau" if which in PHASE_DEMOS + (PPLAN,) else "dmp"
    refused(handles, key, which, _lib.MPK_ENOTIMPL, "DMP has no probabilistic interface", name=LIMITS_NAME.get(which), ip=None)


@pytest.mark.parametrize("which", PHASE_DEMOS + (PPLAN,))
def test_a_shared_phase_wins_over_a_missing_start(handles, which):
    from fancy_gym_amd import _lib
    for key in ("promp", "prodmp", "dmp"):
        refused(handles, key, which, _lib.MPK_ENOTIMPL, "learns neither tau nor delay", ip=None)


@pytest.mark.parametrize("which", VJPS)
def test_a_missing_g_wins_over_no_gradient_asked_for(handles, which):
    from fancy_gym_amd import _lib
    refused(handles, handle_of(which), which, _lib.MPK_EINVAL, "NULL g", g=None, out=None, out2=None)
