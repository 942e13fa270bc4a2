"""
GPU tests of the demonstration entry points with a per-episode phase: TrajectoryEngine.demonstration_log_prob_given_timing,
demonstration_log_prob_vjp_given_timing, condition_on_demonstration_given_timing (mpk_demonstration_phase_log_prob / _vjp / _condition:
k_demo_log_prob<.., phase[, grad]>, k_demo_condition<.., phase>) on handles that learn tau and / or delay.

The reference, the bounds and the cases are tests/demonstration_phase_ref.py's: per episode the float64 CPU oracle at that episode's own
tau / delay, the DENSE formulas over the kept entries, the project's 1e-5 rules with the float32-table floor.
tests/test_demo_phase_host.py checks the floor cap and the information form's algebra on every case without a GPU.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from . import demonstration_phase_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def mp_of(name):
    return PR.cfg(name)[2].trajectory_generator_type


def inits(name, cs):
    """a ProMP takes None where its basis has no init_pos column to show that it may; everything else its initial conditions"""
    if mp_of(name) == "promp" and PR.cfg(name)[1].basis_generator_type != "zero_rbf":
        return None, None
    return dev(cs["ip"]), dev(cs["iv"])


def pick(cs, **kw):
    return [kw.get(k, None) if kw.get(k, None) is not None else dev(cs[k]) for k in ("mu", "L", "pos", "sd")]


def log_prob(eng, name, cs, **kw):
    return eng.demonstration_log_prob_given_timing(*pick(cs, **kw), *inits(name, cs))


def vjp(eng, name, cs, **kw):
    return eng.demonstration_log_prob_vjp_given_timing(dev(cs["g"]), *pick(cs, **kw), *inits(name, cs))


def condition(eng, name, cs, out=None, **kw):
    return eng.condition_on_demonstration_given_timing(*pick(cs, **kw), *inits(name, cs), out=out)


def episodes(cs, rows):
    B = cs["mu"].shape[0]
    return {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in cs.items()}


def upper(P):
    return dev(np.triu(np.ones((P, P), bool), 1))


# ---- 1. parity of the likelihood and its gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,sigma,missing", PR.gpu_cases())
def test_log_prob_and_gradients_match_the_dense_formula(name, B, sigma, missing):
    eng = PR.engine_for(name)
    cs = PR.log_prob_case(name, B, sigma, missing)
    what = f"{name} B={B} sigma={sigma} missing={missing}"
    mu = dev(cs["mu"]).requires_grad_(True)
    L = dev(cs["L"]).requires_grad_(True)
    lp = eng.demonstration_log_prob_given_timing(mu, L, dev(cs["pos"]), dev(cs["sd"]), *inits(name, cs))
    assert eng.last_kernel() == f"k_demo_log_prob<{mp_of(name)}, phase>", eng.last_kernel()
    assert lp.dtype == torch.float64 and lp.shape == (B,)
    (lp * dev(cs["g"])).sum().backward()                                           # ONE backward launch
    assert eng.last_kernel() == f"k_demo_log_prob<{mp_of(name)}, phase, grad>", eng.last_kernel()
    PR.check_log_prob((lp, mu.grad, L.grad), cs, what + " autograd")
    g_mu, g_L = vjp(eng, name, cs)
    assert same((g_mu, g_L), (mu.grad, L.grad))
    assert same((lp.detach(),), (log_prob(eng, name, cs),))
    eng.check_range()                                                              # the tables' range covers the clipped timings


# ---- 2. parity of the posterior -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,sigma,missing", PR.gpu_cases())
def test_posterior_matches_the_dense_batch_formula(name, B, sigma, missing):
    eng = PR.engine_for(name)
    cs = PR.condition_case(name, B, sigma, missing)
    mu, L = condition(eng, name, cs)
    assert eng.last_kernel() == f"k_demo_condition<{mp_of(name)}, phase>", eng.last_kernel()
    assert mu.shape == cs["mu"].shape and L.shape == cs["L"].shape and mu.dtype == L.dtype == torch.float32
    PR.check_condition(mu, L, cs, f"{name} B={B} sigma={sigma} missing={missing}")
    assert not bits(L[:, upper(L.shape[1])]).any()                                 # exact zero bits
    eng.check_range()


# ---- 3. composition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,missing", [(0.1, True), (1e-3, False)])
@pytest.mark.parametrize("name", ["tt_prodmp_70_steps", "promp_zero_12_basis_3_dof", PR.LIMIT])
def test_a_prefix_and_then_the_rest_are_the_whole(name, sigma, missing):
    """conditioning on a prefix and then on the rest is conditioning on the whole (the intermediate posterior passes through float32 once:
    inside the bound of the whole), and log p(prefix) under the prior + log p(rest) under the prefix's posterior = log p(whole)"""
    eng = PR.engine_for(name)
    B = 3
    cs = dict(PR.condition_case(name, B, sigma, missing))
    cs.update(PR.log_prob_case(name, B, sigma, missing))
    T = cs["pos"].shape[1]
    cut = (2 * T) // 5
    first, rest = cs["sd"].copy(), cs["sd"].copy()
    first[:, cut:] = np.inf
    rest[:, :cut] = np.inf
    one = condition(eng, name, cs)
    mid = condition(eng, name, cs, sd=dev(first))
    two = condition(eng, name, cs, sd=dev(rest), mu=mid[0], L=mid[1])
    PR.check_condition(one[0], one[1], cs, f"{name} sigma={sigma} one call")
    PR.check_condition(two[0], two[1], cs, f"{name} sigma={sigma} prefix of {cut} steps, then the rest")
    whole = log_prob(eng, name, cs)
    chain = log_prob(eng, name, cs, sd=dev(first)) + log_prob(eng, name, cs, sd=dev(rest), mu=mid[0], L=mid[1])
    tol = PR.bounds(cs)[0]
    err = (chain - whole).abs().cpu().numpy()
    print(f"[demo-phase] {name} sigma={sigma}: chain rule across step {cut}: max err {err.max():.3e}  bound {np.min(tol):.3e}")
    PR.check_log_prob((whole, None, None), cs, f"{name} sigma={sigma} whole")
    assert not (err > tol).any()


# ---- 4. the timing matters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beerpong_promp", "tt_prodmp_70_steps"])
def test_a_wrong_tau_scores_differently(name):
    """every episode's tau replaced by the batch mean: the scores leave the right-tau scores by more than the bound, which a kernel that
    read one shared table could not do (the episodes differ in nothing but what the timing does to their rows)"""
    eng = PR.engine_for(name)
    B = 9
    cs = PR.log_prob_case(name, B, 1e-2, False)
    right = log_prob(eng, name, cs)
    PR.check_log_prob((right, None, None), cs, f"{name} right tau")
    mu = cs["mu"].copy()
    mu[:, 0] = mu[:, 0].mean()
    wrong = log_prob(eng, name, cs, mu=dev(mu))
    tol = PR.bounds(cs)[0]
    diff = (wrong - right).abs().cpu().numpy()
    inside = np.arange(B) % 3 == 1                                                 # (an episode outside the bounds may clip to the same tau)
    print(f"[demo-phase] {name}: |wrong tau - right tau| {diff}  bound {tol}")
    assert (diff[inside] > 10.0 * np.max(tol)).all()
    # and the same demonstrations under two handles' worth of timing are two different posteriors
    a, b = condition(eng, name, cs), condition(eng, name, cs, mu=dev(mu))
    assert not torch.equal(bits(a[0][1, 1:]), bits(b[0][1, 1:]))


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tt_prodmp_70_steps", "promp_zero_12_basis_3_dof", "prodmp_13_basis_1_dof_no_goal"])
def test_edges(name):
    eng = PR.engine_for(name)
    B = 3
    cs = PR.inputs(name, B, 0.1, True)
    P, Pl, off, D, T = PR.shape(name)
    up = upper(Pl)
    lower = ~up
    mu0, L0 = dev(cs["mu"]), dev(cs["L"])
    lp, (g_mu, g_L), post = log_prob(eng, name, cs), vjp(eng, name, cs), condition(eng, name, cs)
    assert torch.isfinite(lp).all() and torch.isfinite(g_mu).all() and torch.isfinite(g_L).all() and torch.isfinite(post[0]).all()
    # the factor's strict upper triangle is NaN in the case and never read: finite values there change no bit
    Lf = torch.tril(torch.nan_to_num(L0))
    assert same((lp,), (log_prob(eng, name, cs, L=Lf),)) and same(post, condition(eng, name, cs, L=Lf))
    # nothing kept in episode 1 (inf, NaN, negative): 0.0, zero gradients, the prior's bits; the neighbours as before
    bad = np.array([np.inf, np.nan, -1.0], np.float32)
    sd = cs["sd"].copy()
    sd[1] = bad[np.arange(sd[1].size) % 3].reshape(sd[1].shape)
    lp1, (gm1, gL1), post1 = log_prob(eng, name, cs, sd=dev(sd)), vjp(eng, name, cs, sd=dev(sd)), condition(eng, name, cs, sd=dev(sd))
    assert bits(lp1[1]).item() == 0 and not bits(gm1[1]).any() and not bits(gL1[1]).any()
    assert torch.equal(bits(post1[0][1]), bits(mu0[1])) and torch.equal(bits(post1[1][1][lower]), bits(L0[1][lower]))
    assert not bits(post1[1][1][up]).any()
    for b in (0, 2):
        assert same((lp1[b], gm1[b], gL1[b], post1[0][b], post1[1][b]), (lp[b], g_mu[b], g_L[b], post[0][b], post[1][b])), b
    # one DoF with nothing kept: its rows of g_params_L are exact zeros, its block of the mean moves only through the prior's correlation
    sdd = cs["sd"].copy()
    sdd[:, :, D - 1] = np.inf
    ref = PR.log_prob_references(cs, sd=sdd)
    ref["off"] = off
    gmd, gLd = vjp(eng, name, cs, sd=dev(sdd))
    PR.check_log_prob((log_prob(eng, name, cs, sd=dev(sdd)), gmd, gLd), ref, f"{name} the last DoF unobserved")
    if D > 1:
        K = Pl // D
        assert not bits(gLd[:, (D - 1) * K:]).any() and not bits(gmd[:, off + (D - 1) * K:]).any()
    refc = PR.condition_references(cs, sd=sdd)
    refc.update(off=off, mu=cs["mu"])
    PR.check_condition(*condition(eng, name, cs, sd=dev(sdd)), refc, f"{name} the last DoF unobserved")
    # a sigma == 0 in episode 1: NaN there and nowhere else
    sd0 = cs["sd"].copy()
    sd0[1, 5 % T, D - 1] = 0.0
    lp0, (gm0, gL0), post0 = log_prob(eng, name, cs, sd=dev(sd0)), vjp(eng, name, cs, sd=dev(sd0)), condition(eng, name, cs, sd=dev(sd0))
    assert torch.isnan(lp0[1]) and torch.isnan(gm0[1, off:]).all() and not bits(gm0[1, :off]).any()
    assert torch.isnan(gL0[1][lower]).all() and not bits(gL0[1][up]).any()
    assert torch.isnan(post0[0][1, off:]).all() and torch.equal(bits(post0[0][1, :off]), bits(mu0[1, :off]))
    assert torch.isnan(post0[1][1][lower]).all() and not bits(post0[1][1][up]).any()
    for b in (0, 2):
        assert same((lp0[b], gm0[b], gL0[b], post0[0][b], post0[1][b]), (lp[b], g_mu[b], g_L[b], post[0][b], post[1][b])), b
    # a NaN in a kept pos of episode 1, and a NaN in the lower triangle of its factor: inside the episode
    y = cs["pos"].copy()
    sdk = cs["sd"].copy()
    y[1, 7 % T, 0], sdk[1, 7 % T, 0] = np.nan, 0.1
    Ln = cs["L"].copy()
    Ln[1, Pl - 1, 0] = np.nan
    for kw in (dict(pos=dev(y), sd=dev(sdk)), dict(L=dev(Ln))):
        lpn, (gmn, gLn), postn = log_prob(eng, name, cs, **kw), vjp(eng, name, cs, **kw), condition(eng, name, cs, **kw)
        assert torch.isnan(lpn[1]) and torch.isnan(postn[0][1, off:]).all() and torch.isnan(gmn[1, off:]).all()
        assert torch.equal(bits(postn[0][1, :off]), bits(mu0[1, :off])) and not bits(gmn[1, :off]).any()
        for b in (0, 2):
            assert same((lpn[b], gmn[b], gLn[b], postn[0][b], postn[1][b]), (lp[b], g_mu[b], g_L[b], post[0][b], post[1][b])), b


@pytest.mark.parametrize("name", ["tt_prodmp_70_steps", "beerpong_promp", "promp_10_basis_11_dof"])
def test_determinism_alignment_permutation_and_in_place(name):
    eng = PR.engine_for(name)
    B = 9
    cs = PR.inputs(name, B, 0.1, True)
    first = (log_prob(eng, name, cs), *vjp(eng, name, cs), *condition(eng, name, cs))
    again = (log_prob(eng, name, cs), *vjp(eng, name, cs), *condition(eng, name, cs))
    assert same(first, again)                                                      # two launches: equal bits
    # views offset by 1, 2, 3 floats into larger buffers
    for shift in (1, 2, 3):
        def view(x):
            buf = torch.empty(x.numel() + 4, dtype=x.dtype, device="cuda")
            v = buf[shift:shift + x.numel()].view(x.shape)
            v.copy_(x)
            return v
        kw = {k: view(dev(cs[k])) for k in ("mu", "L", "pos", "sd")}
        assert all(v.data_ptr() % 16 != 0 and v.is_contiguous() for v in kw.values())
        assert same(first, (log_prob(eng, name, cs, **kw), *vjp(eng, name, cs, **kw), *condition(eng, name, cs, **kw))), shift
    # permuting the batch permutes the result
    perm = np.random.default_rng(3).permutation(B)
    pc = episodes(cs, perm)
    moved = (log_prob(eng, name, pc), *vjp(eng, name, pc), *condition(eng, name, pc))
    idx = dev(perm)
    assert same(moved, tuple(x[idx] for x in first))
    # alone or in the batch
    alone = episodes(cs, slice(4, 5))
    assert same((log_prob(eng, name, alone), *condition(eng, name, alone)), (first[0][4:5], first[3][4:5], first[4][4:5]))
    # in place: the outputs are the inputs
    mu, L = dev(cs["mu"]).clone(), dev(cs["L"]).clone()
    got = condition(eng, name, cs, mu=mu, L=L, out=(mu, L))
    assert got[0].data_ptr() == mu.data_ptr() and got[1].data_ptr() == L.data_ptr() and same((mu, L), first[3:])


def test_a_wave_takes_a_second_episode():
    """B from the launch plan at the smallest Pl of the table: the episodes past workgroups x waves are a second trip of a wave's loop"""
    name = min(PR.TABLE, key=lambda n: PR.shape(n)[1])
    assert name == "prodmp_13_basis_1_dof_no_goal"
    eng = PR.engine_for(name)
    blocks, waves, lds = eng.condition_on_demonstration_plan(1 << 20, timing="given")
    B = blocks * waves + 5
    assert eng.condition_on_demonstration_plan(B, timing="given") == (blocks, waves, lds) and 0 < lds <= 163840
    print(f"[demo-phase] {name}: B = {B} -> {blocks} workgroups x {waves} waves, {lds} bytes of LDS")
    base = PR.inputs(name, 9, 0.1, True)
    cs = {k: (np.ascontiguousarray(np.resize(v, (B,) + v.shape[1:])) if isinstance(v, np.ndarray) and v.shape[:1] == (9,) else v)
          for k, v in base.items()}
    first = (log_prob(eng, name, cs), *vjp(eng, name, cs), *condition(eng, name, cs))
    assert all(torch.isfinite(x).all() for x in first)
    tail = episodes(cs, slice(B - 5, B))
    assert same(tuple(x[B - 5:] for x in first), (log_prob(eng, name, tail), *vjp(eng, name, tail), *condition(eng, name, tail)))
    ref = PR.log_prob_references(dict(tail, g=tail["g"]))
    ref["off"] = tail["off"]
    PR.check_log_prob(tuple(x[B - 5:] for x in first[:3]), ref, f"{name} the last five of {B}")


def test_a_prodmp_timing_beyond_the_precomputed_range_is_reported():
    from oracle import mp_oracle as O
    from .test_gpu_trajectory import make_engine
    # tau may go down to 0.05 on a table pre-computed for the scaled time up to pre_compute_length_factor: 0.6 / 0.05 = 12 is beyond it
    pc = O.PhaseCfg("exp", tau=0.6, alpha_phase=3.0, learn_tau=True, tau_bound=(0.05, 0.6))
    eng = make_engine(pc, O.BasisCfg("prodmp", num_basis=4, alpha=15), O.TrajCfg("prodmp", action_dim=2), 0.02, 0.6)
    P, T = eng.num_params, eng.num_steps
    B = 3
    mu = torch.zeros((B, P), device="cuda")
    mu[:, 0] = torch.tensor([0.6, 0.05, 0.6])
    L = torch.eye(P - 1, device="cuda").expand(B, -1, -1).contiguous()
    y, z = torch.zeros((B, T, 2), device="cuda"), torch.zeros((B, 2), device="cuda")
    eng.demonstration_log_prob_given_timing(mu[:1], L[:1], y[:1], 0.1, z[:1], z[:1])
    eng.check_range()
    for call in (lambda: eng.demonstration_log_prob_given_timing(mu, L, y, 0.1, z, z),
                 lambda: eng.demonstration_log_prob_vjp_given_timing(torch.ones(B, dtype=torch.float64), mu, L, y, 0.1, z, z),
                 lambda: eng.condition_on_demonstration_given_timing(mu, L, y, 0.1, z, z)):
        call()
        with pytest.raises(RuntimeError):
            eng.check_range()
        eng.check_range()                                                          # the flag was cleared


# ---- 6. refusals, all before any launch ------------------------------------------------------------------------------------------------------
def test_refusals_of_the_python_layer_and_of_the_c_entries():
    from fancy_gym_amd import _lib
    from .test_gpu_trajectory import CFG3, make_engine
    from .test_gpu_traj_fit import phase_engine
    stream = torch.cuda.current_stream().cuda_stream
    ptr = torch.zeros(1 << 18, device="cuda").data_ptr()

    def raw(eng, which, B=1, **kw):
        a = dict(params=ptr, L=ptr, ip=ptr, iv=ptr, pos=ptr, sd=ptr, out=ptr, out2=ptr)
        a.update(kw)
        lib = eng._lib
        if which == "mpk_demonstration_phase_log_prob":
            return lib.mpk_demonstration_phase_log_prob(eng._h, a["params"], a["L"], a["ip"], a["iv"], 0.0, a["pos"], a["sd"], a["out"], B,
                                                        stream)
        if which == "mpk_demonstration_phase_log_prob_vjp":
            return lib.mpk_demonstration_phase_log_prob_vjp(eng._h, a["params"], a["L"], a["ip"], a["iv"], 0.0, a["pos"], a["sd"], ptr,
                                                            a["out"], a["out2"], B, stream)
        if which == "mpk_demonstration_phase_condition":
            return lib.mpk_demonstration_phase_condition(eng._h, a["params"], a["L"], a["ip"], a["iv"], 0.0, a["pos"], a["sd"], a["out"],
                                                         a["out2"], B, stream)
        return lib.mpk_demonstration_phase_plan(eng._h, B, None, None, None)

    entries = ("mpk_demonstration_phase_log_prob", "mpk_demonstration_phase_log_prob_vjp", "mpk_demonstration_phase_condition",
               "mpk_demonstration_phase_plan")

    def refused(eng, word):
        before = eng.last_kernel()
        for which in entries:
            assert raw(eng, which) == _lib.MPK_ENOTIMPL and word in _lib.last_error(), (which, _lib.last_error())
            assert which in _lib.last_error()
        assert eng.last_kernel() == before                                         # nothing was launched

    shared = PR.R.engine_for("cfg2_prodmp")
    refused(shared, "learns neither tau nor delay")
    z7 = torch.zeros((1, 7), device="cuda")
    with pytest.raises(ValueError, match="learns neither tau nor delay"):
        shared.demonstration_log_prob_given_timing(torch.zeros((1, 42)), torch.zeros((1, 42, 42)), torch.zeros((1, shared.num_steps, 7)),
                                                   0.1, z7, z7)
    from oracle import mp_oracle as O
    dmp = make_engine(O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0, learn_tau=True, tau_bound=(0.5, 1.0)), *CFG3[1:])
    refused(dmp, "DMP has no probabilistic interface")
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        dmp.condition_on_demonstration_given_timing(torch.zeros((1, dmp.num_params)), torch.zeros((1, 1, 1)),
                                                    torch.zeros((1, dmp.num_steps, dmp.num_dof)), 0.1)
    for name, Pl in zip(PR.OVER_LIMIT, (224, 256)):                               # over the LDS limit
        eng = phase_engine(name)
        refused(eng, "do not fit the CU's 163840 bytes of LDS")
        P, D, T = eng.num_params, eng.num_dof, eng.num_steps
        z = torch.zeros((1, D), device="cuda")
        with pytest.raises(NotImplementedError, match=f"{Pl} parameters .* do not fit the CU's"):
            eng.demonstration_log_prob_given_timing(torch.zeros((1, P)), torch.zeros((1, Pl, Pl)), torch.zeros((1, T, D)), 0.1, z, z)
        with pytest.raises(NotImplementedError, match="do not fit the CU's"):
            eng.condition_on_demonstration_plan(1, timing="given")
    wide = PR.engine_for("promp_17_dof")
    refused(wide, "at most 16 DoF and 16 table columns")
    with pytest.raises(NotImplementedError, match="at most 16 DoF"):
        wide.demonstration_log_prob_given_timing(torch.zeros((1, 35)), torch.zeros((1, 34, 34)), torch.zeros((1, wide.num_steps, 17)), 0.1)
    # the limit shape has a plan
    blocks, waves, lds = PR.engine_for(PR.LIMIT).condition_on_demonstration_plan(7, timing="given")
    assert blocks * waves >= 7 and waves == 1 and 0 < lds <= 163840
    # the arguments, on a handle that runs
    name = "tt_prodmp_70_steps"
    eng = PR.engine_for(name)
    before = eng.last_kernel()
    for which in entries[:3]:
        for kw, word in ((dict(params=None), "NULL params"), (dict(L=None), "NULL params"), (dict(pos=None), "NULL pos or obs_std"),
                         (dict(sd=None), "NULL pos or obs_std"), (dict(ip=None), "init_pos and init_vel"),
                         (dict(iv=None), "init_pos and init_vel"), (dict(B=0), "B must be >= 1")):
            assert raw(eng, which, **kw) == _lib.MPK_EINVAL and word in _lib.last_error(), (which, kw, _lib.last_error())
    assert raw(eng, entries[3], B=0) == _lib.MPK_EINVAL
    cs = PR.inputs(name, 3, 0.1, True)
    P, Pl, off, D, T = PR.shape(name)
    ip, iv = dev(cs["ip"]), dev(cs["iv"])
    with pytest.raises(ValueError, match=f"Pl = {Pl}"):
        eng.demonstration_log_prob_given_timing(dev(cs["mu"]), torch.zeros((3, P, P)), dev(cs["pos"]), 0.1, ip, iv)
    with pytest.raises(ValueError, match="init_pos / init_vel may be None only for a ProMP"):
        eng.condition_on_demonstration_given_timing(dev(cs["mu"]), dev(cs["L"]), dev(cs["pos"]), 0.1)
    with pytest.raises(ValueError, match=rf"out\[1\] must be a contiguous float32 tensor of shape \(3, {Pl}, {Pl}\)"):
        eng.condition_on_demonstration_given_timing(dev(cs["mu"]), dev(cs["L"]), dev(cs["pos"]), 0.1, ip, iv,
                                                    out=(torch.empty((3, P), device="cuda"), torch.empty((3, P, P), device="cuda")))
    for k in ("pos", "sd", "ip"):
        args = dict(pos=dev(cs["pos"]), sd=dev(cs["sd"]), ip=ip.clone())
        args[k].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="requires grad"):
            eng.demonstration_log_prob_given_timing(dev(cs["mu"]), dev(cs["L"]), args["pos"], args["sd"], args["ip"], iv)
    # without the opt-in the handle refuses as before
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        eng.demonstration_log_prob(dev(cs["mu"]), dev(cs["L"]), dev(cs["pos"]), 0.1, ip, iv)
    assert eng.last_kernel() == before


# ---- 7. the thin callers ---------------------------------------------------------------------------------------------------------------------
def test_the_generator_calls_are_the_engine_calls():
    from fancy_gym_amd.black_box.factory import get_basis_generator, get_phase_generator, get_trajectory_generator
    D, N = 3, 4
    pg = get_phase_generator("linear", tau=1.0, learn_tau=True, tau_bound=(0.5, 1.0))
    gen = get_trajectory_generator("promp", D, get_basis_generator("rbf", pg, num_basis=4))
    gen.set_duration(1.0, 0.02)
    P = gen.num_params
    Pl = P - 1
    rng = np.random.default_rng(71)
    p0 = np.concatenate([[0.8], rng.standard_normal(Pl)]).astype(np.float32)
    L0 = PR.random_factor(Pl, 1, seed=72)[0]
    gen.set_params(p0)
    gen.set_initial_conditions(0.0, np.zeros(D, np.float32), np.zeros(D, np.float32))
    gen.set_mp_params_variances(L0)
    eng = gen.engine()
    T = eng.num_steps
    y = rng.standard_normal((N, T, D)).astype(np.float32)
    std = np.full((T, D), 0.05, np.float32)
    std[(2 * T) // 5:] = np.inf
    taus = np.array([[0.6], [0.7], [0.8], [1.2]], np.float32)
    z = torch.zeros((N, D), device="cuda")
    for ph in (None, taus):
        rows = np.repeat(p0[None], N, 0)
        if ph is not None:
            rows[:, :1] = ph
        lp = gen.log_prob_of_trajectories_given_timing(y, std, phase_params=ph)
        assert eng.last_kernel() == "k_demo_log_prob<promp, phase>" and lp.device.type == "cpu"
        want = eng.demonstration_log_prob_given_timing(dev(rows), dev(np.repeat(L0[None], N, 0)), dev(y), dev(std), z, z, 0.0)
        assert same((lp,), (want.cpu(),))
        mean, L = gen.condition_on_trajectories_given_timing(y, std, phase_params=ph)
        assert eng.last_kernel() == "k_demo_condition<promp, phase>"
        wantc = eng.condition_on_demonstration_given_timing(dev(rows), dev(np.repeat(L0[None], N, 0)), dev(y), dev(std), z, z, 0.0)
        assert same((mean, L), (wantc[0].cpu(), wantc[1].cpu())) and np.array_equal(mean[:, :1].numpy(), rows[:, :1])
    with pytest.raises(NotImplementedError, match="learns tau / delay"):
        gen.log_prob_of_trajectories(y, std)
    with pytest.raises(ValueError, match=r"phase_params must be \[4, 1\]"):
        gen.condition_on_trajectories_given_timing(y, std, phase_params=taus[:2])


def test_the_black_box_calls_are_the_engine_calls():
    from fancy_gym_amd import BatchedBlackBox
    from fancy_gym_amd.black_box.factory import get_basis_generator, get_controller, get_phase_generator, get_trajectory_generator
    B, D = 5, 7
    pg_, dg_ = 0.01 * np.array([120., 120., 120., 120., 50., 30., 10.]), 0.01 * np.array([10., 10., 10., 10., 6., 5., 3.])
    phase = get_phase_generator("exp", tau=1.5, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.5, 1.5),
                                delay_bound=(0.0, 0.2))
    basis = get_basis_generator("prodmp", phase, num_basis=3, basis_bandwidth_factor=2, alpha=10)
    tg = get_trajectory_generator("prodmp", D, basis)
    bb = BatchedBlackBox(tg, get_controller("motor", p_gains=pg_, d_gains=dg_), B, 0.02, 1.0, act_low=-1.0, act_high=1.0,
                         plant="double_integrator")
    gen = torch.Generator().manual_seed(3)
    q0 = (torch.rand((B, D), generator=gen, dtype=torch.float64) - 0.5).cuda()
    bb.reset(q0)
    P, T = bb.engine.num_params, bb.engine.num_steps
    Pl = P - 2
    mu = torch.randn((B, P), generator=gen)
    mu[:, 0], mu[:, 1] = torch.linspace(0.4, 1.6, B), torch.linspace(-0.05, 0.25, B)
    mu = mu.cuda()
    L = dev(PR.random_factor(Pl, B, seed=5))
    zero = torch.zeros((B, D), device="cuda")
    y = bb.engine.trajectory(mu, q0.float(), zero, 0.0)[0] + 0.05 * torch.randn((B, T, D), generator=gen).cuda()
    sd = torch.full((T, D), 0.05)
    sd[T // 2:] = float("inf")
    lp = bb.demonstration_log_prob_given_timing(mu, L, y, sd)
    assert bb.engine.last_kernel() == "k_demo_log_prob<prodmp, phase>"
    assert same((lp,), (bb.engine.demonstration_log_prob_given_timing(mu, L, y, sd, q0.float(), zero, 0.0),))
    post = bb.condition_on_demonstration_given_timing(mu, L, y, sd)
    assert bb.engine.last_kernel() == "k_demo_condition<prodmp, phase>"
    want = bb.engine.condition_on_demonstration_given_timing(mu, L, y, sd, q0.float(), zero, 0.0)
    assert same(post, want) and torch.equal(bits(post[0][:, :2]), bits(mu[:, :2]))
    out = (torch.empty_like(post[0]), torch.empty_like(post[1]))
    got = bb.condition_on_demonstration_given_timing(mu, L, y, sd, out=out)
    assert got[0] is out[0] and same(out, want)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        bb.demonstration_log_prob(mu, L, y, sd)


# ---- 8. the example --------------------------------------------------------------------------------------------------------------------------
def test_the_example_at_a_reduced_size():
    path = os.path.join(ROOT, "examples", "batched_promp_time_aligned.py")
    spec = importlib.util.spec_from_file_location("batched_promp_time_aligned", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lls, held, held_forced, err_prior, err_post, inside = mod.run(demos=64, iters=5, verbose=False, held_out=16, samples=32)
    print(f"[demo-phase] example: mean log-likelihood per iteration {['%.3f' % x for x in lls]}; held-out mean log-likelihood {held:.3f} at "
          f"each demonstration's own tau, {held_forced:.3f} forced to the mean tau; held-out rest, rms error of the prior mean "
          f"{err_prior:.4f}, of the posterior mean {err_post:.4f}, {100 * inside:.1f} % inside 3 predicted std")
    assert np.isfinite(lls).all() and all(b >= a for a, b in zip(lls, lls[1:])) and lls[-1] > lls[0]
    assert np.isfinite([held, held_forced]).all() and held > held_forced
    assert err_post < err_prior
