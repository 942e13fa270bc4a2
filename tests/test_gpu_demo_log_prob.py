"""
mpk_demonstration_log_prob / mpk_demonstration_log_prob_vjp on the GPU: the log-likelihood of whole demonstrations [B, T, D] under a
Gaussian over the MP parameters, evaluated in the information (Pl x Pl) form, and its gradient w.r.t. the mean and the factor.

Yardstick: the DENSE n x n formula in float64 numpy per episode and float64 torch autograd of it on the CPU, rows from the float64
Jacobian of the CPU oracle (tests/demonstration_log_prob_ref.py on tests/trajectory_log_prob_ref.py).  Bounds, that module's:
    log_prob             |got - ref| <= max(1e-5 (max_b |ref| + n), 4 x the float32-table floor)
    g_params, g_params_L |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the float32-table floor)
(tests/test_demo_log_prob_host.py asserts 4 x floor <= 1e-2 x scale on every case used here).  Every comparison prints both maxima
before it asserts.
"""
import numpy as np
import pytest
import torch

from fancy_gym_amd import _lib
from oracle import mp_oracle as O
from tests import demonstration_log_prob_ref as DR
from tests import trajectory_condition_ref as R

from .test_gpu_traj_condition import bits, dev, inits, mp_of, shifted
from .test_gpu_traj_log_prob import same
from .test_gpu_trajectory import CFG3, make_engine

pytestmark = pytest.mark.gpu


def run(eng, name, cs, *, pos=None, sd=None, mu=None, L=None, g=None, grad=True, wrap=dev):
    """(log_prob, g_params, g_params_L) of the bare entry points"""
    ip, iv = inits(name, cs)
    if wrap is not dev:
        ip, iv = (None if ip is None else wrap(ip)), (None if iv is None else wrap(iv))
    mu = wrap(cs["mu"]) if mu is None else mu
    L = wrap(cs["L"]) if L is None else L
    y = wrap(cs["pos"] if pos is None else pos)
    s = wrap(cs["sd"] if sd is None else sd)
    it = R.config(name)[5]
    lp = eng.demonstration_log_prob(mu, L, y, s, ip, iv, it)
    if not grad:
        return lp, None, None
    gm, gL = eng.demonstration_log_prob_vjp(dev(cs["g"]) if g is None else g, mu, L, y, s, ip, iv, it)
    return lp, gm, gL


def one_episode(cs, b, B):
    return {k: (v[b:b + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) and k != "c" else v) for k, v in cs.items()}


# ---- 1. forward and gradients against the dense reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,sigma,missing", DR.gpu_cases())
def test_log_prob_and_gradients_match_the_dense_reference(name, B, sigma, missing):
    eng = DR.engine_for(name)
    cs = DR.case(name, B, sigma, missing)
    lp, gm, gL = run(eng, name, cs)
    torch.cuda.synchronize()
    assert eng.last_kernel() == f"k_demo_log_prob<{mp_of(name)}, grad>", eng.last_kernel()
    assert lp.shape == (B,) and lp.dtype == torch.float64 and gm.dtype == gL.dtype == torch.float32
    assert gm.shape == cs["mu"].shape and gL.shape == cs["L"].shape
    DR.check((lp, gm, gL), cs, f"{name} B={B} sigma={sigma} missing={missing} n={int(cs['n'][0])}")
    P = cs["mu"].shape[1]
    assert not bits(gL[:, dev(np.triu(np.ones((P, P), bool), 1))]).any()           # the strict upper triangle: exact zeros


def test_the_limit_case_is_among_them():
    assert ("prodmp_12_columns_16_dof", 3, 1e-3, False) in DR.gpu_cases()
    cs = DR.case("prodmp_12_columns_16_dof", 3, 1e-3, False)
    assert (cs["n"] == 480).all() and cs["mu"].shape[1] == 160


# ---- 2. autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded"])
def test_autograd_backward_is_the_vjp_launch(name):
    eng = DR.engine_for(name)
    B = 3
    cs = DR.case(name, B, 0.1, True)
    ip, iv = inits(name, cs)
    it = R.config(name)[5]
    y, sd, g = dev(cs["pos"]), dev(cs["sd"]), dev(cs["g"])
    want = run(eng, name, cs)
    mu = dev(cs["mu"]).requires_grad_(True)
    L = torch.tril(torch.nan_to_num(dev(cs["L"]))).requires_grad_(True)
    lp = eng.demonstration_log_prob(mu, L, y, sd, ip, iv, it)
    assert lp.requires_grad and eng.last_kernel() == f"k_demo_log_prob<{mp_of(name)}>"
    (lp * g).sum().backward()
    assert eng.last_kernel() == f"k_demo_log_prob<{mp_of(name)}, grad>"
    assert same((lp.detach(), mu.grad, L.grad), want)
    # only the mean requires grad: the factor's gradient is not computed
    mu2 = dev(cs["mu"]).requires_grad_(True)
    lp2 = eng.demonstration_log_prob(mu2, L.detach(), y, sd, ip, iv, it)
    (lp2 * g).sum().backward()
    assert same((mu2.grad,), (want[1],))
    # a mean and a factor shared by the batch, expanded from one row: the sum over the batch
    m1 = dev(cs["mu"][0]).requires_grad_(True)
    L1 = torch.tril(torch.nan_to_num(dev(cs["L"][0]))).requires_grad_(True)
    lp3 = eng.demonstration_log_prob(m1.expand(B, -1), L1.expand(B, -1, -1), y, sd, ip, iv, it)
    (lp3 * g).sum().backward()
    gm, gL = eng.demonstration_log_prob_vjp(g, m1.detach().expand(B, -1), L1.detach().expand(B, -1, -1), y, sd, ip, iv, it)
    for got, each in ((m1.grad, gm), (L1.grad, gL)):                        # (torch's own float32 sum over the batch)
        assert (got - each.double().sum(0)).abs().max() <= 1e-6 * each.abs().sum(0).max()
    # without requires_grad, or under no_grad: no graph; obs_std broadcasts from [T, D]
    lp4 = eng.demonstration_log_prob(mu.detach(), L.detach(), y, sd, ip, iv, it)
    assert not lp4.requires_grad and lp4.grad_fn is None and same((lp4,), (want[0],))
    with torch.no_grad():
        assert not eng.demonstration_log_prob(mu, L, y, sd, ip, iv, it).requires_grad
    with pytest.raises(NotImplementedError, match="pos requires grad"):
        eng.demonstration_log_prob(mu, L, y.clone().requires_grad_(True), sd, ip, iv, it)
    full = eng.demonstration_log_prob(mu.detach(), L.detach(), y, 0.1, ip, iv, it)
    assert same((full,), (eng.demonstration_log_prob(mu.detach(), L.detach(), y, torch.full(y.shape[1:], 0.1), ip, iv, it),))


# ---- 3. the two likelihood kernels agree where both apply --------------------------------------------------------------------------------
def test_two_kept_steps_are_trajectory_log_prob_on_those_steps():
    name = "cfg2_prodmp"
    eng = DR.engine_for(name)
    B = 3
    cs = DR.case(name, B, 1e-2, False)
    steps = [31, 77]
    sd = np.full_like(cs["sd"], np.inf)
    sd[:, steps] = cs["sd"][:, steps]
    ref = DR.references(name, cs["mu"], cs["L"], cs["c"], cs["pos"], sd, cs["g"])
    assert (ref["n"] == 14).all()
    lp, gm, gL = run(eng, name, cs, sd=sd)
    ip, iv = inits(name, cs)
    args = (dev(cs["mu"]), dev(cs["L"]), steps, dev(np.ascontiguousarray(cs["pos"][:, steps])), dev(np.ascontiguousarray(sd[:, steps])),
            ip, iv, R.config(name)[5])
    lp2 = eng.trajectory_log_prob(*args)
    gm2, gL2 = eng.trajectory_log_prob_vjp(dev(cs["g"]), *args)
    assert eng.last_kernel() == "k_traj_log_prob<prodmp, grad>"
    err = (lp - lp2).abs().cpu().numpy()
    print(f"[demo] information form vs the dense kernel, n = 14: log_prob {err.max():.3e} (|ref| {np.abs(ref['ref_lp']).max():.3e})")
    assert (err <= 1e-8 * (np.abs(ref["ref_lp"]) + 14)).all()
    DR.check((lp, gm, gL), ref, "two kept steps, k_demo_log_prob")
    DR.check((lp2, gm2, gL2), ref, "two kept steps, k_traj_log_prob")


# ---- 4. edge semantics -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded"])
def test_edges(name):
    eng = DR.engine_for(name)
    B = 3
    cs = DR.case(name, B, 0.1, True)
    P = cs["mu"].shape[1]
    D = cs["sd"].shape[2]
    Kloc = P // D
    lower = dev(np.tril(np.ones((P, P), bool)))
    first = run(eng, name, cs)
    # episode 1 entirely removed (inf, NaN, negative), DoF 0 of episode 0 removed
    bad = np.array([np.inf, np.nan, -1.0], np.float32)
    sd = cs["sd"].copy()
    sd[1] = bad[np.arange(sd[1].size) % 3].reshape(sd[1].shape)
    sd[0, :, 0] = np.inf
    ref = DR.references(name, cs["mu"], cs["L"], cs["c"], cs["pos"], sd, cs["g"])
    assert ref["n"][1] == 0 and 0 < ref["n"][0] < ref["n"][2]
    lp, gm, gL = run(eng, name, cs, sd=sd)
    DR.check((lp, gm, gL), ref, f"{name} an episode and a DoF removed")
    assert lp[1].item() == 0.0 and not np.signbit(lp[1].item())
    assert not bits(gm[1]).any() and not bits(gL[1]).any()
    assert not bits(gm[0, :Kloc]).any() and not bits(gL[0, :Kloc]).any() and gL[0, Kloc:].abs().max() > 0
    assert same(tuple(x[2:3] for x in (lp, gm, gL)), tuple(x[2:3] for x in first))
    # a sigma == 0 in episode 1: NaN there, the neighbours bit-identical to a run without it
    sd0 = cs["sd"].copy()
    sd0[1, 5, D - 1] = 0.0
    lp, gm, gL = run(eng, name, cs, sd=sd0)
    assert torch.isnan(lp[1]) and torch.isnan(gm[1]).all() and torch.isnan(gL[1][lower]).all() and (gL[1][~lower] == 0).all()
    for b in (0, 2):
        assert same(tuple(x[b:b + 1] for x in (lp, gm, gL)), tuple(x[b:b + 1] for x in first)), b
    # a NaN in pos stays inside its episode (and in a removed entry it is not even read into the result)
    y = cs["pos"].copy()
    y[1, 7, 0] = np.nan
    sdk = cs["sd"].copy()
    sdk[1, 7, 0] = 0.1
    lp, gm, gL = run(eng, name, cs, pos=y, sd=sdk)
    assert torch.isnan(lp[1])
    for b in (0, 2):
        assert same(tuple(x[b:b + 1] for x in (lp, gm, gL)), tuple(x[b:b + 1] for x in first)), b
    sdk[1, 7, 0] = np.inf
    y2 = cs["pos"].copy()
    y2[1, 7, 0] = 0.0
    assert same(run(eng, name, cs, pos=y, sd=sdk), run(eng, name, cs, pos=y2, sd=sdk))


# ---- 5. determinism, isolation and alignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prodmp_1_dof", "cfg4_prodmp_init_time"])
def test_determinism_isolation_and_alignment(name):
    eng = DR.engine_for(name)
    B = 65
    cs = DR.case(name, B, 0.1, True)
    first = run(eng, name, cs)
    assert same(first, run(eng, name, cs))
    for b in range(B):
        alone = run(eng, name, one_episode(cs, b, B))
        assert same(tuple(x[b:b + 1] for x in first), alone), b
    # every float32 pointer one float past a 16-byte boundary
    assert same(first, run(eng, name, cs, wrap=shifted))


def test_determinism_at_the_limit_shape():
    name = "prodmp_12_columns_16_dof"
    eng = DR.engine_for(name)
    cs = DR.case(name, 3, 1e-3, False)
    first = run(eng, name, cs)
    assert same(first, run(eng, name, cs)) and same(first, run(eng, name, cs, wrap=shifted))
    assert same(tuple(x[2:3] for x in first), run(eng, name, one_episode(cs, 2, 3)))


# ---- 6. refusals that need the handle --------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry():
    stream = torch.cuda.current_stream().cuda_stream
    ptr = torch.zeros(1 << 18, device="cuda").data_ptr()

    def raw(eng, B=1, **kw):
        a = dict(params=ptr, L=ptr, ip=ptr, iv=ptr, pos=ptr, sd=ptr, out=ptr)
        a.update(kw)
        return eng._lib.mpk_demonstration_log_prob(eng._h, a["params"], a["L"], a["ip"], a["iv"], 0.0, a["pos"], a["sd"], a["out"], B, stream)

    def raw_vjp(eng, g=ptr, gm=ptr, gL=ptr):
        return eng._lib.mpk_demonstration_log_prob_vjp(eng._h, ptr, ptr, ptr, ptr, 0.0, ptr, ptr, g, gm, gL, 1, stream)

    def both(eng, word):
        before = eng.last_kernel()
        for rc in (raw(eng), raw_vjp(eng)):
            assert rc == _lib.MPK_ENOTIMPL and word in _lib.last_error(), _lib.last_error()
        assert eng.last_kernel() == before                                   # nothing was launched

    both(make_engine(*CFG3), "DMP has no probabilistic interface")
    pc = O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0, learn_tau=True, tau_bound=(0.5, 3.0))
    eng = make_engine(pc, O.BasisCfg("prodmp", num_basis=5, alpha=10), O.TrajCfg("prodmp", action_dim=3), 0.02, 1.0)
    both(eng, "learned tau / delay")
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        eng.demonstration_log_prob(torch.zeros((1, eng.num_params)), torch.zeros((1, eng.num_params, eng.num_params)),
                                   torch.zeros((1, eng.num_steps, 3)), 0.1, torch.zeros((1, 3)), torch.zeros((1, 3)))
    both(R.engine_for("prodmp_wide_20_dof"), "at most 16 DoF and 16 table columns")
    # 16 DoF x 16 basis functions: Pl = 256 is within 64 x 4, but the packed triangle alone is 263 KB
    eng = make_engine(O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=16), O.TrajCfg("promp", action_dim=16), 0.02, 0.6)
    assert eng.num_params == 256
    both(eng, "do not fit the CU's 163840 bytes of LDS")
    with pytest.raises(NotImplementedError, match="256 parameters .* do not fit the CU's"):
        eng.demonstration_log_prob(torch.zeros((1, 256)), torch.zeros((1, 256, 256)), torch.zeros((1, eng.num_steps, 16)), 0.1)
    # the arguments, on a handle that runs
    eng = DR.engine_for("cfg2_prodmp")
    before = eng.last_kernel()
    for kw, word in ((dict(params=None), "NULL params"), (dict(L=None), "NULL params"), (dict(pos=None), "NULL pos or obs_std"),
                     (dict(sd=None), "NULL pos or obs_std"), (dict(out=None), "NULL log_prob"), (dict(ip=None), "init_pos and init_vel"),
                     (dict(B=0), "B must be >= 1")):
        assert raw(eng, **kw) == _lib.MPK_EINVAL and word in _lib.last_error(), (kw, _lib.last_error())
    assert raw_vjp(eng, g=None) == _lib.MPK_EINVAL and "NULL g" in _lib.last_error()
    assert raw_vjp(eng, gm=None, gL=None) == _lib.MPK_EINVAL and "both NULL" in _lib.last_error()
    assert eng.last_kernel() == before
    # either gradient output alone
    cs = DR.case("cfg2_prodmp", 3, 0.1, True)
    want = run(eng, "cfg2_prodmp", cs)
    ip, iv = inits("cfg2_prodmp", cs)
    args = (dev(cs["g"]), dev(cs["mu"]), dev(cs["L"]), dev(cs["pos"]), dev(cs["sd"]), ip, iv, 0.0)
    gm, none = eng.demonstration_log_prob_vjp(*args, need=(True, False))
    none2, gL = eng.demonstration_log_prob_vjp(*args, need=(False, True))
    assert none is None and none2 is None and same((gm, gL), want[1:])
    with pytest.raises(ValueError, match=r"pos must be \[3, 100, 7\]"):
        eng.demonstration_log_prob(dev(cs["mu"]), dev(cs["L"]), dev(cs["pos"][:, :50]), 0.1, ip, iv)


# ---- 7. thin calls ---------------------------------------------------------------------------------------------------------------------------
def test_a_batched_black_box_scores_from_its_own_state():
    from fancy_gym_amd import BatchedBlackBox
    from fancy_gym_amd.black_box.factory import get_basis_generator, get_controller, get_phase_generator, get_trajectory_generator
    B, D = 5, 7
    pg_, dg_ = 0.01 * np.array([120., 120., 120., 120., 50., 30., 10.]), 0.01 * np.array([10., 10., 10., 10., 6., 5., 3.])
    phase = get_phase_generator("exp", tau=1.5, alpha_phase=3.0)
    basis = get_basis_generator("prodmp", phase, num_basis=5, basis_bandwidth_factor=2, alpha=10)
    tg = get_trajectory_generator("prodmp", D, basis)
    bb = BatchedBlackBox(tg, get_controller("motor", p_gains=pg_, d_gains=dg_), B, 0.02, 2.0, act_low=-1.0, act_high=1.0,
                         plant="double_integrator")
    gen = torch.Generator().manual_seed(3)
    q0 = (torch.rand((B, D), generator=gen, dtype=torch.float64) - 0.5).cuda()
    bb.reset(q0)
    P, T = bb.engine.num_params, bb.engine.num_steps
    mu = torch.randn((B, P), generator=gen).cuda().requires_grad_(True)
    L = torch.tril(torch.nan_to_num(dev(R.random_factor(P, B, seed=5))))
    y = (torch.rand((B, T, D), generator=gen) - 0.5).cuda()
    lp = bb.demonstration_log_prob(mu, L, y, 0.1)
    assert bb.engine.last_kernel() == "k_demo_log_prob<prodmp>" and lp.requires_grad
    want = bb.engine.demonstration_log_prob(mu.detach(), L, y, 0.1, q0.float(), torch.zeros((B, D), device="cuda"), 0.0)
    assert same((lp.detach(),), (want,))
    lp.sum().backward()
    gm, _ = bb.engine.demonstration_log_prob_vjp(torch.ones(B, dtype=torch.float64, device="cuda"), mu.detach(), L, y, 0.1, q0.float(),
                                                 torch.zeros((B, D), device="cuda"), 0.0, need=(True, False))
    assert _ is None and same((mu.grad,), (gm,))


# ---- 8. the example --------------------------------------------------------------------------------------------------------------------------
def test_the_example_improves_the_likelihood():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "batched_promp_from_demonstrations.py")
    spec = importlib.util.spec_from_file_location("batched_promp_from_demonstrations", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    start, end, generating, off = mod.run(demos=64, iters=40, verbose=False)
    print(f"[demo] example: mean log-likelihood start {start:.3f} end {end:.3f} generating {generating:.3f}, mean off by {off:.3f}")
    assert np.isfinite([start, end, generating, off]).all() and end > start
