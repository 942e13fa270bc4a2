"""
mpk_trajectory_condition / TrajectoryEngine.condition on the GPU: a Gaussian over the MP parameters conditioned on observed points.

Yardstick: the batch formula in float64 numpy per episode, rows from the float64 Jacobian of the CPU oracle and offsets from the oracle's
trajectory at zero parameters (tests/trajectory_condition_ref.py).  Bound, per output array -- the posterior mean, and the posterior
covariance tril(L') tril(L')^T formed in float64 from the returned float32 factor, never the factor itself (the helper says why):
    |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x the float32-table floor)
Every comparison prints both maxima before it asserts.
"""
import numpy as np
import pytest
import torch

from fancy_gym_amd import BatchedBlackBox, _lib
from fancy_gym_amd.black_box.factory import get_basis_generator, get_controller, get_phase_generator, get_trajectory_generator
from oracle import mp_oracle as O
from tests import trajectory_condition_ref as R

from .test_gpu_trajectory import CFG3, RTOL, make_engine

pytestmark = pytest.mark.gpu

PARITY = ("cfg1_promp_zero_padded", "cfg2_prodmp", "prodmp_relative_goal", "promp_16_columns_3_dof", "prodmp_12_columns_16_dof",
          "prodmp_1_dof", "cfg4_prodmp_init_time", "cfg2_prodmp_97_steps")
WITH_VEL = ("cfg2_prodmp", "cfg1_promp_zero_padded")
EXACT = ("cfg1_promp_zero_padded", "cfg2_prodmp", "promp_16_columns_3_dof", "cfg4_prodmp_init_time")


def dev(x):
    return None if x is None else torch.as_tensor(x, device="cuda")


def bits(x):
    return x.contiguous().view(torch.int32)


def mp_of(name):
    return R.config(name)[2].trajectory_generator_type


def inits(name, cs):
    """(init_pos, init_vel) as the engine takes them; None (zeros) for the ProMP whose basis is not zero-padded: it reads neither"""
    return (None, None) if name == "promp_16_columns_3_dof" else (dev(cs["ip"]), dev(cs["iv"]))


def run(eng, name, cs, *, steps=None, pos="case", vel="case", out=None, mu=None, L=None):
    pos = cs["pos"] if isinstance(pos, str) else pos
    vel = cs["vel"] if isinstance(vel, str) else vel
    ip, iv = inits(name, cs)
    yp, sp = (None, None) if pos is None else (dev(pos[0]), dev(pos[1]))
    yv, sv = (None, None) if vel is None else (dev(vel[0]), dev(vel[1]))
    return eng.condition(dev(cs["mu"]) if mu is None else mu, dev(cs["L"]) if L is None else L, cs["steps"] if steps is None else steps,
                         yp, sp, ip, iv, R.config(name)[5], obs_vel=yv, obs_vel_std=sv, out=out)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 1e-3])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name,vel", [(n, False) for n in PARITY] + [(n, True) for n in WITH_VEL])
def test_posterior_matches_the_batch_formula(name, vel, B, sigma):
    eng = R.engine_for(name)
    cs = R.case(name, B, 3, sigma, seed=1, vel=vel)
    mu, L = run(eng, name, cs)
    torch.cuda.synchronize()
    assert eng.last_kernel() == f"k_traj_condition<{mp_of(name)}>", eng.last_kernel()
    assert mu.shape == cs["mu"].shape and L.shape == cs["L"].shape and mu.dtype == L.dtype == torch.float32
    R.check(mu, L, cs, f"{name} B={B} sigma={sigma} vel={vel}")
    assert (torch.diagonal(L, dim1=1, dim2=2) >= 0).all()


# ---- 2. exact via-points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT)
def test_exact_via_points(name):
    """sigma = 0, two steps: parity; the posterior mean's trajectory passes through the observed positions; the posterior's standard
    deviation there is the reference's (about 0), finite and non-negative -- the project rule on the trajectory / on the std array"""
    eng = R.engine_for(name)
    B = 3
    cs = R.case(name, B, 2, 0.0, seed=2)
    J, P, D, T = R.jacobian(name)
    mu, L = run(eng, name, cs)
    R.check(mu, L, cs, f"{name} sigma=0")
    steps = list(cs["steps"])
    y = cs["pos"][0].astype(np.float64)
    z = torch.zeros((B, D), device="cuda")
    ip, iv = inits(name, cs)
    pos = eng.trajectory(mu, z if ip is None else ip, z if iv is None else iv, R.config(name)[5])[0].cpu().numpy().astype(np.float64)
    ref_pos = np.einsum("tdp,bp->btd", J[0][..., :P], cs["ref_mu"]) + cs["c"][0]
    err = np.abs(pos[:, steps] - y)
    tol = RTOL * np.abs(ref_pos).max() + RTOL * np.abs(y)
    print(f"[cond] {name} via-points: max|pos| {np.abs(ref_pos).max():.3e}  max residual {err.max():.3e}  project rule "
          f"{RTOL * np.abs(ref_pos).max():.3e}")
    assert not (err > tol).any()
    std = eng.trajectory_std(L, R.config(name)[5], vel=False)[0].cpu().numpy().astype(np.float64)
    ref_std = np.sqrt(np.maximum(np.einsum("tdp,bpq,tdq->btd", J[0][..., :P], cs["ref_Sigma"], J[0][..., :P]), 0.0))
    err = np.abs(std[:, steps] - ref_std[:, steps])
    tol = RTOL * ref_std.max() + RTOL * ref_std[:, steps]
    print(f"[cond] {name} std at the via-points: max|ref std| {ref_std.max():.3e}  ref there {ref_std[:, steps].max():.3e}  got there "
          f"{std[:, steps].max():.3e}  project rule {RTOL * ref_std.max():.3e}")
    assert np.isfinite(std).all() and (std >= 0).all()
    assert not (err > tol).any()


# ---- 3. skips are exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded"])
def test_skipped_observations_are_exact(name):
    eng = R.engine_for(name)
    B = 3
    cs = R.case(name, B, 3, 0.1, seed=3, vel=True)
    (yp, sp), (yv, sv) = cs["pos"], cs["vel"]
    mu0, L0 = dev(cs["mu"]), dev(cs["L"])
    # nothing observed: the prior comes back bit for bit
    inf = np.full_like(sp, np.inf)
    mu, L = run(eng, name, cs, pos=(yp, inf), vel=(yv, inf))
    assert torch.equal(bits(mu), bits(mu0)) and torch.equal(bits(torch.tril(L)), bits(torch.tril(L0)))
    # a whole step and all velocities marked +inf / NaN / negative: the run that never lists them
    bad = np.array([np.inf, np.nan, -1.0], np.float32)
    sp2, sv2 = sp.copy(), bad[np.arange(sv.size) % 3].reshape(sv.shape)
    sp2[:, 1, :] = bad[np.arange(sp[:, 1, :].size) % 3].reshape(sp[:, 1, :].shape)
    got = run(eng, name, cs, pos=(yp, sp2), vel=(yv, sv2))
    keep = [0, 2]
    want = run(eng, name, cs, steps=[cs["steps"][m] for m in keep], pos=(yp[:, keep], sp[:, keep]), vel=None)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    # single DoFs of one episode skipped: the float64 reference without them, inside the bound
    sp3 = sp.copy()
    sp3[1, :, ::2] = np.inf
    sp3[2, 0, 1] = np.nan
    ref = R.references(name, cs["mu"], cs["L"], cs["steps"], cs["c"], ((yp, sp3), None))
    mu, L = run(eng, name, cs, pos=(yp, sp3), vel=None)
    R.check(mu, L, ref, f"{name} some DoFs skipped")
    # one episode not observed at all: unchanged, its neighbours as in the run that observes everybody
    sp4 = sp.copy()
    sp4[1] = np.inf
    full = run(eng, name, cs, vel=None)
    mu, L = run(eng, name, cs, pos=(yp, sp4), vel=None)
    assert torch.equal(bits(mu[1]), bits(mu0[1])) and torch.equal(bits(torch.tril(L[1])), bits(torch.tril(L0[1])))
    for b in (0, 2):
        assert torch.equal(bits(mu[b]), bits(full[0][b])) and torch.equal(bits(L[b]), bits(full[1][b]))
        assert not torch.equal(bits(mu[b]), bits(mu0[b]))


# ---- 4. triangle discipline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "prodmp_12_columns_16_dof", "promp_16_columns_3_dof"])
def test_the_upper_triangle_is_never_read_and_comes_back_zero(name):
    eng = R.engine_for(name)
    cs = R.case(name, 3, 3, 1e-3, seed=1)
    P = cs["mu"].shape[1]
    upper = np.triu(np.ones((P, P), bool), 1)
    assert np.isnan(cs["L"][:, upper]).all()
    mu, L = run(eng, name, cs)
    assert torch.isfinite(mu).all() and torch.isfinite(L).all()
    assert (L[:, dev(upper)] == 0).all() and not torch.signbit(L[:, dev(upper)]).any()


# ---- 5. determinism and layout -----------------------------------------------------------------------------------------------------------
def shifted(x):
    """a copy of x in storage of its own, one float past a 16-byte boundary"""
    x = dev(x)
    buf = torch.empty(x.numel() + 8, device="cuda", dtype=x.dtype)
    start = 1 + (-(buf.data_ptr() // 4) % 4)
    view = buf[start:start + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("name", ["cfg2_prodmp", "prodmp_12_columns_16_dof", "cfg1_promp_zero_padded"])
def test_determinism_isolation_alignment_and_the_in_place_form(name):
    eng = R.engine_for(name)
    B = 65
    cs = R.case(name, B, 3, 1e-3, seed=1, vel=name in WITH_VEL)
    first = run(eng, name, cs)
    again = run(eng, name, cs)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(bits(first[1]), bits(again[1]))
    # an episode alone is the episode in the batch
    for b in (0, 17, 64):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in cs.items()}
        for k in ("pos", "vel"):
            one[k] = None if cs[k] is None else (cs[k][0][b:b + 1], cs[k][1][b:b + 1])
        alone = run(eng, name, one)
        assert torch.equal(bits(alone[0][0]), bits(first[0][b])) and torch.equal(bits(alone[1][0]), bits(first[1][b])), b
    # every pointer one float past a 16-byte boundary
    ip, iv = inits(name, cs)
    obs = [None if cs[k] is None else (shifted(cs[k][0]), shifted(cs[k][1])) for k in ("pos", "vel")]
    out = (shifted(np.zeros_like(cs["mu"])), shifted(np.zeros_like(cs["mu"], shape=cs["L"].shape)))
    got = eng.condition(shifted(cs["mu"]), shifted(cs["L"]), cs["steps"], obs[0] and obs[0][0], obs[0] and obs[0][1],
                        None if ip is None else shifted(ip), None if iv is None else shifted(iv), R.config(name)[5],
                        obs_vel=obs[1] and obs[1][0], obs_vel_std=obs[1] and obs[1][1], out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(bits(got[0]), bits(first[0])) and torch.equal(bits(got[1]), bits(first[1]))
    # in place: the outputs are the inputs
    mu, L = dev(cs["mu"]).clone(), dev(cs["L"]).clone()
    got = run(eng, name, cs, mu=mu, L=L, out=(mu, L))
    assert got[0].data_ptr() == mu.data_ptr() and got[1].data_ptr() == L.data_ptr()
    assert torch.equal(bits(mu), bits(first[0])) and torch.equal(bits(L), bits(first[1]))


# ---- 6. one call or two ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 1e-3])
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded", "prodmp_12_columns_16_dof"])
def test_two_calls_are_one_call(name, sigma):
    """(t1, t2, t3) at once, or (t1) and then (t2, t3) on its result -- which passes through float32 once: both inside the bound"""
    eng = R.engine_for(name)
    cs = R.case(name, 3, 3, sigma, seed=4)
    y, sd = cs["pos"]
    one = run(eng, name, cs)
    mid = run(eng, name, cs, steps=cs["steps"][:1], pos=(y[:, :1], sd[:, :1]))
    two = run(eng, name, cs, steps=cs["steps"][1:], pos=(y[:, 1:], sd[:, 1:]), mu=mid[0], L=mid[1])
    R.check(one[0], one[1], cs, f"{name} sigma={sigma} one call")
    R.check(two[0], two[1], cs, f"{name} sigma={sigma} two calls")


# ---- 7. refusals, all before any launch --------------------------------------------------------------------------------------------------
def test_refusals():
    stream = torch.cuda.current_stream().cuda_stream
    scratch = torch.zeros(1 << 16, device="cuda")
    ptr = scratch.data_ptr()
    import ctypes as C

    def raw(eng, steps=(1, 2), M=None, params=ptr, L=ptr, ip=ptr, iv=ptr, pos=ptr, pos_std=ptr, vel=None, vel_std=None, out=ptr,
            L_out=ptr, B=1):
        arr = (C.c_int32 * max(len(steps), 1))(*steps)
        return eng._lib.mpk_trajectory_condition(eng._h, params, L, ip, iv, 0.0, arr, len(steps) if M is None else M, pos, pos_std, vel,
                                                 vel_std, out, L_out, B, stream)

    def tensors(eng, B=2, M=2):
        P, D = eng.num_params, eng.num_dof
        return (torch.zeros((B, P), device="cuda"), torch.zeros((B, P, P), device="cuda"), torch.zeros((B, M, D), device="cuda"),
                torch.zeros((B, D), device="cuda"))

    # a DMP
    eng = make_engine(*CFG3)
    before = eng.last_kernel()
    mu, L, y, z = tensors(eng)
    with pytest.raises(NotImplementedError, match="DMP has no probabilistic interface"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z)
    assert raw(eng) == _lib.MPK_ENOTIMPL and "DMP" in _lib.last_error() and eng.last_kernel() == before
    # a learned tau
    pc = O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0, learn_tau=True, tau_bound=(0.5, 3.0))
    bc, tc = O.BasisCfg("prodmp", num_basis=5, alpha=10), O.TrajCfg("prodmp", action_dim=3)
    eng = make_engine(pc, bc, tc, 0.02, 1.0)
    before = eng.last_kernel()
    mu, L, y, z = tensors(eng)
    with pytest.raises(NotImplementedError, match="learned tau / delay"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z)
    assert raw(eng) == _lib.MPK_ENOTIMPL and "tau" in _lib.last_error() and eng.last_kernel() == before
    # 17 columns, 20 DoF
    for name in ("prodmp_17_columns_7_dof", "prodmp_wide_20_dof"):
        eng = R.engine_for(name)
        before = eng.last_kernel()
        mu, L, y, z = tensors(eng, B=1)
        with pytest.raises(NotImplementedError, match="at most 16 DoF and 16 table columns"):
            eng.condition(mu, L, [1, 2], y, 0.1, z, z)
        assert raw(eng) == _lib.MPK_ENOTIMPL and "at most 16 DoF and 16 table columns" in _lib.last_error()
        assert eng.last_kernel() == before
    # 16 DoF x 16 basis functions: Pl = 256, the triangle alone is 263 KB
    eng = make_engine(O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=16), O.TrajCfg("promp", action_dim=16), 0.02, 0.6)
    assert eng.num_params == 256
    before = eng.last_kernel()
    mu, L, y, _ = tensors(eng, B=1)
    with pytest.raises(NotImplementedError, match="256 parameters .* do not fit the CU's"):
        eng.condition(mu, L, [1, 2], y, 0.1)
    assert eng.last_kernel() == before
    # the arguments, on a handle that would run
    name = "cfg2_prodmp"
    eng = R.engine_for(name)
    T = eng.num_steps
    before = eng.last_kernel()
    mu, L, y, z = tensors(eng)
    with pytest.raises(ValueError, match="M must be 1..32"):
        eng.condition(mu, L, [], torch.zeros((2, 0, 7), device="cuda"), 0.1, z, z)
    with pytest.raises(ValueError, match="M must be 1..32"):
        eng.condition(mu, L, list(range(33)), torch.zeros((2, 33, 7), device="cuda"), 0.1, z, z)
    for steps in ([2, 1], [3, 3], [-1, 4], [5, T]):
        with pytest.raises(ValueError, match="strictly increasing step indices"):
            eng.condition(mu, L, steps, y, 0.1, z, z)
    with pytest.raises(ValueError, match="come in pairs"):
        eng.condition(mu, L, [1, 2], y, None, z, z)
    with pytest.raises(ValueError, match="come in pairs"):
        eng.condition(mu, L, [1, 2], y, 0.1, z, z, obs_vel=y)
    with pytest.raises(ValueError, match="nothing is observed"):
        eng.condition(mu, L, [1, 2], None, None, z, z)
    with pytest.raises(ValueError, match="may be None only for a ProMP"):
        eng.condition(mu, L, [1, 2], y, 0.1)
    with pytest.raises(ValueError, match="does not broadcast"):
        eng.condition(mu, L, [1, 2], y, torch.zeros(5), z, z)
    assert raw(eng, M=0) == _lib.MPK_EINVAL and "M must be 1..32" in _lib.last_error()
    assert raw(eng, steps=tuple(range(33))) == _lib.MPK_EINVAL and "M must be 1..32" in _lib.last_error()
    assert raw(eng, steps=(4, 4)) == _lib.MPK_EINVAL and "strictly increasing" in _lib.last_error()
    assert raw(eng, steps=(4, T)) == _lib.MPK_EINVAL and "strictly increasing" in _lib.last_error()
    assert raw(eng, pos=None, pos_std=None) == _lib.MPK_EINVAL and "nothing is observed" in _lib.last_error()
    assert raw(eng, pos_std=None) == _lib.MPK_EINVAL and "in pairs" in _lib.last_error()
    assert raw(eng, vel_std=ptr) == _lib.MPK_EINVAL and "in pairs" in _lib.last_error()
    assert raw(eng, ip=None) == _lib.MPK_EINVAL and "init_pos and init_vel are required" in _lib.last_error()
    assert raw(eng, params=None) == _lib.MPK_EINVAL and raw(eng, L=None) == _lib.MPK_EINVAL
    assert raw(eng, out=None) == _lib.MPK_EINVAL and raw(eng, L_out=None) == _lib.MPK_EINVAL and "NULL params" in _lib.last_error()
    assert raw(eng, B=0) == _lib.MPK_EINVAL and "B must be >= 1" in _lib.last_error()
    assert eng.last_kernel() == before                                       # nothing was launched
    # a ProMP with one time step has no velocity to observe
    eng = make_engine(O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=6), O.TrajCfg("promp", action_dim=3), 0.02, 0.02)
    assert eng.num_steps == 1
    mu, L, y, _ = tensors(eng, M=1)
    with pytest.raises(ValueError, match="promp needs at least two time steps"):
        eng.condition(mu, L, [0], None, None, obs_vel=y, obs_vel_std=0.1)


# ---- 8. wiring ---------------------------------------------------------------------------------------------------------------------------
def make_mp(mp, D=3):
    pg = get_phase_generator("exp", tau=1.0, alpha_phase=3.0)
    bg = get_basis_generator("prodmp" if mp == "prodmp" else "rbf", pg, num_basis=4)
    gen = get_trajectory_generator(mp, D, bg)
    gen.set_duration(1.0, 0.02)
    return gen


@pytest.mark.parametrize("mp", ["prodmp", "promp"])
def test_generator_conditioning_is_the_engine_call(mp):
    gen = make_mp(mp)
    Pl = gen.num_params
    rng = np.random.default_rng(71)
    L0 = R.random_factor(Pl, 1, seed=72)[0]
    p0 = rng.standard_normal(Pl).astype(np.float32)
    ip, iv = rng.uniform(-1, 1, 3).astype(np.float32), np.zeros(3, np.float32)
    gen.set_params(p0)
    gen.set_initial_conditions(0.0, ip, iv)
    gen.set_mp_params_variances(L0)
    prior_std = gen.get_traj_pos_std().clone()
    y = rng.uniform(-1, 1, (2, 3)).astype(np.float32)
    gen.condition_on_observations([1.0, 0.5], y, 0.0, vel=np.zeros((2, 3), np.float32), vel_std=[np.inf, 0.01])
    eng = gen.engine()
    assert eng.last_kernel() == f"k_traj_condition<{mp}>"
    want = eng.condition(dev(p0[None]), dev(L0[None]), [24, 49], dev(y[::-1].copy()[None]), 0.0, dev(ip[None]), dev(iv[None]), 0.0,
                         obs_vel=torch.zeros((1, 2, 3), device="cuda"), obs_vel_std=torch.tensor([0.01, np.inf])[:, None])
    assert torch.equal(bits(torch.from_numpy(gen.params.reshape(1, -1))), bits(want[0].cpu()))
    assert torch.equal(bits(torch.from_numpy(gen.params_L[None])), bits(want[1].cpu()))
    pos, std = gen.get_traj_pos(), gen.get_traj_pos_std()
    ref_pos = eng.trajectory(want[0], dev(ip[None]), dev(iv[None]), 0.0)[0][0].cpu()
    ref_std = eng.trajectory_std(want[1], 0.0)[0][0].cpu()
    assert torch.equal(bits(std), bits(ref_std))
    assert (pos - ref_pos).abs().max() <= RTOL * ref_pos.abs().max()                  # (the one-episode host path is another launch)
    assert (pos[[49, 24]] - torch.from_numpy(y)).abs().max() <= 2 * RTOL * pos.abs().max()
    assert (std[[24, 49]] <= 1e-4 * prior_std.max()).all() and (std <= prior_std * (1 + 1e-5) + 1e-6).all()
    smp = gen.sample_trajectories(num_smp=8)[0]
    assert (smp[:, [49, 24]] - torch.from_numpy(y)).abs().max() <= 1e-3 * max(1.0, float(pos.abs().max()))


def test_a_batched_black_box_conditions_from_its_own_state_and_steps_on_the_result():
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
    P = bb.engine.num_params
    mu = torch.randn((B, P), generator=gen).cuda()
    L = dev(R.random_factor(P, B, seed=5))
    y = (torch.rand((B, 2, D), generator=gen) - 0.5).cuda()
    post, post_L = bb.condition(mu, L, [40, 99], y, 0.0)
    assert bb.engine.last_kernel() == "k_traj_condition<prodmp>"
    want = bb.engine.condition(mu, L, [40, 99], y, 0.0, q0.float(), torch.zeros((B, D), device="cuda"), 0.0)
    assert torch.equal(bits(post), bits(want[0])) and torch.equal(bits(post_L), bits(want[1]))
    assert bb._plan_params(post) is post                                      # no copy on the way into the plan
    out = bb.step(post)
    des = out["des_pos"]
    assert (des[:, [40, 99]] - y).abs().max() <= 2 * RTOL * des.abs().max()
    smp = bb.engine.sample_trajectories(post, post_L, q0.float(), torch.zeros((B, D), device="cuda"), num_samples=4)[0]
    assert (smp[:, :, [40, 99]] - y[:, None]).abs().max() <= 1e-3 * max(1.0, float(des.abs().max()))


def test_a_captured_launch_replays_to_the_same_bits():
    """after one warm call the launch allocates nothing and synchronises nothing, and the steps live in the launch arguments: it can be
    captured (one linear stream), and the replay gives the bits"""
    name = "cfg2_prodmp"
    eng = R.engine_for(name)
    B = 33
    cs = R.case(name, B, 3, 1e-3, seed=6)
    mu, L, ip, iv = dev(cs["mu"]), dev(cs["L"]), dev(cs["ip"]), dev(cs["iv"])
    y, sd = dev(cs["pos"][0]), dev(cs["pos"][1])
    out = (torch.empty_like(mu), torch.empty_like(L))
    eng.condition(mu, L, cs["steps"], y, sd, ip, iv, out=out)                # warm: builds the tables of (init_time, T)
    torch.cuda.synchronize()
    want = (out[0].clone(), out[1].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.condition(mu, L, cs["steps"], y, sd, ip, iv, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out[0].zero_(); out[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eng.last_kernel() == "k_traj_condition<prodmp>"
    assert torch.equal(bits(out[0]), bits(want[0])) and torch.equal(bits(out[1]), bits(want[1]))
    del g
    eng.unpin_tables()
