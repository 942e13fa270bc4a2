"""
mpk_trajectory_fit / TrajectoryEngine.fit_trajectory / BatchedBlackBox.fit_trajectory on the GPU.

Yardstick: tests/trajectory_fit_ref.py -- the float64 fit of the float64 oracle's affine map.  The comparison is on the RECONSTRUCTION,
never on raw parameters (cfg2's and cfg3's Gram matrices have condition numbers of 1e9 .. 4e10: at reg = 1e-9 even the float64 fit misses
the generating parameters by 1e-2 .. 2e-1 while it reconstructs to 1e-6 of the scale):

    |Psi p_gpu - Psi p_ref| <= max(RTOL max|y| + RTOL |Psi p_ref|, 4 x max|Psi p_f32 - Psi p_ref|)

RTOL = 1e-5 is the project's rule (tests/test_gpu_trajectory.py); p_f32 is the all-float32 CPU fit, the measured floor -- the rule of
tests/test_gpu_traj_vjp.py::check with the float32 fit in the float32 einsum's place.  cfg1 and cfg4 additionally compare params by the
same rule (cfg1's smallest Gram eigenvalue is 3.6; cfg4's, at init_time 0.5, is 4.7e-8 against 7.3, so its params comparison rests on the
float32 fit's floor -- profiles/r18_traj_fit.md).  Every comparison prints its maxima before it asserts.

The per-episode-phase kernel k_phase_fit<MP, KQ> (section 4): PHASE_KQ lists the rows and the instantiation each takes -- all five, one to
four right-hand-side slots a lane --; beside them the lane map's round boundaries, the batch wrap-around, the not-positive-definite
result and the shared route's factor cache (profiles/r19_phase_fit_edges.md).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import mp_oracle as O

from . import trajectory_fit_ref as R
from .test_gpu_trajectory import RTOL, make_engine
from .test_gpu_traj_vjp import config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = 1e-9
WELL_CONDITIONED = ("cfg1_promp_zero_padded", "cfg4_prodmp_init_time")

SHARED = ["cfg1_promp_zero_padded", "cfg2_prodmp", "cfg3_dmp_response", "cfg4_prodmp_init_time", "prodmp_relative_goal",
          "prodmp_relative_goal_after_scale",
          "cfg2_prodmp_97_steps", "cfg1_promp_199_steps",                              # the masked tail chunk
          "prodmp_1_dof", "prodmp_8_dof", "prodmp_11_dof", "prodmp_12_columns_16_dof",  # D = 1, 8, 11, 16
          "prodmp_16_columns_7_dof", "promp_16_columns_3_dof"]                          # exactly 16 table columns
SHARED += [f"prodmp_{T}_steps_{D}_dof" for D in (3, 7) for T in (1, 2, 3, 5)]            # under-determined: reg decides


@functools.lru_cache(maxsize=None)
def design(name):
    pc, bc, tc, dt, duration, init_time, _ = config(name)
    return R.Design(pc, bc, tc, dt, duration, init_time)


@functools.lru_cache(maxsize=None)
def case(name, B, seed, reg=REG):
    """demonstrations and both CPU fits, computed once and shared (read-only)"""
    ds = design(name)
    y, ip, iv, gen = R.demonstrations(ds, B, seed)
    c = ds.offset(ip, iv)
    out = dict(y=y, ip=ip, iv=iv, gen=gen, c=c, p64=R.fit64(ds, y, c, reg), p32=R.fit32(ds, y, c, reg))
    for v in out.values():
        v.setflags(write=False)
    return out


def engine_for(name):
    pc, bc, tc, dt, duration, _, _ = config(name)
    return make_engine(pc, bc, tc, dt, duration)


def dev(x):
    return x.cuda() if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).cuda()


def tolerance(ds, cs):
    rec = ds.reconstruct(cs["p64"])
    floor = np.abs(ds.reconstruct(cs["p32"]) - rec).max()
    return rec, np.maximum(RTOL * np.abs(cs["y"]).max() + RTOL * np.abs(rec), 4.0 * floor), floor


def check(name, ds, cs, params, what):
    """the reconstruction rule of the module docstring; returns err / tol (max)"""
    got = np.asarray(params.cpu().numpy() if isinstance(params, torch.Tensor) else params, np.float64)
    assert got.shape == (cs["y"].shape[0], ds.P), (what, got.shape)
    rec, tol, floor = tolerance(ds, cs)
    err = np.abs(ds.reconstruct(ds.unpack(got)) - rec)
    ratio = (err / tol).max()
    print(f"[fit] {what}: max|y| {np.abs(cs['y']).max():.3e}  max err {err.max():.3e}  f32-fit floor {floor:.3e}  "
          f"project rule {RTOL * np.abs(cs['y']).max():.3e}  err/tol {ratio:.3f}")
    assert np.isfinite(got).all() and not (err > tol).any(), f"{what}: max err {err.max():.3e}, {(err > tol).sum()} outside"
    if name in WELL_CONDITIONED:
        p64 = ds.pack(cs["p64"])
        pf = np.abs(ds.pack(cs["p32"].astype(np.float64)) - p64).max()
        perr = np.abs(got - p64)
        ptol = np.maximum(RTOL * np.abs(p64).max() + RTOL * np.abs(p64), 4.0 * pf)
        print(f"[fit] {what} params: max|p| {np.abs(p64).max():.3e}  max err {perr.max():.3e}  f32-fit floor {pf:.3e}  "
              f"err/tol {(perr / ptol).max():.3f}")
        assert not (perr > ptol).any(), f"{what} params: max err {perr.max():.3e}"
    return ratio


def fit(eng, name, cs, **kw):
    return eng.fit_trajectory(dev(cs["y"]), dev(cs["ip"]), dev(cs["iv"]), config(name)[5], reg=REG, **kw)


# ---- 1. parity with the float64 fit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name", SHARED)
def test_fit_matches_the_float64_fit(name, B):
    eng = engine_for(name)
    ds, cs = design(name), case(name, B, B)
    assert eng.num_steps == ds.T and eng.num_params == ds.P
    params = fit(eng, name, cs)
    torch.cuda.synchronize()
    mp = "dmp_resp" if "dmp_response" in name else config(name)[2].trajectory_generator_type
    assert eng.last_kernel() == f"k_traj_fit_tile<{mp}>", eng.last_kernel()
    assert params.dtype == torch.float32 and not params.requires_grad
    check(name, ds, cs, params, f"{name} B={B}")


def test_sixteen_table_columns():
    """the 16-column handle's fit solves a 14 x 14 system per DoF in the table's 16 slots"""
    ds = design("prodmp_16_columns_7_dof")
    assert ds.Kloc == 14 and design("promp_16_columns_3_dof").Kloc == 16


# ---- 2. properties -------------------------------------------------------------------------------------------------------------------
def bits(x):
    return x.view(torch.int32)


@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded", "prodmp_5_steps_3_dof"])
def test_deterministic_and_alignment_free(name):
    """two launches give equal bits, and so does pos taken as a view 1, 2 and 3 floats into a larger buffer"""
    eng = engine_for(name)
    cs = case(name, 5, 21)
    first = fit(eng, name, cs)
    assert torch.equal(bits(first), bits(fit(eng, name, cs)))
    y = dev(cs["y"])
    for shift in (1, 2, 3):
        buf = torch.empty(y.numel() + 4, device="cuda")
        view = buf[shift:shift + y.numel()].view(y.shape)
        view.copy_(y)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        got = eng.fit_trajectory(view, dev(cs["ip"]), dev(cs["iv"]), config(name)[5], reg=REG)
        assert torch.equal(bits(first), bits(got)), shift


def test_batch_wraps_around_the_grid():
    """more episode groups than the capped grid covers in one pass (two episodes per group, four waves, at most 8 workgroups per CU):
    the rule, and the bits of the same episodes fitted in two halves"""
    name = "cfg2_prodmp_25_steps"
    B = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 117
    eng = engine_for(name)
    ds, cs = design(name), case(name, B, 11)
    big = fit(eng, name, cs)
    check(name, ds, cs, big, f"{name} B={B}")
    half = B // 2 + 1                                   # odd split: the second half's groups pair other episodes
    y, ip, iv = dev(cs["y"]), dev(cs["ip"]), dev(cs["iv"])
    parts = [eng.fit_trajectory(y[lo:hi], ip[lo:hi], iv[lo:hi], 0.0, reg=REG) for lo, hi in ((0, half), (half, B))]
    assert torch.equal(bits(big), bits(torch.cat(parts)))


@pytest.mark.parametrize("name", ["cfg2_prodmp", "prodmp_1_dof"])
def test_a_nan_stays_in_its_episode(name):
    eng = engine_for(name)
    cs = case(name, 19, 5)
    clean = fit(eng, name, cs)
    y = dev(cs["y"]).clone()
    y[7, 3, 0] = float("nan")
    got = eng.fit_trajectory(y, dev(cs["ip"]), dev(cs["iv"]), config(name)[5], reg=REG)
    keep = [b for b in range(19) if b != 7]
    assert torch.equal(bits(got[keep]), bits(clean[keep]))
    assert torch.isnan(got[7]).any()


@pytest.mark.parametrize("name", ["cfg1_promp_zero_padded", "cfg2_prodmp", "cfg3_dmp_response", "cfg4_prodmp_init_time"])
def test_the_forward_of_the_fit_is_no_worse_than_the_reference(name):
    """trajectory(fit_trajectory(y)) has an objective no larger than trajectory(p_ref rounded to float32) plus the tolerance"""
    eng = engine_for(name)
    ds, cs = design(name), case(name, 6, 31)
    it = config(name)[5]
    ip, iv = dev(cs["ip"]), dev(cs["iv"])
    params = fit(eng, name, cs)
    pos_fit = eng.trajectory(params, ip, iv, it)[0].cpu().numpy().astype(np.float64)
    p_ref32 = ds.pack(cs["p64"]).astype(np.float32)
    pos_ref = eng.trajectory(dev(p_ref32), ip, iv, it)[0].cpu().numpy().astype(np.float64)
    _, tol, _ = tolerance(ds, cs)
    y = cs["y"].astype(np.float64)

    def obj(pos, p, slack):
        return ((np.abs(pos - y) + slack) ** 2).sum(axis=1) + REG * (ds.unpack(p.astype(np.float64)) ** 2).sum(axis=2)
    got, ref = obj(pos_fit, params.cpu().numpy(), 0.0), obj(pos_ref, p_ref32, tol)
    print(f"[fit] {name} objective: fit {got.max():.6e}  reference + tolerance {ref.max():.6e}  min margin {(ref - got).min():.3e}")
    assert (got <= ref).all()


@pytest.mark.parametrize("name", WELL_CONDITIONED)
def test_exact_demonstrations_come_back(name):
    """float32 demonstrations the handle itself produced: trajectory(fit(y)) returns y to the project's rule"""
    eng = engine_for(name)
    ds = design(name)
    it = config(name)[5]
    _, ip, iv, gen = R.demonstrations(ds, 4, 41)
    y = eng.trajectory(dev(gen), dev(ip), dev(iv), it)[0]
    params = eng.fit_trajectory(y, dev(ip), dev(iv), it, reg=REG)
    back = eng.trajectory(params, dev(ip), dev(iv), it)[0].cpu().numpy().astype(np.float64)
    ref = y.cpu().numpy().astype(np.float64)
    err = np.abs(back - ref)
    tol = RTOL * np.abs(ref).max() + RTOL * np.abs(ref)
    print(f"[fit] {name} exact demonstrations: max|y| {np.abs(ref).max():.3e}  max err {err.max():.3e}")
    assert not (err > tol).any()


@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded", "cfg3_dmp_response"])
def test_large_reg_is_the_adjoint_contraction(name):
    """reg = 1e6: the fit tends to Psi^T (y - c) / reg, which is trajectory_vjp(y - c, None)[0] / reg -- the new contraction against
    the existing one, by the RTOL rule (the neglected term is |Psi^T Psi| / reg <= 2e-4 of the result; the rule is applied to
    (Psi^T Psi + reg I) p, which the fit makes equal to Psi^T (y - c) exactly)"""
    eng = engine_for(name)
    ds, cs = design(name), case(name, 5, 51)
    it, big = config(name)[5], 1e6
    params = eng.fit_trajectory(dev(cs["y"]), dev(cs["ip"]), dev(cs["iv"]), it, reg=big)
    resid = dev((cs["y"].astype(np.float64) - cs["c"]).astype(np.float32))
    g = eng.trajectory_vjp(resid, None, it, need=(True, False, False))[0].cpu().numpy().astype(np.float64)
    p = ds.unpack(params.cpu().numpy().astype(np.float64))
    lhs = np.einsum("dtk,dtl,bdl->bdk", ds.Psi, ds.Psi, p) + big * p
    lhs = ds.pack(lhs)[:, ds.off:]
    g = g[:, ds.off:]
    err = np.abs(lhs - g)
    tol = RTOL * np.abs(g).max() + RTOL * np.abs(g)
    print(f"[fit] {name} adjoint tie-in: max|Psi^T r| {np.abs(g).max():.3e}  max err {err.max():.3e}")
    assert not (err > tol).any()


# ---- 3. refusals that need a device handle: the documented exception, the limit in the message, no launch -------------------------------
def test_refusals_happen_before_any_launch():
    wide_cols, wide_dof = engine_for("prodmp_17_columns_7_dof"), engine_for("prodmp_wide_20_dof")
    for eng, D in ((wide_cols, 7), (wide_dof, 20)):
        y = torch.zeros((2, eng.num_steps, D), device="cuda")
        z = torch.zeros((2, D), device="cuda")
        eng.trajectory(torch.zeros((2, eng.num_params), device="cuda"), z, z)
        before = eng.last_kernel()
        with pytest.raises(NotImplementedError, match="at most 16 DoF and 16 table columns"):
            eng.fit_trajectory(y, z, z)
        assert eng.last_kernel() == before
    # a DMP off its response route: alpha ds > 1
    dmp = make_engine(O.PhaseCfg("exp", tau=0.3), O.BasisCfg("rbf", num_basis=5), O.TrajCfg("dmp", action_dim=4, alpha=25.0), 0.02, 0.4)
    y, z = torch.zeros((2, dmp.num_steps, 4), device="cuda"), torch.zeros((2, 4), device="cuda")
    with pytest.raises(NotImplementedError, match="response rows only"):
        dmp.fit_trajectory(y, z, z)
    assert dmp.last_kernel() == ""
    # phase_params on a shared-phase handle
    eng = engine_for("cfg2_prodmp")
    y, z = torch.zeros((2, eng.num_steps, 7), device="cuda"), torch.zeros((2, 7), device="cuda")
    with pytest.raises(ValueError, match="phase_params"):
        eng.fit_trajectory(y, z, z, phase_params=torch.ones((2, 1), device="cuda"))
    with pytest.raises(ValueError, match="reg"):
        eng.fit_trajectory(y, z, z, reg=0.0)
    assert eng.last_kernel() == ""


# ---- 4. per-episode phase: learned tau / delay, per-episode init_time (k_phase_fit) ----------------------------------------------------
def phase_fit_kq(bc, tc):
    """the instantiation k_phase_fit<MP, KQ> a configuration takes, by phase_fit_limits' rule (csrc/mpk_traj_fit.hip): a ProMP needs its
    KT table columns (the basis functions, plus the init_pos column of a zero-padded basis), a ProDMP num_basis + 3 (weights, goal, y_b,
    v_b); KQ = 1 for a ProMP that needs <= 4, 2 for <= 8, else 4 (at most 16); a lane row holds KS = 4 KQ columns"""
    prodmp = tc.trajectory_generator_type == "prodmp"
    need = bc.num_basis + 3 if prodmp else bc.num_basis + int(bc.basis_generator_type == "zero_rbf")
    assert need <= 16, need
    return 1 if need <= 4 and not prodmp else (2 if need <= 8 else 4)


ROUND_T, ROUND_D = (1, 2, 3, 63, 64, 65, 129), (1, 7)


def round_config(kind, D, T):
    """the lane map's round boundaries: T steps of dt = 0.01 exactly.  ProMP: linear phase, 5 plain RBFs, learned tau (the phase runs to
    1 at tau = T dt); ProDMP: 4 basis functions, learned tau and delay"""
    dt = 0.01
    if kind == "promp":
        return (O.PhaseCfg("linear", tau=T * dt, learn_tau=True, tau_bound=(0.5 * T * dt, T * dt)),
                O.BasisCfg("rbf", num_basis=5, basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=D, weights_scale=0.9), dt, T * dt)
    return (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.4, 1.0), delay_bound=(0.0, 0.008)),
            O.BasisCfg("prodmp", num_basis=4, alpha=20, basis_bandwidth_factor=3),
            O.TrajCfg("prodmp", action_dim=D, weights_scale=0.6, goal_scale=1.2, auto_scale_basis=True), dt, T * dt)


# name -> the KQ of k_phase_fit<MP, KQ> the row must take (tests/test_traj_fit_host.py holds it against phase_fit_kq and checks that the
# table reaches all five instantiations and every count of right-hand-side slots); D x KS = DoF x 4 KQ entries of Psi^T (y - c), 64 a slot
PHASE_KQ = {
    "tt_prodmp_70_steps": 2, "tt_prodmp_350_steps": 2, "beerpong_promp": 1, "cfg4_three_clocks": 2,
    # the learned-phase and phase-vjp tables' rows
    "promp_5dof_learn_both": 2,                   # zero-padded, tau and delay
    "prodmp_3dof_learn_tau": 2,                   # the goal fitted, weights_scale and goal_scale
    "promp_16dof_learn_tau": 1,                   # D = 16: D x KS = 64, one slot exactly full
    "tt_prodmp_replan": 2,                        # goal_offset given and ignored (the reference's default mode)
    "promp_exp_learn_both": 2,                    # exp phase, no zero padding: nothing given
    "prodmp_after_scale_no_weights": 2,           # the goal alone, init_pos joins the scaled goal
    # new shapes
    "promp_16_basis_16_dof": 4,                   # D x KS = 256: all four slots of every lane; P = 258
    "promp_9_basis_5_dof": 4,                     # D x KS = 80: two slots, the second part full
    "promp_8_basis_9_dof": 2,                     # D x KS = 72
    "promp_10_basis_11_dof": 4,                   # D x KS = 176: three slots
    "promp_zero_12_basis_3_dof": 4,               # 13 columns, the padding column given
    "prodmp_13_basis_16_dof_relative_goal": 4,    # the largest LDS block, D x KS = 256
    "prodmp_6_basis_three_clocks": 4,             # the smallest KQ-4 ProDMP; per-episode init_time, no learned timing
    "prodmp_13_basis_1_dof_no_goal": 4,
    "prodmp_4_basis_12_dof_goal_offset_add": 2,   # the goal-offset column given (mode 'add'); D x KS = 96
    "promp_round_t5_d3": 2, "prodmp_round_t5_d3": 2,      # the wrap-around test's episodes
}
PHASE_KQ.update({f"promp_round_t{T}_d{D}": 2 for T in ROUND_T for D in ROUND_D})
PHASE_KQ.update({f"prodmp_round_t{T}_d{D}": 2 for T in ROUND_T for D in ROUND_D})
PHASE_TABLE = [n for n in PHASE_KQ if "_round_t" not in n or n.endswith("_t5_d3")]


@functools.lru_cache(maxsize=None)
def phase_configs():
    from . import phase_vjp_ref as V
    from .test_gpu_learned_phase import CONFIGS as LP, CONFIGS_ALL
    tt, bp, c4 = LP["tt_prodmp"], LP["beerpong_promp"], CONFIGS_ALL["cfg4_prodmp_replan"]
    clocks = np.array([0.0, 0.4, 0.8], np.float32)
    out = {
        # name: (pc, bc, tc, dt, duration, per-episode init_time)
        "tt_prodmp_70_steps": tt[:4] + (70 * tt[3], None),            # two lane rounds, the second ragged
        "tt_prodmp_350_steps": tt[:5] + (None,),
        "beerpong_promp": bp[:5] + (None,),
        "cfg4_three_clocks": c4[:5] + (clocks,),
    }
    for name in ("promp_5dof_learn_both", "prodmp_3dof_learn_tau", "promp_16dof_learn_tau"):
        out[name] = LP[name][:5] + (None,)
    out["tt_prodmp_replan"] = LP["tt_prodmp_replan"][:4] + (40 * LP["tt_prodmp_replan"][3], None)
    for name in ("promp_exp_learn_both", "prodmp_after_scale_no_weights"):
        out[name] = V.EXTRA[name] + (None,)
    lin = dict(learn_tau=True, tau_bound=(0.4, 0.6))
    both = dict(learn_tau=True, learn_delay=True, tau_bound=(0.4, 0.6), delay_bound=(0.0, 0.1))
    out.update({
        "promp_16_basis_16_dof": (O.PhaseCfg("linear", tau=0.6, **both), O.BasisCfg("rbf", num_basis=16, basis_bandwidth_factor=3),
                                  O.TrajCfg("promp", action_dim=16), 0.02, 0.6, None),
        "promp_9_basis_5_dof": (O.PhaseCfg("linear", tau=0.6, **lin), O.BasisCfg("rbf", num_basis=9, basis_bandwidth_factor=3),
                                O.TrajCfg("promp", action_dim=5, weights_scale=0.8), 0.02, 0.6, None),
        "promp_8_basis_9_dof": (O.PhaseCfg("linear", tau=0.6, **lin), O.BasisCfg("rbf", num_basis=8, basis_bandwidth_factor=3),
                                O.TrajCfg("promp", action_dim=9), 0.02, 0.5, None),
        "promp_10_basis_11_dof": (O.PhaseCfg("linear", tau=0.6, **lin), O.BasisCfg("rbf", num_basis=10, basis_bandwidth_factor=3),
                                  O.TrajCfg("promp", action_dim=11), 0.02, 0.6, None),
        "promp_zero_12_basis_3_dof": (O.PhaseCfg("linear", tau=0.6, learn_delay=True, delay_bound=(0.0, 0.1)),
                                      O.BasisCfg("zero_rbf", num_basis=12, num_basis_zero_start=1, num_basis_zero_goal=1,
                                                 basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=3), 0.02, 0.7, None),
        "prodmp_13_basis_16_dof_relative_goal": (O.PhaseCfg("exp", tau=0.6, alpha_phase=3.0, **both),
                                                 O.BasisCfg("prodmp", num_basis=13, alpha=25, basis_bandwidth_factor=3),
                                                 O.TrajCfg("prodmp", action_dim=16, weights_scale=0.7, goal_scale=1.3, auto_scale_basis=True,
                                                           relative_goal=True), 0.02, 0.5, None),
        "prodmp_6_basis_three_clocks": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=6, alpha=15),
                                        O.TrajCfg("prodmp", action_dim=3, auto_scale_basis=True), 0.02, 0.6, clocks),
        "prodmp_13_basis_1_dof_no_goal": (O.PhaseCfg("exp", tau=0.6, alpha_phase=3.0, **lin),
                                          O.BasisCfg("prodmp", num_basis=13, alpha=25, basis_bandwidth_factor=3),
                                          O.TrajCfg("prodmp", action_dim=1, auto_scale_basis=True, disable_goal=True), 0.02, 0.7, None),
        "prodmp_4_basis_12_dof_goal_offset_add": (O.PhaseCfg("exp", tau=0.6, alpha_phase=3.0, **lin),
                                                  O.BasisCfg("prodmp", num_basis=4, alpha=15, basis_bandwidth_factor=2),
                                                  O.TrajCfg("prodmp", action_dim=12, goal_scale=0.8, goal_offset_mode="add",
                                                            goal_offset=-0.7), 0.02, 0.5, None),
    })
    for kind in ("promp", "prodmp"):
        out[f"{kind}_round_t5_d3"] = round_config(kind, 3, 5) + (None,)
        for T in ROUND_T:
            for D in ROUND_D:
                out[f"{kind}_round_t{T}_d{D}"] = round_config(kind, D, T) + (None,)
    assert set(out) == set(PHASE_KQ)
    return out


def phase_values(pc, B, rng):
    """[B, n_phase] float32: episode b inside the bounds (b % 3 == 1), on them (b % 3 == 2) or outside them (b % 3 == 0)"""
    cols = []
    for on, (lo, hi) in ((pc.learn_tau, pc.tau_bound), (pc.learn_delay, pc.delay_bound)):
        if not on:
            continue
        v = np.empty(B)
        for b in range(B):
            kind = b % 3
            if kind == 1:
                v[b] = lo + rng.uniform(0.2, 0.8) * (hi - lo)
            elif kind == 2:
                v[b] = hi if (b // 3) % 2 == 0 else lo
            else:
                v[b] = hi + 0.25 * (hi - lo) if (b // 3) % 2 == 0 else lo - 0.25 * (hi - lo)
        cols.append(v)
    return np.stack(cols, axis=1).astype(np.float32) if cols else np.zeros((B, 0), np.float32)


class FirstStepDesign(R.Design):
    """a one-step ProMP.  The oracle's finite-difference velocity needs two steps, so this is the first step of the two-step grid of the
    same configuration: the same first time (asserted), hence the same phase and row"""

    def __init__(self, pc, bc, tc, dt, duration, init_time=0.0, phase=()):
        assert O.num_steps(duration, dt) == 1 and tc.trajectory_generator_type == "promp"
        assert np.array_equal(O.make_times(duration, dt, init_time), O.make_times(2 * dt, dt, init_time)[:1])
        super().__init__(pc, bc, tc, dt, 2 * dt, init_time, phase)
        self.Psi = np.ascontiguousarray(self.Psi[:, :1])
        self.Psi.setflags(write=False)
        self.T = 1

    def offset(self, init_pos, init_vel):
        return super().offset(init_pos, init_vel)[:, :1]

    def forward(self, params, init_pos, init_vel):
        return super().forward(params, init_pos, init_vel)[:, :1]


@functools.lru_cache(maxsize=None)
def phase_case(name, B, seed=0):
    """per episode: its own design (the oracle at that episode's tau / delay / init_time), demonstration and CPU fits"""
    pc, bc, tc, dt, duration, clocks = phase_configs()[name]
    rng = np.random.default_rng(100 + seed + B)
    phase = phase_values(pc, B, rng)
    it = None if clocks is None else clocks[np.arange(B) % len(clocks)]
    one_step = tc.trajectory_generator_type == "promp" and O.num_steps(duration, dt) == 1
    eps = []
    for b in range(B):
        ds = (FirstStepDesign if one_step else R.Design)(pc, bc, tc, dt, duration, 0.0 if it is None else float(it[b]), phase[b])
        y, ip, iv, _ = R.demonstrations(ds, 1, 1000 * seed + 10 * B + b)
        c = ds.offset(ip, iv)
        eps.append(dict(ds=ds, y=y, ip=ip, iv=iv, c=c, p64=R.fit64(ds, y, c, REG), p32=R.fit32(ds, y, c, REG)))
    stack = lambda k: np.concatenate([e[k] for e in eps])      # noqa: E731
    return dict(eps=eps, phase=phase, it=it, y=stack("y"), ip=stack("ip"), iv=stack("iv"), cfg=(pc, bc, tc, dt, duration))


def phase_engine(name):
    pc, bc, tc, dt, duration, _ = phase_configs()[name]
    return make_engine(pc, bc, tc, dt, duration)


def phase_fit(eng, cs, y=None):
    n_phase = cs["phase"].shape[1]
    it = 0.0 if cs["it"] is None else dev(cs["it"])
    return eng.fit_trajectory(dev(cs["y"]) if y is None else y, dev(cs["ip"]), dev(cs["iv"]), it, reg=REG,
                              phase_params=dev(cs["phase"]) if n_phase else None)


def phase_check(cs, params, what):
    got = params.cpu().numpy()
    n_phase = cs["phase"].shape[1]
    assert np.array_equal(got[:, :n_phase].view(np.int32), cs["phase"].view(np.int32)), "the phase parameters come back as given"
    recs = [e["ds"].reconstruct(e["p64"]) for e in cs["eps"]]
    floor = max(np.abs(e["ds"].reconstruct(e["p32"]) - r).max() for e, r in zip(cs["eps"], recs))
    scale = np.abs(cs["y"]).max()
    worst = 0.0
    for b, (e, rec) in enumerate(zip(cs["eps"], recs)):
        p = e["ds"].unpack(got[b:b + 1].astype(np.float64))
        err = np.abs(e["ds"].reconstruct(p) - rec)
        tol = np.maximum(RTOL * scale + RTOL * np.abs(rec), 4.0 * floor)
        worst = max(worst, (err / tol).max())
        assert np.isfinite(got[b]).all() and not (err > tol).any(), f"{what} episode {b}: max err {err.max():.3e}, floor {floor:.3e}"
    print(f"[fit] {what}: max|y| {scale:.3e}  f32-fit floor {floor:.3e}  project rule {RTOL * scale:.3e}  err/tol {worst:.3f}")


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("name", PHASE_TABLE)
def test_per_episode_phase_fit_matches_the_float64_fit(name, B):
    eng = phase_engine(name)
    cs = phase_case(name, B)
    params = phase_fit(eng, cs)
    torch.cuda.synchronize()
    mp = cs["cfg"][2].trajectory_generator_type
    assert eng.last_kernel() == f"k_phase_fit<{mp}>", eng.last_kernel()
    phase_check(cs, params, f"{name} B={B}")
    assert eng.fit_status() is False
    eng.check_range()


def test_per_episode_phase_fit_properties():
    """equal bits from two launches and from views 1, 2, 3 floats into a larger buffer; a NaN stays in its episode; the forward of the
    fit is what the fit promised (positions at the clipped timing reproduce the reference's reconstruction)"""
    phase_fit_properties("tt_prodmp_70_steps")


@pytest.mark.parametrize("name", ["promp_9_basis_5_dof", "prodmp_13_basis_16_dof_relative_goal"])
def test_per_episode_phase_fit_properties_of_sixteen_column_rows(name):
    """the same properties where a lane row has 16 columns (KQ = 4), ProMP and ProDMP: the forward's per-episode kernel takes these
    handles too"""
    assert PHASE_KQ[name] == 4
    phase_fit_properties(name)


def phase_fit_properties(name):
    eng = phase_engine(name)
    cs = phase_case(name, 9)
    first = phase_fit(eng, cs)
    assert torch.equal(bits(first), bits(phase_fit(eng, cs)))
    y = dev(cs["y"])
    for shift in (1, 2, 3):
        buf = torch.empty(y.numel() + 4, device="cuda")
        view = buf[shift:shift + y.numel()].view(y.shape)
        view.copy_(y)
        assert torch.equal(bits(first), bits(phase_fit(eng, cs, view))), shift
    bad = y.clone()
    bad[4, 10, 2] = float("nan")
    got = phase_fit(eng, cs, bad)
    keep = [b for b in range(9) if b != 4]
    assert torch.equal(bits(got[keep]), bits(first[keep])) and torch.isnan(got[4]).any()
    assert eng.fit_status() is False                    # a NaN demonstration is not a Gram matrix without a factor
    pos = eng.trajectory(first, dev(cs["ip"]), dev(cs["iv"]), 0.0)[0].cpu().numpy().astype(np.float64)
    for b, e in enumerate(cs["eps"]):
        ref = e["ds"].reconstruct(e["p64"])[0] + e["c"][0]
        floor = np.abs(e["ds"].reconstruct(e["p32"]) - e["ds"].reconstruct(e["p64"])).max()
        err = np.abs(pos[b] - ref)
        tol = np.maximum(RTOL * np.abs(cs["y"]).max() + RTOL * np.abs(ref), 4.0 * floor)
        assert not (err > tol).any(), (b, err.max())


def test_per_episode_phase_refusals():
    from .test_gpu_learned_phase import CONFIGS as LP
    pc, bc, tc, dt, duration = LP["tt_prodmp"][:5]
    eng = make_engine(pc, bc, tc, dt, duration)
    y, z = torch.zeros((2, eng.num_steps, 7), device="cuda"), torch.zeros((2, 7), device="cuda")
    with pytest.raises(ValueError, match="phase_params"):
        eng.fit_trajectory(y, z, z)
    with pytest.raises(ValueError, match=r"phase_params must be \[2, 2\]"):
        eng.fit_trajectory(y, z, z, phase_params=torch.ones((2, 1), device="cuda"))
    assert eng.last_kernel() == ""
    # a DMP with a per-episode init_time
    dmp = engine_for("cfg3_dmp_response")
    y, z = torch.zeros((2, dmp.num_steps, 7), device="cuda"), torch.zeros((2, 7), device="cuda")
    with pytest.raises(NotImplementedError, match="Euler recurrence"):
        dmp.fit_trajectory(y, z, z, torch.zeros(2, device="cuda"))
    assert dmp.last_kernel() == ""


def test_per_episode_phase_limits_are_refused_before_any_launch():
    """beyond the wave kernel's shapes: NotImplementedError with the limit in the message, nothing launched; an empty batch on a
    learned-phase handle is an empty result, nothing launched either"""
    tau = dict(learn_tau=True, tau_bound=(0.4, 0.6))
    wide = {
        "17 ProMP basis functions": (O.PhaseCfg("linear", tau=0.6, **tau), O.BasisCfg("rbf", num_basis=17), O.TrajCfg("promp", action_dim=3),
                                     "<= 16 columns"),
        "14 ProDMP basis functions": (O.PhaseCfg("exp", tau=0.6, **tau), O.BasisCfg("prodmp", num_basis=14, alpha=25),
                                      O.TrajCfg("prodmp", action_dim=3), "<= 16 columns"),
        "17 DoF": (O.PhaseCfg("linear", tau=0.6, **tau), O.BasisCfg("rbf", num_basis=3), O.TrajCfg("promp", action_dim=17), "<= 16 DoF"),
    }
    for what, (pc, bc, tc, limit) in wide.items():
        eng = make_engine(pc, bc, tc, 0.02, 0.6)
        D = tc.action_dim
        y, z = torch.zeros((2, eng.num_steps, D), device="cuda"), torch.zeros((2, D), device="cuda")
        before = eng.last_kernel()
        with pytest.raises(NotImplementedError, match=limit):
            eng.fit_trajectory(y, z, z, phase_params=torch.full((2, 1), 0.5, device="cuda"))
        assert eng.last_kernel() == before, what
    name = "promp_9_basis_5_dof"
    eng = phase_engine(name)
    empty = eng.fit_trajectory(torch.zeros((0, eng.num_steps, 5), device="cuda"), torch.zeros((0, 5), device="cuda"),
                               torch.zeros((0, 5), device="cuda"), phase_params=torch.zeros((0, 1), device="cuda"))
    assert tuple(empty.shape) == (0, eng.num_params) and empty.dtype == torch.float32 and eng.last_kernel() == ""


@pytest.mark.parametrize("D", ROUND_D)
@pytest.mark.parametrize("T", ROUND_T)
@pytest.mark.parametrize("kind", ["promp", "prodmp"])
def test_per_episode_phase_fit_at_the_round_boundaries(kind, T, D):
    """lane <-> time step, 64 steps a round: one step, a round less one, a full round, a round and one, two rounds and one.  With fewer
    steps than fitted columns (5) reg decides, as in the shared table's under-determined rows"""
    name = f"{kind}_round_t{T}_d{D}"
    eng = phase_engine(name)
    cs = phase_case(name, 3)
    assert eng.num_steps == T == cs["eps"][0]["ds"].T
    params = phase_fit(eng, cs)
    torch.cuda.synchronize()
    assert eng.last_kernel() == f"k_phase_fit<{kind}>", eng.last_kernel()
    phase_check(cs, params, f"{name} B=3")
    assert eng.fit_status() is False
    eng.check_range()


@pytest.mark.parametrize("name", ["promp_round_t5_d3", "prodmp_round_t5_d3"])
def test_per_episode_batch_wraps_around_the_grid(name):
    """every wave of the capped grid (four waves a workgroup, at most 8 workgroups per CU) takes at least two episodes, the last trip
    part full.  The batch is the 9 reference-checked episodes of the parity test, tiled: an episode never leaves its wave and its sums
    run in a fixed order, so every row has the bits it has in the 9-episode launch"""
    B = 2 * 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    eng = phase_engine(name)
    cs = phase_case(name, 9)
    small = phase_fit(eng, cs)
    idx = np.arange(B) % 9
    big = eng.fit_trajectory(dev(cs["y"][idx]), dev(cs["ip"][idx]), dev(cs["iv"][idx]), 0.0, reg=REG, phase_params=dev(cs["phase"][idx]))
    assert tuple(big.shape) == (B, eng.num_params) and eng.fit_status() is False
    same = (bits(big) == bits(small)[torch.from_numpy(idx).cuda()]).all(dim=1)
    assert bool(same.all()), f"{int((~same).sum())} of {B} rows differ, the first at {int((~same).nonzero()[0])}"


NPD_REG = 1e-300


def npd_config():
    """a ProMP (linear phase, 8 plain RBFs, 3 DoF) of 12 steps without learned timing: the per-episode init_time tensor selects the phase.
    init_time = 0 gives 12 distinct rows (smallest Gram eigenvalue 5e-2); init_time = 1e6 clips the phase to 1 at every step: 12 equal
    rows, a Gram matrix of rank 1.  (With 5 steps the ordinary episodes' 8 x 8 Gram matrix would have rank 5 and no factor either.)"""
    T, dt = 12, 0.01
    return (O.PhaseCfg("linear", tau=T * dt), O.BasisCfg("rbf", num_basis=8, basis_bandwidth_factor=3), O.TrajCfg("promp", action_dim=3),
            dt, T * dt)


def test_an_episode_without_a_factor_is_flagged_and_stays_alone():
    """16 ordinary episodes interleaved with 16 whose Gram matrix has rank 1, at reg = 1e-300 (which the first addition absorbs): pivots
    1 .. 7 of the deficient ones are rounding residue of either sign.  The float64 emulation of the kernel's order
    (tests/test_traj_fit_host.py::test_the_rank_one_gram_matrix_loses_a_pivot) loses pivot 2 (-1.8e-48 after 1.2e-63 and 2.2e-62); the
    device's rounding may differ, so: fit_status() is True exactly if a row carries a NaN; a row that carries one is NaN throughout;
    the ordinary episodes have the bits they have without the deficient ones beside them, and match their float64 fit; the next launch
    clears the flag; and the deficient episodes (all 16 see the same matrix) were flagged"""
    pc, bc, tc, dt, duration = npd_config()
    eng = make_engine(pc, bc, tc, dt, duration)
    ds = R.Design(pc, bc, tc, dt, duration, 0.0)
    n = 16
    y, ip, iv, _ = R.demonstrations(ds, 2 * n, 77)
    c = ds.offset(ip[:n], iv[:n])
    cs = dict(y=y[:n], p64=R.fit64(ds, y[:n], c, NPD_REG), p32=R.fit32(ds, y[:n], c, NPD_REG))
    order = np.arange(2 * n).reshape(2, n).T.reshape(-1)              # ordinary 0, deficient 0, ordinary 1, ...
    clock = np.where(order < n, 0.0, 1e6).astype(np.float32)
    mixed = eng.fit_trajectory(dev(y[order]), dev(ip[order]), dev(iv[order]), dev(clock), reg=NPD_REG)
    torch.cuda.synchronize()
    assert eng.last_kernel() == "k_phase_fit<promp>"
    status = eng.fit_status()
    alone = eng.fit_trajectory(dev(y[:n]), dev(ip[:n]), dev(iv[:n]), torch.zeros(n, device="cuda"), reg=NPD_REG)
    status_alone = eng.fit_status()
    nan = torch.isnan(mixed).cpu().numpy()
    flagged = nan.any(axis=1)
    print(f"[fit] not positive definite: fit_status {status}, rows with a NaN {np.flatnonzero(flagged).tolist()}, "
          f"flag after the ordinary launch {status_alone}")
    assert status is bool(flagged.any())                               # flag and rows agree
    assert (nan.all(axis=1) == flagged).all()                          # a flagged row is whole
    assert not flagged[0::2].any()
    assert torch.equal(bits(mixed[0::2]), bits(alone))                 # ordinary episodes are untouched
    check("npd_ordinary", ds, cs, alone, "ordinary episodes at reg 1e-300")
    assert status_alone is False                                       # the flag is cleared
    assert flagged[1::2].all(), "the rank-1 episodes kept seven positive pivots on this device: the path was not reached"


def test_the_factor_cache_evicts_and_rebuilds():
    """get_fit_factor keeps 16 factors keyed by (init_time, T, reg) and reuses the oldest slot's device buffer: 18 keys evict the first,
    which then comes back with the bits it had, the bits a fresh handle gives; a new grid with the same step count invalidates all"""
    name = "cfg2_prodmp"
    pc, bc, tc, dt, duration = config(name)[:5]
    cs = case(name, 3, 3)
    y, ip, iv = dev(cs["y"]), dev(cs["ip"]), dev(cs["iv"])
    eng = engine_for(name)

    def run(e, it=0.0, reg=REG):
        return e.fit_trajectory(y, ip, iv, it, reg=reg)
    first = run(eng)
    fresh = run(engine_for(name))
    assert torch.equal(bits(first), bits(fresh))
    regs = [REG * (1 + i) for i in range(18)]
    seen = [run(eng, reg=r) for r in regs]
    assert torch.equal(bits(seen[0]), bits(first)) and not torch.equal(bits(seen[17]), bits(first))
    assert torch.equal(bits(run(eng, reg=regs[0])), bits(first))
    assert torch.equal(bits(run(eng, reg=regs[17])), bits(seen[17]))
    assert torch.equal(bits(run(engine_for(name), reg=regs[17])), bits(seen[17]))
    clocks = [0.02 * i for i in range(18)]
    seen = [run(eng, it=t) for t in clocks]
    assert torch.equal(bits(seen[0]), bits(first)) and not torch.equal(bits(seen[17]), bits(first))
    assert torch.equal(bits(run(eng, it=clocks[0])), bits(first))
    assert torch.equal(bits(run(eng, it=clocks[17])), bits(seen[17]))
    assert torch.equal(bits(run(engine_for(name), it=clocks[17])), bits(seen[17]))
    # another grid of the same 100 steps: the key (init_time, T, reg) is the cached one, the factor is not
    eng.set_duration(0.5 * duration, 0.5 * dt)
    assert eng.num_steps == cs["y"].shape[1]
    other = run(eng)
    assert torch.equal(bits(other), bits(run(make_engine(pc, bc, tc, 0.5 * dt, 0.5 * duration)))) and not torch.equal(bits(other), bits(first))
    eng.set_duration(duration, dt)
    assert torch.equal(bits(run(eng)), bits(first))
    # ... and another horizon (50 steps of the first grid) and back
    eng.set_duration(0.5 * duration, dt)
    short = y[:, :eng.num_steps].contiguous()
    assert short.shape[1] == 50
    assert torch.equal(bits(eng.fit_trajectory(short, ip, iv, 0.0, reg=REG)),
                       bits(make_engine(pc, bc, tc, dt, 0.5 * duration).fit_trajectory(short, ip, iv, 0.0, reg=REG)))
    eng.set_duration(duration, dt)
    assert torch.equal(bits(run(eng)), bits(first))
    assert eng.last_kernel() == "k_traj_fit_tile<prodmp>"


# ---- 5. the layers above the engine -----------------------------------------------------------------------------------------------------
def oracle_config_of(eng):
    """the oracle's configuration of an engine's handle (the inverse of tests/test_gpu_trajectory.py::make_engine)"""
    c = eng.config
    inv = lambda table, v: next(k for k, x in table.items() if x == v)      # noqa: E731
    from fancy_gym_amd import _lib
    pc = O.PhaseCfg(eng.phase_type, tau=c.tau, delay=c.delay, alpha_phase=c.alpha_phase, learn_tau=bool(c.learn_tau),
                    learn_delay=bool(c.learn_delay), tau_bound=tuple(c.tau_bound), delay_bound=tuple(c.delay_bound))
    bc = O.BasisCfg(eng.basis_type, num_basis=c.num_basis, basis_bandwidth_factor=c.basis_bandwidth_factor,
                    num_basis_outside=c.num_basis_outside, num_basis_zero_start=c.num_basis_zero_start,
                    num_basis_zero_goal=c.num_basis_zero_goal, alpha=c.basis_alpha, dt=c.basis_dt,
                    pre_compute_length_factor=c.pre_compute_length_factor)
    tc = O.TrajCfg(eng.mp_type, action_dim=c.num_dof, weights_scale=c.weights_scale, goal_scale=c.goal_scale, alpha=c.dmp_alpha,
                   auto_scale_basis=bool(c.auto_scale_basis), relative_goal=bool(c.relative_goal), disable_goal=bool(c.disable_goal),
                   disable_weights=bool(c.disable_weights), relative_goal_mode=inv(_lib.RELATIVE_GOAL_MODES, c.relative_goal_mode),
                   goal_offset_mode=inv(_lib.GOAL_OFFSET_MODES, c.goal_offset_mode), goal_offset=c.goal_offset)
    return pc, bc, tc, c.dt, c.duration


def test_batched_black_box_fit_trajectory():
    """make_batched("fancy_ProDMP/HoleReacher-v0", 4, random_start=False): the box's fit equals the engine-level call with the box's own
    initial conditions bit for bit, and get_trajectory of it reproduces a smooth demonstration to the rule"""
    from fancy_gym_amd import make_batched
    bb = make_batched("fancy_ProDMP/HoleReacher-v0", 4, random_start=False)
    bb.reset(seed=3)
    eng = bb.engine
    T, D = eng.num_steps, eng.num_dof
    t = torch.linspace(0.0, 1.0, T, device="cuda")[None, :, None]
    phase = torch.arange(4, device="cuda")[:, None, None] * 0.3 + torch.arange(D, device="cuda")[None, None, :] * 0.5
    start = bb.q.float()[:, None, :]
    demo = (start + 0.8 * torch.sin(2.0 * t + phase) - 0.8 * torch.sin(phase) + 0.3 * t * t).contiguous()
    params = bb.fit_trajectory(demo)
    assert eng.last_kernel() == "k_traj_fit_tile<prodmp>" and params.shape == (4, eng.num_params)
    ip, iv = bb.q.float(), bb.qd.float()
    assert torch.equal(bits(params), bits(eng.fit_trajectory(demo, ip, iv, 0.0, reg=1e-9)))
    des = bb.get_trajectory(params)["des_pos"].cpu().numpy().astype(np.float64)
    ds = R.Design(*oracle_config_of(eng), 0.0)
    assert (ds.T, ds.D, ds.P) == (T, D, eng.num_params)
    y, ip_h, iv_h = demo.cpu().numpy(), ip.cpu().numpy(), iv.cpu().numpy()
    c = ds.offset(ip_h, iv_h)
    cs = dict(y=y, p64=R.fit64(ds, y, c, REG), p32=R.fit32(ds, y, c, REG))
    check("hole_reacher_prodmp", ds, cs, params, "BatchedBlackBox.fit_trajectory")
    rec, tol, _ = tolerance(ds, cs)
    err = np.abs(des - (rec + c))
    print(f"[fit] BatchedBlackBox get_trajectory(fit): max |des_pos - reference reconstruction| {err.max():.3e}, "
          f"max |des_pos - demonstration| {np.abs(des - y).max():.3e}")
    assert not (err > tol + RTOL * np.abs(rec + c).max()).any()       # the fit's rule plus the forward's own 1e-5 contract
    assert isinstance(bb.step(params), dict)                          # ... and it can be handed straight to step


def test_learn_mp_params_from_trajs_on_the_device():
    """mp_pytorch's name on the MPInterface: the result reproduces what the engine-level call gives, defaults from the first samples"""
    from fancy_gym_amd.black_box.factory import get_basis_generator, get_phase_generator, get_trajectory_generator
    pg = get_phase_generator("exp", tau=1.5, alpha_phase=3.0)
    gen = get_trajectory_generator("prodmp", 3, get_basis_generator("prodmp", pg, num_basis=4, alpha=10))
    gen.set_duration(1.0, 0.02)
    eng = gen.engine()
    grid = eng.times()
    T = grid.shape[0]
    rng = np.random.default_rng(2)
    want = rng.standard_normal((5, eng.num_params)).astype(np.float32)
    ip, iv = rng.uniform(-1, 1, (5, 3)).astype(np.float32), rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    y = eng.trajectory(dev(want), dev(ip), dev(iv), 0.0)[0]
    out = gen.learn_mp_params_from_trajs(np.broadcast_to(grid, (5, T)), y, init_time=0.0, init_pos=ip, init_vel=iv)
    assert set(out) == {"params", "init_time", "init_pos", "init_vel"} and out["params"].shape == (5, eng.num_params)
    assert torch.equal(bits(out["params"]), bits(eng.fit_trajectory(y, dev(ip), dev(iv), 0.0, reg=1e-9)))
    back = eng.trajectory(out["params"], dev(ip), dev(iv), 0.0)[0]
    err = (back - y).abs().max().item()
    print(f"[fit] learn_mp_params_from_trajs: max |trajectory(fit) - demonstration| {err:.3e} of max {y.abs().max().item():.3e}")
    assert err <= 2 * RTOL * y.abs().max().item()
    # the defaulting rule: init_time = times[..., 0], init_pos the first sample, init_vel the first finite difference; the T samples
    # behind the first lie on the handle's grid and are fitted
    t_all = np.concatenate([[0.25], grid + np.float32(0.25)]).astype(np.float32)
    y_all = torch.cat([dev(ip[:1])[:, None, :], eng.trajectory(dev(want[:1]), dev(ip[:1]), dev(iv[:1]), 0.25)[0]], dim=1)[0]
    d = gen.learn_mp_params_from_trajs(t_all, y_all)
    assert d["params"].shape == (eng.num_params,) and float(d["init_time"]) == 0.25
    fd = ((y_all[1] - y_all[0]) / float(t_all[1] - t_all[0])).cpu()
    assert torch.equal(d["init_pos"], y_all[0].cpu()) and torch.equal(d["init_vel"], fd)
    assert torch.equal(bits(d["params"]), bits(eng.fit_trajectory(y_all[None, 1:], y_all[None, 0], dev(fd)[None], 0.25, reg=1e-9)[0]))
    assert gen.params is not None and gen.init_time == 0.25
    with pytest.raises(ValueError, match=f"needs {T + 1} samples"):
        gen.learn_mp_params_from_trajs(t_all[1:], y_all[1:])


def test_the_example_runs_and_lands_inside_the_rule(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("batched_demonstration_fit", os.path.join(ROOT, "examples", "batched_demonstration_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    eng = mod.make_engine()
    e_fit, e_adam, params = mod.run(envs=8, adam_iters=20, engine=eng)
    printed = capsys.readouterr().out
    assert "closed form: RMS reconstruction error" in printed and "one launch of k_traj_fit_tile<prodmp>" in printed and "Adam, 20" in printed
    want, ip, iv = mod.demonstrations(eng, 8, 0.05, 0)
    ds = design("cfg2_prodmp")                         # the example's handle is cfg2's
    y, ip_h, iv_h = want.cpu().numpy(), ip.cpu().numpy(), iv.cpu().numpy()
    c = ds.offset(ip_h, iv_h)
    cs = dict(y=y, p64=R.fit64(ds, y, c, REG), p32=R.fit32(ds, y, c, REG))
    check("example", ds, cs, params, "examples/batched_demonstration_fit.py --envs 8")
    ref_rms = np.sqrt(((ds.reconstruct(cs["p64"]) + c - y) ** 2).mean())
    print(f"[fit] example: RMS {e_fit:.4e}, float64 reference {ref_rms:.4e}, Adam after 20 iterations {e_adam:.4e}")
    assert abs(e_fit - ref_rms) <= 1e-4 * ref_rms + 1e-6 and e_fit <= e_adam
