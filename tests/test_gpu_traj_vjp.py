"""
mpk_trajectory_vjp and the autograd wiring of TrajectoryEngine.trajectory on the GPU.

Yardstick: the float64 CPU oracle (oracle/mp_oracle.py).  With a shared phase the trajectory is affine in (params, init_pos, init_vel),
so column i of the Jacobian is f(e_i) - f(0) in float64; J is built explicitly per configuration (a few hundred inputs at most, one
batched oracle call, cached) and the reference gradient is J^T g in float64.

Bound (per output array): the larger of the project's rule 1e-5 * max|ref| + 1e-5 * |ref| (tests/test_gpu_trajectory.py) and 4 x the
error of a plain float32 CPU torch.einsum of the float32-rounded J with g against the same float64 value -- what any float32 sum over T
pays.  Every comparison prints both maxima before it asserts.
"""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import mp_oracle as O

from .test_gpu_trajectory import CFG1, CFG2, CFG3, CFG4, RTOL, make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    # name: (pc, bc, tc, dt, duration, init_time, route)
    "cfg1_promp_zero_padded": CFG1 + (0.0, "tile"),
    "cfg2_prodmp": CFG2 + (0.0, "tile"),
    "cfg3_dmp_response": CFG3 + (0.0, "tile"),
    "cfg4_prodmp_init_time": CFG4 + (25 * 0.02, "tile"),
    "prodmp_relative_goal": (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                             O.TrajCfg("prodmp", action_dim=3, relative_goal=True, weights_scale=0.7, goal_scale=1.3), 0.02, 1.0,
                             0.0, "tile"),
    "prodmp_relative_goal_after_scale": (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=4, alpha=10),
                                         O.TrajCfg("prodmp", action_dim=2, relative_goal=True, goal_scale=1.3,
                                                   relative_goal_mode="after_scale", disable_weights=True), 0.02, 0.5, 0.0, "tile"),
    "prodmp_12_columns_16_dof": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=9, alpha=15),
                                 O.TrajCfg("prodmp", action_dim=16), 0.02, 0.6, 0.0, "tile"),
    "promp_wide_20_basis": (O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=20), O.TrajCfg("promp", action_dim=3),
                            0.02, 1.0, 0.0, "generic"),
    "prodmp_wide_20_dof": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=4, alpha=10),
                           O.TrajCfg("prodmp", action_dim=20), 0.02, 0.5, 0.0, "generic"),
    # horizons that are no multiple of 4: the masked tail chunk
    "cfg2_prodmp_97_steps": CFG2[:4] + (1.94, 0.0, "tile"),
    "cfg1_promp_199_steps": CFG1[:4] + (3.98, 0.0, "tile"),
    "promp_plain_rbf_50_steps": (O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=6), O.TrajCfg("promp", action_dim=5),
                                 0.02, 1.0, 0.0, "tile"),
    # the tile limit of 16 contraction columns (accumulator rows 12 .. 15 reach real columns) and the first generic shape behind it;
    # prodmp: num_basis weights + goal + the two boundary columns, promp (rbf): num_basis (COLUMNS below, checked against the oracle)
    "prodmp_16_columns_7_dof": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=13, alpha=15),
                                O.TrajCfg("prodmp", action_dim=7), 0.02, 0.6, 0.0, "tile"),
    "prodmp_17_columns_7_dof": (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=14, alpha=15),
                                O.TrajCfg("prodmp", action_dim=7), 0.02, 0.6, 0.0, "generic"),
    "promp_16_columns_3_dof": (O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=16), O.TrajCfg("promp", action_dim=3),
                               0.02, 0.8, 0.0, "tile"),
    # DoF counts: 1 (16 episodes per group, no shift), 8 (a full power of two), 11 (one episode per group, five idle tile columns)
    "prodmp_1_dof": (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                     O.TrajCfg("prodmp", action_dim=1), 0.02, 1.0, 0.0, "tile"),
    "prodmp_8_dof": (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                     O.TrajCfg("prodmp", action_dim=8), 0.02, 0.6, 0.0, "tile"),
    "prodmp_11_dof": (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                      O.TrajCfg("prodmp", action_dim=11), 0.02, 0.6, 0.0, "tile"),
}
# horizons of 1, 2, 3 and 5 steps: T * D below the alignment head, a single chunk, the odd tail chunk without a paired iteration
for _D in (3, 7):
    for _T in (1, 2, 3, 5):
        CONFIGS[f"prodmp_{_T}_steps_{_D}_dof"] = (O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0), O.BasisCfg("prodmp", num_basis=5, alpha=10),
                                                  O.TrajCfg("prodmp", action_dim=_D), 0.02, _T * 0.02, 0.0, "tile")
    for _T in (2, 3, 5):
        CONFIGS[f"promp_{_T}_steps_{_D}_dof"] = (O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=6),
                                                 O.TrajCfg("promp", action_dim=_D), 0.02, _T * 0.02, 0.0, "tile")
# contraction columns of the configurations that are named after them
COLUMNS = {"prodmp_12_columns_16_dof": 12, "prodmp_16_columns_7_dof": 16, "prodmp_17_columns_7_dof": 17, "promp_16_columns_3_dof": 16}
# cfg2's handle (7 DoF, two episodes per group) around the horizon at which its gradient images no longer fit a CU's LDS
LDS_BOUNDARY = {f"cfg2_prodmp_{_T}_steps": CFG2[:4] + (_T * 0.02, 0.0, _route) for _T, _route in ((277, "tile"), (280, "tile"), (281, "generic"))}
# ... and cfg2 at 25 steps (an odd T * D: every episode's rows start at another alignment) for the batch that wraps around the grid
OTHER = dict(LDS_BOUNDARY, cfg2_prodmp_25_steps=CFG2[:4] + (0.5, 0.0, "tile"))


def config(name):
    return CONFIGS[name] if name in CONFIGS else OTHER[name]


@functools.lru_cache(maxsize=None)
def jacobian(name):
    """float64 J [2, T, D, n] over the n = P + 2 D inputs of ONE episode (the map is the same for every episode) and (P, D, T)"""
    pc, bc, tc, dt, duration, init_time, _ = config(name)
    P, D = O.num_params(pc, bc, tc), tc.action_dim
    n = P + 2 * D
    x = np.zeros((n + 1, n))
    x[1:] = np.eye(n)
    pos, vel = O.get_trajectory(pc, bc, tc, x[:, :P], duration, dt, init_time, x[:, P:P + D], x[:, P + D:], dtype=np.float64)
    J = np.stack([pos[1:] - pos[0], vel[1:] - vel[0]])                   # [2, n, T, D]
    J = np.ascontiguousarray(np.moveaxis(J, 1, -1))                      # [2, T, D, n]
    J.setflags(write=False)
    return J, P, D, pos.shape[1]


def grads(name, B, seed):
    _, P, D, T = jacobian(name)
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, T, D)).astype(np.float32), rng.standard_normal((B, T, D)).astype(np.float32)


def reference(name, gp, gv):
    """(J^T g in float64 [B, n], the error of the float32 CPU einsum of the float32-rounded J against it [B, n])"""
    J, _, _, _ = jacobian(name)
    ref = np.zeros((gp.shape[0], J.shape[-1]))
    e32 = torch.zeros(ref.shape, dtype=torch.float32)
    for j, g in enumerate((gp, gv)):
        if g is not None:
            ref += np.einsum("tdn,btd->bn", J[j], g.astype(np.float64))
            e32 += torch.einsum("tdn,btd->bn", torch.from_numpy(J[j].astype(np.float32)), torch.from_numpy(g))
    return ref, np.abs(e32.numpy().astype(np.float64) - ref)


def split(name, x):
    _, P, D, _ = jacobian(name)
    return x[:, :P], x[:, P:P + D], x[:, P + D:]


def check(name, got, ref, e32, what):
    """per output array: |got - ref| <= max(1e-5 max|ref| + 1e-5 |ref|, 4 x max einsum error); prints the measured maxima first"""
    for label, g, r, e in zip(("g_params", "g_init_pos", "g_init_vel"), got, split(name, ref), split(name, e32)):
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == r.shape, (what, label, g.shape, r.shape)
        scale = np.abs(r).max() if r.size else 0.0
        err = np.abs(g - r)
        tol = np.maximum(RTOL * scale + RTOL * np.abs(r), 4.0 * (e.max() if e.size else 0.0))
        print(f"[vjp] {what} {label}: max|ref| {scale:.3e}  max err {err.max():.3e}  max f32-einsum err {e.max():.3e}  "
              f"project rule {RTOL * scale:.3e}")
        assert np.isfinite(g).all() and not (err > tol).any(), f"{what} {label}: max err {err.max():.3e}, {(err > tol).sum()} outside"


def engine_for(name):
    pc, bc, tc, dt, duration, _, _ = config(name)
    return make_engine(pc, bc, tc, dt, duration)


def dev(x):
    return torch.as_tensor(x, device="cuda")


# ---- 1. parity against J^T g ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_vjp_matches_the_float64_jacobian(name, B):
    init_time, route = CONFIGS[name][5], CONFIGS[name][6]
    eng = engine_for(name)
    gp, gv = grads(name, B, seed=B)
    got = eng.trajectory_vjp(dev(gp), dev(gv), init_time)
    torch.cuda.synchronize()
    mp = "dmp_resp" if "dmp_response" in name else config(name)[2].trajectory_generator_type
    assert eng.last_kernel() == f"k_traj_vjp_{route}<{mp}>", eng.last_kernel()
    ref, e32 = reference(name, gp, gv)
    check(name, got, ref, e32, f"{name} B={B}")
    steps = re.search(r"_(\d+)_steps", name)
    assert steps is None or eng.num_steps == int(steps.group(1))
    if name in COLUMNS:
        # the columns a DoF contracts: the inputs its trajectory depends on (prodmp: its parameters, init_pos, init_vel)
        J, P, D, _ = jacobian(name)
        used = np.abs(J).sum(axis=(0, 1)).astype(bool)                      # [D, n]
        assert used[0].sum() == COLUMNS[name] and (used.sum(axis=1) == COLUMNS[name]).all()


def test_promp_with_one_step_is_refused():
    eng = make_engine(O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=6), O.TrajCfg("promp", action_dim=3), 0.02, 0.02)
    assert eng.num_steps == 1
    g = torch.ones((2, 1, 3), device="cuda")
    with pytest.raises(ValueError, match="promp needs at least two time steps"):
        eng.trajectory_vjp(g, g)


def tile_lds_bytes(T, D):
    """launch_traj_vjp's arithmetic: the transposed tables [2][TP][16] and, per wave, the (pos, vel) images of a group's episodes"""
    sh = int(np.ceil(np.log2(D))) if D > 1 else 0
    ntw, tp = 16 >> sh, (T + 3) // 4 * 4
    stride = (tp * D + 3 + 31) // 32 * 32 + (0 if ntw == 1 else max(32 // ntw, 4))
    return (2 * tp * 16 + 4 * 2 * ntw * stride) * 4, tp, stride


@pytest.mark.parametrize("B", [1, 3])
def test_lds_fallback_boundary(B):
    """a 7-DoF handle: T = 280 takes a CU's whole LDS (163 840 bytes) and is still the tile route, T = 281 is the generic route"""
    assert tile_lds_bytes(280, 7) == (163840, 280, 2000) and tile_lds_bytes(277, 7)[0] == 163840
    assert tile_lds_bytes(276, 7)[0] < 163840 < tile_lds_bytes(281, 7)[0]
    kernels = []
    for name in LDS_BOUNDARY:
        eng = engine_for(name)
        assert eng.num_steps == int(name.split("_")[2])
        gp, gv = grads(name, B, seed=B)
        got = eng.trajectory_vjp(dev(gp), dev(gv), 0.0)
        torch.cuda.synchronize()
        kernels.append(eng.last_kernel())
        ref, e32 = reference(name, gp, gv)
        check(name, got, ref, e32, f"{name} B={B}")
    assert kernels == ["k_traj_vjp_tile<prodmp>", "k_traj_vjp_tile<prodmp>", "k_traj_vjp_generic<prodmp>"], kernels


# ---- 1b. batches beyond the grid caps: the grid-stride loops wrap ------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_cu,extra,kernel", [
    ("prodmp_12_columns_16_dof", 32, 809, "k_traj_vjp_tile<prodmp>"),       # one episode per group: four waves x at most 8 per CU
    ("cfg2_prodmp_25_steps", 64, 117, "k_traj_vjp_tile<prodmp>"),           # two per group; odd: the last group after the wrap part full
    ("promp_wide_20_basis", 8, 77, "k_traj_vjp_generic<promp>"),            # one episode per workgroup, at most 8 per CU
])
def test_batch_wraps_around_the_grid(name, per_cu, extra, kernel):
    """more episodes than the grid covers in one pass (the launchers cap it at 8 workgroups per CU whatever the LDS allows): every row
    against J^T g, and the bits of the same gradients launched in slices of 64 episodes -- an episode's reduction never leaves its
    tile column (its thread), so the grouping cannot change them -- and of a second identical launch"""
    B = per_cu * torch.cuda.get_device_properties(0).multi_processor_count + extra
    eng = engine_for(name)
    gp_h, gv_h = grads(name, B, seed=11)
    gp, gv = dev(gp_h), dev(gv_h)
    big = eng.trajectory_vjp(gp, gv, 0.0)
    torch.cuda.synchronize()
    assert eng.last_kernel() == kernel
    ref, e32 = reference(name, gp_h, gv_h)
    check(name, big, ref, e32, f"{name} B={B}")
    again = eng.trajectory_vjp(gp, gv, 0.0)
    for x, y in zip(big, again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    parts = []
    for i, lo in enumerate(range(0, B, 64)):
        own = []
        for g in (gp, gv):                      # storage of its own, 4, 8 or 12 bytes past a 16-byte boundary
            part = g[lo:lo + 64]
            buf = torch.empty(part.numel() + 4, device="cuda")
            view = buf[1 + i % 3:1 + i % 3 + part.numel()].view(part.shape)
            view.copy_(part)
            assert view.data_ptr() % 16 == 4 * (1 + i % 3) and view.is_contiguous()
            own.append(view)
        parts.append(eng.trajectory_vjp(own[0], own[1], 0.0))
        assert eng.last_kernel() == kernel
    for j, x in enumerate(big):
        assert torch.equal(x.view(torch.int32), torch.cat([p[j] for p in parts]).view(torch.int32)), j


# ---- 2. adjoint identity against the forward kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg1_promp_zero_padded", "cfg2_prodmp", "cfg3_dmp_response", "prodmp_relative_goal",
                                  "prodmp_wide_20_dof"])
def test_adjoint_identity_with_the_forward_kernels(name):
    """<g_pos, pos(x + delta) - pos(x)> + <g_vel, vel(x + delta) - vel(x)> = <vjp(g), delta> for a step in params, in init_pos and in
    init_vel, the forward being the trajectory kernels as they are.  Bound: the parity bound of item 1 scaled to the inner product,
    sum(bound_el |delta|) -- every term of <vjp(g), delta> may be off by its element's bound -- plus what the float32 FORWARD
    difference itself is off by, measured, not bounded: the same inner product with the float64 J, <g, J delta>, is at hand, and 4 x
    its gap to the forward's value is allowed on top (the forward is the reference of this test, not the code under test)."""
    init_time = CONFIGS[name][5]
    eng = engine_for(name)
    J, P, D, T = jacobian(name)
    B = 5
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, P + 2 * D)).astype(np.float32)
    gp, gv = grads(name, B, seed=3)
    got = [g.cpu().numpy().astype(np.float64) for g in eng.trajectory_vjp(dev(gp), dev(gv), init_time)]
    ref, e32 = reference(name, gp, gv)
    bound_el = [np.maximum(RTOL * np.abs(r).max() + RTOL * np.abs(r), 4.0 * e.max()) for r, e in zip(split(name, ref), split(name, e32))]

    def forward(v):
        p, ip, iv = split(name, v)
        pos, vel = eng.trajectory(dev(np.ascontiguousarray(p)), dev(np.ascontiguousarray(ip)), dev(np.ascontiguousarray(iv)), init_time)
        return pos.cpu().numpy().astype(np.float64), vel.cpu().numpy().astype(np.float64)

    pos0, vel0 = forward(x)
    for i, label in enumerate(("params", "init_pos", "init_vel")):
        delta = np.zeros_like(x)
        lo, hi = (0, P, P + D)[i], (P, P + D, P + 2 * D)[i]
        delta[:, lo:hi] = rng.standard_normal((B, hi - lo)).astype(np.float32)
        pos1, vel1 = forward(x + delta)
        lhs = (gp * (pos1 - pos0)).sum() + (gv * (vel1 - vel0)).sum()
        rhs = (got[i] * delta[:, lo:hi]).sum()
        lhs64 = sum(np.einsum("btd,tdn,bn->", g.astype(np.float64), J[j], delta.astype(np.float64)) for j, g in enumerate((gp, gv)))
        fwd = 4.0 * abs(lhs - lhs64)
        tol = (bound_el[i] * np.abs(delta[:, lo:hi])).sum() + fwd
        print(f"[vjp] adjoint {name} {label}: lhs {lhs:.6e} rhs {rhs:.6e} |diff| {abs(lhs - rhs):.3e} tol {tol:.3e} (forward gap {abs(lhs - lhs64):.3e})")
        assert abs(lhs - rhs) <= tol, (label, lhs, rhs, tol)
        # (an input the configuration never reads has a zero gradient and an unchanged trajectory)
        if not np.abs(split(name, np.abs(J).sum(axis=(0, 1, 2))[None])[i]).any():
            assert lhs == 0.0 and rhs == 0.0


# ---- 3. null pointers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_199_steps", "prodmp_wide_20_dof"])
def test_null_gradients_and_null_outputs(name):
    init_time = CONFIGS[name][5]
    eng = engine_for(name)
    _, P, D, T = jacobian(name)
    B = 9
    gp, gv = (dev(g) for g in grads(name, B, seed=1))
    zero = torch.zeros_like(gp)
    for a, b in (((gp, None), (gp, zero)), ((None, gv), (zero, gv))):
        got, want = eng.trajectory_vjp(*a, init_time), eng.trajectory_vjp(*b, init_time)
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    full = eng.trajectory_vjp(gp, gv, init_time)
    # only g_params, written into the middle of a sentinel-filled buffer: nothing lands outside its own [B, P] block (the two
    # outputs that are not asked for go to the library as NULL, so this shows no stray store, not the guard inside the kernel)
    guard = 8
    buf = torch.full((guard + B * P + guard + 2 * B * D + guard,), 12345.0, device="cuda")
    out_p = buf[guard:guard + B * P].view(B, P)
    res = eng.trajectory_vjp(gp, gv, init_time, need=(True, False, False), out=(out_p, None, None))
    torch.cuda.synchronize()
    assert res[0] is out_p and res[1] is None and res[2] is None
    assert torch.equal(out_p, full[0])
    assert (buf[:guard] == 12345.0).all() and (buf[guard + B * P:] == 12345.0).all()
    # only the boundary state
    res = eng.trajectory_vjp(gp, gv, init_time, need=(False, True, True))
    assert res[0] is None and torch.equal(res[1], full[1]) and torch.equal(res[2], full[2])


# ---- 4. autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg1_promp_zero_padded", "cfg3_dmp_response", "promp_wide_20_basis"])
def test_autograd_backward_is_the_vjp_launch(name):
    init_time = CONFIGS[name][5]
    eng = engine_for(name)
    _, P, D, T = jacobian(name)
    B = 6
    rng = np.random.default_rng(5)
    params, ip, iv = (dev(rng.standard_normal(s).astype(np.float32)) for s in ((B, P), (B, D), (B, D)))
    gp, gv = (dev(g) for g in grads(name, B, seed=2))
    plain_pos, plain_vel = eng.trajectory(params, ip, iv, init_time)
    forward_kernel = eng.last_kernel()
    assert plain_pos.grad_fn is None and not plain_pos.requires_grad
    for t in (params, ip, iv):
        t.requires_grad_()
    pos, vel = eng.trajectory(params, ip, iv, init_time)
    assert eng.last_kernel() == forward_kernel and pos.grad_fn is not None
    assert torch.equal(pos.detach(), plain_pos) and torch.equal(vel.detach(), plain_vel)
    (pos * gp + vel * gv).sum().backward()
    assert eng.last_kernel().startswith("k_traj_vjp_")
    want = eng.trajectory_vjp(gp, gv, init_time)
    for t, w in zip((params, ip, iv), want):
        assert t.grad is not None and torch.equal(t.grad.view(torch.int32), w.view(torch.int32))
    # one output alone: the other arrives as None and its term is skipped
    for t in (params, ip, iv):
        t.grad = None
    pos, vel = eng.trajectory(params, ip, iv, init_time)
    pos.sum().backward()
    want = eng.trajectory_vjp(torch.ones_like(gp), None, init_time)
    for t, w in zip((params, ip, iv), want):
        assert torch.equal(t.grad, w)
    # only params requires grad: needs_input_grad leaves the boundary outputs uncomputed
    p2 = params.detach().clone().requires_grad_()
    pos, vel = eng.trajectory(p2, ip.detach(), iv.detach(), init_time)
    (pos * gp + vel * gv).sum().backward()
    assert torch.equal(p2.grad, eng.trajectory_vjp(gp, gv, init_time)[0])


def test_without_requires_grad_nothing_changes():
    """same launch, same tensors, out= honoured; under no_grad a leaf that requires grad takes the plain path too"""
    eng = engine_for("cfg2_prodmp")
    _, P, D, T = jacobian("cfg2_prodmp")
    B = 33
    rng = np.random.default_rng(9)
    params, ip, iv = (dev(rng.standard_normal(s).astype(np.float32)) for s in ((B, P), (B, D), (B, D)))
    pos, vel = eng.trajectory(params, ip, iv)
    kernel = eng.last_kernel()
    assert kernel.startswith("k_traj_") and "vjp" not in kernel
    out = (torch.empty_like(pos), torch.empty_like(vel))
    got = eng.trajectory(params, ip, iv, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], pos) and torch.equal(out[1], vel)
    assert pos.grad_fn is None and out[0].grad_fn is None
    rp, rv = O.get_trajectory(*CONFIGS["cfg2_prodmp"][:3], params.cpu().numpy(), 2.0, 0.02, 0.0, ip.cpu().numpy(), iv.cpu().numpy(),
                              dtype=np.float64)
    assert np.abs(pos.cpu().numpy() - rp).max() <= 2e-5 * np.abs(rp).max()
    leaf = params.clone().requires_grad_()
    with torch.no_grad():
        p2, _ = eng.trajectory(leaf, ip, iv)
    assert p2.grad_fn is None and torch.equal(p2, pos) and eng.last_kernel() == kernel


def test_refusals():
    pc = O.PhaseCfg("exp", tau=1.5, alpha_phase=3.0, learn_tau=True, tau_bound=(0.5, 3.0))
    bc, tc = O.BasisCfg("prodmp", num_basis=5, alpha=10), O.TrajCfg("prodmp", action_dim=3)
    eng = make_engine(pc, bc, tc, 0.02, 1.0)
    B, P = 4, O.num_params(pc, bc, tc)
    params = torch.ones((B, P), device="cuda")
    z = torch.zeros((B, 3), device="cuda")
    pos, _ = eng.trajectory(params, z, z)                     # not differentiated: works as before
    assert pos.grad_fn is None
    with pytest.raises(NotImplementedError, match="shared phase"):
        eng.trajectory(params.clone().requires_grad_(), z, z)
    with pytest.raises(NotImplementedError, match="tau"):
        eng.trajectory_vjp(torch.zeros_like(pos), None)
    # a per-episode init_time array
    eng2 = engine_for("cfg2_prodmp")
    p2 = torch.zeros((B, eng2.num_params), device="cuda", requires_grad=True)
    z7 = torch.zeros((B, 7), device="cuda")
    with pytest.raises(NotImplementedError, match="init_time"):
        eng2.trajectory(p2, z7, z7, torch.zeros(B, device="cuda"))
    # a DMP off its response route
    pc3, bc3, tc3, dt3, dur3 = CFG3
    eng3 = make_engine(pc3, bc3, tc3, dt3, dur3)
    eng3.set_option("dmp_response", 0)
    with pytest.raises(NotImplementedError, match="response"):
        eng3.trajectory_vjp(torch.zeros((B, eng3.num_steps, 7), device="cuda"), None)


def test_batched_black_box_keeps_the_graph():
    from fancy_gym_amd import make_batched
    B = 8
    bb = make_batched("fancy_ProDMP/SimpleReacher-v0", B)
    bb.reset(seed=3)
    P = bb.engine.num_params
    rng = np.random.default_rng(4)
    raw = rng.standard_normal((B, P)).astype(np.float32)
    plain = bb.get_trajectory(dev(raw))
    assert plain["des_pos"].grad_fn is None
    params = dev(raw).requires_grad_()
    traj = bb.get_trajectory(params)
    assert torch.equal(traj["des_pos"].detach(), plain["des_pos"]) and torch.equal(traj["des_vel"].detach(), plain["des_vel"])
    g = dev(rng.standard_normal(tuple(traj["des_pos"].shape)).astype(np.float32))
    (traj["des_pos"] * g).sum().backward()
    want = bb.engine.trajectory_vjp(g, None, 0.0)[0]
    assert params.grad is not None and torch.equal(params.grad, want) and params.grad.abs().max() > 0


# ---- 5. determinism and layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_prodmp", "cfg2_prodmp_97_steps", "cfg1_promp_199_steps", "prodmp_12_columns_16_dof"])
def test_deterministic_alignment_free_and_routes_agree(name, mpk_option):
    init_time = CONFIGS[name][5]
    eng = engine_for(name)
    _, P, D, T = jacobian(name)
    B = 65
    gp_h, gv_h = grads(name, B, seed=8)
    gp, gv = dev(gp_h), dev(gv_h)
    a = eng.trajectory_vjp(gp, gv, init_time)
    b = eng.trajectory_vjp(gp, gv, init_time)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    # the same values 4, 8 and 12 bytes past a 16-byte boundary
    for off in (1, 2, 3):
        shifted = []
        for g in (gp, gv):
            buf = torch.empty(g.numel() + 4, device="cuda")
            view = buf[off:off + g.numel()].view(g.shape)
            view.copy_(g)
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            shifted.append(view)
        c = eng.trajectory_vjp(shifted[0], shifted[1], init_time)
        for x, y in zip(a, c):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), off
    assert eng.last_kernel().startswith("k_traj_vjp_tile<")
    mpk_option("vjp_generic", 1)
    gen = eng.trajectory_vjp(gp, gv, init_time)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("k_traj_vjp_generic<")
    ref, e32 = reference(name, gp_h, gv_h)
    check(name, gen, ref, e32, f"{name} generic route")
    # tile against generic: both lie within the bound of the same float64 value; against each other, the bound once more
    for label, x, y, r, e in zip(("g_params", "g_init_pos", "g_init_vel"), a, gen, split(name, ref), split(name, e32)):
        tol = np.maximum(RTOL * np.abs(r).max() + RTOL * np.abs(r), 4.0 * e.max())
        err = np.abs(x.cpu().numpy().astype(np.float64) - y.cpu().numpy().astype(np.float64))
        print(f"[vjp] {name} tile vs generic {label}: max diff {err.max():.3e}")
        assert not (err > tol).any(), label


# ---- 6. fit ------------------------------------------------------------------------------------------------------------------------------
def test_adam_fit_of_the_example_converges():
    """200 Adam steps (lr 0.1) of examples/batched_trajectory_fit.py at B = 64 bring the trajectory MSE below 1e-3 of its start.  The
    same loop in float64 on the CPU with the oracle's J reaches 3.7e-5 of the start (lr 0.03: 1.8e-4, lr 0.3: 4.3e-6)."""
    spec = importlib.util.spec_from_file_location("batched_trajectory_fit", os.path.join(ROOT, "examples", "batched_trajectory_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, err = mod.fit(envs=64, iters=200, lr=0.1, seed=0, verbose=False)
    print(f"[vjp] fit: MSE {losses[0]:.4e} -> {losses[-1]:.4e} ({losses[-1] / losses[0]:.2e}), mean |parameter error| {err:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < 1e-3 * losses[0]
