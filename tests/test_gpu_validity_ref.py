"""
The validity gate against the REFERENCE's own two functions (TableTennisEnv.check_traj_validity / _get_traj_invalid_penalty,
table_tennis_env.py:282-309) on every route that implements it (include/mpk.h, mpk_validity_gate):
  * k_validity                 mpk_traj_validity(_penalty); the separate-launch fallback of the gated entry points
  * gate_pass                  k_traj_quad / duo / mono <.., closed, gate>
  * k_traj_pipe<.., gate>
  * gate_scan_tile/_verdict    k_episode_return (gated)
  * k_phase_fused (gated)      plain, lean and PIPE forms
The contract is the reference's, line for line: `valid = not (time_invalid or any(pos > high) or any(pos < low))` in float64 on the fp32
positions and the RAW tau / delay, so a NaN position, tau, delay or limit never makes a plan invalid while +-inf positions do; the penalty
of an invalid plan is numpy's (NaN where a NaN enters it), the penalty of a valid plan is 0.
tests/golden/ref_validity.npz (tests/golden/make_ref_validity_golden.py) carries the reference's verdicts on hand-made positions;
the routes are then run on computed plans with NaN weights, non-finite raw tau / delay and limits set exactly on / one float64 below a
plan's extreme position, against the oracle (oracle.traj_validity / traj_invalid_penalty, pinned to the same fixture on the CPU).
"""
import functools
import os

import numpy as np
import pytest
import torch

from fancy_gym_amd import RolloutSpec
from oracle import mp_oracle as O
from tests.test_gpu_learned_phase import CONFIGS_ALL, JNT_HIGH, JNT_LOW, _bb, _separate_step, _state, cu, eq
from tests.test_gpu_trajectory import make_engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_validity.npz")
CASES = tuple(str(c) for c in np.load(GOLD)["cases"])

# (the gated entry points take <= 16 DoF -- "validity gate: num_dof too large" beyond; 17 DoF meets k_validity in the fixture test above)
ROUTE_CONFIGS = dict(CONFIGS_ALL)
SHARED = ("cfg5_promp_tabletennis", "cfg4_prodmp_replan", "dmp_5dof_response")
# (name, option overrides, lean): the kernels each row has to reach are asserted in test_every_route_was_reached
ROUTES = [
    ("tt_prodmp", (), False), ("tt_prodmp", (), True), ("tt_prodmp", (("phase_pipe", 1),), False), ("tt_prodmp", (("phase_pipe", 0),), False),
    ("tt_prodmp", (("phase_pipe", 0),), True),
    ("tt_prodmp_replan", (), False), ("tt_prodmp_replan", (), True), ("tt_prodmp_replan", (("phase_pipe", 1),), True),
    ("promp_5dof_learn_both", (), False), ("promp_5dof_learn_both", (), True), ("promp_5dof_learn_both", (("phase_pipe", 1),), False),
    ("cfg5_promp_tabletennis", (("quad", 4),), False), ("cfg5_promp_tabletennis", (("quad", 2),), False),
    ("cfg5_promp_tabletennis", (("quad", 1),), False), ("cfg5_promp_tabletennis", (("pipe", 1),), False),
    ("cfg5_promp_tabletennis", (("quad", 0),), False), ("cfg5_promp_tabletennis", (), True),
    ("cfg4_prodmp_replan", (), False), ("cfg4_prodmp_replan", (("pipe", 1),), False), ("cfg4_prodmp_replan", (("quad", 2),), False),
    ("cfg4_prodmp_replan", (), True),
    ("dmp_5dof_response", (), False), ("dmp_5dof_response", (), True),   # (non-lean: no gated DMP kernel -> the separate launches)
]


@functools.lru_cache(maxsize=None)
def _engine(name):
    pc, bc, tc, dt, dur = ROUTE_CONFIGS[name][:5]
    return make_engine(pc, bc, tc, dt, dur, device=0)


@functools.lru_cache(maxsize=None)
def _fixture_engine(D):
    return make_engine(O.PhaseCfg("linear", tau=1.0), O.BasisCfg("rbf", num_basis=2, basis_bandwidth_factor=3),
                       O.TrajCfg("promp", action_dim=D), 0.02, 1.0, device=0)


def _nan_eq(a, b, what):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), \
        f"{what}: {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())} of {a.size} entries differ"


def _penalty_matches(got, want, valid, what, rel=1e-12):
    """got (a route) against want (the reference's form) on the plans both call invalid; 0 on valid ones"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert np.all(got[valid] == 0.0), f"{what}: a valid plan's penalty is not 0: {got[valid][got[valid] != 0.0][:5]}"
    g, w = got[~valid], want[~valid]
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN at {np.flatnonzero(np.isnan(g) != np.isnan(w))[:8]}"
    inf = np.isinf(w)
    assert np.array_equal(g[inf], w[inf]) and not np.isinf(g[~inf]).any(), f"{what}: infinite penalties differ"
    fin = np.isfinite(w)
    err = np.abs(g[fin] - w[fin])
    assert np.all(err <= rel * np.abs(w[fin])), f"{what}: max |diff| {err.max() if err.size else 0:.3e}"


# ---- 1. mpk_traj_validity / mpk_traj_validity_penalty on the reference's own verdicts --------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_k_validity_equals_the_reference_on_its_fixture(case):
    """k_validity (mpk_traj_validity and mpk_traj_validity_penalty) on positions exactly on / one float32 beside the limits, NaN and
    +-inf positions, raw tau / delay, NaN limits, lo > hi, limits beyond the float32 range: `valid` bit for bit, the penalty of an
    invalid plan NaN / inf where the reference's is and 1e-12 relative elsewhere, 0 for a valid plan"""
    z = np.load(GOLD)
    g = lambda n: z[f"{case}_{n}"]
    pos, act, lo, hi, tb, db, want_v, want_p = g("pos"), g("action"), g("lo"), g("hi"), g("tb"), g("db"), g("valid"), g("penalty")
    B, T, D = pos.shape
    eng = _fixture_engine(D)
    P = eng.num_params
    params = np.zeros((B, P), np.float32)
    params[:, :2] = act
    v_only = eng.traj_validity(cu(pos), lo, hi, cu(params), tuple(tb), tuple(db))
    v, pen = eng.traj_validity(cu(pos), lo, hi, cu(params), tuple(tb), tuple(db), with_penalty=True)
    torch.cuda.synchronize()
    eq(v_only, want_v, f"{case}: valid (mpk_traj_validity)")
    eq(v, want_v, f"{case}: valid (mpk_traj_validity_penalty)")
    _penalty_matches(pen.cpu().numpy(), want_p, want_v, f"{case}: penalty")


# ---- 2. every gated route on computed plans ---------------------------------------------------------------------------------------------
def _route_inputs(name, B):
    pc, bc, tc = ROUTE_CONFIGS[name][:3]
    rng = np.random.default_rng(5)
    P = O.num_params(pc, bc, tc)
    raw = (0.35 * rng.standard_normal((B, P))).astype(np.float32)
    n_ph = int(pc.learn_tau) + int(pc.learn_delay)
    if pc.learn_tau:
        raw[:, 0] = rng.uniform(pc.tau_bound[0] - 0.05, pc.tau_bound[1] + 0.05, B)
    if pc.learn_delay:
        raw[:, 1] = rng.uniform(pc.delay_bound[0] - 0.02, pc.delay_bound[1] + 0.02, B)
    quirk = name == "cfg5_promp_tabletennis"
    if quirk:
        raw[:, 0] = rng.uniform(0.75, 1.55, B); raw[:, 1] = rng.uniform(0.04, 0.16, B)
    ip = (0.3 * rng.uniform(-1, 1, (B, tc.action_dim))).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, tc.action_dim)).astype(np.float32)
    lo_hi = O.params_bounds(pc, bc, tc)
    params = raw.copy()
    params[:, :n_ph] = np.clip(raw[:, :n_ph], lo_hi[0, :n_ph], lo_hi[1, :n_ph])
    # a NaN weight in a few plans (the executed params and the raw action alike)
    for b, c in ((3, n_ph + 1), (7, P - 1), (11, n_ph)):
        params[b, c] = np.nan; raw[b, c] = np.nan
    chk = n_ph == 2 or quirk
    if chk:
        # non-finite RAW tau / delay; the params the plan executes stay what they were (clipped)
        for b, c, v in ((20, 0, np.nan), (21, 1, np.nan), (22, 0, np.inf), (23, 1, -np.inf), (24, 0, -np.inf), (25, 1, np.inf),
                        (26, 0, np.nan), (27, 0, np.nan)):
            raw[b, c] = v
        raw[26, 1] = 5.0                                  # NaN tau beside an out-of-bounds delay: invalid, NaN penalty
        raw[28, 0] = np.float32(1.5)                      # tau exactly on its upper bound (1.5 is fp32-exact)
    return raw, params, ip, iv, chk


def _limits(name, D):
    if D <= 7:
        return JNT_LOW[:D] * 0.45, JNT_HIGH[:D] * 0.45
    return np.full(D, -1.0), np.full(D, 1.0)


def _run_route(eng, name, closed, params, raw, ip, iv, gate, lean, every_, mpt, horizon):
    B = params.shape[0]
    q0, qd0 = ip.astype(np.float64), iv.astype(np.float64)
    A, S = _state(B, q0, qd0), _state(B, q0, qd0)
    g = dict(gate, raw_params=raw)
    if lean:
        r = eng.episode_return(params, cu(ip), cu(iv), closed, A["q"], A["qd"], replan=(A["ts"], A["ps"], A["dn"], every_, mpt, horizon),
                               init_time=0.0, condition=True, gate=g)
    else:
        r = eng.replan_step(params, cu(ip), cu(iv), closed, A["q"], A["qd"], A["ts"], A["ps"], A["dn"], every_, mpt, horizon,
                            init_time=0.0, condition=True, gate=g)
    kernel = eng.last_kernel()
    s = _separate_step(eng, params, cu(ip), cu(iv), closed, S["q"], S["qd"], S["ts"], S["ps"], S["dn"], every_, mpt, horizon, 0.0,
                       gate=gate, raw=raw)
    torch.cuda.synchronize()
    return r, s, A, S, kernel


def _route_label(kernel, lean, traj_kernel):
    """the gate implementation a launch used; traj_kernel: what mpk_trajectory launches for the same plan under the same options"""
    base = kernel.split("<")[0]
    if base in ("k_traj_quad", "k_traj_duo", "k_traj_mono", "k_traj_pipe") and kernel.endswith(",closed,gate>") and not lean:
        return base + "<gate>"
    if base == "k_episode_return" and lean:
        return "k_episode_return<gate>"
    if base == "k_phase_fused" and ",closed" in kernel:
        return "k_phase_fused" + ("<pipe>" if ",pipe," in kernel else "") + ("<lean>" if lean else "")
    # the separate-launch fallback of the gated entry points: the plan by the trajectory kernel, then k_validity
    assert not lean and kernel == traj_kernel, f"unknown gate route: {kernel} (lean={lean}, trajectory kernel {traj_kernel})"
    return "k_validity"


@functools.lru_cache(maxsize=None)
def _routes_of(name):
    """runs every ROUTES row of `name` (asserting as it goes) and returns the gate implementations reached"""
    from fancy_gym_amd import _lib
    pc, bc, tc, dt, dur, (pg, dg), every, mpt = ROUTE_CONFIGS[name]
    eng = _engine(name)
    T, D = eng.num_steps, eng.num_dof
    B = 600
    horizon = T
    every_ = every or horizon + 1
    closed = RolloutSpec("motor", D, pg, dg, -1.0, 1.0, plant="double_integrator", dt=dt)
    raw, params, ip, iv, chk = _route_inputs(name, B)
    quirk = name == "cfg5_promp_tabletennis"
    tb, db = ((0.8, 1.5), (0.05, 0.15)) if quirk else (pc.tau_bound, pc.delay_bound)
    base_lo, base_hi = _limits(name, D)
    # the plan once, on its own: the boundary rows are cut from its positions
    pos0, _ = eng.trajectory(params, cu(ip), cu(iv), 0.0)
    torch.cuda.synchronize()
    p0 = pos0.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok0 = O.traj_validity(raw, p0, base_lo, base_hi, tb if chk else None, db if chk else None)
    ok0[:30] = False                                      # (not an injected row)
    assert ok0.sum() > 10, ok0.sum()
    e1 = e2 = np.flatnonzero(ok0)[0]                      # ONE plan on both limits: it alone decides that it stays inside
    d1, d2 = 0, min(1, D - 1)
    mx, mn = p0[e1, :, d1].max(), p0[e2, :, d2].min()
    on_lo, on_hi = base_lo.copy(), base_hi.copy(); on_hi[d1] = mx; on_lo[d2] = mn
    past_lo, past_hi = base_lo.copy(), base_hi.copy()
    past_hi[d1] = np.nextafter(mx, -np.inf); past_lo[d2] = np.nextafter(mn, np.inf)
    reached = set()
    for rname, opts, lean in ROUTES:
        if rname != name:
            continue
        _lib.reset_options()
        for k, v in opts:
            _lib.set_option(k, int(v))
        try:
            eng.trajectory(params, cu(ip), cu(iv), 0.0)
            traj_kernel = eng.last_kernel()
            for tag, lo, hi in (("base", base_lo, base_hi), ("on", on_lo, on_hi), ("past", past_lo, past_hi)):
                what = f"{name} {opts} lean={lean} {tag}"
                gate = dict(pos_low=lo, pos_high=hi, check_tau_delay=chk, tau_bound=tb, delay_bound=db)
                r, s, A, S, kernel = _run_route(eng, name, closed, params, raw, ip, iv, gate, lean, every_, mpt, horizon)
                reached.add(_route_label(kernel, lean, traj_kernel))
                posn = s["pos"].cpu().numpy()
                with np.errstate(invalid="ignore"):
                    want_v = O.traj_validity(raw, posn, lo, hi, tb if chk else None, db if chk else None)
                    want_p = O.traj_invalid_penalty(raw, posn, lo, hi, tb if chk else None, db if chk else None)
                if tag == "on":
                    assert want_v[e1] and want_v[e2], what            # a position exactly on the limit is inside
                if tag == "past":
                    assert not want_v[e1] and not want_v[e2], what    # one float64 beyond it is not
                sv = s["valid"].cpu().numpy().astype(bool)
                eq(sv, want_v, f"{what}: valid (k_validity) vs the reference's form")
                _penalty_matches(s["penalty"].cpu().numpy(), want_p, want_v, f"{what}: penalty (k_validity)")
                rv = r["valid"].cpu().numpy().astype(bool)
                eq(rv, want_v, f"{what}: valid ({kernel}) vs the reference's form")
                _penalty_matches(r["penalty"].cpu().numpy(), want_p, want_v, f"{what}: penalty ({kernel})")
                _penalty_matches(r["penalty"].cpu().numpy(), s["penalty"].cpu().numpy(), want_v, f"{what}: penalty, {kernel} vs k_validity")
                if chk:                               # (+inf tau; NaN tau beside an out-of-bounds delay: invalid, NaN penalty)
                    assert not rv[22] and not rv[26] and np.isnan(r["penalty"][26].item()), what
                    # tau exactly on its upper bound is inside: row 28's verdict is its positions' alone
                    with np.errstate(invalid="ignore"):
                        pos_only = O.traj_validity(raw, posn, lo, hi)
                    assert rv[28] == pos_only[28] and sv[28] == pos_only[28], what
                for key in ("q", "qd"):
                    _nan_eq(A[key], S[key], f"{what}: {key}")
                for key in ("ts", "ps", "dn"):
                    eq(A[key], S[key], f"{what}: {key}")
                eq(r["seg_len"], s["seg_len"], f"{what}: seg_len")
                _nan_eq(r["cond_pos"], s["cond_pos"], f"{what}: cond_pos"); _nan_eq(r["cond_vel"], s["cond_vel"], f"{what}: cond_vel")
                if not lean:
                    _nan_eq(r["pos"], s["pos"], f"{what}: pos"); _nan_eq(r["vel"], s["vel"], f"{what}: vel")
                    _nan_eq(r["actions"], s["actions"], f"{what}: actions")
                if tag == "base":                     # (both verdicts; the boundary rows' limits may leave few plans inside)
                    assert (~want_v).sum() > 5 and want_v.sum() > 5, what
        finally:
            _lib.reset_options()
    return frozenset(reached)


@pytest.mark.parametrize("name", sorted({r[0] for r in ROUTES}))
def test_every_gated_route_equals_the_reference_on_computed_plans(name):
    """NaN weights, NaN / +-inf raw tau / delay, limits exactly on / one float64 inside a plan's extreme position: valid and penalty of
    the gated step (every forced form) and of its separate launches against the reference's form, and the two paths against each
    other (plant, integer state, condition, positions / actions NaN-aware)"""
    assert _routes_of(name)


def test_every_route_was_reached():
    """the launches above went through every implementation of the gate: a route that silently stopped being chosen fails here"""
    reached = set()
    for name in sorted({r[0] for r in ROUTES}):
        reached |= _routes_of(name)
    want = {"k_validity", "k_traj_pipe<gate>", "k_episode_return<gate>", "k_phase_fused", "k_phase_fused<lean>", "k_phase_fused<pipe>"}
    print("gate routes reached:", ", ".join(sorted(reached)))
    assert want <= reached, (sorted(want - reached), sorted(reached))
    assert reached & {"k_traj_quad<gate>", "k_traj_duo<gate>", "k_traj_mono<gate>"}, sorted(reached)


@pytest.mark.parametrize("name", ["tt_prodmp", "cfg5_promp_tabletennis"])
def test_batched_black_box_separate_launches_gate_like_the_reference(name):
    """BatchedBlackBox.step(fuse=False) -- trajectory, k_validity, advance, rollout, gather -- and the fused step on the same first
    plan (NaN weights, NaN / +-inf raw tau / delay): `valid` and `invalid_penalty` against the reference's form on the plan's own
    positions, and the two steps against each other"""
    B = 600
    raw, _, ip, iv, chk = _route_inputs(name, B)
    D = ip.shape[1]
    lo, hi = _limits(name, D)
    apart, fused = (_bb(name, B, pos_limits=(lo, hi), check_tau_delay=chk) for _ in range(2))
    for bb in (apart, fused):
        bb.reset(ip.astype(np.float64), iv.astype(np.float64))
    c = apart.step(raw, fuse=False)
    a = fused.step(raw)
    torch.cuda.synchronize()
    tb, db = apart.tau_bound, apart.delay_bound
    with np.errstate(invalid="ignore"):
        posn = c["des_pos"].cpu().numpy()
        want_v = O.traj_validity(raw, posn, lo, hi, tb if chk else None, db if chk else None)
        want_p = O.traj_invalid_penalty(raw, posn, lo, hi, tb if chk else None, db if chk else None)
    eq(c["valid"], want_v, f"{name}: valid (fuse=False)")
    _penalty_matches(c["invalid_penalty"].cpu().numpy(), want_p, want_v, f"{name}: penalty (fuse=False)")
    eq(a["valid"], want_v, f"{name}: valid (fused, {fused.engine.last_kernel()})")
    _penalty_matches(a["invalid_penalty"].cpu().numpy(), want_p, want_v, f"{name}: penalty (fused)")
    _nan_eq(a["des_pos"], c["des_pos"], f"{name}: des_pos")
    for key in ("trajectory_length", "done", "terminated", "truncated"):
        eq(a[key], c[key], f"{name}: {key}")
    assert (~want_v).sum() > 5 and want_v.sum() > 5
    if chk and np.isfinite(np.r_[tb, db]).all():
        assert not want_v[22] and not want_v[26] and np.isnan(want_p[26])
