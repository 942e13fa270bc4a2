"""Reacher observations on the device (mpk_reacher_observation, mpk_reacher_step_observations): the rows against the reference fixture,
BatchedBlackBox(observations=True) against the host wrappers of both families, the step-observation replay against the rollout's end
state, nothing changed without the flag, captured episodes against eager ones, and the refused calls"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fancy_gym_amd import BatchedBlackBox, RolloutSpec, TrajectoryEngine, _gym, _lib

from .test_gpu_hole_reacher import LIM, batched, host_env

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_reacher_obs.npz")
ENVS = {0: "simple_reacher", 1: "hole_reacher"}
_engines = {}


def engine(n):
    if n not in _engines:
        _engines[n] = TrajectoryEngine("promp", "linear", "zero_rbf", n, 5, dt=0.01, duration=2.0, tau=2.0, num_basis_zero_start=1,
                                       device=0)
    return _engines[n]


def cuda(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")


def assert_rows(got, ref64, what, exact_cols=()):
    """got (float32) == float32(ref64) bit for bit, except where ref64 lies within 2 ulp(f64) of a float32 rounding midpoint: there one
    float32 ulp is allowed (counted and printed).  exact_cols: no exception"""
    got = np.asarray(got, np.float32)
    want = np.asarray(ref64, np.float64).astype(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    for c in exact_cols:
        assert not diff[..., c].any(), (what, "column", c)
    if diff.any():
        idx = np.argwhere(diff)
        for i in map(tuple, idx):
            g, w, r = got[i], want[i], float(np.asarray(ref64)[i])
            assert np.nextafter(w, g) == g, (what, i, g, w, r)
            mid = (float(w) + float(g)) / 2.0
            assert abs(r - mid) <= 2 * np.spacing(abs(r)), (what, i, g, w, r)
        print(f"{what}: {len(idx)} element(s) within 2 ulp(f64) of a float32 midpoint, one float32 ulp apart")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(GOLDEN))


def test_device_rows_equal_the_fixture(ref):
    keys = sorted({(int(k), int(n), bool(rs), bool(w)) for k, n, rs, w in
                   zip(ref["kind"], ref["n_links"], ref["random_start"], ref["width_given"])})
    assert len(keys) == 12
    for kind, n, rs, wg in keys:
        rows = np.flatnonzero((ref["kind"] == kind) & (ref["n_links"] == n) & (ref["random_start"] == rs) & (ref["width_given"] == wg))
        nf = 3 * n + (4 if kind == 1 else 3)
        q, qd = cuda(ref["q"][rows, :n]), cuda(ref["qd"][rows, :n])
        task = cuda(ref["task"][rows, :2] if kind == 0 else ref["task"][rows])
        steps = cuda(ref["steps"][rows], torch.int32)
        eng = engine(n)
        mask = ref["context_mask"][rows[0], :nf]
        col_mask = sum(1 << c for c in np.flatnonzero(mask))
        full = eng.reacher_observation(ENVS[kind], q, qd, task, steps).cpu().numpy()
        ctx = eng.reacher_observation(ENVS[kind], q, qd, task, steps, col_mask=col_mask).cpu().numpy()
        ta = eng.reacher_observation(ENVS[kind], q, qd, task, steps, time_div=200.0).cpu().numpy()
        what = (ENVS[kind], n, rs, wg)
        assert_rows(full, ref["obs64"][rows, :nf], what, exact_cols=(nf - 1,))
        assert_rows(ctx, ref["obs64"][rows, :nf][:, mask], what + ("context",))
        assert_rows(ta, ref["ta64"][rows, :nf + 1], what + ("time aware",), exact_cols=(nf - 1, nf))


# ---- BatchedBlackBox against the host wrappers ------------------------------------------------------------------------------------
def simple_host(name, mp_type="ProMP", random_start=True, every=None):
    kw = {"verbose": 2}
    if every is not None:
        kw.update(replanning_schedule=lambda pos, vel, obs, action, t: t % every == 0)
    return _gym.make(f"fancy_{mp_type}/{name}-v0", random_start=random_start, mp_config_override={"black_box_kwargs": kw})


def simple_batched(env, B, random_start=True, **kw):
    return BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=0.01, duration=2.0, act_low=-1000.0, act_high=1000.0,
                           plant="double_integrator", reward="simple_reacher", max_episode_steps=200,
                           env_kwargs={"random_start": random_start}, **kw)


def np_(x):
    return x.cpu().numpy()


def compare_step(envs, bb_out, params, tag):
    """host env b's step against the batched step: obs, and step_observations over the executed steps"""
    obs = np_(bb_out["obs"])
    steps = np_(bb_out["step_observations"]) if "step_observations" in bb_out else None
    n_exec = np_(bb_out["trajectory_length"])
    for b, env in enumerate(envs):
        o, _, term, trunc, info = env.step(params[b])
        n = info["trajectory_length"]
        assert n_exec[b] == n, (tag, b)
        assert_rows(obs[b:b + 1], np.asarray(o, np.float64)[None], (tag, "obs", b))
        if steps is not None:
            assert_rows(steps[b, :n], np.asarray(info["step_observations"], np.float64), (tag, "step_observations", b))
            assert not steps[b, n:].any(), (tag, b)
    return obs


@pytest.mark.parametrize("mp_type", ["ProMP", "DMP"])
def test_hole_reacher_observations_equal_the_host_wrappers(mp_type):
    B, seed = 24, 300
    envs = [host_env(mp_type) for _ in range(B)]
    reset_obs = np.stack([e.reset(seed=seed + b)[0] for b, e in enumerate(envs)])
    bb = batched(envs[0], B, verbose=2, observations=True)
    assert bb.observation_space == envs[0].observation_space
    bb.reset(seed=seed)
    assert_rows(np_(bb.observe()), reset_obs.astype(np.float64), "reset")
    rng = np.random.default_rng(4)
    scale = np.geomspace(0.01, 2.0, B)[:, None] * (1.0 if mp_type == "ProMP" else 0.05)
    params = (rng.standard_normal((B, envs[0].action_space.shape[0])) * scale).astype(np.float32)
    out = bb.step(params)
    assert out["terminated"].any() and not out["terminated"].all()          # collided episodes in the batch
    compare_step(envs, out, params, mp_type)


def test_hole_reacher_replanning_observations_over_a_whole_episode():
    B, seed, every = 16, 700, 50
    envs = [host_env("ProMP", every) for _ in range(B)]
    reset_obs = np.stack([e.reset(seed=seed + b)[0] for b, e in enumerate(envs)])
    bb = batched(envs[0], B, replanning_every=every, verbose=2, observations=True)
    assert bb.observation_space == envs[0].observation_space
    bb.reset(seed=seed)
    assert_rows(np_(bb.observe()), reset_obs.astype(np.float64), "reset")
    rng = np.random.default_rng(9)
    live = np.ones(B, bool)
    for plan in range(200 // every):
        params = (rng.standard_normal((B, envs[0].action_space.shape[0])) * np.geomspace(0.01, 1.0, B)[:, None]).astype(np.float32)
        out = bb.step(params)
        obs, steps, n_exec = np_(out["obs"]), np_(out["step_observations"]), np_(out["trajectory_length"])
        for b in range(B):
            if not live[b]:
                assert n_exec[b] == 0 and not steps[b].any()
                continue
            o, _, term, trunc, info = envs[b].step(params[b])
            n = info["trajectory_length"]
            assert n_exec[b] == n and obs.shape[1] == 3 * 5 + 5
            assert_rows(obs[b:b + 1], np.asarray(o, np.float64)[None], ("replan obs", plan, b), exact_cols=(18, 19))
            assert_rows(steps[b, :n], np.asarray(info["step_observations"], np.float64), ("replan steps", plan, b), exact_cols=(18, 19))
            live[b] = not (term or trunc)
    assert not live.any()


@pytest.mark.parametrize("name,n", [("SimpleReacher", 2), ("LongSimpleReacher", 5)])
@pytest.mark.parametrize("random_start", [True, False])
def test_simple_reacher_observations_equal_the_host_wrappers(name, n, random_start):
    B, seed = 8, 40
    envs = [simple_host(name, random_start=random_start) for _ in range(B)]
    reset_obs = np.stack([e.reset(seed=seed + b)[0] for b, e in enumerate(envs)])
    bb = simple_batched(envs[0], B, random_start, verbose=2, observations=True)
    assert bb.observation_space == envs[0].observation_space
    bb.reset(seed=seed)
    assert_rows(np_(bb.observe()), reset_obs.astype(np.float64), "reset")
    params = (np.random.default_rng(3).standard_normal((B, envs[0].action_space.shape[0])) * 50).astype(np.float32)
    compare_step(envs, bb.step(params), params, (name, random_start))


# ---- the replay against the rollout -----------------------------------------------------------------------------------------------
def random_plan(B, D, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pos = (torch.randn((B, 200, D), generator=g, device="cuda") * scale).cumsum(1).float() * 0.05 + 1.0
    vel = torch.randn((B, 200, D), generator=g, device="cuda") * scale
    return pos.contiguous(), vel.float().contiguous()


@pytest.mark.parametrize("B", [1, 1000, 65536])
@pytest.mark.parametrize("kind,ctrl", [("simple_reacher", "motor"), ("simple_reacher", "velocity"), ("hole_reacher", "motor"),
                                       ("hole_reacher", "velocity")])
def test_replay_end_state_equals_the_rollout(B, kind, ctrl):
    D = 5 if kind == "hole_reacher" else 2
    eng = engine(D)
    plant = "velocity_direct" if kind == "hole_reacher" else "double_integrator"
    lim = LIM if kind == "hole_reacher" else 1000.0
    spec = RolloutSpec(ctrl, D, 0.6, 0.075, -lim, lim, plant=plant, dt=0.01)
    pos, vel = random_plan(B, D, 11 + B, 1.0 if ctrl == "velocity" else 5.0)
    g = torch.Generator(device="cuda").manual_seed(B)
    q0 = (torch.rand((B, D), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 2.0
    qd0 = torch.zeros_like(q0) if kind == "hole_reacher" else torch.randn((B, D), generator=g, device="cuda", dtype=torch.float64)
    q0[:, 0] += 1.5
    step0 = torch.randint(0, 2, (B,), generator=g, device="cuda", dtype=torch.int32)     # both sides of the dtype rule
    q, qd = q0.clone(), qd0.clone()
    if kind == "hole_reacher":
        hole = torch.stack([torch.full((B,), 2.0, device="cuda", dtype=torch.float64),
                            torch.full((B,), 0.3, device="cuda", dtype=torch.float64),
                            torch.ones(B, device="cuda", dtype=torch.float64)], 1).contiguous()
        n_steps = torch.randint(0, 201, (B,), generator=g, device="cuda", dtype=torch.int32)
        r = eng.hole_reacher_rollout(spec, pos, vel, q, qd, hole, n_steps=n_steps, step0=step0, want_actions=False, want_rewards=False)
        n_exec, task = r["n_exec"], hole
    else:
        goal = torch.rand((B, 2), generator=g, device="cuda", dtype=torch.float64)
        n_exec = torch.randint(0, 201, (B,), generator=g, device="cuda", dtype=torch.int32)
        eng.reacher_rollout(spec, pos, vel, q, qd, goal, n_steps=n_exec, step0=step0)
        task = goal
    steps, qe, qde = eng.reacher_step_observations(kind, spec, pos, vel, q0, qd0, task, n_exec, step0, end_state=True)
    torch.cuda.synchronize()
    assert torch.equal(qe, q) and torch.equal(qde, qd)
    n = n_exec.cpu().numpy()
    # the last executed row is the observation of the state the rollout left; rows behind it are 0
    obs = eng.reacher_observation(kind, q, qd, task, step0 + n_exec).cpu().numpy()
    s = steps.cpu().numpy()
    has = n > 0
    rows = np.arange(B)[has]
    assert np.array_equal(s[rows, n[has] - 1], obs[has])
    t = np.arange(200)[None, :]
    assert not s[t >= n[:, None]].any()
    assert s.shape == (B, 200, 3 * D + (4 if kind == "hole_reacher" else 3))


@pytest.mark.parametrize("reward", ["simple_reacher", "hole_reacher"])
def test_last_step_observation_is_obs_without_replanning(reward):
    B = 32
    if reward == "hole_reacher":
        env = host_env("ProMP")
        bb = batched(env, B, verbose=2, observations=True)
    else:
        env = simple_host("LongSimpleReacher")
        bb = simple_batched(env, B, verbose=2, observations=True)
    bb.reset(seed=5)
    params = (np.random.default_rng(2).standard_normal((B, env.action_space.shape[0])) * 0.5).astype(np.float32)
    out = bb.step(params)
    n = np_(out["trajectory_length"])
    last = np_(out["step_observations"])[np.arange(B), n - 1]
    mask = np.array([bool(bb._obs_mask >> c & 1) for c in range(last.shape[1])])
    assert np.array_equal(last[:, mask], np_(out["obs"]))


# ---- nothing changes without the flag; graphs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward", ["simple_reacher", "hole_reacher"])
@pytest.mark.parametrize("verbose", [2, 1])
def test_the_flag_changes_nothing_else(reward, verbose):
    B = 64
    env = host_env("ProMP") if reward == "hole_reacher" else simple_host("SimpleReacher")
    make = (lambda **kw: batched(env, B, verbose=verbose, **kw)) if reward == "hole_reacher" else \
        (lambda **kw: simple_batched(env, B, verbose=verbose, **kw))
    params = (np.random.default_rng(1).standard_normal((B, env.action_space.shape[0])) * 0.5).astype(np.float32)
    outs = {}
    for flag in (False, True):
        bb = make(observations=flag)
        bb.reset(seed=77)
        outs[flag] = {k: np_(v) for k, v in bb.step(params).items() if isinstance(v, torch.Tensor)}
        outs[flag]["q_after"], outs[flag]["qd_after"] = np_(bb.q), np_(bb.qd)
        if not flag:
            assert bb.observation_space is None
            with pytest.raises(ValueError, match="observations=True"):
                bb.observe()
    off, on = outs[False], outs[True]
    assert "obs" not in off and "step_observations" not in off
    assert set(on) - set(off) == ({"obs", "step_observations"} if verbose >= 2 else {"obs"})
    for k in off:
        assert np.array_equal(off[k], on[k]), k


@pytest.mark.parametrize("reward", ["simple_reacher", "hole_reacher"])
def test_captured_episode_observations_equal_eager_ones(reward):
    B, n_plans = 48, 2
    env = host_env("ProMP") if reward == "hole_reacher" else simple_host("SimpleReacher")
    make = (lambda: batched(env, B, verbose=2, observations=True)) if reward == "hole_reacher" else \
        (lambda: simple_batched(env, B, verbose=2, observations=True))
    rng = np.random.default_rng(6)
    params = [(rng.standard_normal((B, env.action_space.shape[0])) * 0.5).astype(np.float32) for _ in range(n_plans)]
    eager, gbb = make(), make()
    eager.reset(seed=123)
    gbb.reset(seed=123)
    graph = gbb.capture_episode(n_plans, sample=True)
    for k in range(n_plans):
        graph.params[k].copy_(torch.as_tensor(params[k]))
    for rep in range(2):
        eager.reset(sample=True)
        want0 = eager.observe().clone()
        want = []
        for k in range(n_plans):
            o = eager.step(params[k])
            want.append({key: o[key].clone() for key in ("obs", "step_observations")})
        want_after = eager.observe().clone()
        outs = graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(graph.reset_obs, want0), rep
        for k in range(n_plans):
            for key in ("obs", "step_observations"):
                assert torch.equal(outs[k][key], want[k][key]), (rep, k, key)
        assert torch.equal(outs[-1]["obs"], want_after)
    # without sample: the captured reset observation is the eager one of the same inputs
    eager2, gbb2 = make(), make()
    eager2.reset(seed=999)
    init_pos = eager2.q.clone()
    task = (eager2.hole if reward == "hole_reacher" else eager2.goal).clone()
    want0 = eager2.observe().clone()
    graph2 = gbb2.capture_episode(1)
    graph2.init_pos.copy_(init_pos)
    (graph2.hole if reward == "hole_reacher" else graph2.goal).copy_(task)
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(graph2.reset_obs, want0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_observations_refuse_other_rewards_and_pos_limits():
    env = simple_host("SimpleReacher")
    with pytest.raises(ValueError, match="reacher"):
        BatchedBlackBox(env.traj_gen, env.tracking_controller, 4, dt=0.01, duration=2.0, plant="double_integrator", observations=True)
    with pytest.raises(ValueError, match="pos_limits"):
        simple_batched(env, 4, observations=True, pos_limits=([-3.0] * 2, [3.0] * 2))


def test_entry_points_reject_bad_arguments():
    eng = engine(2)
    lib, h = eng._lib, eng._h
    B = 4
    q = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
    task = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
    steps = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.empty((B, 200, 9), dtype=torch.float32, device="cuda")
    plan = torch.zeros((B, 200, 2), dtype=torch.float32, device="cuda")
    spec = RolloutSpec("motor", 2, 0.6, 0.075, -1000.0, 1000.0, plant="double_integrator", dt=0.01)

    def cfg(env=0, n=2, mask=0, div=0.0):
        c = _lib.mpk_obs_cfg()
        c.env, c.n_links, c.col_mask, c.time_div = env, n, mask, div
        return c

    def obs(c, qp=q.data_ptr(), op=out.data_ptr()):
        return lib.mpk_reacher_observation(h, C.byref(c) if c is not None else None, qp, q.data_ptr(), task.data_ptr(),
                                           steps.data_ptr(), op, B, None)

    def step_obs(c, qp=q.data_ptr(), pp=plan.data_ptr()):
        return lib.mpk_reacher_step_observations(h, C.byref(c), C.byref(spec.c), pp, plan.data_ptr(), qp, q.data_ptr(), task.data_ptr(),
                                                 steps.data_ptr(), steps.data_ptr(), out.data_ptr(), None, None, B, 200, None)

    for bad, msg in ((cfg(env=2), "unknown env"), (cfg(n=17), "n_links"), (cfg(n=0), "n_links"), (cfg(n=5), "num_dof"),
                     (cfg(mask=1 << 9), "outside the full row"), (cfg(div=-1.0), "time_div"), (cfg(div=float("nan")), "time_div"),
                     (None, "cfg is NULL")):
        assert obs(bad) == _lib.MPK_EINVAL, msg
        assert msg in lib.mpk_last_error().decode(), (msg, lib.mpk_last_error())
        if bad is not None:
            assert step_obs(bad) == _lib.MPK_EINVAL and msg in lib.mpk_last_error().decode()
    assert obs(cfg(), qp=None) == _lib.MPK_EINVAL and "NULL" in lib.mpk_last_error().decode()
    assert obs(cfg(), op=None) == _lib.MPK_EINVAL and "NULL" in lib.mpk_last_error().decode()
    assert step_obs(cfg(), qp=None) == _lib.MPK_EINVAL and "NULL" in lib.mpk_last_error().decode()
    assert step_obs(cfg(), pp=None) == _lib.MPK_EINVAL and "NULL" in lib.mpk_last_error().decode()
    # a hole reacher cfg with the torque plant, a simple one with the direct plant
    direct = RolloutSpec("velocity", 2, 0.0, 0.0, -LIM, LIM, plant="velocity_direct", dt=0.01)
    assert lib.mpk_reacher_step_observations(h, C.byref(cfg(env=1)), C.byref(spec.c), plan.data_ptr(), plan.data_ptr(), q.data_ptr(),
                                             q.data_ptr(), task.data_ptr(), steps.data_ptr(), steps.data_ptr(), out.data_ptr(), None,
                                             None, B, 200, None) == _lib.MPK_EINVAL
    assert lib.mpk_reacher_step_observations(h, C.byref(cfg()), C.byref(direct.c), plan.data_ptr(), plan.data_ptr(), q.data_ptr(),
                                             q.data_ptr(), task.data_ptr(), steps.data_ptr(), steps.data_ptr(), out.data_ptr(), None,
                                             None, B, 200, None) == _lib.MPK_EINVAL
    # and the good calls pass
    assert obs(cfg()) == 0 and step_obs(cfg()) == 0
    torch.cuda.synchronize()
