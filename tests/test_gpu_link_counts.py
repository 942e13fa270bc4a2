"""The reacher kernels at link counts other than 2 and 5 against the REFERENCE (tests/golden/ref_reacher_links.npz, written by
tests/golden/make_ref_link_count_golden.py): 1, 3, 7, 8, 9, 15, 16 links.  From 8 entries on np.sum of a vector adds with eight
accumulators, not in index order, and the reference's rewards are such sums over the links; the kernels' run-time link count, the
self-collision loop over all link pairs and the observation layout are the other things these counts reach.

Rewards: bit for bit on every executed step that pays no distance term (no sin / cos enters them), rtol 1e-12 where one is paid (device
against host libm, the bound of tests/test_gpu_hole_reacher.py).  State, actions, flags, observations, generator words: bit for bit.
That holds for all three reward functions: vel_acc's two non-zero products are added as np.dot adds them (fused, one rounding each).
Each comparison prints its figures first (`[links] ...`): rows that differ and the largest relative difference.

HoleReacher has no reference STEP with one link (the generator says why), so its plans and traces start at three links."""
import json
import os

import numpy as np
import pytest
import torch

from fancy_gym_amd import BatchedStepEnv, RolloutSpec, TrajectoryEngine
from oracle import mp_oracle as O

from .test_gpu_step_env import Chain, policy_actions

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_reacher_links.npz"))
TRACES = json.loads(str(GOLD["traces"]))
REW_FCTS = tuple(str(f) for f in GOLD["rew_fct"])
LINKS = (1, 3, 7, 8, 9, 15, 16)
HOLE_LINKS = LINKS[1:]
HORIZONS = ((12, 0), (25, 176))
LIM = float(np.float32(2 * np.pi))
ENVS = {0: "simple_reacher", 1: "hole_reacher"}
HOLE_KW = dict(random_start=True, hole_width=None, hole_x=None, hole_depth=1.0)
_engines = {}


def engine(D):
    if D not in _engines:
        _engines[D] = TrajectoryEngine("promp", "linear", "zero_rbf", D, 5, dt=0.01, duration=2.0, tau=2.0, num_basis_zero_start=1,
                                       device=0)
    return _engines[D]


def cuda(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")


def cpu(t):
    return t.detach().cpu().numpy()


def check_rewards(tag, got, want, executed, paid):
    """bit equality on the executed steps without a distance term, rtol 1e-12 with one, exact zeros behind the break; the figures are
    printed before anything is asserted.  Returns the number of rewards without a distance term that differ, and how many there are"""
    plain = executed & ~paid
    differ = plain & (got != want)
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"[links] {tag}: {int(differ.sum())} of {int(plain.sum())} rewards without a distance term differ, largest relative "
          f"difference {float(rel[plain].max()) if plain.any() else 0.0:.3e}; with one: {int((executed & paid).sum())} rewards, largest "
          f"relative difference {float(rel[executed & paid].max()) if (executed & paid).any() else 0.0:.3e}")
    assert not differ.any(), (tag, int(differ.sum()), float(rel[plain].max()))
    np.testing.assert_allclose(got[executed & paid], want[executed & paid], rtol=1e-12, atol=0, err_msg=tag)
    assert not got[~executed].any(), tag
    return int(differ.sum()), int(plain.sum())


# ---- (a) mpk_hole_reacher_rollout against the reference's black-box plans -----------------------------------------------------------
def plan(k):
    return GOLD["plan__" + k]


def plan_rows(D, ctrl, T, step0, B):
    rows = np.flatnonzero((plan("D") == D) & (plan("ctrl") == ctrl) & (plan("T") == T))
    assert len(rows) >= 5 and (plan("step0")[rows] == step0).all()
    return rows, rows[np.arange(B) % len(rows)]


def run_plans(D, ctrl, idx, T, rew_fct, agg):
    """the episodes idx of the fixture through mpk_hole_reacher_rollout2: every output as a numpy array, q / qd after the plan"""
    eng, B = engine(D), len(idx)
    spec = RolloutSpec(("motor", "velocity")[ctrl], D, 1.0, 0.1, -LIM, LIM, plant="velocity_direct", dt=0.01)
    q, qd = cuda(plan("q0")[idx, :D], torch.float64), cuda(plan("qd0")[idx, :D], torch.float64)
    state = torch.full((B, 2), np.nan, dtype=torch.float64, device="cuda")
    o = eng.hole_reacher_rollout(spec, cuda(plan("des_pos")[idx, :T, :D]), cuda(plan("des_vel")[idx, :T, :D]), q, qd,
                                 cuda(plan("hole")[idx], torch.float64), collision_penalty=100.0,
                                 n_steps=cuda(plan("n_steps")[idx], torch.int32), step0=cuda(plan("step0")[idx], torch.int32),
                                 rew_fct=rew_fct, reward_state=state, aggregation=agg)
    assert torch.equal(o["ret"], eng.reward_aggregate(o["rewards"], o["n_exec"], agg)), (D, ctrl, T, rew_fct, agg)
    out = {k: cpu(v) for k, v in o.items() if isinstance(v, torch.Tensor)}
    out["q"], out["qd"] = cpu(q), cpu(qd)
    return out


def plan_masks(idx, T, step0, rew_fct):
    """(executed, paid) [B, T]: the steps a plan ran, and those of them that pay a distance term -- env step 199, and but for vel_acc
    the colliding step"""
    t, n = np.arange(T)[None], plan("n_exec")[idx][:, None]
    paid = np.broadcast_to(step0 + t == 199, (len(idx), T)).copy()
    if rew_fct != "vel_acc":
        paid |= plan("collided")[idx, None] & (t == n - 1)
    return t < n, paid


@pytest.mark.parametrize("rew_fct", REW_FCTS)
@pytest.mark.parametrize("ctrl", [0, 1])
@pytest.mark.parametrize("D", HOLE_LINKS)
def test_hole_reacher_rollout_equals_the_reference_plans(D, ctrl, rew_fct):
    """the fixture's episodes tiled to 259 (a full 256-lane workgroup and a part-full wave): every copy the same bits, with both
    wall tests, and the in-kernel return of every aggregation equal to the aggregate of the stored rewards"""
    B, r = 259, REW_FCTS.index(rew_fct)
    eng = engine(D)
    for T, step0 in HORIZONS:
        rows, idx = plan_rows(D, ctrl, T, step0, B)
        tag = f"k_hole_rollout D {D} {('motor', 'velocity')[ctrl]} {rew_fct} T {T}"
        executed, paid = plan_masks(idx, T, step0, rew_fct)
        first = None
        for sampled in (0, 1):
            eng.set_option("hole_sampled", sampled)
            try:
                for agg in ("sum", "mean", "last"):
                    out = run_plans(D, ctrl, idx, T, rew_fct, agg)
                    for k, v in out.items():
                        assert np.array_equal(v, v[np.arange(B) % len(rows)], equal_nan=True), (tag, k, "copies differ")
                    assert np.array_equal(out["n_exec"], plan("n_exec")[idx]), tag
                    assert np.array_equal(out["collided"].astype(bool), plan("collided")[idx]), tag
                    assert np.array_equal(out["success"].astype(bool), plan("success")[r, idx]), tag
                    assert np.array_equal(out["q"], plan("q")[idx, :D]) and np.array_equal(out["qd"], plan("qd")[idx, :D]), tag
                    assert np.array_equal(out["actions"], plan("actions")[idx, :T, :D]), tag
                    assert not out["actions"][~executed].any(), tag
                    if first is None:
                        first = out["rewards"]
                        check_rewards(tag, first, plan("rewards")[r][idx, :T], executed, paid)
                    else:                 # the other wall test, the other aggregations: the same step rewards
                        assert np.array_equal(out["rewards"], first), (tag, sampled, agg)
            finally:
                eng.set_option("hole_sampled")


# ---- (b) BatchedStepEnv(n_links=D) against the reference's vector-env traces ---------------------------------------------------------
def step_env(tr, n, rew_fct):
    if tr["env"] == "simple_reacher":
        return BatchedStepEnv(n, env="simple_reacher", n_links=tr["n_links"], device=0)
    kw = tr["kwargs"]
    assert kw["random_start"] and kw["hole_width"] is None and kw["hole_x"] is None and kw["hole_depth"] == 1
    return BatchedStepEnv(n, env="hole_reacher", n_links=tr["n_links"], rew_fct=rew_fct, collision_penalty=float(kw["collision_penalty"]),
                          allow_self_collision=kw["allow_self_collision"], allow_wall_collision=kw["allow_wall_collision"],
                          env_kwargs=dict(HOLE_KW), device=0)


TRACE_CASES = [(t["name"], f) for t in TRACES for f in (REW_FCTS if t["env"] == "hole_reacher" else (None,))]


def run_trace(tr, rew_fct):
    """the trace's seeded reset (checked here) and its S steps on the device: every output and the state after every step"""
    name = tr["name"]
    g = lambda k: GOLD[f"{name}__{k}"]      # noqa: E731
    hole = tr["env"] == "hole_reacher"
    env = step_env(tr, tr["N"], rew_fct)
    obs0, info0 = env.reset(seed=tr["seed"])
    assert info0 == {}
    np.testing.assert_array_equal(cpu(obs0), g("obs0"))
    np.testing.assert_array_equal(cpu(env.q), g("q0"))
    np.testing.assert_array_equal(cpu(env.qd), g("qd0"))
    np.testing.assert_array_equal(cpu(env.task), g("task0"))
    np.testing.assert_array_equal(cpu(env.rng).view(np.uint64), g("rng0"))
    acts = torch.from_numpy(g("actions")).to(env.device)
    keys = ("obs", "reward", "terminated", "truncated", "final_obs", "_final_obs") + (("is_collided", "is_success") if hole else ())
    state = ("q", "qd", "traj_steps", "task", "rng")
    rec = {k: [] for k in keys + state}
    for t in range(tr["S"]):
        obs, rew, term, trunc, info = env.step(acts[t])
        for k, v in (("obs", obs), ("reward", rew), ("terminated", term), ("truncated", trunc)):
            rec[k].append(v.clone())
        for k in keys[4:]:
            rec[k].append(info[k].clone())
        for k in state:
            rec[k].append(getattr(env, k).clone())
    return {k: cpu(torch.stack(v)) for k, v in rec.items()}


def trace_paid(name, rew_fct):
    """the steps that pay a distance term: SimpleReacher from env step 199 on (the step that truncates); HoleReacher at step 199 and,
    but for vel_acc, at the colliding step"""
    paid = GOLD[f"{name}__truncated"].copy()
    if rew_fct not in (None, "vel_acc"):
        paid |= GOLD[f"{name}__is_collided"]
    return paid


@pytest.mark.parametrize("name, rew_fct", TRACE_CASES)
def test_step_env_equals_the_reference_traces(name, rew_fct):
    """what tests/test_gpu_step_env.py: test_reference_traces checks, at these link counts: every row, every step"""
    tr = next(t for t in TRACES if t["name"] == name)
    g = lambda k: GOLD[f"{name}__{k}"]      # noqa: E731
    hole = tr["env"] == "hole_reacher"
    r = REW_FCTS.index(rew_fct) if hole else None
    out = run_trace(tr, rew_fct)
    for k in ("q", "qd", "task", "final_obs", "terminated", "truncated") + (("is_collided",) if hole else ()):
        np.testing.assert_array_equal(out[k], g(k), err_msg=f"{name} {k}")
    if hole:
        np.testing.assert_array_equal(out["is_success"], g("is_success")[r], err_msg=name)
    np.testing.assert_array_equal(out["traj_steps"], g("steps"), err_msg=name)
    np.testing.assert_array_equal(out["rng"].view(np.uint64), g("rng"), err_msg=name)
    want_obs = g("final_obs").copy()
    want_mask = np.zeros(g("terminated").shape, bool)
    for (t, b), o in zip(g("reset_at"), g("reset_obs")):
        want_obs[t, b] = o
        want_mask[t, b] = True
    np.testing.assert_array_equal(out["obs"], want_obs, err_msg=name)
    np.testing.assert_array_equal(out["_final_obs"], want_mask, err_msg=name)
    np.testing.assert_array_equal(want_mask, g("terminated") | g("truncated"))
    want = g("reward")[r] if hole else g("reward")
    check_rewards(f"k_reacher_env_step {name} {rew_fct}", out["reward"], want, np.ones(want.shape, bool), trace_paid(name, rew_fct))


def test_vel_acc_rewards_without_a_distance_term_equal_the_reference_bit_for_bit():
    """The reference forms a reward as np.dot(features, factors).  Under "simple" and "unbounded" a step without a distance term has
    ONE non-zero product, and every way of adding gives the same bits.  Under "vel_acc" it has two, vel_cost * -1e-4 and
    acc_cost * -1e-6, and np.dot's loop over five entries is a chain of fused multiply-adds in index order: one rounding per entry.
    The kernels rounded each product before adding and missed one reward in five by a unit in the last place -- at EVERY link
    count, the five of the existing fixture included, where rtol 1e-12 let it pass (profiles/r20_link_counts.md).
    hole_vel_acc_reward (mpk_hole_geom.h) is the chain.  Here: every vel_acc reward of the link-count fixture once more in one
    place, and the five-link episodes of tests/golden/ref_hole_rewards.npz, whose own test keeps rtol 1e-12 for every step"""
    differ = total = 0
    for D in HOLE_LINKS:
        for ctrl in (0, 1):
            for T, step0 in HORIZONS:
                rows, idx = plan_rows(D, ctrl, T, step0, len(plan_rows(D, ctrl, T, step0, 1)[0]))
                out = run_plans(D, ctrl, idx, T, "vel_acc", "sum")
                executed, paid = plan_masks(idx, T, step0, "vel_acc")
                d, n = check_rewards(f"vel_acc plans D {D} ctrl {ctrl} T {T}", out["rewards"], plan("rewards")[1][idx, :T], executed, paid)
                differ, total = differ + d, total + n
    assert differ == 0 and total >= 1000
    # five links: whole episodes (T = 200, step0 = 0) of the fixture that had five links only
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hole_rewards.npz"))
    assert str(ref["rew_fct"][1]) == "vel_acc"
    eng, T, D = engine(5), 200, 5
    for ctrl in (0, 1):
        idx = np.flatnonzero((ref["ctrl"] == ctrl) & (ref["penalty"] == 100.0) & ~ref["allow_self"] & ~ref["allow_wall"])
        assert len(idx) >= 9
        spec = RolloutSpec(("motor", "velocity")[ctrl], D, 1.0, 0.1, -LIM, LIM, plant="velocity_direct", dt=0.01)
        q, qd = cuda(ref["q0"][idx], torch.float64), torch.zeros((len(idx), D), dtype=torch.float64, device="cuda")
        o = eng.hole_reacher_rollout(spec, cuda(ref["des_pos"][idx]), cuda(ref["des_vel"][idx]), q, qd, cuda(ref["hole"][idx], torch.float64),
                                     collision_penalty=100.0, rew_fct="vel_acc")
        n = ref["n_exec"][idx]
        assert np.array_equal(cpu(o["n_exec"]), n) and np.array_equal(cpu(o["actions"]), ref["actions"][idx])
        t = np.arange(T)[None]
        d, total = check_rewards(f"vel_acc five links ctrl {ctrl}", cpu(o["rewards"]), ref["rewards"][1][idx], t < n[:, None],
                                 np.broadcast_to(t == 199, (len(idx), T)))
        assert d == 0 and total >= 1000


@pytest.mark.parametrize("rew_fct", REW_FCTS)
@pytest.mark.parametrize("B", [3, 131])
@pytest.mark.parametrize("D", HOLE_LINKS)
def test_one_launch_step_equals_the_two_launch_chain(D, B, rew_fct):
    """k_reacher_env_step<kMaxD> against k_hole_rollout<0> with T = 1 followed by k_reacher_autoreset, bit for bit; 131 = one 128-lane
    workgroup and three lanes"""
    steps = 205
    env = BatchedStepEnv(B, env="hole_reacher", n_links=D, rew_fct=rew_fct, env_kwargs=dict(HOLE_KW), device=0)
    env.reset(seed=77)
    chain = Chain(B, rew_fct, 77, D=D)
    acts = policy_actions(B, D, steps, 5 + B + D, env.device)
    acts[:, : max(1, B // 3), 0] *= 0.05            # a third of the rows never swing: they live to the step limit
    acts[:, : max(1, B // 3), 1:] *= 2.0 / D
    n_trunc = n_coll = 0
    for t in range(steps):
        before = chain.traj_steps.clone()
        want = chain.step(acts[t])
        obs, rew, term, trunc, info = env.step(acts[t])
        tag = f"D {D} B {B} {rew_fct} step {t}"
        assert torch.equal(obs, want["obs"]) and torch.equal(info["final_obs"], want["final_obs"]), tag
        assert torch.equal(rew, want["reward"]), tag
        assert torch.equal(term.view(torch.uint8), want["collided"]) and torch.equal(info["is_collided"], term), tag
        assert torch.equal(trunc, before + 1 >= 200), tag
        assert torch.equal(info["is_success"].view(torch.uint8), want["success"]), tag
        assert torch.equal(info["_final_obs"].view(torch.uint8), want["reset_mask"]), tag
        assert torch.equal(info["_final_obs"], term | trunc) and torch.equal(want["done"].view(torch.bool), term | trunc), tag
        for k in ("q", "qd", "traj_steps", "task", "rng"):
            assert torch.equal(getattr(env, k), getattr(chain, k)), (tag, k)
        if rew_fct == "unbounded":
            assert torch.equal(env.reward_state, chain.reward_state), tag
        n_trunc += int(trunc.sum())
        n_coll += int(term.sum())
    assert n_trunc >= 1 and (n_coll >= 1 or B < 100)


# ---- (c) observations and resets -----------------------------------------------------------------------------------------------------
def task_of(kind, task):
    return cuda(task[:, :2] if kind == 0 else task, torch.float64)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D", LINKS)
def test_observation_rows_equal_the_reference(D, kind):
    rows = np.flatnonzero((GOLD["obs__kind"] == kind) & (GOLD["obs__n_links"] == D))
    assert len(rows) >= 4
    n = 3 * D + (4 if kind == 1 else 3)
    got = engine(D).reacher_observation(ENVS[kind], cuda(GOLD["obs__q"][rows, :D]), cuda(GOLD["obs__qd"][rows, :D]),
                                        task_of(kind, GOLD["obs__task"][rows]), cuda(GOLD["obs__steps"][rows], torch.int32))
    want = GOLD["obs__obs"][rows, :n]
    assert not np.isnan(want).any() and np.isnan(GOLD["obs__obs"][rows, n:]).all()
    np.testing.assert_array_equal(cpu(got).view(np.uint32), want.view(np.uint32), err_msg=f"{ENVS[kind]} {D} links")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D", LINKS)
def test_resets_and_autoresets_equal_the_reference(D, kind):
    """reset(seed) then three unseeded resets: through mpk_reacher_reset, and the unseeded ones again through mpk_reacher_autoreset
    with every other row selected (the rows left out stay where they are)"""
    rows = np.flatnonzero((GOLD["reset__kind"] == kind) & (GOLD["reset__n_links"] == D))
    B, n = len(rows), 3 * D + (4 if kind == 1 else 3)
    assert B >= 4
    eng, env = engine(D), ENVS[kind]
    kw = dict(HOLE_KW) if kind == 1 else dict(random_start=True, target=None)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    seeds = torch.from_numpy(GOLD["reset__seed"][rows].view(np.int64)).cuda()
    want = {k: GOLD["reset__" + k][rows] for k in ("q0", "task", "rng", "obs")}

    def fresh():
        return dict(q=torch.full((B, D), 7.0, **f64), qd=torch.full((B, D), 7.0, **f64), ts=torch.full((B,), 3, **i32),
                    ps=torch.full((B,), 3, **i32), done=torch.ones(B, dtype=torch.uint8, device="cuda"),
                    rng=torch.zeros((B, 5), dtype=torch.int64, device="cuda"), task=torch.empty((B, 2 if kind == 0 else 3), **f64))

    def same(s, k, sel=slice(None)):
        tag = (env, D, k)
        assert np.array_equal(cpu(s["q"])[sel], want["q0"][sel, k, :D]), tag
        assert np.array_equal(cpu(s["task"])[sel], want["task"][sel, k, :s["task"].shape[1]]), tag
        assert np.array_equal(cpu(s["rng"]).view(np.uint64)[sel], want["rng"][sel, k]), tag
        assert not s["qd"][sel].any() and not s["ts"][sel].any(), tag
        obs = cpu(eng.reacher_observation(env, s["q"], s["qd"], s["task"], s["ts"]))
        assert np.array_equal(obs.view(np.uint32)[sel], want["obs"][sel, k, :n].view(np.uint32)), tag
        return obs

    s = fresh()
    for k in range(4):
        eng.reacher_reset(env, s["q"], s["qd"], s["ts"], s["ps"], s["done"], s["rng"], s["task"], seeds=seeds if k == 0 else None, **kw)
        same(s, k)
    # the autoreset: rows 0, 2, 4, ... are reset (k -> k + 1), the others keep the state and the observation they had
    s = fresh()
    eng.reacher_reset(env, s["q"], s["qd"], s["ts"], s["ps"], s["done"], s["rng"], s["task"], seeds=seeds, **kw)
    entry = same(s, 0)
    sel = np.arange(B) % 2 == 0
    s["done"].copy_(torch.from_numpy(sel.astype(np.uint8)))
    final, obs, mask = eng.reacher_autoreset(env, s["q"], s["qd"], s["ts"], s["ps"], s["done"], s["rng"], s["task"], **kw)
    assert np.array_equal(cpu(mask).astype(bool), sel)
    assert np.array_equal(cpu(final).view(np.uint32), entry.view(np.uint32))
    after = same(s, 1, sel)
    same(s, 0, ~sel)
    assert np.array_equal(cpu(obs).view(np.uint32), after.view(np.uint32))
    assert np.array_equal(cpu(obs)[~sel].view(np.uint32), entry[~sel].view(np.uint32))


# ---- SimpleReacher's black-box rollout against the oracle in numpy's order of additions ------------------------------------------------
@pytest.mark.parametrize("mode", ["tiles", "quad", "pipe", "tiles_rt", "generic"])
@pytest.mark.parametrize("D", [7, 8, 9, 16, 20])
def test_simple_reacher_rollout_equals_the_oracle(D, mode, mpk_option):
    """k_pd_rollout_tiles (one / four groups per wave, link count compiled in where there is an instantiation / at run time),
    k_pd_rollout_pipe and the lane-per-(episode, link) kernel, which adds across lanes in tree order and keeps 1e-12 throughout.
    The tile kernels take at most 16 DoF (kMaxD): with 20 links every mode is the lane-per-(episode, link) kernel and its bound"""
    B, T = 67, 12
    if mode == "pipe":
        mpk_option("pd_pipe", 1)
    else:
        mpk_option("pd_quad", "2" if mode == "quad" else "0")
    if mode == "generic":
        mpk_option("pd_simple", "1")
    if mode == "tiles_rt":
        mpk_option("pd_generic", "1")
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=3, dt=0.01,
                           duration=T * 0.01, tau=T * 0.01)
    rng = np.random.default_rng(100 + D)
    des_pos = rng.standard_normal((B, T, D)).astype(np.float32)
    des_vel = rng.standard_normal((B, T, D)).astype(np.float32)
    goal = rng.uniform(-D, D, (B, 2))
    n_steps = np.where(rng.uniform(size=B) < 0.5, T, rng.integers(0, T + 1, B)).astype(np.int32)
    step0 = (182 + np.arange(B) % 19).astype(np.int32)          # 182 .. 200: step 199 first, last, inside and behind the plans
    q0, qd0 = rng.uniform(-1, 1, (B, D)), rng.uniform(-1, 1, (B, D))
    pg, dg = rng.uniform(0.1, 1.0, D), rng.uniform(0.01, 0.1, D)
    spec = RolloutSpec("motor", D, pg, dg, -2.0, 1.5, plant="double_integrator", dt=0.01)
    q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    act, rew = eng.reacher_rollout(spec, torch.tensor(des_pos, device="cuda"), torch.tensor(des_vel, device="cuda"), q, qd,
                                   torch.tensor(goal), n_steps=torch.tensor(n_steps), step0=torch.tensor(step0))
    ra, rr, rq, rqd = O.reacher_rollout(des_pos, des_vel, "motor", pg, dg, -2.0, 1.5, 0.01, q0, qd0, goal, n_steps=n_steps, step0=step0)
    assert np.array_equal(cpu(act), ra.astype(np.float32))
    assert np.array_equal(cpu(q), rq) and np.array_equal(cpu(qd), rqd)
    t = np.arange(T)[None]
    executed = t < n_steps[:, None]
    paid = step0[:, None] + t >= 199
    assert (paid & executed).any() and (~paid & executed).any()
    tag = f"reacher_rollout {mode} D {D}"
    if mode == "generic" or D > 16:
        np.testing.assert_allclose(cpu(rew)[executed], rr[executed], rtol=1e-12, atol=0, err_msg=tag)
        assert not cpu(rew)[~executed].any()
    else:
        check_rewards(tag, cpu(rew), rr, executed, paid)


def test_episode_return_at_nine_links_equals_the_separate_launches():
    D, T, B = 9, 200, 131
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="zero_rbf", num_dof=D, num_basis=5,
                           num_basis_zero_start=1, dt=0.01, duration=2.0, tau=2.0)
    rng = np.random.default_rng(9)
    params = (rng.standard_normal((B, eng.num_params)) * 0.4).astype(np.float32)
    ip, iv = rng.uniform(-1, 1, (B, D)).astype(np.float32), np.zeros((B, D), np.float32)
    q0, goal = rng.uniform(-1, 1, (B, D)), rng.uniform(-3, 3, (B, 2))
    n_steps = torch.tensor(rng.integers(0, T + 1, B).astype(np.int32))
    step0 = torch.tensor(rng.integers(0, 260, B).astype(np.int32))
    spec = RolloutSpec("motor", D, 0.6, 0.075, -2.0, 1.5, plant="double_integrator", dt=0.01)
    for agg in ("sum", "mean", "last"):
        q, qd = torch.tensor(q0, device="cuda"), torch.zeros((B, D), dtype=torch.float64, device="cuda")
        r = eng.episode_return(params, ip, iv, spec, q, qd, n_steps=n_steps, reward="simple_reacher", goal=torch.tensor(goal),
                               step0=step0, steps_before_reward=199, aggregation=agg)
        assert eng.last_kernel() == "k_episode_return<promp,reacher>"
        q2, qd2 = torch.tensor(q0, device="cuda"), torch.zeros((B, D), dtype=torch.float64, device="cuda")
        pos, vel = eng.trajectory(params, ip, iv, 0.0)
        _, rew = eng.reacher_rollout(spec, pos, vel, q2, qd2, torch.tensor(goal), n_steps=n_steps, step0=step0, want_actions=False)
        want = eng.reward_aggregate(rew, n_steps, agg)
        assert torch.equal(r["ret"], want), (agg, float((r["ret"] - want).abs().max()))
        assert torch.equal(q, q2) and torch.equal(qd, qd2)
    # ... and the separate launch is the oracle's: rewards without a distance term bit for bit
    _, rr, _, _ = O.reacher_rollout(cpu(pos), cpu(vel), "motor", 0.6, 0.075, -2.0, 1.5, 0.01, q0, np.zeros((B, D)), goal,
                                    n_steps=n_steps.numpy(), step0=step0.numpy())
    t = np.arange(T)[None]
    check_rewards("reacher_rollout behind k_episode_return D 9", cpu(rew), rr, t < n_steps.numpy()[:, None],
                  step0.numpy()[:, None] + t >= 199)
