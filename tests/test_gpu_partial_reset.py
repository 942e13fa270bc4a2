"""Per-episode autoreset on the device (mpk_reacher_autoreset; BatchedBlackBox.reset(mask=...) / reset_done(); BatchedVectorEnv(...,
partial_resets=True)): the replanning vector env against host wrappers that are reset one by one, rows a masked reset must not touch,
the one launch against the three it replaces, the mode without replanning against the default mode, captured steps against eager ones,
and the refused calls.

Comparison rules, as the suites these tests build on state them: an observation against a HOST env through assert_rows of
tests/test_gpu_reacher_obs.py (float32 of the host's float64 row bit for bit, one float32 ulp only at a rounding midpoint), returns
against host envs within 1e-10 * (1 + |return|) (tests/test_gpu_hole_reacher.py, tests/test_gpu_batched_make.py), device against
device with torch.equal."""
import numpy as np
import pytest
import torch

from fancy_gym_amd import BatchedVectorEnv, _gym, make_batched, make_batched_vec

from .reacher_reset_ref import Episode
from .test_gpu_batched_make import IDS, is_hole, np_, params_for
from .test_gpu_reacher_obs import assert_rows

pytestmark = pytest.mark.gpu

HORIZON = 200           # the TimeLimit of every registered reacher id
# per-family factors on the plans: DMP weights are forcing terms (0.05, test_gpu_batched_make.params_for); ProDMP weights of the scale
# below collide nowhere within 200 steps (host wrappers alone: at factors 1, 3 and 8 every env of the every = 25 batch ran to the step
# limit in lockstep), 20 gives the mixed batch the comparison needs -- host_conditions asserts it on the host side
FAMILY_SCALE = {"fancy_ProMP": 1.0, "fancy_DMP": 0.05, "fancy_ProDMP": 20.0}


def plan_params(fid, n_params, B, k):
    """the plans of vector step k: from gentle to wild over the batch, scaled as
    test_replanning_steps_do_not_end_the_episode_and_reset_all_together scales them (np.geomspace(0.01, 1.0, B): a HoleReacher batch then
    holds episodes that collide in their first plans and episodes that reach the step limit), times the per-family factors of
    FAMILY_SCALE and, for SimpleReacher, torques of some size (50, test_gpu_batched_make.params_for)"""
    rng = np.random.default_rng(1000 + k)
    scale = np.geomspace(0.01, 1.0, B)[:, None] * FAMILY_SCALE[fid.split("/")[0]] * (1.0 if is_hole(fid) else 50.0)
    return (rng.standard_normal((B, n_params)) * scale).astype(np.float32)


def host_override(every):
    return {"black_box_kwargs": {"replanning_schedule": lambda pos, vel, obs, action, t: t % every == 0}}


def host_run(fid, B, every, seed, n_steps):
    """B host wrappers over n_steps plans, each env reset on its own (``e.reset()``: its stream continues) right after the step that
    terminated or truncated it.  Returns (reset observations [B, n], per-step records, the envs' step counters at the end); a record
    holds, per env, what BatchedVectorEnv.step returns for it."""
    envs = [_gym.make(fid, mp_config_override=host_override(every)) for _ in range(B)]
    n_params = envs[0].action_space.shape[0]
    first = np.stack([e.reset(seed=seed + b)[0] for b, e in enumerate(envs)]).astype(np.float64)
    episodes = None
    if not is_hole(fid):
        # the host SimpleReacherEnv departs from the reference on unseeded resets (DESIGN, "Known and not fixed here"): its continued
        # episodes come from the NumPy restatement of the reference's reset and are put into the host env
        episodes = [Episode(0, envs[0].unwrapped.n_links) for _ in range(B)]
        for b, ep in enumerate(episodes):
            q0, task = ep.reset(seed + b)
            assert np.array_equal(q0, envs[b].unwrapped.q) and np.array_equal(task[:2], envs[b].unwrapped.goal)
    records = []
    for k in range(n_steps):
        params = plan_params(fid, n_params, B, k)
        rec = dict(params=params, obs=[], final_obs=[], ret=[], terminated=[], truncated=[], length=[], collided=[], success=[])
        for b, e in enumerate(envs):
            o, ret, term, trunc, info = e.step(params[b])
            rec["ret"].append(ret), rec["terminated"].append(bool(term)), rec["truncated"].append(bool(trunc))
            rec["length"].append(info["trajectory_length"])
            if is_hole(fid):
                rec["collided"].append(bool(info["is_collided"][-1])), rec["success"].append(bool(info["is_success"][-1]))
            rec["final_obs"].append(np.asarray(o, np.float64))
            if term or trunc:
                o, _ = e.reset()
                if episodes is not None:
                    raw = e.unwrapped
                    q0, task = episodes[b].reset()
                    raw.q, raw._start_pos, raw.goal = q0.copy(), q0.copy(), task[:2].copy()
                    o = e.observation(np.append(raw._observe(), 0.0))          # TimeAwareObservation at t = 0
            rec["obs"].append(np.asarray(o, np.float64))
        rec["reset"] = np.array(rec["terminated"]) | np.array(rec["truncated"])
        records.append(rec)
    counters = np.array([e.current_traj_steps for e in envs])
    return first, records, counters


def host_conditions(fid, records, counters):
    """what the HOST wrappers alone must show for the comparison to mean something (asserted before the device is looked at)"""
    resets = np.stack([r["reset"] for r in records])            # [steps, B]
    assert (resets.sum(0) >= 2).all(), ("every env passes through at least two resets", resets.sum(0))
    if is_hole(fid):
        # (SimpleReacher has no early termination: its episodes all end at the step limit, together)
        assert any(0 < r.sum() < r.size for r in resets), "no step in which some envs are reset and some run on"
        assert len(set(counters.tolist())) > 1, ("the batch never left lockstep", counters)
    return resets


CASES = [(f"fancy_{mp}/HoleReacher-v0", every) for mp in ("ProMP", "DMP", "ProDMP") for every in (50, 25)] + \
        [("fancy_ProMP/SimpleReacher-v0", 50)]


@pytest.mark.parametrize("fid,every", CASES)
def test_vector_env_equals_host_wrappers_that_reset_one_by_one(fid, every):
    """B host wrappers, each reset on its own, against make_batched_vec(..., replanning_every=every, partial_resets=True): per step and
    env trajectory_length, flags, return, is_collided / is_success, _final_obs, final_obs where set, obs; at the end the counters.

    The host wrapper's plans are shared-phase plans (B = 1, one init_time).  Out of lockstep the batch plans ProMP with the
    per-episode-phase kernels, which give the same bits, and DMP / ProDMP once per clock value with the shared-phase kernels
    (BatchedBlackBox._trajectory): their per-episode-phase kernels are ~1e-6 of the scale away from the shared route, which showed here
    as observations one float32 ulp off the host's from the first step on."""
    B, seed = 16, 700
    n_steps = 3 * HORIZON // every + 2
    first, records, counters = host_run(fid, B, every, seed, n_steps)
    host_conditions(fid, records, counters)
    vec = make_batched_vec(fid, B, partial_resets=True, mp_config_override={"black_box_kwargs": {"replanning_every": every}})
    obs, info = vec.reset(seed=seed)
    assert info == {}
    assert_rows(np_(obs), first, (fid, every, "reset"))
    for k, rec in enumerate(records):
        obs, rewards, terminated, truncated, info = vec.step(rec["params"])
        assert rewards.dtype == torch.float64 and terminated.dtype == torch.bool and truncated.dtype == torch.bool
        assert info["_final_obs"].dtype == torch.bool and tuple(info["_final_obs"].shape) == (B,)
        assert tuple(info["final_obs"].shape) == tuple(obs.shape) and obs.dtype == torch.float32
        obs, rewards, terminated, truncated = np_(obs), np_(rewards), np_(terminated), np_(truncated)
        final, was_reset, length = np_(info["final_obs"]), np_(info["_final_obs"]), np_(info["trajectory_length"])
        for b in range(B):
            tag = (fid, every, k, b)
            print(tag, "length", length[b], rec["length"][b], "return", rewards[b], rec["ret"][b], "flags", terminated[b], truncated[b],
                  "reset", was_reset[b])
            assert length[b] == rec["length"][b], tag
            assert bool(terminated[b]) == rec["terminated"][b] and bool(truncated[b]) == rec["truncated"][b], tag
            assert abs(rewards[b] - rec["ret"][b]) <= 1e-10 * (1 + abs(rec["ret"][b])), (tag, rewards[b], rec["ret"][b])
            if is_hole(fid):
                assert bool(info["is_collided"][b]) == rec["collided"][b] and bool(info["is_success"][b]) == rec["success"][b], tag
            assert bool(was_reset[b]) == bool(rec["reset"][b]), tag
            if rec["reset"][b]:
                assert_rows(final[b:b + 1], rec["final_obs"][b][None], tag + ("final_obs",))
            assert_rows(obs[b:b + 1], rec["obs"][b][None], tag + ("obs",))
    assert np.array_equal(np_(vec.bb.traj_steps), counters)


# ---- rows a masked reset must not touch ----------------------------------------------------------------------------------------------
STATE = ("q", "qd", "traj_steps", "plan_steps", "done", "_task_buf", "_rng")


def mid_episode(fid, B, seed=5, **black_box):
    """a replanning batch after two plans: some HoleReacher rows collided (done), the others are in mid-episode"""
    black_box = {"replanning_every": 50, **black_box}
    bb = make_batched(fid, B, mp_config_override={"black_box_kwargs": black_box})
    bb.reset(seed=seed)
    env = _gym.make(fid)
    for k in range(2):
        bb.step(plan_params(fid, env.action_space.shape[0], B, k))
    return bb


def snapshot(bb):
    snap = {k: getattr(bb, k).clone() for k in STATE}
    if bb.condition_pos is not None:
        snap["condition_pos"], snap["condition_vel"] = bb.condition_pos.clone(), bb.condition_vel.clone()
    return snap


@pytest.mark.parametrize("B", [1, 7, 1000, 65537])
@pytest.mark.parametrize("fid,cond", [("fancy_ProMP/HoleReacher-v0", False), ("fancy_ProMP/HoleReacher-v0", True),
                                      ("fancy_DMP/SimpleReacher-v0", False)])
def test_masked_reset_leaves_the_other_rows_alone(fid, cond, B):
    black_box = {"condition_on_desired": True} if cond else {}
    gen = torch.Generator().manual_seed(B)
    masks = {"none": torch.zeros(B, dtype=torch.bool), "all": torch.ones(B, dtype=torch.bool), "random": torch.rand(B, generator=gen) < 0.4}
    for name, m in masks.items():
        bb, whole = mid_episode(fid, B, **black_box), mid_episode(fid, B, **black_box)
        before = snapshot(bb)
        assert cond == ("condition_pos" in before)
        for k in before:                                        # the two batches are the same batch
            assert torch.equal(before[k], snapshot(whole)[k]), (name, k)
        if is_hole(fid) and B >= 1000:
            assert bool(bb.done.any()) and not bool(bb.done.all())
        bb.reset(sample=True, mask=m.cuda() if name == "random" else (m.numpy() if name == "all" else m.to(torch.uint8)))
        whole.reset(sample=True)
        after = snapshot(bb)
        m = m.cuda()
        for k in STATE:
            assert torch.equal(after[k][~m], before[k][~m]), (name, k, "outside the mask")
            assert torch.equal(after[k][m], getattr(whole, k)[m]), (name, k, "inside the mask")
        if cond:
            # rows outside keep the desired state they condition on; rows inside hold the fp32 image of their start state
            for key, x in (("condition_pos", bb.q), ("condition_vel", bb.qd)):
                assert torch.equal(after[key][~m], before[key][~m]), (name, key)
                assert torch.equal(after[key][m], x.float()[m]), (name, key)
        assert bb._lockstep is None and torch.equal(bb.observe()[m], whole.observe()[m])
    # reset_done() is the mask = done form
    a, b = mid_episode(fid, B), mid_episode(fid, B)
    done = a.done.bool().clone()
    a.reset_done()
    b.reset(sample=True, mask=done)
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not bool(a.done.any())


@pytest.mark.parametrize("B", [7, 1000])
def test_masked_seeded_reset_seeds_the_selected_rows(B):
    fid = "fancy_ProDMP/HoleReacher-v0"
    bb, whole = mid_episode(fid, B), mid_episode(fid, B)
    before = snapshot(bb)
    m = (torch.arange(B) % 3 == 1).cuda()
    bb.reset(seed=900, mask=m)
    whole.reset(seed=900)
    for k in STATE:
        assert torch.equal(getattr(bb, k)[~m], before[k][~m]) and torch.equal(getattr(bb, k)[m], getattr(whole, k)[m]), k


# ---- the one launch against the three it replaces ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [7, 1000, 65537])
@pytest.mark.parametrize("every", [None, 50])
@pytest.mark.parametrize("fid", ["fancy_ProMP/HoleReacher-v0", "fancy_ProDMP/SimpleReacher-v0", "fancy_DMP/LongSimpleReacher-v0"])
def test_autoreset_equals_observe_masked_reset_observe(fid, every, B):
    """context rows (no replanning: every row is done) and time-aware rows (replanning: the rows that ended)"""
    override = {"black_box_kwargs": {"replanning_every": every}} if every else None
    fused, three = (make_batched(fid, B, mp_config_override=override) for _ in range(2))
    n_params = _gym.make(fid).action_space.shape[0]
    for bb in (fused, three):
        bb.reset(seed=77)
    for k in range(3 if every is None else 5):
        params = plan_params(fid, n_params, B, k)
        for bb in (fused, three):
            bb._step(params, True)
        done = three.done.bool().clone()
        if every and is_hole(fid) and B >= 1000:
            assert bool(done.any()) and not bool(done.all()), k
        final, obs, reset_mask = fused.autoreset()
        want_final = three.observe()
        three.reset(sample=True, mask=done)
        want_obs = three.observe()
        assert torch.equal(final, want_final) and torch.equal(obs, want_obs) and torch.equal(reset_mask, done), k
        assert final.data_ptr() != obs.data_ptr()
        for name in STATE:
            assert torch.equal(getattr(fused, name), getattr(three, name)), (k, name)
        assert torch.equal(obs[~done], final[~done])


# ---- without replanning: the default mode's results ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", IDS)
def test_without_replanning_the_mode_returns_what_the_default_mode_returns(fid):
    B = 24
    env = _gym.make(fid)
    default, partial = make_batched_vec(fid, B, verbose=2), make_batched_vec(fid, B, verbose=2, partial_resets=True)
    assert not default.partial_resets and partial.partial_resets
    o0, _ = default.reset(seed=3)
    o1, _ = partial.reset(seed=3)
    assert torch.equal(o0, o1)
    for k in range(3):
        params = params_for(fid, env, B, 20 + k)
        want, got = default.step(params), partial.step(params)
        for g, w, name in zip(got[:4], want[:4], ("obs", "rewards", "terminated", "truncated")):
            assert torch.equal(g, w), (k, name)
        assert set(got[4]) == set(want[4]) | {"_final_obs"}
        for key in want[4]:
            assert torch.equal(got[4][key], want[4][key]), (k, key)
        assert got[4]["_final_obs"].dtype == torch.bool and bool(got[4]["_final_obs"].all())
        assert torch.equal(partial.bb._rng, default.bb._rng), k


# ---- captured against eager -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid,cond", [("fancy_ProMP/HoleReacher-v0", False), ("fancy_ProDMP/HoleReacher-v0", True),
                                      ("fancy_DMP/SimpleReacher-v0", False)])
def test_captured_replanning_steps_equal_eager_steps(fid, cond):
    B, seed, every = 1000, 31, 50
    black_box = {"replanning_every": every, **({"condition_on_desired": True} if cond else {})}
    n_params = _gym.make(fid).action_space.shape[0]
    eager, graphed = (make_batched_vec(fid, B, partial_resets=True, mp_config_override={"black_box_kwargs": black_box}) for _ in range(2))
    eager.reset(seed=seed)
    first, _ = graphed.reset(seed=seed)
    graph = graphed.capture()
    assert torch.equal(graphed.bb.observe(), first)             # capturing left the episodes where they were
    n_steps = 2 * HORIZON // every                              # two whole episodes of the slowest env
    resets = torch.zeros(B, dtype=torch.int64, device="cuda")
    for k in range(n_steps):
        params = torch.as_tensor(plan_params(fid, n_params, B, k), device="cuda")
        want = eager.step(params)
        graph.actions.copy_(params)
        got = graph.replay()
        torch.cuda.synchronize()
        for g, w, name in zip(got[:4], want[:4], ("obs", "rewards", "terminated", "truncated")):
            assert torch.equal(g, w), (k, name)
        assert got[4].keys() == want[4].keys()
        for key in want[4]:
            assert torch.equal(got[4][key], want[4][key]), (k, key)
        for name in STATE:
            assert torch.equal(getattr(graphed.bb, name), getattr(eager.bb, name)), (k, name)
        resets += want[4]["_final_obs"]
    assert int(resets.min()) >= 2
    if is_hole(fid):
        assert len(torch.unique(eager.bb.traj_steps)) > 1       # the batch left lockstep
    # eager steps go on from a replay
    params = plan_params(fid, n_params, B, 99)
    want, got = eager.step(params), graphed.step(params)
    for g, w in zip(got[:4], want[:4]):
        assert torch.equal(g, w)
    assert torch.equal(got[4]["final_obs"], want[4]["final_obs"]) and torch.equal(graphed.bb._rng, eager.bb._rng)


# ---- refused calls -------------------------------------------------------------------------------------------------------------------
def test_refused_calls_name_the_offender():
    fid = "fancy_ProMP/HoleReacher-v0"
    replanning = {"black_box_kwargs": {"replanning_every": 50}}
    with pytest.raises(ValueError, match="partial resets"):
        make_batched_vec(fid, 4, partial_resets=True, mp_config_override={"black_box_kwargs": {"learn_sub_trajectories": True}})
    with pytest.raises(ValueError, match="observations"):
        BatchedVectorEnv(make_batched(fid, 4, observations=False), partial_resets=True)
    with pytest.raises(ValueError, match="learned tau"):
        make_batched_vec(fid, 4, partial_resets=True, mp_config_override={"phase_generator_kwargs": {"learn_tau": True}})
    vec = make_batched_vec(fid, 4, partial_resets=True, mp_config_override=replanning)
    with pytest.raises(ValueError, match="seed"):
        vec.capture()
    with pytest.raises(ValueError, match="reset"):
        vec.step(np.zeros((4, vec.single_action_space.shape[0]), np.float32))
    with pytest.raises(ValueError, match="options"):
        vec.reset(seed=0, options={"random_start": False})
    # the default mode still refuses to capture a replanning step
    default = make_batched_vec(fid, 4, mp_config_override=replanning)
    default.reset(seed=0)
    with pytest.raises(ValueError, match="replanning"):
        default.capture()
    bb = make_batched(fid, 4, mp_config_override=replanning)
    with pytest.raises(ValueError, match="reset\\(seed"):
        bb.reset_done()
    with pytest.raises(ValueError, match="reset\\(seed"):
        bb.reset(sample=True, mask=np.ones(4, bool))
    bb.reset(seed=1)
    hole = bb.hole.clone()
    with pytest.raises(ValueError, match="mask"):
        bb.reset(mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="init_pos / goal / hole"):
        bb.reset(hole=hole, sample=True, mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="mask.*init_pos"):
        bb.reset(hole=hole, mask=np.ones(4, bool))
    with pytest.raises(ValueError, match=r"mask must be \[4\]"):
        bb.reset(sample=True, mask=np.ones(5, bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        bb.reset(sample=True, mask=np.ones(4, np.float32))
    bb.reset(hole=hole)
    with pytest.raises(ValueError, match="drawn on the device"):
        bb.reset_done()
    with pytest.raises(ValueError, match="observations"):
        make_batched(fid, 4, observations=False).autoreset()
    # the C entry point: observation buffers and their layout go together
    bb.reset(seed=1)
    eng = bb.engine
    with pytest.raises(AssertionError):
        eng.reacher_autoreset("hole_reacher", bb.q, bb.qd, bb.traj_steps, bb.plan_steps, bb.done, bb._rng, bb._task_buf,
                              mask=torch.ones(3, dtype=torch.uint8, device="cuda"))
