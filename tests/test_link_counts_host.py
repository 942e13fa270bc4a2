"""The link-count fixture (tests/golden/ref_reacher_links.npz) without a GPU: it holds what tests/test_gpu_link_counts.py needs (every
link count, every collision kind a link count allows, both verdicts, margins), it CAN tell numpy's order of additions from the order
of the indices (from 8 links on some stored reward is not the left-to-right sum), the oracle's statement of numpy's order is np.sum's
bit for bit, and the NumPy host envs reproduce the step traces at these link counts"""
import json
import os

import numpy as np
import pytest

from oracle import mp_oracle as O

from .test_step_env_host import _host_env, _load_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "ref_reacher_links.npz")
GOLD = np.load(PATH)
TRACES = json.loads(str(GOLD["traces"]))
REW_FCTS = ("simple", "vel_acc", "unbounded")
LINKS = (1, 3, 7, 8, 9, 15, 16)
HOLE_LINKS = LINKS[1:]          # the reference's HoleReacher cannot step with one link (make_ref_link_count_golden.py: HOLE_LINKS)
F32 = np.float32


def plan(k):
    return GOLD["plan__" + k]


def in_order(x):
    """the sum of every row of x [B, n] in the order of the indices, every addition rounded to x's dtype"""
    s = x[:, 0].copy()
    for d in range(1, x.shape[1]):
        s = s + x[:, d]
    return s


def test_fixture_covers_what_it_must():
    assert tuple(GOLD["rew_fct"]) == REW_FCTS
    assert sorted(set(plan("D").tolist())) == list(HOLE_LINKS)
    for D in HOLE_LINKS:
        for ctrl in (0, 1):
            m = (plan("D") == D) & (plan("ctrl") == ctrl)
            assert 10 <= m.sum() <= 14, (D, ctrl, int(m.sum()))                   # about a dozen
            assert set(plan("kind")[m].tolist()) == {0, 1, 2, 3}, (D, ctrl)       # survivors, joint limit, links crossing, wall
            for T, step0 in ((12, 0), (25, 176)):
                h = m & (plan("T") == T)
                assert (plan("step0")[h] == step0).all() and plan("collided")[h].any() and (~plan("collided")[h]).any(), (D, ctrl, T)
                assert (plan("n_exec")[h & ~plan("collided")] == min(T, 200 - step0)).all()
            assert (plan("kind")[m] != 0).tolist() == plan("collided")[m].tolist()
    assert plan("margin").min() >= 1e-9
    # is_success, stored per reward function: "unbounded" says yes to every plan that passes step 199 without a collision and no to
    # the others; "simple" and "vel_acc" want the end effector within 5 mm of the hole's bottom, which none of these plans reaches (the
    # five-link traces of ref_step_envs.npz hold those)
    assert plan("success").shape == (3, len(plan("D")))
    assert plan("success")[2].any() and not plan("success")[2].all() and not plan("success")[:2].any()
    names = {t["name"]: t for t in TRACES}
    for D in LINKS:
        S = 205 if D in (8, 9, 16) else 40
        tr = names[f"simple{D}"]
        assert tr["S"] == S and tr["n_links"] == D and 2 <= tr["N"] <= 3
        assert GOLD[f"simple{D}__actions"].dtype == F32 and GOLD[f"simple{D}__truncated"].any() == (S > 200)
        a = GOLD[f"simple{D}__actions"].astype(np.float64) * 256
        assert np.array_equal(a, np.round(a))                                    # the 2^-8 grid
        if D not in HOLE_LINKS:
            assert f"hole{D}" not in names
            continue
        tr = names[f"hole{D}"]
        g = lambda k: GOLD[f"hole{D}__{k}"]      # noqa: E731
        assert tr["S"] == S and 2 <= tr["N"] <= 3 and g("reward").shape == (3, S, tr["N"])
        assert g("margin").min() >= 1e-9 and g("is_collided").any()
        a = g("actions").astype(np.float64) * 256
        assert np.array_equal(a, np.round(a))
        if S > 200:                      # a row that lives to the step limit: truncated, paid at step 199
            assert (g("truncated") & ~g("is_collided")).any()
    for kind in (0, 1):
        for D in LINKS:
            assert ((GOLD["reset__kind"] == kind) & (GOLD["reset__n_links"] == D)).sum() >= 4
            assert ((GOLD["obs__kind"] == kind) & (GOLD["obs__n_links"] == D)).sum() >= 4
    meta = json.loads(str(GOLD["meta"]))
    assert "hole_reacher/hole_reacher.py" in meta["reference_files"] and len(meta["generator"]) == 64
    assert os.path.getsize(PATH) <= 942075          # no larger than the largest fixture before it (ref_step_envs.npz)


def plan_acc_cost(e, order):
    """sum(acc ** 2) of plan e's steps 1 .. n_exec - 1 under the velocity controller, in float32 as base_reacher_direct.py:25 computes
    it from a float32 action and the float32 velocity the step before left"""
    D, n = int(plan("D")[e]), int(plan("n_exec")[e])
    a = plan("actions")[e, :n, :D]
    acc = (a[1:] - a[:-1]) / F32(0.01)
    assert acc.dtype == F32
    return order(acc * acc)


@pytest.mark.parametrize("D", HOLE_LINKS)
def test_stored_rewards_follow_numpys_order_and_from_8_links_on_not_the_index_order(D):
    # (a) the simple reward of the velocity controller's steps without a distance term: acc_cost * -5e-8 (hr_simple_reward.py)
    n_rows = n_differ = 0
    for e in np.flatnonzero((plan("D") == D) & (plan("ctrl") == 1)):
        n = int(plan("n_exec")[e])
        t = np.arange(1, n)
        plain = (plan("step0")[e] + t != 199) & ~(plan("collided")[e] & (t == n - 1))
        want = plan("rewards")[0, e, 1:n][plain]
        got = plan_acc_cost(e, O.np_sum_rows).astype(np.float64)[plain] * -5e-8
        assert np.array_equal(got, want), e
        n_rows += int(plain.sum())
        n_differ += int((plan_acc_cost(e, in_order).astype(np.float64)[plain] * -5e-8 != want).sum())
    assert n_rows >= 40
    assert (n_differ > 0) == (D >= 8), (D, n_differ, n_rows)
    # (b) SimpleReacher's steps without a distance term: 0 - (action ** 2).sum() in float32 (simple_reacher.py:68)
    g = lambda k: GOLD[f"simple{D}__{k}"]      # noqa: E731
    a = g("actions").reshape(-1, D)
    plain = ~g("truncated").reshape(-1)
    want = g("reward").reshape(-1)[plain]
    assert np.array_equal(0.0 - O.np_sum_rows(a * a).astype(np.float64)[plain], want)
    assert ((0.0 - in_order(a * a).astype(np.float64)[plain] != want).any()) == (D >= 8)
    # (c) HoleReacher's steps without a distance term under the simple reward, from an episode's second step on (the action of the
    # step before is the float32 velocity): acc_cost * -5e-8 again
    g = lambda k: GOLD[f"hole{D}__{k}"]      # noqa: E731
    a, ended = g("actions"), g("truncated") | g("is_collided")
    acc = ((a[1:] - a[:-1]) / F32(0.01)).reshape(-1, D)
    plain = (~ended[1:] & ~ended[:-1]).reshape(-1)
    want = g("reward")[0, 1:].reshape(-1)[plain]
    assert plain.sum() >= 70
    assert np.array_equal(O.np_sum_rows(acc * acc).astype(np.float64)[plain] * -5e-8, want)
    assert ((in_order(acc * acc).astype(np.float64)[plain] * -5e-8 != want).any()) == (D >= 8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_oracles_statement_of_numpys_order_is_np_sum_bit_for_bit(dtype):
    rng = np.random.default_rng(5)
    for n in range(1, 22):
        x = (rng.standard_normal((500, n)) ** 2 * 10.0 ** rng.uniform(-3, 3, (500, n))).astype(dtype)
        got = O.np_sum_rows(x)
        assert got.dtype == dtype
        want = np.array([np.sum(np.ascontiguousarray(row)) for row in x])
        assert np.array_equal(got, want), n
        differ = int((in_order(x) != want).sum())
        assert (differ > 50) == (n >= 8), (n, differ)


HOST_CASES = [(t["name"], f) for t in TRACES for f in (REW_FCTS if t["env"] == "hole_reacher" else (None,))]


@pytest.mark.parametrize("name, rew_fct", HOST_CASES)
def test_host_envs_reproduce_the_traces(name, rew_fct):
    """tests/test_step_env_host.py: test_host_envs_reproduce_the_reference_traces at these link counts"""
    tr = dict(next(t for t in TRACES if t["name"] == name))
    g = lambda k: GOLD[f"{name}__{k}"]      # noqa: E731
    hole = tr["env"] == "hole_reacher"
    if hole:
        tr["kwargs"] = dict(tr["kwargs"], rew_fct=rew_fct)
    rewards = g("reward")[REW_FCTS.index(rew_fct)] if hole else g("reward")
    success = g("is_success")[REW_FCTS.index(rew_fct)] if hole else None
    acts = g("actions")
    for b in range(tr["N"]):
        env = _host_env(tr)
        _load_state(env, hole, g("q0")[b], g("qd0")[b], g("task0")[b], 0)
        np.testing.assert_array_equal(env._observe(), g("obs0")[b])
        elapsed = 0
        for t in range(tr["S"]):
            obs, reward, terminated, truncated, info = env.step(acts[t, b])
            elapsed += 1
            truncated = elapsed >= 200
            np.testing.assert_array_equal(obs, g("final_obs")[t, b], err_msg=f"{name} env {b} step {t}")
            assert terminated == g("terminated")[t, b] and truncated == g("truncated")[t, b], (name, b, t)
            ref = rewards[t, b]
            assert abs(reward - ref) <= 4 * np.finfo(np.float64).eps * max(abs(ref), 1.0), (name, b, t, reward, ref)
            if hole:
                assert info["is_collided"] == g("is_collided")[t, b] and bool(info["is_success"]) == success[t, b]
            if terminated or truncated:
                _load_state(env, hole, g("q")[t, b], g("qd")[t, b], g("task")[t, b], 0)
                elapsed = 0
            else:
                np.testing.assert_array_equal(env.q, g("q")[t, b])
                np.testing.assert_array_equal(np.asarray(env.qd, np.float64), g("qd")[t, b])
                assert env.steps == g("steps")[t, b]
