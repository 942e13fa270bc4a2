"""
GPU suite, part 2: the drop-in surface (BlackBoxWrapper / make_bb on the reference's toy fixture env), the device
rollout kernels against the oracle (bit-exact in float64), the integer replanning state (bit-exact), the batched
validity check, the committed golden fixtures, and size-independent properties at BASELINE's full batch sizes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fancy_gym_amd
from fancy_gym_amd import BatchedBlackBox, RolloutSpec
from fancy_gym_amd.black_box.factory import (get_basis_generator, get_controller, get_phase_generator,
                                             get_trajectory_generator)
from oracle import mp_oracle as O
from tests.golden.make_golden import CONFIGS
from tests.test_gpu_trajectory import CFG2, CFG3, CFG4, CFG5, close, fd_atol, inputs, make_engine
from tests.toy_env import DoubleIntegratorWrapper, ToyWrapper, register_toys

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEED = 1
PG = 0.01 * np.array([120., 120., 120., 120., 50., 30., 10.])
DG = 0.01 * np.array([10., 10., 10., 10., 6., 5., 3.])


@pytest.fixture(scope="module", autouse=True)
def _toys():
    register_toys()


def toy_bb(mp_type, bb=None, phase=None, basis=None, traj=None, env_id="toy-v0", wrapper=ToyWrapper, **kw):
    basis_type = "prodmp" if mp_type == "prodmp" else "rbf"
    phase_type = "exp" if mp_type in ("prodmp", "dmp") else "linear"
    env = fancy_gym_amd.make_bb(env_id, [wrapper], dict(bb or {}),
                                {"trajectory_generator_type": mp_type, **(traj or {})}, {"controller_type": "motor"},
                                {"phase_generator_type": phase_type, **(phase or {})},
                                {"basis_generator_type": basis_type, **(basis or {})}, **kw)
    env.action_space.seed(SEED)      # the reference samples unseeded; fixed here so that failures reproduce
    return env


# ---- golden fixtures through the HIP path ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_hip_path_reproduces_golden(name):
    cfg = CONFIGS[name]
    z = np.load(os.path.join(GOLD, name + ".npz"))
    pc, bc, tc, dt = cfg["pc"], cfg["bc"], cfg["tc"], cfg["dt"]
    eng = make_engine(pc, bc, tc, dt, cfg["duration"])
    fd = tc.trajectory_generator_type == "promp"
    for k, it in enumerate(z["init_times"]):
        pos, vel = eng.trajectory(z["params"], z["init_pos"], z["init_vel"], float(it))
        for ref_p, ref_v in ((z[f"pos32_{k}"], z[f"vel32_{k}"]), (z[f"tpos_{k}"], z[f"tvel_{k}"])):
            close(pos.cpu().numpy(), ref_p, f"{name} pos")
            close(vel.cpu().numpy(), ref_v, f"{name} vel", atol=fd_atol(ref_p, dt) if fd else 0.0)
        if f"idx_{k}" in z.files and not (pc.learn_tau or pc.learn_delay):
            idx, idxb = eng.prodmp_indices(float(it))
            assert np.array_equal(idx, z[f"idx_{k}"][0]) and idxb == int(z[f"idxb_{k}"][0])


# ---- BlackBoxWrapper on the reference's toy fixture ------------------------------------------------------------------
@pytest.mark.parametrize("mp_type", ["promp", "dmp", "prodmp"])
@pytest.mark.parametrize("verbose", [1, 2])
def test_step_contract_and_verbosity(mp_type, verbose):
    """test/test_black_box.py:88-135: info keys, trajectory_length == max_episode_steps"""
    env = toy_bb(mp_type, {"verbose": verbose})
    for _ in range(2):
        env.reset(seed=SEED)
        obs, reward, terminated, truncated, info = env.step(env.action_space.sample())
        assert info["trajectory_length"] == env.spec.max_episode_steps == 50
        assert truncated and not terminated and reward == 50.0
        assert obs.shape == env.observation_space.shape
        assert "toy" in info and len(info["toy"]) == 50
        keys = ["positions", "velocities", "step_actions", "step_observations", "step_rewards"]
        assert all((k in info) == (verbose >= 2) for k in keys)
        if verbose >= 2:
            assert info["positions"].shape == (50, 1) and info["positions"].dtype == np.float32
            assert info["step_actions"].shape == (50, 1)


@pytest.mark.parametrize("mp_type", ["promp", "dmp", "prodmp"])
@pytest.mark.parametrize("agg", [np.sum, np.mean, np.median, lambda x: np.mean(x[::2])])
def test_reward_aggregation(mp_type, agg):
    """test/test_black_box.py:138-150"""
    env = toy_bb(mp_type, {"reward_aggregation": agg})
    env.reset(seed=SEED)
    _, reward, *_ = env.step(env.action_space.sample())
    assert reward == agg(np.ones(50, ))


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("tau", [0.25, 0.5, 0.75, 1])
def test_learn_tau(mp_type, tau):
    """test/test_black_box.py:219-261, exact plateau after tau for the linear phase"""
    env = toy_bb(mp_type, {"verbose": 2}, {"learn_tau": True, "learn_delay": False})
    env.reset(seed=SEED)
    done = True
    for _ in range(3):
        if done:
            env.reset(seed=SEED)
        action = env.action_space.sample()
        action[0] = tau
        _, _, terminated, truncated, info = env.step(action)
        done = terminated or truncated
        assert info["trajectory_length"] == 50
        n = int(np.round(tau / env.dt))
        pos, vel = info["positions"].flatten(), info["velocities"].flatten()
        if mp_type == "promp":
            assert np.all(pos[n:] == pos[-1]) and np.all(vel[n:] == vel[-1])
        assert np.all(pos[:n - 1] != pos[-1]) and np.all(vel[:n - 2] != vel[-1])


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("delay", [0, 0.25, 0.5, 0.75])
def test_learn_delay(mp_type, delay):
    """test/test_black_box.py:266-307, exact plateau before the delay"""
    env = toy_bb(mp_type, {"verbose": 2}, {"learn_tau": False, "learn_delay": True})
    env.reset(seed=SEED)
    action = env.action_space.sample()
    action[0] = delay
    _, _, _, _, info = env.step(action)
    n = int(np.round(delay / env.dt))
    pos, vel = info["positions"].flatten(), info["velocities"].flatten()
    assert np.all(pos[:max(1, n - 1)] == pos[0]) and np.all(vel[:max(1, n - 2)] == vel[0])
    assert np.all(pos[max(1, n):] != pos[0]) and np.all(vel[max(1, n)] != vel[0])


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("tau,delay", [(0.25, 0.25), (0.5, 0.5), (0.25, 0.75), (0.75, 0.25)])
def test_learn_tau_and_delay(mp_type, tau, delay):
    """test/test_black_box.py:312-368: action[0] = tau, action[1] = delay"""
    env = toy_bb(mp_type, {"verbose": 2}, {"learn_tau": True, "learn_delay": True})
    env.reset(seed=SEED)
    action = env.action_space.sample()
    action[0], action[1] = tau, delay
    _, _, _, _, info = env.step(action)
    nt, nd = int(np.round(tau / env.dt)), int(np.round(delay / env.dt))
    pos, vel = info["positions"].flatten(), info["velocities"].flatten()
    if mp_type == "promp":
        assert np.all(pos[nd + nt:] == pos[-1]) and np.all(vel[nd + nt:] == vel[-1])
    assert np.all(pos[:nd - 1] == pos[0]) and np.all(vel[:nd - 2] == vel[0])
    ap, av = pos[nd: nd + nt - 1], vel[nd: nd + nt - 2]
    assert np.all(ap != pos[-1]) and np.all(ap != pos[0]) and np.all(av != vel[-1]) and np.all(av != vel[0])


@pytest.mark.parametrize("mp_type", ["promp", "dmp"])
def test_learn_sub_trajectories(mp_type):
    """test/test_replanning_sequencing.py:64-109: plan length == round(tau / dt)"""
    env = fancy_gym_amd.make_bb("toy-v0", [ToyWrapper], {"learn_sub_trajectories": True, "verbose": 2},
                                {"trajectory_generator_type": mp_type}, {"controller_type": "motor"},
                                {"phase_generator_type": "exp"}, {"basis_generator_type": "rbf"})
    assert env.learn_sub_trajectories and env.traj_gen.learn_tau
    env.reset(seed=SEED)
    done = True
    for _ in range(10):
        if done:
            env.reset(seed=SEED)
        action = env.action_space.sample()
        _, _, terminated, truncated, info = env.step(action)
        done = terminated or truncated
        n = info["trajectory_length"]
        clipped = np.clip(action[0], *env.tau_bound)
        if not done:
            assert n == np.round(clipped / env.dt) == np.round(env.traj_gen.tau.numpy() / env.dt)
        else:
            assert n <= np.round(clipped / env.dt)


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("max_planning_times", [1, 2, 3, 4])
@pytest.mark.parametrize("sub", [5, 10])
def test_max_planning_times(mp_type, max_planning_times, sub):
    """test/test_replanning_sequencing.py:165-194: #step() calls per episode == max_planning_times"""
    env = toy_bb(mp_type, {"max_planning_times": max_planning_times, "verbose": 2,
                           "replanning_schedule": lambda pos, vel, obs, action, t: t % sub == 0})
    env.reset(seed=SEED)
    done, n, lengths = False, 0, []
    while not done:
        _, _, terminated, truncated, info = env.step(env.action_space.sample())
        done = terminated or truncated
        lengths.append(info["trajectory_length"])
        n += 1
    assert n == max_planning_times
    assert lengths == [k for _, k in O.replanning_segments(50, sub, max_planning_times)]


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("delay", [0.1, 0.25, 0.5])
def test_replanning_with_learn_delay(mp_type, delay):
    """test/test_replanning_sequencing.py:231-282: the delay plateau only shows in the first plan"""
    sub, mpt = 10, 3
    env = toy_bb(mp_type, {"max_planning_times": mpt, "verbose": 2,
                           "replanning_schedule": lambda pos, vel, obs, action, t: t % sub == 0},
                 {"learn_tau": False, "learn_delay": True})
    env.reset(seed=SEED)
    done, k = False, 0
    while not done:
        action = env.action_space.sample()
        action[0] = delay
        _, _, terminated, truncated, info = env.step(action)
        done = terminated or truncated
        n = int(np.round(delay / env.dt))
        pos, vel = info["positions"].flatten(), info["velocities"].flatten()
        if k == 0:
            assert np.all(pos[:max(1, n - 1)] == pos[0]) and np.all(vel[:max(1, n - 2)] == vel[0])
        elif n < sub:
            assert np.all(pos[1:max(1, n - 1)] != pos[0])
        assert np.all(pos[max(1, n):] != pos[0])
        k += 1
    assert k == mpt


@pytest.mark.parametrize("mp_type", ["promp", "dmp", "prodmp"])
def test_length(mp_type):
    """test/test_black_box.py:117-135: without replanning one step() simulates max_episode_steps steps"""
    basis = "prodmp" if mp_type == "prodmp" else "rbf"
    env = fancy_gym_amd.make_bb("toy-v0", [ToyWrapper], {}, {"trajectory_generator_type": mp_type},
                                {"controller_type": "motor"}, {"phase_generator_type": "exp"},
                                {"basis_generator_type": basis})
    for _ in range(5):
        env.reset(seed=SEED)
        _, _, _, _, info = env.step(env.action_space.sample())
        assert info["trajectory_length"] == env.spec.max_episode_steps == 50


@pytest.mark.parametrize("mp_type", ["promp", "dmp", "prodmp"])
@pytest.mark.parametrize("replanning_time", [10, 100, 1000])
def test_replanning_time(mp_type, replanning_time):
    """test/test_replanning_sequencing.py:112-160: every plan ends on the schedule, episodes end every
    max_episode_steps // replanning_time plans (TimeAwareObservation is added once, the spaces agree)"""
    def schedule(c_pos, c_vel, obs, c_action, t):
        return t % replanning_time == 0
    env = toy_bb(mp_type, {"replanning_schedule": schedule, "verbose": 2},
                 phase={"phase_generator_type": "exp" if "dmp" in mp_type else "linear"})
    env.reset(seed=SEED)
    assert env.do_replanning and callable(env.replanning_schedule) and env.spec.max_episode_steps == 50
    per_episode = max(50 // replanning_time, 1)
    for i in range(3 * per_episode):
        _, _, terminated, truncated, info = env.step(env.action_space.sample())
        if terminated or truncated:
            assert (i + 1) % per_episode == 0
            env.reset(seed=SEED)
        n = info["trajectory_length"]
        assert n == min(replanning_time, 50) and (schedule(None, None, None, None, n) or n == 50)


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("max_planning_times", [1, 2, 3, 4])
@pytest.mark.parametrize("sub", [5, 10])
@pytest.mark.parametrize("tau", [0.5, 1.0, 1.5, 2.0])
def test_replanning_with_learn_tau(mp_type, max_planning_times, sub, tau):
    """test/test_replanning_sequencing.py:196-228: a learned tau does not change the number of plans per episode"""
    env = toy_bb(mp_type, {"max_planning_times": max_planning_times, "verbose": 2,
                           "replanning_schedule": lambda pos, vel, obs, action, t: t % sub == 0},
                 {"learn_tau": True, "learn_delay": False})
    env.reset(seed=SEED)
    done, n = False, 0
    while not done:
        action = env.action_space.sample()
        action[0] = tau
        _, _, terminated, truncated, _ = env.step(action)
        done = terminated or truncated
        n += 1
    assert n == max_planning_times


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("max_planning_times", [1, 3])
@pytest.mark.parametrize("sub", [5, 10, 15])
@pytest.mark.parametrize("delay", [0, 0.25, 0.5, 0.75])
@pytest.mark.parametrize("tau", [0.5, 0.75, 1.0])
def test_replanning_with_learn_delay_and_tau(mp_type, max_planning_times, sub, delay, tau):
    """test/test_replanning_sequencing.py:284-335: the delay plateau (exact ==) shows in the first plan only, and the
    number of plans per episode stays max_planning_times"""
    env = toy_bb(mp_type, {"max_planning_times": max_planning_times, "verbose": 2,
                           "replanning_schedule": lambda pos, vel, obs, action, t: t % sub == 0},
                 {"learn_tau": True, "learn_delay": True})
    env.reset(seed=SEED)
    done, k = False, 0
    while not done:
        action = env.action_space.sample()
        action[0], action[1] = tau, delay
        _, _, terminated, truncated, info = env.step(action)
        done = terminated or truncated
        n = int(np.round(delay / env.dt))
        pos, vel = info["positions"].flatten(), info["velocities"].flatten()
        if k == 0:
            assert np.all(pos[:max(1, n - 1)] == pos[0]) and np.all(vel[:max(1, n - 2)] == vel[0])
            assert np.all(pos[max(1, n):] != pos[0]) and np.all(vel[max(1, n)] != vel[0])
        k += 1
    assert k == max_planning_times


@pytest.mark.parametrize("mp_type", ["promp", "prodmp"])
@pytest.mark.parametrize("max_planning_times", [1, 2, 3, 4])
@pytest.mark.parametrize("sub", [5, 10])
def test_replanning_schedule(mp_type, max_planning_times, sub):
    """test/test_replanning_sequencing.py:338-364: after max_planning_times plans the episode is over"""
    env = toy_bb(mp_type, {"max_planning_times": max_planning_times, "verbose": 2,
                           "replanning_schedule": lambda pos, vel, obs, action, t: t % sub == 0},
                 {"learn_tau": False, "learn_delay": False})
    env.reset(seed=SEED)
    done = False
    for _ in range(max_planning_times):
        _, _, terminated, truncated, _ = env.step(env.action_space.sample())
        done = terminated or truncated
    assert done


def test_single_episode_step_matches_oracle_on_a_closed_loop_plant():
    """BlackBoxWrapper.step end to end on the double integrator: desired trajectory from the HIP kernels, host PD loop"""
    env = fancy_gym_amd.make_bb("dint-v0", [DoubleIntegratorWrapper], {"verbose": 2},
                                {"trajectory_generator_type": "prodmp"},
                                {"controller_type": "motor", "p_gains": PG, "d_gains": DG},
                                {"phase_generator_type": "exp", "tau": 1.5},
                                {"basis_generator_type": "prodmp", "num_basis": 5, "alpha": 10,
                                 "basis_bandwidth_factor": 2})
    env.reset(seed=3)
    q0, qd0 = env.get_wrapper_attr("current_pos"), env.get_wrapper_attr("current_vel")
    action = env.action_space.sample()
    _, ret, terminated, truncated, info = env.step(action)
    pc, bc, tc, dt, dur = CFG2
    rp, rv = O.get_trajectory(pc, bc, tc, action[None], dur, dt, 0.0, q0[None], qd0[None], dtype=np.float64)
    close(info["positions"][None], rp, "positions")
    close(info["velocities"][None], rv, "velocities")
    # host controller on the device trajectory == oracle rollout on the same trajectory, bit for bit
    ra, rq, rqd = O.rollout(info["positions"][None], info["velocities"][None], "motor", PG, DG, -1.0, 1.0,
                            "double_integrator", dt, q0[None], qd0[None])
    assert np.array_equal(info["step_actions"], ra[0])
    assert np.array_equal(env.get_wrapper_attr("current_pos"), rq[0])
    assert info["trajectory_length"] == 100 and truncated


# ---- device rollout / fused actions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("controller", ["motor", "position", "velocity"])
@pytest.mark.parametrize("plant", ["static", "double_integrator"])
@pytest.mark.parametrize("B", [1, 37, 1000])
@pytest.mark.parametrize("simple", ["tiles", "simple", "quad", "tiles_rt"])
def test_pd_rollout_is_bit_exact_in_float64(controller, plant, B, simple, monkeypatch, mpk_option):
    if simple == "simple":
        mpk_option("pd_simple", "1")      # the generic one-lane-per-(episode, DoF) kernel
    if simple == "tiles_rt":
        mpk_option("pd_generic", "1")     # the tile kernel with the DoF count at run time (7 is compiled in otherwise)
    mpk_option("pd_quad", "2" if simple == "quad" else "0")   # four groups per wave / one
    pc, bc, tc, dt, dur = CFG2
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=11)
    pos, vel = eng.trajectory(params, ip, iv, 0.0)
    rng = np.random.default_rng(B)
    n_steps = rng.integers(0, 101, B).astype(np.int32)
    q0, qd0 = ip.astype(np.float64), iv.astype(np.float64)
    q = torch.tensor(q0, device="cuda"); qd = torch.tensor(qd0, device="cuda")
    spec = RolloutSpec(controller, 7, PG, DG, -1.0, 1.0, plant=plant, dt=dt)
    act = eng.pd_rollout(spec, pos, vel, q, qd, n_steps=torch.tensor(n_steps))
    ra, rq, rqd = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), controller, PG, DG, -1.0, 1.0, plant, dt, q0, qd0,
                            n_steps=n_steps)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
@pytest.mark.parametrize("simple", ["tiles", "simple", "quad"])
def test_device_controllers_equal_the_reference_controllers(cfg, simple, mpk_option):
    """tests/golden/ref_controllers.npz: outputs of the reference's OWN PDController / PosController / VelController
    (fancy_gym/black_box/controller/*.py, loaded unmodified by tests/golden/make_ref_controller_golden.py) on seeded float32
    desired (+) float64 state, clipped as black_box_wrapper.py:178-179 does.  mpk_pd_rollout on the fixture's desired
    trajectories must return those actions bit for bit (float64 arithmetic, one float32 rounding at the store) -- frozen
    state for all three controllers, and the double integrator with the reference's controller in the loop."""
    if simple == "simple":
        mpk_option("pd_simple", "1")
    mpk_option("pd_quad", "2" if simple == "quad" else "0")
    z = np.load(os.path.join(GOLD, "ref_controllers.npz"))
    assert "generated from /root/reference controller/*.py" in str(z["meta"])
    g = lambda n: z[f"{cfg}_{n}"]
    dp, dv, q0, qd0 = g("des_pos"), g("des_vel"), g("q0"), g("qd0")
    B, T, D = dp.shape
    dt = float(g("dt"))
    # any engine of the right DoF count and horizon carries the rollout entry points
    eng = fancy_gym_amd.TrajectoryEngine("promp", "linear", "rbf", D, 4, dt=dt, duration=T * dt, tau=T * dt, device=0)
    assert eng.num_steps == T
    dpos, dvel = torch.tensor(dp, device="cuda"), torch.tensor(dv, device="cuda")
    lo, hi = g("lo").astype(np.float64), g("hi").astype(np.float64)
    for ctrl, key in (("motor", "pd_clip"), ("position", "pos_clip"), ("velocity", "vel_clip")):
        spec = RolloutSpec(ctrl, D, g("p_gains"), g("d_gains"), lo, hi, plant="static")
        q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
        act = eng.pd_rollout(spec, dpos, dvel, q, qd)
        assert np.array_equal(act.cpu().numpy(), g(key).astype(np.float32)), (cfg, ctrl)
        assert np.array_equal(q.cpu().numpy(), q0) and np.array_equal(qd.cpu().numpy(), qd0)
    spec = RolloutSpec("motor", D, g("p_gains"), g("d_gains"), lo, hi, plant="double_integrator", dt=dt)
    q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    act = eng.pd_rollout(spec, dpos, dvel, q, qd)
    assert np.array_equal(act.cpu().numpy(), g("loop_act").astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), g("loop_q")) and np.array_equal(qd.cpu().numpy(), g("loop_qd"))


def test_device_metaworld_controller_equals_the_reference_controller():
    """the reference's MetaWorldController outputs (ref_controllers.npz) against RolloutSpec('metaworld') on the motor kernels"""
    z = np.load(os.path.join(GOLD, "ref_controllers.npz"))
    mi, mo = z["metaworld_in"], z["metaworld_out"]
    n = mi.shape[0]
    eng = fancy_gym_amd.TrajectoryEngine("promp", "linear", "rbf", 4, 4, dt=0.02, duration=0.5, tau=0.5, device=0)
    dp = torch.tensor(mi[:, None, :4].astype(np.float32), device="cuda")       # [n, T = 1, 4]; the inputs are float32-exact
    assert np.array_equal(dp.cpu().numpy()[:, 0].astype(np.float64), mi[:, :4])
    spec = RolloutSpec("metaworld", 4, plant="static")
    q, qd = torch.tensor(mi[:, 4:].copy(), device="cuda"), torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    act = eng.pd_rollout(spec, dp, torch.zeros_like(dp), q, qd)
    assert np.array_equal(act.cpu().numpy()[:, 0], mo.astype(np.float32))


@pytest.mark.parametrize("cfg", [CFG2, CFG5, CFG3], ids=["prodmp", "promp", "dmp_response"])
@pytest.mark.parametrize("controller", ["motor", "position", "velocity"])
@pytest.mark.parametrize("mapping", ["1", "2"])
def test_fused_actions_are_bit_exact(cfg, controller, mapping, monkeypatch):
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 131
    params, ip, iv = inputs(pc, bc, tc, B, seed=5)
    cpos = np.random.default_rng(1).uniform(-1, 1, (B, 7))
    cvel = np.random.default_rng(2).uniform(-1, 1, (B, 7))
    spec = RolloutSpec(controller, 7, PG, DG, -0.8, 0.9, plant="static")
    pos, vel, act = eng.trajectory_actions(params, ip, iv, spec, cpos, cvel, 0.5)
    p2, v2 = eng.trajectory(params, ip, iv, 0.5)
    assert torch.equal(pos, p2) and torch.equal(vel, v2)
    ra, _, _ = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), controller, PG, DG, -0.8, 0.9, "static", dt, cpos, cvel)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))


@pytest.mark.parametrize("cfg", [CFG2, CFG5, CFG4, CFG3], ids=["prodmp", "promp", "prodmp_replan", "dmp_response"])
@pytest.mark.parametrize("controller", ["motor", "position", "velocity"])
@pytest.mark.parametrize("B", [1, 9, 200])
@pytest.mark.parametrize("bulk,quad", [("0", "2"), ("0", "3"), ("0", "4"), ("0", "0"), ("2", "0")])
def test_fused_closed_loop_rollout_is_bit_exact(cfg, controller, B, bulk, quad, monkeypatch, mpk_option):
    """one launch (trajectory + controller + double-integrator plant) == mpk_trajectory + mpk_pd_rollout == oracle;
    k_traj_quad (four recurrences per wave) and both input-staging variants of k_traj_stream"""
    mpk_option("bulk", bulk)
    mpk_option("quad", quad)
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=B)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-1, 1, (B, 7)), rng.uniform(-0.2, 0.2, (B, 7))
    T = eng.num_steps
    n_steps = rng.integers(0, T + 1, B).astype(np.int32)
    spec = RolloutSpec(controller, 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)
    q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    pos, vel, act = eng.trajectory_rollout(params, ip, iv, spec, q, qd, n_steps=torch.tensor(n_steps), init_time=0.5)
    assert eng.last_kernel().endswith("closed>")
    p2, v2 = eng.trajectory(params, ip, iv, 0.5)
    q2, qd2 = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    a2 = eng.pd_rollout(spec, p2, v2, q2, qd2, n_steps=torch.tensor(n_steps))
    assert torch.equal(pos, p2) and torch.equal(vel, v2) and torch.equal(act, a2)
    assert torch.equal(q, q2) and torch.equal(qd, qd2)
    ra, rq, rqd = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), controller, PG, DG, -0.9, 0.9, "double_integrator",
                            dt, q0, qd0, n_steps=n_steps)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)
    # n_steps = NULL executes the whole plan
    q3, qd3 = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    _, _, a3 = eng.trajectory_rollout(params, ip, iv, spec, q3, qd3, init_time=0.5)
    ra, rq, _ = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), controller, PG, DG, -0.9, 0.9, "double_integrator", dt,
                          q0, qd0)
    assert np.array_equal(a3.cpu().numpy(), ra.astype(np.float32)) and np.array_equal(q3.cpu().numpy(), rq)


@pytest.mark.parametrize("cfg", [CFG2, CFG3], ids=["prodmp_closed", "dmp"])
@pytest.mark.parametrize("B", [7, 300, 5000])
def test_serial_kernels_in_every_launch_order_are_bit_identical(cfg, B, mpk_option):
    """option "serial_order": persistent workgroups over XCD-contiguous unit ranges (default), short-lived workgroups in address
    order, persistent without the remap -- for four / two / one groups per wave: the same bits (closed loop and DMP)"""
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    D = tc.action_dim
    params, ip, iv = inputs(pc, bc, tc, B, seed=B)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-1, 1, (B, D)), rng.uniform(-0.2, 0.2, (B, D))
    spec = RolloutSpec("motor", D, PG[:D], DG[:D], -0.9, 0.9, plant="double_integrator", dt=dt)
    closed = tc.trajectory_generator_type != "dmp"

    def run():
        if closed:
            q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
            out = eng.trajectory_rollout(params, ip, iv, spec, q, qd)
            return [x.clone() for x in out] + [q, qd]
        return [x.clone() for x in eng.trajectory(params, ip, iv, 0.0)]
    ref = None
    mpk_option("dmp_response", 0)         # DMP: the serial explicit-Euler kernels (the response route has no serial role)
    for quad in (2, 3, 4):
        for order in (-1, 0, 1, 2):
            mpk_option("quad", quad); mpk_option("serial_order", order)
            got = run()
            assert any(k in eng.last_kernel() for k in ("k_traj_quad", "k_traj_duo", "k_traj_mono")), eng.last_kernel()
            if ref is None:
                ref = got
            for x, y in zip(ref, got):
                assert torch.equal(x, y), (quad, order, eng.last_kernel())


@pytest.mark.parametrize("cfg", [CFG2, CFG5, CFG4], ids=["prodmp", "promp", "prodmp_replan"])
@pytest.mark.parametrize("B", [4104, 6001])
def test_register_lean_pipeline_kernel_is_bit_identical(cfg, B, mpk_option):
    """more than two work units per CU select k_traj_pipe<.., LEAN> (store addresses recomputed per tile: 81 registers): the bits of
    the 100-register instantiation's siblings (k_traj_duo) and of trajectory + rollout as separate kernels; also through
    mpk_replan_step with random integer states"""
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=B)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-1, 1, (B, 7)), rng.uniform(-0.2, 0.2, (B, 7))
    T = eng.num_steps
    n_steps = torch.tensor(rng.integers(0, T + 1, B).astype(np.int32))
    spec = RolloutSpec("motor", 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)

    def run():
        q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
        out = eng.trajectory_rollout(params, ip, iv, spec, q, qd, n_steps=n_steps, init_time=0.25)
        return [x.clone() for x in out] + [q, qd]
    got = run()
    if cfg is not CFG5:                                      # (cfg5's 350-step tables do not fit beside the pipeline's images)
        assert eng.last_kernel().startswith("k_traj_pipe"), eng.last_kernel()
    mpk_option("pipe", 0)
    ref = run()
    assert not eng.last_kernel().startswith("k_traj_pipe")
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    p2, v2 = eng.trajectory(params, ip, iv, 0.25)
    q2, qd2 = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    a2 = eng.pd_rollout(spec, p2, v2, q2, qd2, n_steps=n_steps)
    for x, y in zip(got, [p2, v2, a2, q2, qd2]):
        assert torch.equal(x, y)
    # one replanning step: integer state, plan, rollout, condition gather
    mpk_option("pipe", -1)
    every, mpt, horizon = 25, 3, 2 * T
    ts0 = rng.integers(0, horizon, B).astype(np.int32); ps0 = rng.integers(0, 4, B).astype(np.int32)
    dn0 = (rng.random(B) < 0.2).astype(np.uint8)
    res = []
    for pipe in (-1, 0):
        mpk_option("pipe", pipe)
        st = (torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda"), torch.tensor(ts0, device="cuda"),
              torch.tensor(ps0, device="cuda"), torch.tensor(dn0, device="cuda"))
        r = eng.replan_step(params, ip, iv, spec, *st, every, mpt, horizon, init_time=0.0, condition=True)
        res.append([r[k].clone() for k in ("pos", "vel", "actions", "seg_len", "done", "cond_pos", "cond_vel")] + list(st))
    for x, y in zip(*res):
        assert torch.equal(x, y)


RINGC_OPTS = [dict(), dict(ring_nc=1), dict(ring_nc=2, ring_np=6, ring_ns=1), dict(ring_nc=4, ring_np=2), dict(ring_m=2),
              dict(ring_dbg=4), dict(ring_dbg=16, ring_nc=5, ring_np=1), dict(ring_dbg=32), dict(ring_m=3, ring_nc=2), dict(ring_dbg=8),
              dict(ring_dbg=8 + 4, ring_nc=6, ring_np=5), dict(ring_nc=6, ring_np=2, ring_ns=2)]


@pytest.mark.parametrize("cfg", [CFG2, CFG4], ids=["prodmp", "prodmp_replan"])
@pytest.mark.parametrize("controller", ["motor", "position", "velocity"])
@pytest.mark.parametrize("B", [1, 9, 263, 4104, 20001])
def test_closed_loop_on_the_ring_is_bit_identical(cfg, controller, B, mpk_option):
    """k_traj_ring<.., closed> (producers, store engine for pos / vel, consumer waves running four recurrences per batch) under
    several launch geometries and batch orders == the lane-quarter / pipeline kernels == trajectory + rollout as separate kernels;
    also one replanning step with random integer states and the boundary-condition gather"""
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=B)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-1, 1, (B, 7)), rng.uniform(-0.2, 0.2, (B, 7))
    T = eng.num_steps
    n_steps = torch.tensor(rng.integers(0, T + 1, B).astype(np.int32))
    spec = RolloutSpec(controller, 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)
    keys = ("ring_nc", "ring_np", "ring_ns", "ring_m", "ring_dbg")

    def run(ns):
        q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
        out = eng.trajectory_rollout(params, ip, iv, spec, q, qd, n_steps=ns, init_time=0.25)
        return [x.clone() for x in out] + [q, qd]
    mpk_option("ring", 0)
    ref, ref_full = run(n_steps), run(None)
    assert "k_traj_ring" not in eng.last_kernel()
    p2, v2 = eng.trajectory(params, ip, iv, 0.25)
    q2, qd2 = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    a2 = eng.pd_rollout(spec, p2, v2, q2, qd2, n_steps=n_steps)
    for x, y in zip(ref, [p2, v2, a2, q2, qd2]):
        assert torch.equal(x, y)
    mpk_option("ring", 1)
    for opts in (RINGC_OPTS if controller == "motor" else RINGC_OPTS[:2]):
        for k in keys:
            mpk_option(k, opts.get(k, -1))
        got = run(n_steps)
        assert eng.last_kernel() == "k_traj_ring<prodmp,closed>", eng.last_kernel()
        for i, (x, y) in enumerate(zip(got, ref)):
            assert torch.equal(x, y), (opts, i)
        for i, (x, y) in enumerate(zip(run(None), ref_full)):
            assert torch.equal(x, y), (opts, i, "full horizon")
    for k in keys:
        mpk_option(k, -1)
    # one replanning step: integer state, plan, rollout, condition gather
    every, mpt, horizon = 25, 3, 2 * T
    ts0 = rng.integers(0, horizon, B).astype(np.int32); ps0 = rng.integers(0, 4, B).astype(np.int32)
    dn0 = (rng.random(B) < 0.2).astype(np.uint8)
    res = []
    for ring in (1, 0):
        mpk_option("ring", ring)
        st = (torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda"), torch.tensor(ts0, device="cuda"),
              torch.tensor(ps0, device="cuda"), torch.tensor(dn0, device="cuda"))
        r = eng.replan_step(params, ip, iv, spec, *st, every, mpt, horizon, init_time=0.0, condition=True)
        assert ("k_traj_ring" in eng.last_kernel()) == (ring == 1), eng.last_kernel()
        res.append([r[k].clone() for k in ("pos", "vel", "actions", "seg_len", "done", "cond_pos", "cond_vel")] + list(st))
    for i, (x, y) in enumerate(zip(*res)):
        assert torch.equal(x, y), i


def test_closed_loop_ring_at_the_size_it_is_chosen_for(mpk_option):
    """65 536 episodes (550 MB of outputs: plain stores, the automatic choice): k_traj_ring<.., closed> == k_traj_duo, every output
    and the plant state bit for bit, for a full-horizon step and a replanning step"""
    pc, bc, tc, dt, dur = CFG2
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 65536
    params, ip, iv = inputs(pc, bc, tc, B, seed=11)
    rng = np.random.default_rng(11)
    q0, qd0 = rng.uniform(-1, 1, (B, 7)), rng.uniform(-0.2, 0.2, (B, 7))
    T = eng.num_steps
    spec = RolloutSpec("motor", 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)
    ts0 = rng.integers(0, 2 * T, B).astype(np.int32); ps0 = rng.integers(0, 4, B).astype(np.int32)
    dn0 = (rng.random(B) < 0.2).astype(np.uint8)
    res = {}
    for name, opts in (("ring", {}), ("duo", {"quad": 3})):
        for k in ("quad",):
            mpk_option(k, opts.get(k, -1))
        q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
        out = [x.clone() for x in eng.trajectory_rollout(params, ip, iv, spec, q, qd, init_time=0.25)] + [q, qd]
        assert eng.last_kernel().startswith("k_traj_" + name), eng.last_kernel()
        st = (torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda"), torch.tensor(ts0, device="cuda"),
              torch.tensor(ps0, device="cuda"), torch.tensor(dn0, device="cuda"))
        r = eng.replan_step(params, ip, iv, spec, *st, 25, 3, 2 * T, init_time=0.0, condition=True)
        assert eng.last_kernel().startswith("k_traj_" + name), eng.last_kernel()
        res[name] = out + [r[k].clone() for k in ("pos", "vel", "actions", "seg_len", "done", "cond_pos", "cond_vel")] + list(st)
        del out, r
    for i, (x, y) in enumerate(zip(res["ring"], res["duo"])):
        assert torch.equal(x, y), i
    # ... and the ORACLE directly, on a 256-episode sample of what the ring wrote at the size it is chosen for (round 4 compared it
    # with other kernels only): trajectories to the 1e-5 contract, actions / plant state / integer state exactly
    rows = np.sort(rng.choice(B, 256, replace=False))
    ring = [x[torch.tensor(rows, device=x.device)].cpu().numpy() if x.shape[0] == B else x for x in res["ring"]]
    pos, vel, act, q1, qd1, rpos, rvel, ract, seg, done, cpos, cvel, q2, qd2, ts, ps, dn = ring
    op, ov = O.get_trajectory(pc, bc, tc, params[rows], dur, dt, 0.25, ip[rows], iv[rows], dtype=np.float64)
    close(pos, op, "ring closed pos"); close(vel, ov, "ring closed vel")
    ra, rq, rqd = O.rollout(pos, vel, "motor", PG, DG, -0.9, 0.9, "double_integrator", dt, q0[rows], qd0[rows])
    assert np.array_equal(act, ra.astype(np.float32)) and np.array_equal(q1, rq) and np.array_equal(qd1, rqd)
    # the replanning step: the loop of black_box_wrapper.py:174,197,206 for one episode, from an arbitrary integer state
    want_seg, want_ts, want_ps, want_dn = [], [], [], []
    for b in rows:
        cur, plan, d = int(ts0[b]), int(ps0[b]), int(dn0[b])
        n = 0
        if not d:
            plan += 1
            for t in range(T):
                n = t + 1
                g = t + 1 + cur
                if g >= 2 * T or (g % 25 == 0 and plan < 3):
                    break
            cur += n
            d = int(cur >= 2 * T)
        want_seg.append(n); want_ts.append(cur); want_ps.append(plan); want_dn.append(d)
    assert np.array_equal(seg, want_seg) and np.array_equal(ts, want_ts) and np.array_equal(ps, want_ps) and np.array_equal(dn, want_dn)
    assert np.array_equal(done, want_dn) and 0 < sum(want_dn) < 256 and len(set(want_seg)) > 3
    op, ov = O.get_trajectory(pc, bc, tc, params[rows], dur, dt, 0.0, ip[rows], iv[rows], dtype=np.float64)
    close(rpos, op, "ring replan pos"); close(rvel, ov, "ring replan vel")
    ra, rq, rqd = O.rollout(rpos, rvel, "motor", PG, DG, -0.9, 0.9, "double_integrator", dt, q0[rows], qd0[rows], n_steps=np.array(want_seg))
    assert np.array_equal(ract, ra.astype(np.float32)) and np.array_equal(q2, rq) and np.array_equal(qd2, rqd)
    live = np.array(want_seg) > 0
    last = np.array(want_seg)[live] - 1
    assert np.array_equal(cpos[live], rpos[live, last]) and np.array_equal(cvel[live], rvel[live, last])


def test_closed_loop_ring_declines_shapes_it_does_not_take(mpk_option):
    """cfg5 (350 x 7: T * D = 2 mod 4) stays on the lane-quarter kernels even when the ring is forced"""
    pc, bc, tc, dt, dur = CFG5
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 300
    params, ip, iv = inputs(pc, bc, tc, B, seed=3)
    spec = RolloutSpec("motor", 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)
    q, qd = torch.zeros((B, 7), dtype=torch.float64, device="cuda"), torch.zeros((B, 7), dtype=torch.float64, device="cuda")
    mpk_option("ring", 1)
    eng.trajectory_rollout(params, ip, iv, spec, q, qd)
    assert "k_traj_ring" not in eng.last_kernel() and eng.last_kernel().endswith("closed>")


def test_four_groups_per_wave_while_the_outputs_fit_the_memory_side_cache(mpk_option):
    """the launcher's rule for the serial-recurrence kernels (profiles/r04_closed_loop.md): closed loop at 16 384 / 32 768 and cfg3
    at its BASELINE size on k_traj_quad, smaller launches on k_traj_duo, a few thousand closed-loop episodes on k_traj_pipe, and --
    second half of round 4 -- steps whose outputs exceed the memory-side cache (> 295 MiB) on the ring with consumer waves"""
    pc, bc, tc, dt, dur = CFG2
    eng = make_engine(pc, bc, tc, dt, dur)
    spec = RolloutSpec("motor", 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)
    for B, want in ((4096, "k_traj_pipe"), (8192, "k_traj_duo"), (16384, "k_traj_quad"), (32768, "k_traj_quad"), (40960, "k_traj_ring"), (65536, "k_traj_ring")):
        params, ip, iv = inputs(pc, bc, tc, B, seed=1)
        q, qd = torch.zeros((B, 7), dtype=torch.float64, device="cuda"), torch.zeros((B, 7), dtype=torch.float64, device="cuda")
        eng.trajectory_rollout(params, ip, iv, spec, q, qd)
        assert eng.last_kernel().startswith(want), (B, eng.last_kernel())
    pc, bc, tc, dt, dur = CFG3
    eng = make_engine(pc, bc, tc, dt, dur)
    # round 5: cfg3 contracts the Euler map's response rows on the open-loop kernel families (tiles / stream / ring by size) ...
    for B, want in ((8192, "k_traj_tiles<dmp_resp"), (16384, "k_traj_stream<dmp_resp"), (65536, "k_traj_ring<dmp_resp")):
        params, ip, iv = inputs(pc, bc, tc, B, seed=1)
        eng.trajectory(params, ip, iv, 0.0)
        assert eng.last_kernel().startswith(want), (B, eng.last_kernel())
    # ... and the serial explicit-Euler kernels behind "dmp_response" 0 keep their rule
    mpk_option("dmp_response", 0)
    for B, want in ((8192, "k_traj_duo<dmp>"), (16384, "k_traj_quad<dmp>"), (32768, "k_traj_duo<dmp>")):
        params, ip, iv = inputs(pc, bc, tc, B, seed=1)
        eng.trajectory(params, ip, iv, 0.0)
        assert eng.last_kernel().startswith(want), (B, eng.last_kernel())


@pytest.mark.parametrize("quad", ["0", "2", "pipe"])
@pytest.mark.parametrize("D,T", [(1, 50), (3, 10), (4, 17), (16, 40), (5, 100), (20, 12)])
def test_pd_rollout_on_every_shape_class(D, T, quad, monkeypatch, mpk_option):
    """tile-streaming kernel (D <= 16, float4-aligned; one or four groups per wave), its producer / consumer form (k_pd_rollout_pipe) and
    the generic kernel (everything else) against the oracle"""
    from tests.test_gpu_edge_cases import cfg_for
    if quad == "pipe":
        mpk_option("pd_pipe", 1)
    else:
        mpk_option("pd_quad", quad)
    pc, bc, tc, dt, dur = cfg_for("promp", D, 3, T)
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 23
    params, ip, iv = inputs(pc, bc, tc, B, seed=D)
    pos, vel = eng.trajectory(params, ip, iv, 0.0)
    pg, dg = np.linspace(0.5, 1.5, D), np.linspace(0.05, 0.2, D)
    n_steps = np.random.default_rng(T).integers(0, T + 1, B).astype(np.int32)
    q0, qd0 = ip.astype(np.float64), iv.astype(np.float64)
    q, qd = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    spec = RolloutSpec("motor", D, pg, dg, -0.6, 0.6, plant="double_integrator", dt=dt)
    act = eng.pd_rollout(spec, pos, vel, q, qd, n_steps=torch.tensor(n_steps))
    ra, rq, rqd = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), "motor", pg, dg, -0.6, 0.6, "double_integrator", dt,
                            q0, qd0, n_steps=n_steps)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)
    q2, qd2 = torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda")
    assert eng.pd_rollout(spec, pos, vel, q2, qd2, want_actions=False) is None      # state-only rollout
    _, rq, _ = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), "motor", pg, dg, -0.6, 0.6, "double_integrator", dt, q0, qd0)
    assert np.array_equal(q2.cpu().numpy(), rq)


@pytest.mark.parametrize("name", ["cfg3_dmp", "prodmp_learn_tau_delay", "promp_learn_tau"])
def test_fused_entry_points_cover_every_configuration(name):
    """what the single fused kernel does not cover (dmp, learned tau / delay) runs as trajectory + rollout kernels behind
    the same entry points: actions / plant state bit-exact against the oracle, c_pos / c_vel left untouched"""
    from tests.test_gpu_trajectory import PER_ROW
    pc, bc, tc, dt, dur = CFG3 if name == "cfg3_dmp" else PER_ROW[name]
    eng = make_engine(pc, bc, tc, dt, dur)
    D, B = eng.num_dof, 33
    params, ip, iv = inputs(pc, bc, tc, B, seed=5)
    pg, dg = np.linspace(0.5, 1.5, D), np.linspace(0.05, 0.1, D)
    cp, cv = ip.astype(np.float64) * 0.5, iv.astype(np.float64) + 0.1
    cpt, cvt = torch.tensor(cp, device="cuda"), torch.tensor(cv, device="cuda")
    pos, vel, act = eng.trajectory_actions(params, ip, iv, RolloutSpec("motor", D, pg, dg, -1, 1, plant="static"),
                                           cpt, cvt)
    torch.cuda.synchronize()
    p0, v0 = eng.trajectory(params, ip, iv, 0.0)
    assert torch.equal(pos, p0) and torch.equal(vel, v0)
    ra, _, _ = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), "motor", pg, dg, -1, 1, "static", dt, cp, cv)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(cpt.cpu().numpy(), cp) and np.array_equal(cvt.cpu().numpy(), cv)
    q, qd = torch.tensor(cp, device="cuda"), torch.tensor(cv, device="cuda")
    n_steps = np.random.default_rng(0).integers(0, eng.num_steps + 1, B).astype(np.int32)
    pos, vel, act = eng.trajectory_rollout(params, ip, iv,
                                           RolloutSpec("motor", D, pg, dg, -1, 1, plant="double_integrator", dt=dt),
                                           q, qd, n_steps=torch.tensor(n_steps))
    ra, rq, rqd = O.rollout(pos.cpu().numpy(), vel.cpu().numpy(), "motor", pg, dg, -1, 1, "double_integrator", dt, cp,
                            cv, n_steps=n_steps)
    assert torch.equal(pos, p0) and np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)


def test_rollout_spec_rejects_unknown_controllers_and_bad_gains():
    with pytest.raises(ValueError):
        RolloutSpec("impedance", 7)
    with pytest.raises(ValueError):
        RolloutSpec("metaworld", 7, plant="double_integrator", dt=0.01)     # open loop only: no batchable metaworld plant
    with pytest.raises(ValueError):
        RolloutSpec("motor", 7, p_gains=np.ones(3))


# ---- integer replanning state, validity ------------------------------------------------------------------------------
@pytest.mark.parametrize("every,mpt,horizon", [(25, 4, 100), (5, 3, 50), (10, 1, 50), (7, 100, 50), (25, 2, 100)])
def test_replan_advance_is_bit_exact(every, mpt, horizon):
    pc, bc, tc, dt, dur = CFG4
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 257
    ts = torch.zeros(B, dtype=torch.int32, device="cuda")
    ps = torch.zeros_like(ts)
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ref = O.replanning_segments(horizon, every, mpt)
    for k, (start, n) in enumerate(ref):
        assert int(ts[0]) == start
        seg = eng.replan_advance(ts, ps, done, every, mpt, horizon)
        assert torch.all(seg == n) and torch.all(ps == k + 1) and torch.all(ts == start + n)
        assert bool(done.all()) == (k == len(ref) - 1)
    seg = eng.replan_advance(ts, ps, done, every, mpt, horizon)      # finished episodes are left alone
    assert torch.all(seg == 0) and torch.all(ps == len(ref))


def test_traj_validity_matches_reference_rule():
    """table_tennis_env.py:303-309 incl. the quirk that action[0], action[1] are compared to the tau/delay bounds"""
    pc, bc, tc, dt, dur = CFG5
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 300
    params, ip, iv = inputs(pc, bc, tc, B, seed=9)
    params[:, 0] = np.random.default_rng(0).uniform(0.5, 1.8, B)
    params[:, 1] = np.random.default_rng(1).uniform(0.0, 0.2, B)
    pos, _ = eng.trajectory(params, ip, iv, 0.0)
    lo = np.array([-2.6, -2.0, -2.8, -0.9, -4.8, -1.6, -2.2])
    hi = np.array([2.6, 2.0, 2.8, 3.1, 1.3, 1.6, 2.2])
    p = pos.cpu().numpy().astype(np.float64)
    want_pos = np.all((p >= lo) & (p <= hi), axis=(1, 2))
    got = eng.traj_validity(pos, lo, hi).cpu().numpy()
    assert np.array_equal(got, want_pos) and 0 < want_pos.sum() < B
    tb, db = [0.8, 1.5], [0.05, 0.15]
    want = want_pos & (params[:, 0] >= tb[0]) & (params[:, 0] <= tb[1]) & (params[:, 1] >= db[0]) & (params[:, 1] <= db[1])
    got = eng.traj_validity(pos, lo, hi, torch.tensor(params, device="cuda"), tb, db).cpu().numpy()
    assert np.array_equal(got, want)
    # the reward such a plan earns instead of being executed (table_tennis_env.py:282-289)
    got, pen = eng.traj_validity(pos, lo, hi, torch.tensor(params, device="cuda"), tb, db, with_penalty=True)
    assert np.array_equal(got.cpu().numpy(), want)
    ref = O.traj_invalid_penalty(params, p, lo, hi, tb, db)
    assert np.allclose(pen.cpu().numpy(), ref, rtol=1e-12, atol=1e-15)
    assert np.all(ref[~want] < 0) and np.all(ref[want] == 0)
    got, pen = eng.traj_validity(pos, lo, hi, with_penalty=True)
    assert np.allclose(pen.cpu().numpy(), O.traj_invalid_penalty(params, p, lo, hi), rtol=1e-12, atol=1e-15)


# ---- BatchedBlackBox --------------------------------------------------------------------------------------------------
def _batched(cfg, B, **kw):
    pc, bc, tc, dt, dur = cfg
    pg = get_phase_generator(pc.phase_generator_type, tau=pc.tau, alpha_phase=pc.alpha_phase,
                             learn_tau=pc.learn_tau, learn_delay=pc.learn_delay, tau_bound=list(pc.tau_bound),
                             delay_bound=list(pc.delay_bound))
    bkw = dict(num_basis=bc.num_basis, basis_bandwidth_factor=bc.basis_bandwidth_factor)
    if bc.basis_generator_type == "prodmp":
        bkw["alpha"] = bc.alpha
    bg = get_basis_generator(bc.basis_generator_type, pg, **bkw)
    tkw = dict(weights_scale=tc.weights_scale)
    if tc.trajectory_generator_type == "prodmp":
        tkw.update(goal_scale=tc.goal_scale, auto_scale_basis=tc.auto_scale_basis, disable_goal=tc.disable_goal,
                   relative_goal=tc.relative_goal)
    tg = get_trajectory_generator(tc.trajectory_generator_type, tc.action_dim, bg, **tkw)
    ctrl = get_controller("motor", p_gains=PG, d_gains=DG)
    return BatchedBlackBox(tg, ctrl, B, dt, dur, act_low=-1.0, act_high=1.0, **kw)


def test_batched_episode_equals_oracle_closed_loop():
    B = 64
    bb = _batched(CFG2, B, plant="double_integrator")
    rng = np.random.default_rng(0)
    q0 = rng.uniform(-1, 1, (B, 7))
    bb.reset(q0)
    params = rng.standard_normal((B, 42)).astype(np.float32)
    out = bb.step(params)
    pc, bc, tc, dt, dur = CFG2
    rp, rv = O.get_trajectory(pc, bc, tc, params, dur, dt, 0.0, q0.astype(np.float32), np.zeros((B, 7), np.float32),
                              dtype=np.float64)
    close(out["des_pos"].cpu().numpy(), rp, "des_pos")
    close(out["des_vel"].cpu().numpy(), rv, "des_vel")
    ra, rq, rqd = O.rollout(out["des_pos"].cpu().numpy(), out["des_vel"].cpu().numpy(), "motor", PG, DG, -1.0, 1.0,
                            "double_integrator", dt, q0, np.zeros((B, 7)))
    assert np.array_equal(out["step_actions"].cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(out["current_pos"].cpu().numpy(), rq)
    assert torch.all(out["trajectory_length"] == 100) and bool(out["done"].all())


def test_batched_replanning_follows_the_single_episode_sequence():
    """cfg4: schedule t % 25 == 0, max_planning_times 4, condition_on_desired (box_pushing/mp_wrapper.py:87-91)"""
    B = 48
    bb = _batched(CFG4, B, plant="double_integrator", replanning_every=25, max_planning_times=4,
                  condition_on_desired=True)
    rng = np.random.default_rng(2)
    q0 = rng.uniform(-1, 1, (B, 7))
    bb.reset(q0)
    pc, bc, tc, dt, dur = CFG4
    cond_p, cond_v = q0.astype(np.float32), np.zeros((B, 7), np.float32)
    q, qd = q0.copy(), np.zeros((B, 7))
    for k, (start, n) in enumerate(O.replanning_segments(100, 25, 4)):
        params = rng.standard_normal((B, 35)).astype(np.float32)
        out = bb.step(params)
        assert torch.all(out["trajectory_length"] == n) and int(bb.traj_steps[0]) == start + n
        assert int(bb.plan_steps[0]) == k + 1 and bool(out["done"].all()) == (k == 3)
        rp, rv = O.get_trajectory(pc, bc, tc, params, dur, dt, start * dt, cond_p, cond_v, dtype=np.float64)
        close(out["des_pos"].cpu().numpy(), rp, f"plan {k} pos")
        close(out["des_vel"].cpu().numpy(), rv, f"plan {k} vel")
        dp, dv = out["des_pos"].cpu().numpy(), out["des_vel"].cpu().numpy()
        ra, q, qd = O.rollout(dp, dv, "motor", PG, DG, -1.0, 1.0, "double_integrator", dt, q, qd,
                              n_steps=np.full(B, n))
        assert np.array_equal(out["step_actions"].cpu().numpy(), ra.astype(np.float32))
        assert np.array_equal(out["current_pos"].cpu().numpy(), q)
        cond_p, cond_v = dp[:, n - 1], dv[:, n - 1]           # condition on the desired state where the plan broke


def test_cfg4_at_its_full_per_gpu_batch_against_the_oracle():
    """
    BASELINE cfg4 at the size one GPU runs (65 536 episodes over 8 GPUs = 8 192 each), four plans, AUTOMATIC kernel
    selection (the fused closed-loop kernel the launcher picks at this size -- not a variant forced by an option):
    integer state array_equal against the restated reference loop, actions and plant state bit-exact against the
    oracle's float64 rollout over all 8 192 episodes, trajectories within 1e-5 on a 256-row sample.
    Anchor: envs/mujoco/box_pushing/mp_wrapper.py:87-91; black_box_wrapper.py:150-217.
    """
    B = 8192
    bb = _batched(CFG4, B, plant="double_integrator", replanning_every=25, max_planning_times=4,
                  condition_on_desired=True)
    rng = np.random.default_rng(12)
    q0 = rng.uniform(-1, 1, (B, 7))
    bb.reset(q0)
    pc, bc, tc, dt, dur = CFG4
    rows = np.sort(rng.choice(B, 256, replace=False))
    cond_p, cond_v = q0.astype(np.float32), np.zeros((B, 7), np.float32)
    q, qd = q0.copy(), np.zeros((B, 7))
    cur, plan = np.zeros(B, np.int64), np.zeros(B, np.int64)
    kernels = set()
    for k in range(4):
        params = rng.standard_normal((B, 35)).astype(np.float32)
        out = bb.step(params)
        kernels.add(bb.engine.last_kernel())
        # integer state: the reference loop, episode by episode (all episodes share the schedule here; done per episode
        # anyway so that a kernel that mixed episodes up would be caught)
        n_ref, cur_ref, plan_ref = zip(*[_reference_loop(int(c), int(p), False, 25, 4, 100, 100) for c, p in zip(cur, plan)])
        assert np.array_equal(out["trajectory_length"].cpu().numpy(), np.asarray(n_ref, np.int32))
        assert np.array_equal(bb.traj_steps.cpu().numpy(), np.asarray(cur_ref, np.int32))
        assert np.array_equal(bb.plan_steps.cpu().numpy(), np.asarray(plan_ref, np.int32))
        assert np.array_equal(out["done"].cpu().numpy(), np.asarray(cur_ref) >= 100)
        n = int(n_ref[0])
        start = int(cur[0])
        cur, plan = np.asarray(cur_ref), np.asarray(plan_ref)
        dp, dv = out["des_pos"].cpu().numpy(), out["des_vel"].cpu().numpy()
        rp, rv = O.get_trajectory(pc, bc, tc, params[rows], dur, dt, start * dt, cond_p[rows], cond_v[rows],
                                  dtype=np.float64)
        close(dp[rows], rp, f"plan {k} pos")
        close(dv[rows], rv, f"plan {k} vel")
        ra, q, qd = O.rollout(dp, dv, "motor", PG, DG, -1.0, 1.0, "double_integrator", dt, q, qd, n_steps=np.full(B, n))
        assert np.array_equal(out["step_actions"].cpu().numpy(), ra.astype(np.float32)), f"plan {k} actions"
        assert np.array_equal(out["current_pos"].cpu().numpy(), q) and np.array_equal(out["current_vel"].cpu().numpy(), qd)
        cond_p, cond_v = dp[:, n - 1], dv[:, n - 1]
        assert np.array_equal(bb.condition_pos.cpu().numpy(), cond_p) and np.array_equal(bb.condition_vel.cpu().numpy(), cond_v)
    assert all(kn.endswith("closed>") for kn in kernels), kernels       # the ONE-launch step, whichever variant was chosen


def test_cfg5_fused_actions_at_its_full_per_gpu_batch_against_the_oracle():
    """BASELINE cfg5 (ProMP TableTennis4D, table_tennis/mp_wrapper.py:11-30) at B = 8 192, automatic kernel selection:
    fused open-loop PD actions bit-exact over all episodes, trajectories within 1e-5 on a 256-row sample"""
    pc, bc, tc, dt, dur = CFG5
    B = 8192
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=21)
    pg = 0.5 * np.array([1.0, 4.0, 2.0, 4.0, 1.0, 4.0, 1.0]); dg = 0.1 * pg
    spec = RolloutSpec("motor", 7, pg, dg, -1.0, 1.0, plant="static")
    c_pos, c_vel = ip.astype(np.float64), iv.astype(np.float64)
    pos, vel, act = eng.trajectory_actions(params, ip, iv, spec, c_pos, c_vel)
    torch.cuda.synchronize()
    assert eng.last_kernel() in ("k_traj_tiles<promp,act>", "k_traj_stream<promp,act>"), eng.last_kernel()
    dp, dv = pos.cpu().numpy(), vel.cpu().numpy()
    rows = np.sort(np.random.default_rng(0).choice(B, 256, replace=False))
    rp, rv = O.get_trajectory(pc, bc, tc, params[rows], dur, dt, 0.0, ip[rows], iv[rows], dtype=np.float64)
    close(dp[rows], rp, "pos"); close(dv[rows], rv, "vel", atol=fd_atol(rp, dt))
    ra, _, _ = O.rollout(dp, dv, "motor", pg, dg, -1.0, 1.0, "static", dt, c_pos, c_vel)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))


@pytest.mark.parametrize("name", ["cfg4", "cfg3_dmp", "prodmp_learn_tau_delay"])
def test_batched_fused_and_unfused_steps_agree_bitwise(name):
    """the lean step (mpk_trajectory_rollout: one launch for shared-phase promp / prodmp, two for dmp and learned tau /
    delay) against the step assembled from separate calls, over a replanned episode"""
    from tests.test_gpu_trajectory import PER_ROW
    cfg = {"cfg4": CFG4, "cfg3_dmp": CFG3}.get(name) or PER_ROW[name]
    rng = np.random.default_rng(5)
    B = 40
    q0 = rng.uniform(-1, 1, (B, 7)) * 0.2
    outs = []
    for fuse in (True, False):
        T = int(round(cfg[4] / cfg[3]))
        bb = _batched(cfg, B, plant="double_integrator", replanning_every=T // 4, max_planning_times=4,
                      condition_on_desired=name != "cfg3_dmp")
        bb.reset(q0)
        P = bb.engine.num_params
        r = np.random.default_rng(6)
        seq = []
        for _ in range(4):
            params = (r.standard_normal((B, P)) * 0.3).astype(np.float32)
            if name == "prodmp_learn_tau_delay":
                params[:, 0] = r.uniform(0.9, 1.4, B); params[:, 1] = r.uniform(0.06, 0.14, B)
            o = bb.step(params, fuse=fuse)
            seq.append({k: o[k].clone() for k in ("des_pos", "des_vel", "step_actions", "current_pos", "trajectory_length",
                                                    "done")})
        outs.append(seq)
        if name == "cfg4":
            assert bb.engine.last_kernel().endswith("closed>") == fuse
        assert bool(bb.done.all())
    for a, b in zip(*outs):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_batched_learned_tau_delay_freeze_after_first_plan():
    cfg = (O.PhaseCfg("exp", tau=1.0, alpha_phase=3.0, learn_tau=True, learn_delay=True, tau_bound=(0.5, 1.0),
                      delay_bound=(0.0, 0.2)),
           O.BasisCfg("prodmp", num_basis=4, alpha=25), O.TrajCfg("prodmp", action_dim=7), 0.02, 1.0)
    B = 16
    bb = _batched(cfg, B, plant="static", replanning_every=10, max_planning_times=3)
    bb.reset(np.ones((B, 7)))
    rng = np.random.default_rng(3)
    p1 = rng.standard_normal((B, 37)).astype(np.float32)
    p1[:, 0], p1[:, 1] = rng.uniform(0.3, 1.2, B), rng.uniform(0.0, 0.3, B)
    o1 = bb.step(p1)
    frozen = o1["params"][:, :2].cpu().numpy()
    assert np.all(frozen[:, 0] >= 0.5) and np.all(frozen[:, 0] <= 1.0) and np.all(frozen[:, 1] <= np.float32(0.2))
    p2 = rng.standard_normal((B, 37)).astype(np.float32)
    p2[:, 0], p2[:, 1] = 0.77, 0.11
    o2 = bb.step(p2)
    assert np.array_equal(o2["params"][:, :2].cpu().numpy(), frozen)
    pc, bc, tc, dt, dur = cfg
    full = p2.copy(); full[:, :2] = frozen
    rp, _ = O.get_trajectory(pc, bc, tc, full, dur, dt, 10 * dt, np.ones((B, 7), np.float32),
                             np.zeros((B, 7), np.float32), dtype=np.float64)
    close(o2["des_pos"].cpu().numpy(), rp, "second plan")


# ---- size-independent properties at BASELINE's full sizes ------------------------------------------------------------
@pytest.mark.parametrize("cfg,B", [(CFG2, 4096), (CFG3, 16384), (CFG4, 8192), (CFG5, 8192), (CFG2, 262144)],
                         ids=["cfg2_4096", "cfg3_16384", "cfg4_shard8192", "cfg5_shard8192", "cfg2_262144_stream"])
def test_full_size_properties(cfg, B):
    """
    linearity in the parameters (ProMP / ProDMP / DMP are linear maps of [w, g, y_b, v_b]), batch-order invariance
    (episodes are independent: a permuted batch gives permuted rows bit for bit) and agreement of a random sample of
    rows with the oracle
    """
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    params, ip, iv = inputs(pc, bc, tc, B, seed=B % 97)
    P = torch.tensor(params, device="cuda"); IP = torch.tensor(ip, device="cuda"); IV = torch.tensor(iv, device="cuda")
    pos, vel = eng.trajectory(P, IP, IV, 0.0)
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all()
    perm = torch.randperm(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    pp, vp = eng.trajectory(P[perm], IP[perm], IV[perm], 0.0)
    assert torch.equal(pp, pos[perm]) and torch.equal(vp, vel[perm])
    p2, v2 = eng.trajectory(2 * P, 2 * IP, 2 * IV, 0.0)                   # scaling by 2 is exact in binary fp
    assert torch.equal(p2, 2 * pos) and torch.equal(v2, 2 * vel)
    rows = np.random.default_rng(0).choice(B, 64, replace=False)
    rp, rv = O.get_trajectory(pc, bc, tc, params[rows], dur, dt, 0.0, ip[rows], iv[rows], dtype=np.float64)
    fd = tc.trajectory_generator_type == "promp"
    close(pos[rows].cpu().numpy(), rp, "sample pos")
    close(vel[rows].cpu().numpy(), rv, "sample vel", atol=fd_atol(rp, dt) if fd else 0.0)


# ---- host env bridge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp_type,replan", [("prodmp", False), ("prodmp", True), ("promp", True), ("dmp", False)])
@pytest.mark.parametrize("workers", [0, 3])
def test_vector_black_box_equals_individual_wrappers(mp_type, replan, workers):
    """N host envs planned in ONE launch and tracked on the host == N independent BlackBoxWrapper episodes, bit for bit"""
    from fancy_gym_amd import VectorBlackBox
    bb = {"verbose": 2}
    if replan:
        bb.update(replanning_schedule=lambda pos, vel, obs, action, t: t % 20 == 0, max_planning_times=3,
                  condition_on_desired=True)
    N = 5

    def make():
        return fancy_gym_amd.make_bb("dint-v0", [DoubleIntegratorWrapper], dict(bb),
                                     {"trajectory_generator_type": mp_type},
                                     {"controller_type": "motor", "p_gains": PG, "d_gains": DG},
                                     {"phase_generator_type": "exp" if "dmp" in mp_type else "linear"},
                                     {"basis_generator_type": "prodmp" if mp_type == "prodmp" else "rbf", "num_basis": 4})
    vec = VectorBlackBox([make() for _ in range(N)], num_workers=workers)
    solo = [make() for _ in range(N)]
    vec.reset(seed=11)
    for i, e in enumerate(solo):
        e.reset(seed=11 + i)
    rng = np.random.default_rng(0)
    for _ in range(3 if replan else 1):
        actions = rng.standard_normal((N, vec.action_space.shape[0]))
        obs, rew, term, trunc, infos = vec.step(actions)
        for i, e in enumerate(solo):
            o, r, te, tr, info = e.step(actions[i])
            assert np.array_equal(o, obs[i]) and r == rew[i] and te == term[i] and tr == trunc[i]
            assert info["trajectory_length"] == infos[i]["trajectory_length"]
            for k in ("positions", "velocities", "step_actions"):
                assert np.array_equal(info[k], infos[i][k]), k
    vec.close()


# ---- SimpleReacher on device ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["motor", "position", "velocity"])
@pytest.mark.parametrize("D,B,T", [(2, 1, 200), (5, 300, 200), (5, 65, 37), (7, 130, 100), (16, 9, 12), (20, 7, 10)])
@pytest.mark.parametrize("mode", ["tiles", "quad", "generic", "pipe"])
def test_reacher_rollout_matches_oracle(controller, D, B, T, mode, monkeypatch, mpk_option):
    """actions and plant state bit for bit (float64, no FMA); rewards to 1e-12 (device vs host libm cos / sin).  Kernels:
    tile-streaming with the per-tile parallel reward phase (one or four groups per wave), and the generic
    lane-per-(episode, DoF) kernel with segmented scans"""
    from fancy_gym_amd import TrajectoryEngine
    if mode == "pipe":
        mpk_option("pd_pipe", 1)          # k_pd_rollout_pipe (a consumer wave and three producers per four groups; needs <= 2 episodes per group)
    else:
        mpk_option("pd_quad", "2" if mode == "quad" else "0")
    if mode == "generic":
        mpk_option("pd_simple", "1")
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=3,
                           dt=0.01, duration=T * 0.01, tau=T * 0.01)
    rng = np.random.default_rng(D * 1000 + B)
    des_pos = rng.standard_normal((B, T, D)).astype(np.float32)
    des_vel = rng.standard_normal((B, T, D)).astype(np.float32)
    goal = rng.uniform(-D, D, (B, 2))
    n_steps = rng.integers(0, T + 1, B).astype(np.int32)
    step0 = rng.integers(0, 260, B).astype(np.int32)
    q0 = rng.uniform(-1, 1, (B, D)); qd0 = rng.uniform(-1, 1, (B, D))
    pg = rng.uniform(0.1, 1.0, D); dg = rng.uniform(0.01, 0.1, D)
    spec = RolloutSpec(controller, D, pg, dg, -2.0, 1.5, plant="double_integrator", dt=0.01)
    q = torch.tensor(q0, device="cuda"); qd = torch.tensor(qd0, device="cuda")
    act, rew = eng.reacher_rollout(spec, torch.tensor(des_pos, device="cuda"), torch.tensor(des_vel, device="cuda"), q, qd,
                                   torch.tensor(goal), n_steps=torch.tensor(n_steps), step0=torch.tensor(step0))
    ra, rr, rq, rqd = O.reacher_rollout(des_pos, des_vel, controller, pg, dg, -2.0, 1.5, 0.01, q0, qd0, goal,
                                        n_steps=n_steps, step0=step0)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)
    got = rew.cpu().numpy()
    assert got.shape == (B, T) and np.all(np.abs(got - rr) <= 1e-12 * (1.0 + np.abs(rr))), np.abs(got - rr).max()
    paid = (step0[:, None] + np.arange(T)[None] >= 199) & (np.arange(T)[None] < n_steps[:, None])
    assert paid.any() and (~paid).any()       # both branches of the reward are exercised


@pytest.mark.gpu
@pytest.mark.parametrize("reward", [False, True])
def test_rollout_pipeline_with_several_units_per_workgroup_equals_the_tile_kernel(reward, mpk_option):
    """k_pd_rollout_pipe forced on a launch far beyond its automatic range: every workgroup walks several units (the counters of its
    waves keep counting across them), the last unit is ragged; actions, rewards and plant state are the tile kernel's bits"""
    from fancy_gym_amd import TrajectoryEngine
    D, T, B = 5, 200, 20003
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=3, dt=0.01, duration=T * 0.01,
                           tau=T * 0.01)
    g = torch.Generator().manual_seed(5)
    des_pos = torch.randn((B, T, D), generator=g).cuda(); des_vel = torch.randn((B, T, D), generator=g).cuda()
    q0 = (torch.rand((B, D), generator=g, dtype=torch.float64) * 2 - 1).cuda(); qd0 = (torch.rand((B, D), generator=g, dtype=torch.float64) - 0.5).cuda()
    goal = (torch.rand((B, 2), generator=g, dtype=torch.float64) * 4 - 2).cuda()
    n_steps = torch.randint(0, T + 1, (B,), generator=g, dtype=torch.int32).cuda()
    step0 = torch.randint(0, 60, (B,), generator=g, dtype=torch.int32).cuda()
    spec = RolloutSpec("motor", D, 0.6, 0.075, -2.0, 1.5, plant="double_integrator", dt=0.01)
    outs = []
    for pipe in (0, 1):
        mpk_option("pd_pipe", pipe)
        q, qd = q0.clone(), qd0.clone()
        if reward:
            act, rew = eng.reacher_rollout(spec, des_pos, des_vel, q, qd, goal, n_steps=n_steps, step0=step0, steps_before_reward=199)
        else:
            act, rew = eng.pd_rollout(spec, des_pos, des_vel, q, qd, n_steps=n_steps), torch.zeros(1)
        torch.cuda.synchronize()
        eng.check_range()
        outs.append((act.clone(), rew.clone(), q, qd))
    for a, b, what in zip(outs[0], outs[1], ("actions", "rewards", "q", "qd")):
        assert torch.equal(a, b), what
    assert float(outs[1][0].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sbr", [0, 199, 100000])
@pytest.mark.parametrize("D,B,T", [(5, 300, 200), (5, 37, 100), (2, 40, 200), (7, 50, 64)])
@pytest.mark.parametrize("mode", ["tiles", "quad", "generic", "tiles_rt", "tiles_nohelper", "quad_helper", "duo_helper", "pipe", "pipe_rt"])
def test_reacher_reward_with_and_without_the_distance_term(sbr, D, B, T, mode, mpk_option):
    """simple_reacher.py:62-63: the distance term only from `steps_before_reward` on (199 of 200 steps carry none at the reference's
    setting, :31).  The reward pass evaluates the end effector only where one of a pass's items needs it: steps_before_reward = 0
    keeps the all-live path covered, 100000 the path without any, 199 with step0 = 0 is the reference's episode (the last step
    only).  Rewards without the distance term are -sum(action ** 2) left to right: bit for bit on the tile kernels."""
    from fancy_gym_amd import TrajectoryEngine
    if mode.startswith("pipe"):
        mpk_option("pd_pipe", 1)          # k_pd_rollout_pipe
        if mode == "pipe_rt":
            mpk_option("pd_generic", "1")
    else:
        mpk_option("pd_quad", "2" if mode.startswith("quad") else ("3" if mode.startswith("duo") else "0"))
    if mode == "generic":
        mpk_option("pd_simple", "1")
    if mode == "tiles_rt":
        mpk_option("pd_generic", "1")     # controller and link count at run time (motor on 2 / 5 links are compiled in otherwise)
    # the control-cost pass on two helper waves of the workgroup (automatic with one or two groups per wave) / on the chain waves
    if mode.endswith("_nohelper"):
        mpk_option("pd_helper", 0)
    if mode.endswith("_helper"):
        mpk_option("pd_helper", 1)
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=3,
                           dt=0.01, duration=T * 0.01, tau=T * 0.01)
    rng = np.random.default_rng(sbr + D * 10 + B)
    des_pos = rng.standard_normal((B, T, D)).astype(np.float32)
    des_vel = rng.standard_normal((B, T, D)).astype(np.float32)
    goal = rng.uniform(-D, D, (B, 2))
    n_steps = np.where(rng.uniform(size=B) < 0.5, T, rng.integers(0, T + 1, B)).astype(np.int32)
    q0 = rng.uniform(-1, 1, (B, D)); qd0 = rng.uniform(-1, 1, (B, D))
    spec = RolloutSpec("motor", D, 0.6, 0.075, -2.0, 1.5, plant="double_integrator", dt=0.01)
    q = torch.tensor(q0, device="cuda"); qd = torch.tensor(qd0, device="cuda")
    act, rew = eng.reacher_rollout(spec, torch.tensor(des_pos, device="cuda"), torch.tensor(des_vel, device="cuda"), q, qd,
                                   torch.tensor(goal), n_steps=torch.tensor(n_steps), steps_before_reward=sbr)
    ra, rr, rq, rqd = O.reacher_rollout(des_pos, des_vel, "motor", 0.6, 0.075, -2.0, 1.5, 0.01, q0, qd0, goal,
                                        n_steps=n_steps, steps_before_reward=sbr)
    assert np.array_equal(act.cpu().numpy(), ra.astype(np.float32))
    assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(qd.cpu().numpy(), rqd)
    got = rew.cpu().numpy()
    assert np.all(np.abs(got - rr) <= 1e-12 * (1.0 + np.abs(rr))), np.abs(got - rr).max()
    paid = (np.arange(T)[None] >= sbr) & (np.arange(T)[None] < n_steps[:, None])
    assert paid.any() == (sbr < T)
    if mode != "generic":                     # (the generic kernel sums over the DoF lanes in tree order)
        assert np.array_equal(got[~paid], rr[~paid])
    assert np.all(got[np.arange(T)[None] >= n_steps[:, None]] == 0.0)


@pytest.mark.gpu
def test_reacher_rollout_argument_checks():
    from fancy_gym_amd import TrajectoryEngine
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=3, num_basis=3,
                           dt=0.01, duration=0.1, tau=0.1)
    z = torch.zeros((2, 10, 3), device="cuda")
    q = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):     # the reward is defined on the torque plant only
        eng.reacher_rollout(RolloutSpec("motor", 3, 1.0, 0.1, -1, 1, plant="static"), z, z, q, q.clone(),
                            torch.zeros(2, 2))
    act, rew = eng.reacher_rollout(RolloutSpec("motor", 3, 1.0, 0.1, -1, 1, plant="double_integrator", dt=0.01),
                                   z[:0], z[:0], q[:0], q[:0].clone(), torch.zeros(0, 2))
    assert act.shape == (0, 10, 3) and rew.shape == (0, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("mp_type", ["ProMP", "DMP", "ProDMP"])
def test_batched_simple_reacher_equals_single_episode_wrapper(mp_type):
    """fancy_<MP>/LongSimpleReacher-v0 stepped episode by episode on the host env (BlackBoxWrapper + NumPy plant + NumPy
    reward) against ONE batched device step with reward='simple_reacher': same plans, same actions, same returns"""
    from fancy_gym_amd import _gym
    env = _gym.make(f"fancy_{mp_type}/LongSimpleReacher-v0", mp_config_override={"black_box_kwargs": {"verbose": 2}})
    env.action_space.seed(5)
    B = 6
    starts, goals, actions, returns, infos = [], [], [], [], []
    for b in range(B):
        env.reset(seed=100 + b)
        starts.append(env.unwrapped.q.copy()); goals.append(env.unwrapped.goal.copy())
        a = env.action_space.sample()
        _, ret, term, trunc, info = env.step(a)
        assert trunc and not term and info["trajectory_length"] == 200
        actions.append(a); returns.append(ret); infos.append(info)
    bb = BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=0.01, duration=2.0, act_low=-1000.0,
                         act_high=1000.0, plant="double_integrator", reward="simple_reacher")
    with pytest.raises(ValueError):
        bb.reset(np.stack(starts))
    bb.reset(np.stack(starts), goal=np.stack(goals))
    out = bb.step(np.stack(actions).astype(np.float32))
    assert bool(out["done"].all()) and torch.all(out["trajectory_length"] == 200)
    for b in range(B):
        assert np.array_equal(out["des_pos"][b].cpu().numpy(), infos[b]["positions"])
        assert np.array_equal(out["step_actions"][b].cpu().numpy(),
                              np.asarray(infos[b]["step_actions"]).astype(np.float32))
        sr = np.asarray(infos[b]["step_rewards"], dtype=np.float64)
        assert np.all(np.abs(out["step_rewards"][b].cpu().numpy() - sr) <= 1e-12 * (1 + np.abs(sr)))
        assert abs(float(out["rewards"][b]) - returns[b]) <= 1e-10 * (1 + abs(returns[b]))
        assert np.any(sr[199:] != sr[198])       # the distance term switched on at step 199


@pytest.mark.gpu
@pytest.mark.parametrize("mp_type,agg,cond", [("ProMP", "sum", False), ("ProMP", "mean", False), ("ProMP", "last", False),
                                               ("DMP", "sum", False), ("DMP", "mean", False), ("DMP", "last", False),
                                               ("DMP", "sum", True), ("ProMP", "sum", True)])
def test_batched_sub_trajectories_equal_single_episode_wrappers(mp_type, agg, cond):
    """learn_sub_trajectories (black_box_wrapper.py:98-102; test/test_replanning_sequencing.py:67-109) on the batched path:
    B episodes of fancy_<MP>/LongSimpleReacher-v0, each stepped by its own host BlackBoxWrapper (NumPy plant + reward) until the
    200-step budget ends, against ONE BatchedBlackBox stepping them together -- episodes plan different lengths
    (round(tau / dt)), so they finish after different numbers of plans.  Integers (trajectory_length, done) exactly; plans, actions,
    step rewards and aggregated returns to the 1e-5 contract (a single wrapper evaluates a plan on linspace(0, T_b dt, T_b + 1)[1:],
    the batch on the first T_b points of the longest plan's grid: one fp32 rounding of the grid apart).
    cond: condition_on_desired with sub-trajectories -- the reference stores the desired state only in its break branch
    (black_box_wrapper.py:197-203), which a sub-trajectory that ends before the episode never enters: every plan starts from the
    plant's current state (round 4's batched path planned from the previous plan's desired end state instead: ADVICE r04)."""
    from fancy_gym_amd import _gym
    fn = {"sum": np.sum, "mean": np.mean, "last": (lambda r: r[-1])}[agg]
    env = _gym.make(f"fancy_{mp_type}/LongSimpleReacher-v0",
                    mp_config_override={"black_box_kwargs": {"learn_sub_trajectories": True, "verbose": 2, "reward_aggregation": fn,
                                                             "condition_on_desired": cond}})
    assert env.learn_sub_trajectories and env.traj_gen.learn_tau
    env.action_space.seed(11)
    B, dt = 7, 0.01
    rng = np.random.default_rng(5)
    starts, goals, eps = [], [], []
    for b in range(B):
        env.reset(seed=200 + b)
        starts.append(env.unwrapped.q.copy()); goals.append(env.unwrapped.goal.copy())
        steps, done = [], False
        while not done:
            a = env.action_space.sample()
            a[0] = rng.uniform(0.15, 1.3)                      # sub-trajectories of 15 .. 130 steps
            a[1:] *= 0.05
            _, ret, term, trunc, info = env.step(a)
            done = term or trunc
            steps.append((a.astype(np.float32), ret, info, done))
        eps.append(steps)
    n_plans = max(len(e) for e in eps)
    assert min(len(e) for e in eps) < n_plans                   # the episodes do not finish together
    bb = BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=dt, duration=2.0, act_low=-1000.0, act_high=1000.0,
                         plant="double_integrator", reward="simple_reacher", learn_sub_trajectories=True,
                         max_episode_steps=200, reward_aggregation=agg if agg != "mean" else np.mean, condition_on_desired=cond)
    bb.reset(np.stack(starts), goal=np.stack(goals))
    P = bb.engine.num_params
    for k in range(n_plans):
        acts = np.stack([eps[b][k][0] if k < len(eps[b]) else np.full(P, 0.5, np.float32) for b in range(B)])
        out = bb.step(acts)
        torch.cuda.synchronize()
        for b in range(B):
            n = int(out["trajectory_length"][b])
            if k >= len(eps[b]):
                assert n == 0 and bool(out["done"][b])           # a finished episode is left alone
                continue
            a, ret, info, done = eps[b][k]
            assert n == info["trajectory_length"] and bool(out["done"][b]) == done, (b, k)
            if not done:
                assert n == np.round(np.float32(a[0]) / dt)
            want = np.asarray(info["positions"])[:n]
            got = out["des_pos"][b, :n].cpu().numpy()
            assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0), (b, k)
            wv = np.asarray(info["velocities"])[:n]
            gv = out["des_vel"][b, :n].cpu().numpy()
            assert np.abs(gv - wv).max() <= 1e-5 * max(np.abs(wv).max(), 1.0) + 2 * np.spacing(np.float32(np.abs(want).max())) / dt, (b, k)
            wa = np.asarray(info["step_actions"], dtype=np.float64)
            ga = out["step_actions"][b, :n].cpu().numpy().astype(np.float64)
            assert np.abs(ga - wa).max() <= 1e-4 * max(np.abs(wa).max(), 1.0), (b, k)
            sr = np.asarray(info["step_rewards"], dtype=np.float64)
            gr = out["step_rewards"][b, :n].cpu().numpy()
            assert np.abs(gr - sr).max() <= 1e-4 * max(np.abs(sr).max(), 1.0), (b, k)
            assert np.all(out["step_rewards"][b, n:].cpu().numpy() == 0.0)
            assert abs(float(out["rewards"][b]) - ret) <= 1e-4 * max(abs(ret), 1.0), (b, k, agg)
    assert bool(out["done"].all()) and torch.all(bb.traj_steps == 200)


@pytest.mark.gpu
def test_batched_sub_trajectory_argument_checks():
    with pytest.raises(ValueError, match="sub-trajectory learning and replanning"):
        _batched(CFG2, 4, replanning_every=10, learn_sub_trajectories=True)
    with pytest.raises(ValueError, match="learned tau"):
        _batched(CFG2, 4, learn_sub_trajectories=True)
    with pytest.raises(ValueError, match="reward_aggregation"):
        _batched(CFG2, 4, reward_aggregation=np.max)


@pytest.mark.gpu
def test_captured_episode_with_the_validity_gate():
    """capture_episode with pos_limits (round 6): the gated step is ONE launch (mpk_replan_step_gated) and the host keeps its lockstep
    mirror -- an invalid plan finishes its episode, so every live episode has executed exactly the segments of the integer rule and
    nothing is read back from the device during capture.  A replay equals the eager fused steps bit for bit and the separate launches
    (`fuse=False`: trajectory, k_validity, advance, rollout, gather) bit for bit too, the penalty to 1e-12; invalid plans terminate
    their episodes without a plant step and the others go on replanning"""
    from tests.test_gpu_learned_phase import compare_gated_paths
    B = 160
    lo, hi = np.full(7, -0.9), np.full(7, 0.9)
    kw = dict(plant="double_integrator", replanning_every=25, max_planning_times=4, condition_on_desired=True,
              pos_limits=(lo, hi))
    bb = _batched(CFG4, B, **kw)
    ep = bb.capture_episode(4)
    assert not bb.device_time and "gate" in bb.engine.last_kernel(), bb.engine.last_kernel()
    ref = _batched(CFG4, B, **kw)
    sep = _batched(CFG4, B, **kw)
    P = bb.engine.num_params
    rng = np.random.default_rng(9)
    for trial in range(2):
        q0 = rng.uniform(-0.5, 0.5, (B, 7))
        plans = [(rng.standard_normal((B, P)) * 0.8).astype(np.float32) for _ in range(4)]
        ep.init_pos.copy_(torch.tensor(q0)); ep.init_vel.zero_()
        for k in range(4):
            ep.params[k].copy_(torch.tensor(plans[k]))
        outs = ep.replay()
        torch.cuda.synchronize()
        got = [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs]
        ref.reset(q0); sep.reset(q0)
        n_invalid = 0
        diverged = torch.zeros(B, dtype=torch.bool, device="cuda")
        for k in range(4):
            wd_ref, wd_sep = ref.done.clone(), sep.done.clone()
            want = ref.step(plans[k])
            apart = sep.step(plans[k], fuse=False)
            for key in ("des_pos", "des_vel", "step_actions", "trajectory_length", "done", "valid", "terminated", "truncated", "invalid_penalty"):
                assert torch.equal(got[k][key], want[key]), (trial, k, key)
            # (the separate launches leave lockstep at the first invalid plan -- the host cannot know without a read-back -- and plan the
            # later steps with the per-episode-phase kernels: another kernel family, 2e-6 of the scale instead of the same bits, which
            # may flip the verdict of a plan that touches a limit to within that)
            if k == 0:
                for key in ("des_pos", "des_vel", "step_actions", "trajectory_length", "done", "valid", "terminated", "truncated"):
                    assert torch.equal(got[k][key], apart[key]), (trial, k, key, "separate launches")
                pa, pb = got[k]["invalid_penalty"].cpu().numpy(), apart["invalid_penalty"].cpu().numpy()
                assert np.all(np.abs(pa - pb) <= 1e-12 * np.abs(pb) + 1e-300), np.abs(pa - pb).max()
            # (compared on the episodes that execute this plan in both: a FINISHED episode's plan is evaluated at the batch's shared time
            # by the fused step and at its own frozen time by the separate launches -- nobody reads either)
            diverged = compare_gated_paths(want, apart, wd_ref, wd_sep, diverged, lo, hi, f"trial {trial} plan {k}")
            live = (got[k]["trajectory_length"] > 0) & (apart["trajectory_length"] > 0)
            for key in ("des_pos", "des_vel"):
                scale = float(apart[key].abs().max())
                assert float((got[k][key] - apart[key])[live].abs().max()) <= 1e-5 * scale, (trial, k, key)
            n_invalid += int((~want["valid"]).sum())
        assert 0 < n_invalid < 4 * B
        assert torch.equal(got[-1]["current_pos"], ref.q)
    bb.engine.unpin_tables()


# ---- whole episodes as one hipGraph ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("replan", [True, False])
def test_captured_episode_replays_bit_identically(replan):
    """reset + every plan of an episode captured once, replayed with new inputs: same bits as the eager calls; the basis
    tables of the four init_times are rebuilt by the graph itself (pinned slots), eager calls in between do not disturb"""
    B = 96
    kw = dict(plant="double_integrator")
    if replan:
        kw.update(replanning_every=25, max_planning_times=4, condition_on_desired=True)
    n_plans = 4 if replan else 1
    bb = _batched(CFG4 if replan else CFG2, B, **kw)
    P = bb.engine.num_params
    ep = bb.capture_episode(n_plans)
    ref = _batched(CFG4 if replan else CFG2, B, **kw)
    rng = np.random.default_rng(3)
    for trial in range(3):
        q0 = rng.uniform(-1, 1, (B, 7))
        plans = [rng.standard_normal((B, P)).astype(np.float32) for _ in range(n_plans)]
        ep.init_pos.copy_(torch.tensor(q0)); ep.init_vel.zero_()
        for k in range(n_plans):
            ep.params[k].copy_(torch.tensor(plans[k]))
        outs = ep.replay()
        torch.cuda.synchronize()
        got = [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs]
        ref.reset(q0)
        for k in range(n_plans):
            want = ref.step(plans[k])
            for key in ("des_pos", "des_vel", "step_actions", "trajectory_length", "done"):
                assert torch.equal(got[k][key], want[key]), (trial, k, key)
        # current_pos / current_vel are the plant state tensors themselves: compare after the last plan
        assert torch.equal(got[-1]["current_pos"], ref.q) and torch.equal(got[-1]["current_vel"], ref.qd)
        assert bool(got[-1]["done"].all())
        # an eager call with yet another init_time between replays must not corrupt the graph's tables
        ref.engine.trajectory(torch.tensor(plans[0], device="cuda"), torch.zeros((B, 7), device="cuda"),
                              torch.zeros((B, 7), device="cuda"), 0.02 * (trial + 1))
    bb.engine.unpin_tables()


@pytest.mark.gpu
def test_capture_episode_requirements():
    bb = _batched(CFG2, 8, plant=None)
    with pytest.raises(ValueError):
        bb.capture_episode(1)


@pytest.mark.gpu
def test_batched_invalid_plans_earn_the_penalty_and_do_not_move():
    """TableTennis-style gate (table_tennis_env.py:282-309) on the batched path: the RAW tau / delay of the action are
    checked (not the clipped ones the plan uses), invalid episodes terminate without a plant step and report the penalty"""
    from tests.test_gpu_trajectory import PER_ROW
    pc, bc, tc, dt, dur = PER_ROW["prodmp_learn_tau_delay"]
    B = 200
    lo, hi = np.full(7, -1.2), np.full(7, 1.4)
    bb = _batched((pc, bc, tc, dt, dur), B, plant="double_integrator", pos_limits=(lo, hi), check_tau_delay=True)
    rng = np.random.default_rng(4)
    params, ip, iv = inputs(pc, bc, tc, B, seed=4)
    params = params * 0.3
    params[:, 0] = rng.uniform(0.6, 1.7, B)       # tau_bound (0.8, 1.5): some outside
    params[:, 1] = rng.uniform(0.0, 0.2, B)       # delay_bound (0.05, 0.15)
    q0 = ip.astype(np.float64) * 0.3
    bb.reset(q0)
    out = bb.step(params)
    pos = out["des_pos"].cpu().numpy().astype(np.float64)
    want = (np.all((pos >= lo) & (pos <= hi), axis=(1, 2)) & (params[:, 0] >= 0.8) & (params[:, 0] <= 1.5)
            & (params[:, 1] >= 0.05) & (params[:, 1] <= 0.15))
    assert 0 < want.sum() < B
    assert np.array_equal(out["valid"].cpu().numpy(), want)
    assert np.array_equal(out["terminated"].cpu().numpy(), ~want)
    ref = O.traj_invalid_penalty(params, pos, lo, hi, (0.8, 1.5), (0.05, 0.15))
    assert np.allclose(out["invalid_penalty"].cpu().numpy(), ref, rtol=1e-12, atol=1e-15)
    n = out["trajectory_length"].cpu().numpy()
    assert np.all(n[~want] == 0) and np.all(n[want] == bb.T)
    assert np.array_equal(out["current_pos"].cpu().numpy()[~want], q0[~want])
    assert not np.array_equal(out["current_pos"].cpu().numpy()[want], q0[want])


@pytest.mark.gpu
def test_episode_search_on_the_device_reacher_improves_the_return():
    """examples/batched_reacher_search.py end to end: plan -> track -> reward -> return on the GPU, one captured graph
    per generation; cross-entropy search must find better parameters than it started with"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("batched_reacher_search",
                                                  os.path.join(os.path.dirname(GOLD), "..", "examples",
                                                               "batched_reacher_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.search(pop=512, iters=12, links=5, seed=1, verbose=False)
    best = [h[0] for h in hist]
    assert np.isfinite(best).all()
    assert best[-1] > best[0] and max(best[-3:]) > best[0] + 0.5 * abs(best[0]) * 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("verbose", [2, 1])
def test_table_tennis_example_batch_against_the_separate_launches(verbose):
    """examples/batched_table_tennis_plans.py: its BatchedBlackBox (TableTennis-ProDMP Replan constants, validity gate, one launch per plan)
    against a second instance stepped with the separate launches (fuse=False) on the same raw actions: flags, verdicts and executed
    steps equal, the plant state equal -- over the three plans of an episode"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("batched_table_tennis_plans",
                                                  os.path.join(os.path.dirname(GOLD), "..", "examples", "batched_table_tennis_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    B = 300
    a, b = mod.make_batch(B, verbose), mod.make_batch(B, 2)
    rng = np.random.default_rng(12)
    q0 = rng.uniform(-0.2, 0.2, (B, 7))
    a.reset(q0); b.reset(q0)
    P = a.engine.num_params
    seen = 0
    was_done = np.zeros(B, bool)
    for k in range(3):
        raw = (0.5 * rng.standard_normal((B, P))).astype(np.float32)
        raw[:, 0] = rng.uniform(0.7, 1.6, B); raw[:, 1] = rng.uniform(0.04, 0.16, B)
        oa, ob = a.step(raw), b.step(raw, fuse=False)
        assert a.engine.last_kernel().startswith("k_phase_fused<prodmp,pipe,closed"), a.engine.last_kernel()
        torch.cuda.synchronize()
        for key in ("done", "trajectory_length"):
            assert np.array_equal(oa[key].cpu().numpy(), ob[key].cpu().numpy()), (k, key)
        # (verdict and flags of a plan for an episode that had ALREADY finished are nobody's business -- the reference resets such an
        # episode; the two paths evaluate that plan at different times once episodes drift apart: compared where the plan counts)
        live = ~was_done
        assert live.any()
        for key in ("valid", "terminated", "truncated"):
            assert np.array_equal(oa[key].cpu().numpy()[live], ob[key].cpu().numpy()[live]), (k, key)
        assert np.array_equal(a.q.cpu().numpy(), b.q.cpu().numpy()) and np.array_equal(a.qd.cpu().numpy(), b.qd.cpu().numpy())
        seen += int(oa["terminated"].cpu().numpy()[live].sum())
        was_done = ob["done"].cpu().numpy().astype(bool)
    assert 0 < seen < B


@pytest.mark.gpu
def test_captured_episode_with_learned_phase_and_device_reward():
    """capture covers the plan+execute of a learned tau / delay configuration (one launch since round 6: k_phase_fused with its LDS
    table, > 64 KB of dynamic LDS) and the unfused reward path"""
    from tests.test_gpu_trajectory import PER_ROW
    cfg = PER_ROW["prodmp_learn_tau_delay"]
    B = 2100
    rng = np.random.default_rng(8)
    bb = _batched(cfg, B, plant="double_integrator")
    ep = bb.capture_episode(1)
    ref = _batched(cfg, B, plant="double_integrator")
    for trial in range(2):
        q0 = rng.uniform(-0.2, 0.2, (B, 7))
        params = (rng.standard_normal((B, bb.engine.num_params)) * 0.3).astype(np.float32)
        params[:, 0] = rng.uniform(0.9, 1.4, B); params[:, 1] = rng.uniform(0.06, 0.14, B)
        ep.init_pos.copy_(torch.tensor(q0)); ep.params[0].copy_(torch.tensor(params))
        got = {k: v.clone() for k, v in ep.replay()[0].items() if torch.is_tensor(v)}
        ref.reset(q0)
        want = ref.step(params)
        for key in ("des_pos", "des_vel", "step_actions", "trajectory_length", "done"):
            assert torch.equal(got[key], want[key]), (trial, key)
        assert torch.equal(bb.q, ref.q)
    assert bb.engine.last_kernel().startswith("k_phase_fused<prodmp") or bb.engine.last_kernel() == ""      # (one launch since round 6)
    # device reward (unfused step) inside a graph
    from fancy_gym_amd import _gym
    env = _gym.make("fancy_ProDMP/LongSimpleReacher-v0")
    rb = BatchedBlackBox(env.traj_gen, env.tracking_controller, 64, dt=0.01, duration=2.0, act_low=-1000.0,
                         act_high=1000.0, plant="double_integrator", reward="simple_reacher")
    rep = rb.capture_episode(1)
    rr = BatchedBlackBox(env.traj_gen, env.tracking_controller, 64, dt=0.01, duration=2.0, act_low=-1000.0,
                         act_high=1000.0, plant="double_integrator", reward="simple_reacher")
    q0 = rng.uniform(-1, 1, (64, 5)); goal = rng.uniform(-2, 2, (64, 2))
    params = rng.standard_normal((64, rb.engine.num_params)).astype(np.float32)
    rep.init_pos.copy_(torch.tensor(q0)); rep.goal.copy_(torch.tensor(goal)); rep.params[0].copy_(torch.tensor(params))
    got = rep.replay()[0]["rewards"].clone()
    rr.reset(q0, goal=goal)
    assert torch.equal(got, rr.step(params)["rewards"])


@pytest.mark.timing
@pytest.mark.gpu
def test_bench_prints_the_contract_line_last():
    """bench.py --full: the LAST stdout line is the JSON contract line, with the roofline and cpu_baseline objects"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPK_BENCH_FORCE_DIST="1")          # also walks the RCCL code path with one rank
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("MASTER_ADDR", None); env.pop("MASTER_PORT", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "40", "--warmup", "5", "--full",
                        "--cpu-seconds", "1"], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["steps"] == 40 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["scaling"] == "weak"
    assert d["unit"] == "trajectories/s" and d["value"] > 1e6 and d["vs_baseline"] is None
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert abs(d["roofline"]["achieved"] / d["roofline"]["peak"] - d["roofline"]["frac"]) < 1e-9
    assert set(d["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"} and d["cpu_baseline"]["kind"] == "port"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert "allgather" in d            # the forced one-rank RCCL path ran the collective section


def test_bench_dump_outputs_are_the_timed_steps_outputs(tmp_path):
    """bench.py --dump-outputs DIR: `--steps` timed steps, then pos / vel / act of the last one as float32 .npy, equal bit for bit
    to what TrajectoryEngine.trajectory_actions returns for the same seeded inputs; a second run writes the same files"""
    import bench
    from fancy_gym_amd import RolloutSpec, TrajectoryEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MPK_BENCH_FORCE_DIST"):
        env.pop(k, None)
    B = 512
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                            "--batch", str(B), "--no-cpu", "--no-streaming", "--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 7 and d["ms_per_step"] > 0
        assert d["dump_outputs"]["sampled"] is False
        assert d["dump_outputs"]["arrays"] == {k: [B, 100, 7] for k in ("pos", "vel", "act")}
    eng = TrajectoryEngine("prodmp", "exp", "prodmp", device=0, **bench.CFG)
    spec = RolloutSpec("motor", 7, bench.P_GAINS, bench.D_GAINS, -1.0, 1.0, plant="static")
    params, ip, iv = bench.synth_inputs(B, 0)
    want = eng.trajectory_actions(params, ip, iv, spec, ip.double(), iv.double())
    torch.cuda.synchronize()
    for name, w in zip(("pos", "vel", "act"), want):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        assert np.array_equal(a, w.cpu().numpy()), name


@pytest.mark.gpu
def test_bench_gpus_2_starts_two_ranks_itself_and_gathers_both_shards():
    """
    `python bench.py --gpus 2 --full` with no WORLD_SIZE: the parent spawns the two ranks (torch.distributed.run child, before it
    touches the GPU).  On a 1-GPU box the ranks share the device, which RCCL refuses ("duplicate GPU"), so the rehearsal
    uses gloo (MPK_BENCH_BACKEND); the driver's runs use one rank per GPU and RCCL.  Checks: n_gpus == 2, global batch
    2 B, the all-gather leg ran, every gathered slice equals its rank's shard, and the shards ARE what a single-rank
    engine produces for the per-rank seeds 1000 + r.
    """
    import bench
    from fancy_gym_amd import RolloutSpec, TrajectoryEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPK_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    B = 512
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "3",
                        "--batch", str(B), "--full", "--no-cpu"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2 * B and d["config"]["batch_per_gpu"] == B
    assert d["scaling"] == "weak" and d["steps"] == 20 and d["warmup"] == 3
    # the N-rank line is diagnosable: every rank's wall-clock sample and event-timed kernel average, `value` from the slowest
    assert len(d["per_rank_ms"]) == 2 and len(d["per_rank_kernel_avg_us"]) == 2
    assert abs(max(d["per_rank_ms"]) - d["ms_per_step"] * 20) <= 1e-6 * max(d["per_rank_ms"])
    assert d["kernel_avg_us_max"] == max(d["per_rank_kernel_avg_us"]) > 0
    assert abs(d["event_timed_value"] - 2 * B / (d["kernel_avg_us_max"] * 1e-6)) <= 1e-6 * d["event_timed_value"]
    ag = d["allgather"]
    assert ag["gathered_equals_shards"] is True and len(ag["shard_checksums"]) == 2
    assert ag["bytes_gathered_per_gpu_per_step"] == B * 2 * 100 * 7 * 4
    eng = TrajectoryEngine("prodmp", "exp", "prodmp", device=0, **bench.CFG)
    spec = RolloutSpec("motor", 7, bench.P_GAINS, bench.D_GAINS, -1.0, 1.0, plant="static")
    for rank in range(2):
        params, ip, iv = bench.synth_inputs(B, 1000 + rank)
        pos, vel, _ = eng.trajectory_actions(params, ip, iv, spec, ip.double(), iv.double())
        torch.cuda.synchronize()
        shard = torch.stack([pos, vel])
        assert int(shard.view(torch.int32).to(torch.int64).sum().item()) == ag["shard_checksums"][rank], rank


@pytest.mark.timing
@pytest.mark.gpu
def test_forced_one_rank_rccl_line_pays_nothing_the_plain_line_does_not():
    """
    The N-rank code path of bench.py --full (init_process_group("nccl"), barrier -> synchronize -> t0 -> K steps -> synchronize ->
    t1, closing barrier OUTSIDE the clock, MAX all-reduce of the elapsed time) against the plain one-process line, same
    box, the driver's `--steps 20 --warmup 5`, runs alternated, best of three each: `value` within 3 %.  Round 2's line
    had the closing RCCL barrier inside the 0.19 ms region.
    """
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MPK_BENCH_FORCE_DIST"):
        base.pop(k, None)

    def run(forced):
        env = dict(base, MPK_BENCH_FORCE_DIST="1") if forced else base
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "20", "--warmup", "5", "--full",
                            "--no-cpu", "--no-streaming"], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    plain, forced = [], []
    for _ in range(3):
        plain.append(run(False)); forced.append(run(True))
    assert all("allgather" in d for d in forced) and all("allgather" not in d for d in plain)
    vp, vf = max(d["value"] for d in plain), max(d["value"] for d in forced)
    assert abs(vf / vp - 1.0) < 0.03, (vp, vf, [d["value"] for d in plain], [d["value"] for d in forced])
    ag = forced[-1]["allgather"]
    assert ag.get("gathered_equals_shards") is True and "zero-copy" in ag["via"]


@pytest.mark.timing
def test_bench_line_carries_the_whole_contract():
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --full`: ONE JSON line on stdout, last, with every key
    the measurement contract names -- metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better /
    scaling / vs_baseline / dtype / data / config.workload, roofline {bound, achieved, peak, unit, frac, traffic} for the
    dominant kernel, cpu_baseline {value, unit, cores, kind, sample} -- and numbers that are consistent with each other"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--full"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    # value = units / time, the kernel's share of the step, the roofline arithmetic
    B = d["config"]["batch_per_gpu"]
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["kernel_avg_us"] * 1e-6) / 1e9) <= 1e-6 * rf["achieved"]
    assert rf["algorithmic_bytes_per_launch"] == B * 8624 and rf["kernel"] == "k_traj_tiles<prodmp,act>"
    assert 0.5 * rf["kernel_avg_us"] < d["ms_per_step"] * 1e3 < 3.0 * rf["kernel_avg_us"]
    assert rf["traffic"] is None or 0.9 < rf["traffic"] / rf["algorithmic_bytes_per_launch"] < 1.5
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["unit"] == d["unit"] and cb["value"] > 0
    assert cb["all_cores"]["cores"] >= 1 and cb["all_cores"]["value"] > 0
    assert 1e3 < d["value"] / cb["value"] < 1e6


@pytest.mark.timing
def test_plain_bench_line_is_the_headline_alone():
    """`python bench.py --gpus 1 --steps 20 --warmup 5` (the driver's form) does only what its headline needs: ONE JSON line
    on stdout, last, with metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
    vs_baseline / dtype / data / config and none of the legs of --full; the whole run, from process start to exit, spends
    less than 30 s outside its W + K steps.  The N-rank code path (MPK_BENCH_FORCE_DIST=1) runs no all-gather leg either."""
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MPK_BENCH_FORCE_DIST"):
        base.pop(k, None)
    for forced in (False, True):
        env = dict(base, MPK_BENCH_FORCE_DIST="1") if forced else base
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                           capture_output=True, text=True, timeout=600, env=env, cwd=root)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0]
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
            assert k in d, k
        assert not set(d) & {"roofline", "roofline_streaming", "cpu_baseline", "two_stream", "allgather", "per_rank_ms"}, sorted(d)
        assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True
        assert d["unit"] == "trajectories/s" and d["dtype"] == "f32" and d["config"]["launch"] == "hipgraph"
        assert abs(d["value"] - d["config"]["batch_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        outside = wall - (20 + 5) * d["ms_per_step"] * 1e-3
        assert outside < 30.0, (forced, wall)


def test_rccl_calls_of_the_bench_with_one_rank():
    """The torch.distributed calls bench.py makes for N > 1 -- init_process_group("nccl", device_id=...), barrier,
    all_reduce MAX of the elapsed time, all_gather_into_tensor of the (pos | vel) shard, all_gather of the int64 checksums
    -- over RCCL with world_size 1 (a gpurun box has one GPU, and RCCL refuses two ranks on one device; the two-rank
    rehearsal above runs over gloo)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "rccl_world1.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rccl world-1 ok, backend nccl" in r.stdout


def test_native_rccl_all_gather_single_rank(monkeypatch):
    """mpk_comm_* / mpk_allgather (RCCL bound lazily inside libmpk.so): one rank, out of place and in place"""
    from fancy_gym_amd.distributed import NativeComm
    monkeypatch.setenv("NCCL_DEBUG", "WARN")                  # no version banner on stdout
    comm = NativeComm(rank=0, world=1, device=0)
    shard = torch.randn((2, 5, 100, 7), device="cuda")        # (pos | vel) of 5 episodes
    out = comm.gather_trajectories(shard)
    torch.cuda.synchronize()
    assert out.shape == (1, 2, 5, 100, 7) and torch.equal(out[0], shard)
    full = torch.randn((1, 2, 5, 100, 7), device="cuda")
    keep = full.clone()
    comm.all_gather(full[0], out=full)                         # in place: send == recv + rank * count
    torch.cuda.synchronize()
    assert torch.equal(full, keep)
    with pytest.raises(ValueError):
        comm.all_gather(shard.double())
    comm.close()


def _reference_loop(cur, plan, done, every, mpt, horizon, T):
    """the step loop of black_box_wrapper.py:174-203 reduced to its integer state: steps executed by one plan"""
    if done:
        return 0, cur, plan
    plan += 1                                            # :174  self.plan_steps += 1
    n = 0
    for t in range(T):                                   # :175  for t, (pos, vel) in enumerate(zip(position, velocity))
        n += 1
        cur += 1                                         # :196,205  t + 1 + self.current_traj_steps
        if cur >= horizon:                               # the env's time limit truncates the episode
            break
        if cur % every == 0 and plan < mpt:              # :196  replanning_schedule(...) and plan_steps < max_planning_times
            break
    return n, cur, plan


@pytest.mark.parametrize("cfg", [CFG4, CFG5, CFG3], ids=["prodmp_replan", "promp", "dmp"])
@pytest.mark.parametrize("B", [1, 9, 200, 2100])
@pytest.mark.parametrize("bulk,quad", [("0", "2"), ("0", "3"), ("0", "4"), ("0", "0"), ("2", "0"), ("1", "1"), ("1", "split"),
                                       ("2", "split_em")],
                         ids=["quad", "duo", "mono", "stream", "bulk", "auto_pipe", "split", "split_and_episode_major_forced"])
def test_replan_step_equals_the_separate_kernels(cfg, B, bulk, quad, monkeypatch, mpk_option):
    """mpk_replan_step (integer state + plan + rollout + condition gather; ONE launch for shared-phase promp / prodmp,
    the separate kernels for dmp) == mpk_replan_advance -> mpk_trajectory_rollout -> mpk_condition_gather, bit for bit,
    from random per-episode integer states (finished episodes, different step counters, exhausted planning budgets)"""
    force_split = quad.startswith("split")   # the tile-major kernel with a serial role (never chosen automatically)
    if force_split:
        mpk_option("split", 1)
        if quad == "split_em":          # both forced: split wins and keeps its tile-major geometry (this combination hung
            mpk_option("mapping", 2)    # the GPU before the launcher resolved it -- found by the fuzz test)
            quad = "3"
        else:
            quad = "1"
    mpk_option("bulk", bulk)
    mpk_option("quad", quad)
    pc, bc, tc, dt, dur = cfg
    eng = make_engine(pc, bc, tc, dt, dur)
    T = eng.num_steps
    every, mpt, horizon = max(T // 4, 1), 3, T
    params, ip, iv = inputs(pc, bc, tc, B, seed=B + 3)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-1, 1, (B, 7)), rng.uniform(-0.2, 0.2, (B, 7))
    ts0 = rng.integers(0, horizon, B).astype(np.int32)
    ps0 = rng.integers(0, 4, B).astype(np.int32)
    dn0 = (rng.random(B) < 0.2).astype(np.uint8)
    spec = RolloutSpec("motor", 7, PG, DG, -0.9, 0.9, plant="double_integrator", dt=dt)

    def state():
        return (torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda"), torch.tensor(ts0, device="cuda"),
                torch.tensor(ps0, device="cuda"), torch.tensor(dn0, device="cuda"))

    q, qd, ts, ps, dn = state()
    r = eng.replan_step(params, ip, iv, spec, q, qd, ts, ps, dn, every, mpt, horizon, init_time=0.1, condition=True)
    fused = eng.last_kernel()
    if tc.trajectory_generator_type != "dmp":
        assert fused.endswith("closed>")
        # automatic selection: the producer / consumer pipeline; the split kernel needs whole float4 chunks per trajectory
        split_shape = (T * 7) % 4 == 0 and ((T - (T - 1) // 16 * 16) * 7) % 4 == 0
        if force_split:
            assert fused.startswith("k_traj_split") == split_shape and not fused.startswith("k_traj_pipe"), fused
        else:
            assert fused.startswith("k_traj_pipe") == (quad == "1"), fused
    if quad == "1":
        mpk_option("split", -1)
        mpk_option("quad", "0")      # the wave-specialised kernels against the one-wave-does-everything kernel
    q2, qd2, ts2, ps2, dn2 = state()
    seg = eng.replan_advance(ts2, ps2, dn2, every, mpt, horizon)
    p2, v2, a2 = eng.trajectory_rollout(params, ip, iv, spec, q2, qd2, n_steps=seg, init_time=0.1)
    cp, cv = eng.condition_gather(p2, v2, seg)
    torch.cuda.synchronize()
    assert torch.equal(r["seg_len"], seg) and torch.equal(ts, ts2) and torch.equal(ps, ps2) and torch.equal(dn, dn2)
    assert torch.equal(r["done"], dn2)
    assert torch.equal(r["pos"], p2) and torch.equal(r["vel"], v2) and torch.equal(r["actions"], a2)
    assert torch.equal(q, q2) and torch.equal(qd, qd2)
    assert torch.equal(r["cond_pos"], cp) and torch.equal(r["cond_vel"], cv)
    # the integer rule against the oracle, and without the optional outputs
    for b in range(min(B, 64)):
        n, cur, plan = _reference_loop(int(ts0[b]), int(ps0[b]), bool(dn0[b]), every, mpt, horizon, T)
        assert (int(seg[b]), int(ts[b]), int(ps[b]), bool(dn[b])) == (n, cur, plan, bool(dn0[b]) or cur >= horizon)
    q3, qd3, ts3, ps3, dn3 = state()
    r3 = eng.replan_step(params, ip, iv, spec, q3, qd3, ts3, ps3, dn3, every, mpt, horizon, init_time=0.1)
    assert r3["cond_pos"] is None and torch.equal(r3["actions"], a2) and torch.equal(q3, q2)


def test_replan_step_argument_checks():
    import ctypes as C
    from fancy_gym_amd import _lib
    pc, bc, tc, dt, dur = CFG4
    eng = make_engine(pc, bc, tc, dt, dur)
    B = 4
    params, ip, iv = inputs(pc, bc, tc, B, seed=0)
    spec = RolloutSpec("motor", 7, PG, DG, -1, 1, plant="static")
    z = lambda *s, dt_=torch.float64: torch.zeros(s, dtype=dt_, device="cuda")
    with pytest.raises(ValueError, match="DOUBLE_INTEGRATOR"):
        eng.replan_step(params, ip, iv, spec, z(B, 7), z(B, 7), z(B, dt_=torch.int32), z(B, dt_=torch.int32),
                        z(B, dt_=torch.uint8), 25, 4, 100)
    spec = RolloutSpec("motor", 7, PG, DG, -1, 1, plant="double_integrator", dt=dt)
    with pytest.raises(ValueError, match="every"):
        eng.replan_step(params, ip, iv, spec, z(B, 7), z(B, 7), z(B, dt_=torch.int32), z(B, dt_=torch.int32),
                        z(B, dt_=torch.uint8), 0, 4, 100)
    st = _lib.mpk_replan_state()
    assert _lib.load().mpk_replan_step(eng._h, 0, 0, 0, 0.0, C.byref(spec.c), 0, 0, C.byref(st), 0, 0, 0, B, None) == _lib.MPK_EINVAL


@pytest.mark.parametrize("B", [1, 37, 5000])
def test_episode_reset_is_one_exact_launch(B):
    """mpk_episode_reset: counters to zero, plant state copied (or zeroed), fp32 image = numpy's float32 cast"""
    pc, bc, tc, dt, dur = CFG4
    eng = make_engine(pc, bc, tc, dt, dur)
    rng = np.random.default_rng(B)
    q0, qd0 = rng.uniform(-3, 3, (B, 7)), rng.uniform(-1, 1, (B, 7))
    junk = lambda dt_, *s: torch.full(s, 7, dtype=dt_, device="cuda")
    q, qd = junk(torch.float64, B, 7), junk(torch.float64, B, 7)
    ts, ps, dn = junk(torch.int32, B), junk(torch.int32, B), junk(torch.uint8, B)
    cp, cv = junk(torch.float32, B, 7), junk(torch.float32, B, 7)
    eng.episode_reset(q, qd, ts, ps, dn, torch.tensor(q0, device="cuda"), torch.tensor(qd0, device="cuda"), cond=(cp, cv))
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy(), q0) and np.array_equal(qd.cpu().numpy(), qd0)
    assert np.array_equal(cp.cpu().numpy(), q0.astype(np.float32)) and np.array_equal(cv.cpu().numpy(), qd0.astype(np.float32))
    assert not ts.any() and not ps.any() and not dn.any()
    eng.episode_reset(q, qd, ts, ps, dn)          # no initial state: zeros; no fp32 image
    assert not q.any() and not qd.any() and np.array_equal(cp.cpu().numpy(), q0.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", [(4, 1), (4, 33), (2, 7)])
def test_metaworld_controller_for_a_frozen_state_runs_on_the_motor_kernels(D, B):
    """MetaWorldController.get_action (meta_world_controller.py:15-25) per step on the host against the device actions of
    RolloutSpec('metaworld', plant='static') -- fused with the trajectory and on an existing one; clipped like every action"""
    from fancy_gym_amd import TrajectoryEngine
    ctrl = get_controller("metaworld")
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=4,
                           dt=0.02, duration=0.5, tau=0.5)
    rng = np.random.default_rng(D * 10 + B)
    params = (rng.standard_normal((B, eng.num_params)) * 0.6).astype(np.float32)
    ip, iv = np.zeros((B, D), np.float32), np.zeros((B, D), np.float32)
    c_pos, c_vel = rng.uniform(-1, 1, (B, D)), rng.uniform(-1, 1, (B, D))
    lo, hi = -0.7, 0.9
    spec = RolloutSpec("metaworld", D, act_low=lo, act_high=hi, plant="static")
    pos, vel, act = eng.trajectory_actions(params, ip, iv, spec, c_pos, c_vel)
    dp, dv = pos.cpu().numpy(), vel.cpu().numpy()
    want = np.empty_like(dp, dtype=np.float64)
    for b in range(B):
        for t in range(dp.shape[1]):
            want[b, t] = np.clip(ctrl.get_action(dp[b, t], dv[b, t], c_pos[b], c_vel[b]), lo, hi)
    assert np.array_equal(act.cpu().numpy(), want.astype(np.float32))
    q, qd = torch.tensor(c_pos, device="cuda"), torch.tensor(c_vel, device="cuda")
    act2 = eng.pd_rollout(spec, pos, vel, q, qd)
    assert torch.equal(act2, act) and np.array_equal(q.cpu().numpy(), c_pos)      # the caller's state is untouched
    with pytest.raises(ValueError, match="no device plant"):
        RolloutSpec("metaworld", D, plant="double_integrator", dt=0.02)


# ---- the verbose < 2 step: ONE launch, nothing per step stored (mpk_episode_return, round 5) ---------------------------------------
def _reacher_bb(mp_type, B, **kw):
    """BatchedBlackBox on the generators of fancy_<MP>/LongSimpleReacher-v0 (5 links, 200 steps) with the device reward"""
    from fancy_gym_amd import _gym
    env = _gym.make(f"fancy_{mp_type}/LongSimpleReacher-v0")
    return BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=0.01, duration=2.0, act_low=-1000.0, act_high=1000.0,
                           plant="double_integrator", reward="simple_reacher", **kw), env


@pytest.mark.gpu
@pytest.mark.parametrize("mp_type", ["ProMP", "ProDMP", "DMP"])
@pytest.mark.parametrize("agg", ["sum", "mean", "last"])
@pytest.mark.parametrize("B,quad", [(5, -1), (300, 2), (300, 3), (2100, 4), (9000, -1)])
def test_verbose_1_step_is_one_launch_with_the_same_returns_and_state(mp_type, agg, B, quad, mpk_option):
    """black_box_wrapper.py:215-217 at verbose < 2: (aggregated reward, flags, trajectory_length) -- BatchedBlackBox(verbose=1) is
    mpk_episode_return: plan + controller + plant + SimpleReacher reward + aggregation in one launch that stores nothing per step.
    Against the verbose = 2 path (trajectory kernel + reward rollout + mpk_reward_aggregate): plant state, counters and the
    aggregated rewards BIT FOR BIT; the returns against the oracle's step rewards (np.sum / np.mean / last) to 1e-12."""
    mpk_option("quad", quad)
    mpk_option("tiles_wpb", 8 if B in (300, 2100) and quad != 3 else -1)       # eight-wave workgroups (automatic by the LDS they leave)
    lean, env = _reacher_bb(mp_type, B, reward_aggregation=agg, verbose=1)
    full, _ = _reacher_bb(mp_type, B, reward_aggregation=agg, verbose=2)
    rng = np.random.default_rng(B)
    q0, goal = rng.uniform(-0.5, 0.5, (B, 5)), rng.uniform(-3, 3, (B, 2))
    P = lean.engine.num_params
    params = (rng.standard_normal((B, P)) * 0.3).astype(np.float32)
    lean.reset(q0, goal=goal); full.reset(q0, goal=goal)
    a = lean.step(params)
    assert lean.engine.last_kernel().startswith("k_episode_return<") and "reacher" in lean.engine.last_kernel(), lean.engine.last_kernel()
    mpk_option("quad", -1); mpk_option("tiles_wpb", -1)
    b = full.step(params)
    assert not any(k in a for k in ("des_pos", "des_vel", "step_actions", "step_rewards")) and "step_rewards" in b
    for k in ("rewards", "trajectory_length", "done", "truncated", "terminated", "current_pos", "current_vel"):
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max())
    assert torch.equal(lean.traj_steps, full.traj_steps) and torch.equal(lean.plan_steps, full.plan_steps)
    # ... and the oracle: the reference's reward on the executed plan, aggregated by numpy
    n = min(B, 40)
    dp, dv = b["des_pos"][:n].cpu().numpy(), b["des_vel"][:n].cpu().numpy()
    pg, dg = env.tracking_controller.p_gains, env.tracking_controller.d_gains
    _, rr, rq, _ = O.reacher_rollout(dp, dv, "motor", pg, dg, -1000.0, 1000.0, 0.01, q0[:n], np.zeros((n, 5)), goal[:n])
    want = {"sum": rr.sum(axis=1), "mean": rr.mean(axis=1), "last": rr[:, -1]}[agg]
    got = a["rewards"][:n].cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-12 * (1.0 + np.abs(want))), np.abs(got - want).max()
    assert np.array_equal(a["current_pos"][:n].cpu().numpy(), rq)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [CFG2, CFG4, CFG3], ids=["cfg2", "cfg4_replan", "cfg3_dmp_response"])
@pytest.mark.parametrize("B", [9, 4096])
def test_verbose_1_episode_with_replanning_equals_the_verbose_2_episode(cfg, B):
    """four plans of 25 steps (box_pushing/mp_wrapper.py:87-91: t % 25 == 0, max_planning_times 4, condition_on_desired) through
    mpk_episode_return against mpk_replan_step: integer state, plant state and boundary conditions of every plan bit for bit; without a
    device reward the step returns no `rewards`"""
    replan = cfg is not CFG3
    kw = dict(plant="double_integrator", replanning_every=25 if replan else None, max_planning_times=4 if replan else np.inf,
              condition_on_desired=replan)
    lean, full = _batched(cfg, B, verbose=1, **kw), _batched(cfg, B, verbose=2, **kw)
    rng = np.random.default_rng(B)
    q0 = rng.uniform(-0.5, 0.5, (B, 7))
    P = lean.engine.num_params
    for episode in range(2):
        lean.reset(q0); full.reset(q0)
        for k in range(4 if replan else 1):
            params = (rng.standard_normal((B, P)) * 0.7).astype(np.float32)
            a, b = lean.step(params), full.step(params)
            assert lean.engine.last_kernel().startswith("k_episode_return<"), lean.engine.last_kernel()
            assert "rewards" not in a and "des_pos" not in a and "des_pos" in b
            for key in ("trajectory_length", "done", "truncated", "current_pos", "current_vel"):
                assert torch.equal(a[key], b[key]), (episode, k, key)
            assert torch.equal(lean.traj_steps, full.traj_steps) and torch.equal(lean.plan_steps, full.plan_steps)
            if replan:
                assert torch.equal(lean.condition_pos, full.condition_pos) and torch.equal(lean.condition_vel, full.condition_vel)
        assert bool(a["done"].all())


@pytest.mark.gpu
def test_episode_return_entry_point_without_a_replanning_state():
    """mpk_episode_return with n_steps / step0 instead of the replanning state, against trajectory_rollout + reacher_rollout +
    reward_aggregate on the same inputs; seg_out echoes the executed steps; fallbacks raise NotImplementedError"""
    from fancy_gym_amd import TrajectoryEngine
    D, T, B = 5, 200, 777
    eng = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="zero_rbf", num_dof=D, num_basis=5,
                           num_basis_zero_start=1, dt=0.01, duration=2.0, tau=2.0)
    rng = np.random.default_rng(3)
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
        assert torch.equal(r["ret"], want), (agg, (r["ret"] - want).abs().max())
        assert torch.equal(q, q2) and torch.equal(qd, qd2) and torch.equal(r["seg_len"].cpu(), n_steps)
        ref = {"sum": rew.sum(1), "mean": torch.where(n_steps.cuda() > 0, rew.sum(1) / n_steps.cuda().clamp(min=1), torch.zeros_like(rew[:, 0])),
               "last": torch.where(n_steps.cuda() > 0, rew.gather(1, (n_steps.cuda().long() - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(rew[:, 0]))}[agg]
        assert torch.allclose(want, ref, rtol=1e-13, atol=1e-13)
    # no reward: ret = 0, the state still advances
    q, qd = torch.tensor(q0, device="cuda"), torch.zeros((B, D), dtype=torch.float64, device="cuda")
    r = eng.episode_return(params, ip, iv, spec, q, qd, n_steps=n_steps)
    assert not r["ret"].any() and torch.equal(q, q2)
    # a learned tau (per-episode phase): one launch too since round 6 (k_phase_fused, no device reward) -- with a reward it is not
    eng2 = TrajectoryEngine(device=0, mp_type="promp", phase_type="linear", basis_type="rbf", num_dof=D, num_basis=5, dt=0.01,
                            duration=2.0, tau=2.0, learn_tau=True, tau_bound=(0.5, 2.0))
    p3 = np.ones((3, eng2.num_params), np.float32)
    q3, qd3 = q[:3].clone(), qd[:3].clone()
    r3 = eng2.episode_return(p3, ip[:3], iv[:3], spec, q3, qd3)
    assert eng2.last_kernel() in ("k_phase_fused<promp,closed,lean>", "k_phase_fused<promp,pipe,closed,lean>") and not r3["ret"].any()
    pos3, vel3 = eng2.trajectory(p3, ip[:3], iv[:3], 0.0)
    q4, qd4 = q[:3].clone(), qd[:3].clone()
    eng2.pd_rollout(spec, pos3, vel3, q4, qd4)
    assert torch.equal(q3, q4) and torch.equal(qd3, qd4)
    with pytest.raises(NotImplementedError):
        eng2.episode_return(p3, ip[:3], iv[:3], spec, q[:3].clone(), qd[:3].clone(), reward="simple_reacher", goal=torch.zeros(3, 2))
