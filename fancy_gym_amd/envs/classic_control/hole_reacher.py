"""
Host (NumPy) HoleReacher: a planar chain of unit links that must reach into a hole in the floor without touching it or
itself.  The single-episode counterpart of the device rollout ``TrajectoryEngine.hole_reacher_rollout`` /
``BatchedBlackBox(plant="velocity_direct", reward="hole_reacher")`` and the step-based env behind ``fancy/HoleReacher-v0``.

Behaviour follows fancy_gym/envs/classic_control (read, not copied):
  plant        direct velocity control, dt = 0.01: acc = (a - qd) / dt, qd = a, q += dt * qd
               (base_reacher/base_reacher_direct.py:20-38).  numpy's dtypes are part of the behaviour: a float32 action
               (velocity / position controller, float32 action bounds) makes qd float32, and from then on acc and dt * qd are
               float32 operations
  kinematics   unit links from the origin, angles accumulate                         base_reacher/base_reacher.py:95-103
  collisions   a joint outside [-pi, pi] or two non-adjacent links crossing (ccw with a 1e-12 margin), unless
               allow_self_collision (base_reacher.py:105-119, utils.py:1-9); any of 100 points per link left / right of the
               hole below 0 or over the hole below -depth, unless allow_wall_collision (hole_reacher/hole_reacher.py:126-179)
  reward       rew_fct (hole_reacher.py:48-58), with dist = |ee - (x, -depth)|:
               "simple"     -5e-8 sum(acc^2) every step; at step 199 or on collision also -dist^2 and -collision_penalty
                            * collided; is_success = dist < 0.005 and not collided (hole_reacher/hr_simple_reward.py:19-53)
               "vel_acc"    -1e-4 sum(qd^2) - 1e-6 sum(acc^2) every step; at step 199 only also -dist^2 - collision_penalty
                            * collided * dist^2 and is_success = dist < 0.005 and not collided.  A collision before step 199
                            ends the episode without a distance term (hr_dist_vel_acc_reward.py:20-60; collisions latch)
               "unbounded"  -5e-6 sum(acc^2) every step; the ee is stored at step 180 or on collision; at step 199 or on
                            collision also 0.25 exp(-|stored - goal|) if collided, else exp(-|stored - goal|) if the current
                            ee y > 0, else 1 - stored y; is_success = not collided there (hr_unbounded_reward.py:17-60)
  termination  terminated = collided (hole_reacher.py:76-77); the registration's TimeLimit(200) truncates
  reset        hole width ~ U(0.15, 0.5) unless given, x = +-U(width / 2, 3.5) unless given, then the first joint
               ~ U(pi/4, 3pi/4) when random_start (hole_reacher.py:79-101, base_reacher.py:73-93), in that order
"""
from typing import Optional

import numpy as np

from ... import _gym
from ...black_box.raw_interface_wrapper import RawInterfaceWrapper

STEPS_BEFORE_REWARD = 199
STEP_STORE_EE = 180             # hr_unbounded_reward.py:32
REWARD_FUNCTIONS = ("simple", "vel_acc", "unbounded")
MAX_EPISODE_STEPS = 200
POINTS_PER_LINK = 100


def draw_hole(rng: np.random.Generator, hole_width=None, hole_x=None, hole_depth=None) -> np.ndarray:
    """(x, width, depth) of one episode, drawn as the reference draws it (hole_reacher.py:79-101)"""
    width = rng.uniform(0.15, 0.5) if hole_width is None else float(hole_width)
    if hole_x is None:
        direction = rng.choice([-1, 1])
        x = direction * rng.uniform(width / 2, 3.5)
    else:
        x = float(hole_x)
    depth = rng.uniform(1, 1) if hole_depth is None else float(hole_depth)
    return np.array([x, width, depth], dtype=np.float64)


def draw_start(rng: np.random.Generator, n_links: int, random_start: bool = True) -> np.ndarray:
    """joint angles at reset: the arm straight, its first link at U(pi/4, 3pi/4) or straight up (base_reacher.py:73-93)"""
    q = np.zeros(n_links)
    q[0] = rng.uniform(np.pi / 4, 3 * np.pi / 4) if random_start else np.pi / 2
    return q


def sample_hole_reacher_starts(seeds, n_links: int = 5, random_start: bool = True, hole_width=None, hole_x=None,
                               hole_depth=1.0):
    """(init_pos [B, n_links], hole [B, 3]) for BatchedBlackBox.reset: episode b is what HoleReacherEnv.reset(seed=seeds[b])
    starts from (the defaults are fancy/HoleReacher-v0's)"""
    pos, holes = [], []
    for s in seeds:
        rng = np.random.default_rng(int(s))
        holes.append(draw_hole(rng, hole_width, hole_x, hole_depth))
        pos.append(draw_start(rng, n_links, random_start))
    return np.stack(pos), np.stack(holes)


def link_points(q: np.ndarray, num_points: int = POINTS_PER_LINK) -> np.ndarray:
    """[n_links, num_points, 2]: np.linspace(0, 1, num_points) along every link, each link starting where the last ended"""
    angles = np.cumsum(q)
    t = np.linspace(0, 1, num_points)
    px = np.cos(angles)[:, None] * t
    py = np.sin(angles)[:, None] * t
    for i in range(1, len(q)):
        px[i] = px[i] + px[i - 1, -1]
        py[i] = py[i] + py[i - 1, -1]
    return np.stack([px, py], axis=-1)


def _ccw(a, b, c) -> bool:
    return (c[1] - a[1]) * (b[0] - a[0]) - (b[1] - a[1]) * (c[0] - a[0]) > 1e-12


def _segments_cross(a, b, c, d) -> bool:
    return _ccw(a, c, d) != _ccw(b, c, d) and _ccw(a, b, c) != _ccw(a, b, d)


class HoleReacherEnv(_gym.Env):
    dt = 0.01

    def __init__(self, n_links: int, hole_x: Optional[float] = None, hole_depth: Optional[float] = None,
                 hole_width: Optional[float] = 1.0, random_start: bool = False, allow_self_collision: bool = False,
                 allow_wall_collision: bool = False, collision_penalty: float = 1000, rew_fct: str = "simple",
                 render_mode: Optional[str] = None):
        if rew_fct not in REWARD_FUNCTIONS:
            raise ValueError("Unknown reward function {}".format(rew_fct))
        self.rew_fct = rew_fct
        self.n_links = int(n_links)
        self.initial_x, self.initial_width, self.initial_depth = hole_x, hole_width, hole_depth
        self.random_start = bool(random_start)
        self.allow_self_collision = bool(allow_self_collision)
        self.allow_wall_collision = bool(allow_wall_collision)
        self.collision_penalty = collision_penalty
        self.render_mode = render_mode
        self.steps_before_reward = STEPS_BEFORE_REWARD
        bound = np.concatenate([np.full(2 * self.n_links, np.pi), np.full(self.n_links + 4, np.inf)])
        self.observation_space = _gym.spaces.Box(low=-bound, high=bound, shape=bound.shape)
        vmax = np.full(self.n_links, 2 * np.pi)
        self.action_space = _gym.spaces.Box(low=-vmax, high=vmax, shape=vmax.shape)
        self._start_pos = np.hstack([[np.pi / 2], np.zeros(self.n_links - 1)])
        self.q = self._start_pos.copy()
        self.qd = np.zeros(self.n_links)
        self.acc = np.zeros(self.n_links)
        self.hole = np.array([0.0, 1.0, 1.0])
        self.steps = 0
        self._rng = np.random.default_rng()
        self._is_collided = False       # vel_acc: the collision latch of its reward (reset with the episode)
        self._end_eff_pos = None        # unbounded: the ee of step 180 / of the collision (kept across resets, as the reference's)
        self._update_joints()

    # ---- RawInterfaceWrapper plumbing ---------------------------------------------------------------------------------
    @property
    def current_pos(self) -> np.ndarray:
        return self.q.copy()

    @property
    def current_vel(self) -> np.ndarray:
        return self.qd.copy()

    @property
    def goal(self) -> np.ndarray:
        return np.hstack([self.hole[0], -self.hole[2]])

    @property
    def end_effector(self) -> np.ndarray:
        return self.joints[-1]

    # ---- episode ---------------------------------------------------------------------------------------------------------
    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None):
        if seed is not None:
            self._rng = np.random.default_rng(seed)
        self.hole = draw_hole(self._rng, self.initial_width, self.initial_x, self.initial_depth)
        if (options or {}).get("random_start", self.random_start):
            self.q = draw_start(self._rng, self.n_links)
            self._start_pos = self.q.copy()
        else:
            self.q = self._start_pos.copy()
        self.qd = np.zeros(self.n_links)
        self.steps = 0
        self._is_collided = False
        self._update_joints()
        return self._observe(), {}

    def _update_joints(self):
        angles = np.cumsum(self.q)
        self.joints = np.zeros((self.n_links + 1, 2))
        self.joints[1:] = np.cumsum(np.stack([np.cos(angles), np.sin(angles)], axis=1), axis=0)

    def _observe(self) -> np.ndarray:
        return np.hstack([np.cos(self.q), np.sin(self.q), self.qd, self.hole[1], self.end_effector - self.goal,
                          self.steps]).astype(np.float32)

    def self_collision(self) -> bool:
        if np.any(self.q > np.pi) or np.any(self.q < -np.pi):
            return True
        j = self.joints
        return any(_segments_cross(j[i], j[i + 1], j[k], j[k + 1])
                   for i in range(self.n_links) for k in range(i + 2, self.n_links))

    def wall_collision(self) -> bool:
        pts = link_points(self.q)
        px, py = pts[..., 0], pts[..., 1]
        x, width, depth = self.hole
        left, right = x - width / 2, x + width / 2
        return bool(np.any((px < left) & (py < 0)) or np.any((px > right) & (py < 0))
                    or np.any((px > left) & (px < right) & (py < -depth)))

    def step(self, action):
        # no dtype conversion: the float32 flow of a float32 action is the reference's
        self.acc = (action - self.qd) / self.dt
        self.qd = action
        self.q = self.q + self.dt * self.qd
        self._update_joints()
        if self.rew_fct == "vel_acc":
            reward, success, collided = self._reward_vel_acc()
        elif self.rew_fct == "unbounded":
            reward, success, collided = self._reward_unbounded()
        else:
            reward, success, collided = self._reward_simple()
        self.steps += 1
        info = {"is_success": success, "is_collided": bool(collided), "end_effector": self.end_effector.copy()}
        return self._observe(), reward, bool(collided), False, info

    def _collides(self) -> bool:
        return ((not self.allow_self_collision and self.self_collision())
                or (not self.allow_wall_collision and self.wall_collision()))

    def _reward_simple(self):
        collided = self._collides()
        dist_cost, success = 0.0, False
        if self.steps == self.steps_before_reward or collided:
            dist = np.linalg.norm(self.end_effector - self.goal)
            dist_cost = dist ** 2
            success = bool(dist < 0.005 and not collided)
        acc_cost = np.sum(self.acc ** 2)
        reward = float(np.dot(np.array((dist_cost, acc_cost, float(collided))),
                              np.array((-1, -5e-8, -self.collision_penalty))))
        return reward, success, collided

    def _reward_vel_acc(self):
        if not self._is_collided:
            self._is_collided = self._collides()
            self._collision_dist = np.linalg.norm(self.end_effector - self.goal)
        dist_cost = collision_cost = 0.0
        success = False
        # the distance terms are paid at step 199 only, also after a collision (which has ended the episode before)
        if self.steps == self.steps_before_reward:
            dist = np.linalg.norm(self.end_effector - self.goal)
            success = bool(dist < 0.005 and not self._is_collided)
            dist_cost = dist ** 2
            collision_cost = self._is_collided * self._collision_dist ** 2
        vel_cost = np.sum(self.qd ** 2)
        acc_cost = np.sum(self.acc ** 2)
        reward = float(np.dot(np.array((dist_cost, vel_cost, acc_cost, collision_cost, 0.0)),
                              np.array((-1, -1e-4, -1e-6, -self.collision_penalty, 0))))
        return reward, success, self._is_collided

    def _reward_unbounded(self):
        collided = self._collides()
        if self.steps == STEP_STORE_EE or collided:
            self._end_eff_pos = self.end_effector.copy()
        dist_reward, success = 0.0, False
        if self.steps == self.steps_before_reward or collided:
            dist = np.linalg.norm(self._end_eff_pos - self.goal)
            if collided:
                dist_reward = 0.25 * np.exp(-dist)
            elif self.end_effector[1] > 0:
                dist_reward = np.exp(-dist)
            else:
                dist_reward = 1 - self._end_eff_pos[1]
            success = not collided
        acc_cost = np.sum(self.acc ** 2)
        reward = float(np.dot(np.array((dist_reward, acc_cost)), np.array((1, -5e-6))))
        return reward, success, collided


class HoleReacherMPWrapper(RawInterfaceWrapper):
    """controller / scales of fancy_gym/envs/classic_control/hole_reacher/mp_wrapper.py:9-45"""

    mp_config = {
        "ProMP": {"controller_kwargs": {"controller_type": "velocity"},
                  "trajectory_generator_kwargs": {"weights_scale": 2}},
        "DMP": {"controller_kwargs": {"controller_type": "velocity"},
                "trajectory_generator_kwargs": {"weights_scale": 500},
                "phase_generator_kwargs": {"alpha_phase": 2.5}},
        "ProDMP": {},
    }

    @property
    def context_mask(self) -> np.ndarray:
        env = self.env.unwrapped
        start = [env.random_start] * (3 * env.n_links)
        return np.array(start + [env.initial_width is None, True, True, False])

    @property
    def current_pos(self):
        return self.env.unwrapped.current_pos

    @property
    def current_vel(self):
        return self.env.unwrapped.current_vel
