"""
NumPy restatement of the draw programs of the reacher resets (what TrajectoryEngine.reacher_reset runs per episode on the device):
SimpleReacherEnv.reset (simple_reacher.py:46-54,85-96) and HoleReacherEnv.reset (hole_reacher.py:60-71,79-101), both around
BaseReacherEnv.reset (base_reacher.py:73-93).  Seeding is gymnasium's seeding.np_random, i.e. np.random.default_rng(seed).
"""
import math

import numpy as np

M64 = (1 << 64) - 1
NAN = float("nan")


def _drawn(v) -> bool:
    return v is None or (isinstance(v, float) and math.isnan(v))


class Episode:
    """one episode of a registered-style env: kwargs as the env takes them (None or NaN = drawn); the generator lives in ``rng``"""

    def __init__(self, kind: int, n_links: int, random_start: bool = True, target=None, hole_width=None, hole_x=None,
                 hole_depth=1.0):
        self.kind, self.n = int(kind), int(n_links)
        self.random_start = bool(random_start)
        self.target = None if target is None or any(_drawn(float(t)) for t in target) else np.asarray(target, np.float64)
        self.width = None if _drawn(hole_width) else float(hole_width)
        self.x = None if _drawn(hole_x) else float(hole_x)
        self.depth = None if _drawn(hole_depth) else float(hole_depth)
        self.rng = None

    def _first_joint(self):
        q = np.zeros(self.n) if self.kind == 0 else np.hstack([[np.pi / 2], np.zeros(self.n - 1)])
        if self.random_start:
            q = np.hstack([[self.rng.uniform(np.pi / 4, 3 * np.pi / 4)], np.zeros(self.n - 1)])
        return q

    def _goal(self):
        if self.target is not None:
            return self.target.copy()
        total = float(self.n)
        goal = np.array([total, total])
        while np.linalg.norm(goal) >= total:
            goal = self.rng.uniform(low=-total, high=total, size=2)
        return goal

    def reset(self, seed=None):
        """(q0 [n], task [3]: goal x, y, NaN or hole x, width, depth)"""
        if self.kind == 0:
            if self.rng is not None:
                self._goal()                               # drawn, then overwritten (simple_reacher.py:50)
            if seed is not None:
                self.rng = np.random.default_rng(seed)
            self._first_joint()
            goal = self._goal()
            if seed is not None:
                self.rng = np.random.default_rng(seed)
            q = self._first_joint()
            return q, np.array([goal[0], goal[1], NAN])
        if seed is not None:
            self.rng = np.random.default_rng(seed)
        width = self.rng.uniform(0.15, 0.5) if self.width is None else self.width
        if self.x is None:
            direction = self.rng.choice([-1, 1])
            x = direction * self.rng.uniform(width / 2, 3.5)
        else:
            x = self.x
        depth = self.rng.uniform(1, 1) if self.depth is None else self.depth
        return self._first_joint(), np.array([x, width, depth], np.float64)

    def state_words(self):
        """(state [4] uint64: state high / low, inc high / low, has_uint32, uinteger)"""
        st = self.rng.bit_generator.state
        s, inc = st["state"]["state"], st["state"]["inc"]
        return (np.array([s >> 64, s & M64, inc >> 64, inc & M64], np.uint64), st["has_uint32"], st["uinteger"])


def fixture_episode(ref, e) -> Episode:
    """the Episode of fixture row e"""
    return Episode(int(ref["kind"][e]), int(ref["n_links"][e]), bool(ref["random_start"][e]), tuple(ref["target"][e]),
                   float(ref["hole_width"][e]), float(ref["hole_x"][e]), float(ref["hole_depth"][e]))


def run_resets(ep: Episode, seed: int, n_resets: int = 4):
    """q0 [R, n], task [R, 3], state [R, 4], has_uint32 [R], uinteger [R] for reset(seed=seed), then reset() x (R - 1)"""
    qs, tasks, states, has, u = [], [], [], [], []
    for k in range(n_resets):
        q, t = ep.reset(seed if k == 0 else None)
        s, h, v = ep.state_words()
        qs.append(q); tasks.append(t); states.append(s); has.append(h); u.append(v)
    return np.stack(qs), np.stack(tasks), np.stack(states), np.array(has, np.uint8), np.array(u, np.uint32)
