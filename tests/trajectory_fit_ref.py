"""
Float64 NumPy reference of the closed-form trajectory fit (TrajectoryEngine.fit_trajectory / mpk_trajectory_fit), for the fit's tests.

For a fixed phase the oracle's trajectory is affine in the non-phase parameters:  pos_b(p) = Psi p + c_b.  Psi comes from
``oracle.mp_oracle.get_trajectory(dtype=np.float64)`` probed with unit vectors (the way tests/test_gpu_traj_vjp.py::jacobian builds J),
c_b from the same call with zero parameters and the episode's init_pos / init_vel.  A DoF reads its own block of ``params`` only, so the
fit is one small solve per (episode, DoF):

    p* = solve(Psi^T Psi + reg I, Psi^T (y - c))

``fit32`` is the same fit with float32 Psi, Gram matrix, right-hand side and solve -- what a float32 mp_pytorch would do; its
reconstruction error against ``fit64`` is the measured floor of the tests' tolerance.
"""
import numpy as np

from oracle import mp_oracle as O


class Design:
    """Psi [D, T, Kloc] float64 and the layout of ``params`` for one (configuration, grid, init_time[, tau / delay])"""

    def __init__(self, pc, bc, tc, dt, duration, init_time=0.0, phase=()):
        self.pc, self.bc, self.tc, self.dt, self.duration, self.init_time = pc, bc, tc, dt, duration, float(init_time)
        self.phase = np.asarray(phase, np.float64).reshape(-1)        # the values at the front of params (tau, delay as learned)
        self.P, self.D = O.num_params(pc, bc, tc), tc.action_dim
        self.off = int(bool(pc.learn_tau)) + int(bool(pc.learn_delay))
        assert self.phase.size == self.off
        self.Kloc = (self.P - self.off) // self.D
        assert self.off + self.D * self.Kloc == self.P
        n = self.P - self.off
        x = np.zeros((n + 1, self.P))
        x[:, :self.off] = self.phase
        x[1:, self.off:] = np.eye(n)
        z = np.zeros((n + 1, self.D))
        pos, _ = O.get_trajectory(pc, bc, tc, x, duration, dt, self.init_time, z, z, dtype=np.float64)
        J = np.moveaxis(pos[1:] - pos[0], 0, -1)                     # [T, D, n]
        self.T = J.shape[0]
        self.Psi = np.empty((self.D, self.T, self.Kloc))
        for d in range(self.D):
            blk = slice(d * self.Kloc, (d + 1) * self.Kloc)
            outside = np.delete(J[:, d, :], np.r_[blk], axis=1)
            assert not outside.any(), "a DoF's positions depend on its own parameter block only"
            self.Psi[d] = J[:, d, blk]
        self.Psi.setflags(write=False)

    def offset(self, init_pos, init_vel):
        """c [B, T, D] float64: the trajectory of zero parameters from these initial conditions"""
        B = np.shape(init_pos)[0]
        x = np.zeros((B, self.P))
        x[:, :self.off] = self.phase
        pos, _ = O.get_trajectory(self.pc, self.bc, self.tc, x, self.duration, self.dt, self.init_time,
                                  np.asarray(init_pos, np.float64), np.asarray(init_vel, np.float64), dtype=np.float64)
        return pos

    def forward(self, params, init_pos, init_vel):
        """pos [B, T, D] float64 of full parameter rows"""
        pos, _ = O.get_trajectory(self.pc, self.bc, self.tc, np.asarray(params, np.float64), self.duration, self.dt, self.init_time,
                                  np.asarray(init_pos, np.float64), np.asarray(init_vel, np.float64), dtype=np.float64)
        return pos

    def pack(self, p):
        """p [B, D, Kloc] -> params [B, P] with the phase values in front"""
        B = p.shape[0]
        out = np.empty((B, self.P), p.dtype)
        out[:, :self.off] = self.phase
        out[:, self.off:] = p.reshape(B, -1)
        return out

    def unpack(self, params):
        params = np.asarray(params)
        return params[:, self.off:].reshape(params.shape[0], self.D, self.Kloc)

    def reconstruct(self, p):
        """Psi p [B, T, D] float64 (without c)"""
        return np.einsum("dtk,bdk->btd", self.Psi, np.asarray(p, np.float64))


def fit64(design, y, c, reg):
    """p* [B, D, Kloc] float64"""
    r = np.asarray(y, np.float64) - c
    p = np.empty((r.shape[0], design.D, design.Kloc))
    for d in range(design.D):
        Psi = design.Psi[d]
        M = Psi.T @ Psi + reg * np.eye(design.Kloc)
        p[:, d] = np.linalg.solve(M, Psi.T @ r[:, :, d].T).T
    return p


def fit32(design, y, c, reg):
    """the same fit held in float32 throughout: Psi, the Gram matrix, the right-hand side and the solve"""
    r = np.asarray(y, np.float32) - c.astype(np.float32)
    p = np.empty((r.shape[0], design.D, design.Kloc), np.float32)
    for d in range(design.D):
        Psi = design.Psi[d].astype(np.float32)
        M = Psi.T @ Psi + np.float32(reg) * np.eye(design.Kloc, dtype=np.float32)
        rhs = Psi.T @ r[:, :, d].T
        try:
            sol = np.linalg.solve(M, rhs)
        except np.linalg.LinAlgError:       # exactly singular in float32: the minimum-norm float32 answer
            sol = np.linalg.lstsq(M, rhs, rcond=None)[0]
        assert sol.dtype == np.float32
        p[:, d] = sol.T
    return p


def objective(design, p, y, c, reg):
    """[B, D]: |Psi p + c - y|^2 + reg |p|^2 per (episode, DoF), float64"""
    res = design.reconstruct(p) + c - np.asarray(y, np.float64)
    return (res ** 2).sum(axis=1) + reg * (np.asarray(p, np.float64) ** 2).sum(axis=2)


def demonstrations(design, B, seed):
    """(y [B, T, D] float32, init_pos, init_vel [B, D] float32, the generating params [B, P] float32):
    forward(random params, random init) + 0.05 noise + 2.0, rounded to float32"""
    rng = np.random.default_rng(seed)
    params = rng.standard_normal((B, design.P)).astype(np.float32)
    params[:, :design.off] = design.phase
    ip = rng.uniform(-1, 1, (B, design.D)).astype(np.float32)
    iv = rng.uniform(-1, 1, (B, design.D)).astype(np.float32)
    y = design.forward(params, ip, iv) + 0.05 * rng.standard_normal((B, design.T, design.D)) + 2.0
    return y.astype(np.float32), ip, iv, params
