"""
Trajectory generators with the MPInterface surface ``BlackBoxWrapper`` calls
(reference black_box_wrapper.py:57,62-65,102,106,113-118,124-125,226):
``set_duration, set_params, set_initial_conditions, get_traj_pos, get_traj_vel, get_params_bounds, reset`` and the
attributes ``phase_gn, basis_gn, learn_tau, tau, num_params``.

The arithmetic is NOT here: ``get_traj_pos / get_traj_vel`` launch the HIP kernels through ``TrajectoryEngine``
(created lazily, so configuration objects can be built and inspected on a machine without a GPU).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .basis import BasisGenerator, ProDMPBasisGenerator, ZeroPaddingNormalizedRBFBasisGenerator


class MPInterface:
    mp_type = "abstract"

    def __init__(self, basis_gn: BasisGenerator, num_dof: int, weights_scale: float = 1.0, device=None, **kwargs):
        self.basis_gn = basis_gn
        self.phase_gn = basis_gn.phase_generator
        self.num_dof = int(num_dof)
        self.weights_scale = float(weights_scale)
        self._device = device
        self._engine = None
        self._engine_key = None
        self.duration: Optional[float] = None
        self.dt: Optional[float] = None
        self.reset()

    # ---- configuration -------------------------------------------------------------------------------------------
    @property
    def learn_tau(self) -> bool:
        return self.phase_gn.learn_tau

    @property
    def learn_delay(self) -> bool:
        return self.phase_gn.learn_delay

    @property
    def tau(self) -> torch.Tensor:
        return self.phase_gn.tau

    @property
    def num_basis(self) -> int:
        return self.basis_gn.num_basis

    @property
    def _num_local_params(self) -> int:
        return self.num_basis * self.num_dof

    @property
    def num_params(self) -> int:
        return self._num_local_params + self.basis_gn.num_params

    def get_params_bounds(self) -> torch.Tensor:
        """[2, P]: tau / delay bounds, everything else +-inf (reference black_box_wrapper.py:122-127 unpacks the two
        rows and calls ``.numpy()`` on each)."""
        pb = self.basis_gn.get_params_bounds()
        local = np.empty((2, self._num_local_params), np.float32)
        local[0], local[1] = -np.inf, np.inf
        return torch.from_numpy(np.concatenate([pb, local], axis=1).astype(np.float32))

    def _engine_extra(self) -> dict:
        return {}

    def engine(self):
        """The TrajectoryEngine for the current (duration, dt); built on first use."""
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before a trajectory can be generated")
        from ..engine import TrajectoryEngine
        if self._engine is None:
            pg = self.phase_gn
            kw = dict(mp_type=self.mp_type, phase_type=pg.type_name, num_dof=self.num_dof, dt=self.dt,
                      duration=self.duration, tau=pg._tau0, delay=pg._delay0,
                      alpha_phase=getattr(pg, "alpha_phase", 3.0), learn_tau=pg.learn_tau, learn_delay=pg.learn_delay,
                      tau_bound=getattr(pg, "tau_bound", (1e-5, float("inf"))),
                      delay_bound=getattr(pg, "delay_bound", (0.0, float("inf"))),
                      weights_scale=self.weights_scale, device=self._device)
            kw.update(self.basis_gn.engine_kwargs())
            kw.update(self._engine_extra())
            self._engine = TrajectoryEngine(**kw)
        else:
            self._engine.set_duration(self.duration, self.dt)
        return self._engine

    # ---- per-episode state ---------------------------------------------------------------------------------------
    def reset(self):
        self.basis_gn.reset()
        self.params = None
        self.init_time = None
        self.init_pos = None
        self.init_vel = None
        self.params_L = None
        self._clear()

    def _clear(self):
        self._pos = None
        self._vel = None
        self._pos_std = None
        self._vel_std = None

    def set_duration(self, duration: Optional[float], dt: float, include_init_time: bool = False):
        if include_init_time:
            raise NotImplementedError("include_init_time=True is not used by the black-box path")
        dt = float(dt)
        if duration is None:
            # sub-trajectory mode (reference black_box_wrapper.py:98-102): the plan lasts round(tau / dt) steps
            duration = round(float(self.phase_gn._tau) / dt) * dt
        self.duration, self.dt = float(duration), dt
        self._clear()

    def set_params(self, params) -> np.ndarray:
        params = np.asarray(params, dtype=np.float32)
        assert params.shape[-1] == self.num_params, \
            f"expected {self.num_params} parameters, got {params.shape[-1]}"
        rest = self.basis_gn.set_params(params)
        self.params = np.ascontiguousarray(rest[..., :self._num_local_params])
        self._clear()
        return rest[..., self._num_local_params:]

    def set_initial_conditions(self, init_time, init_pos, init_vel, **_ignored):
        self.init_time = float(np.asarray(init_time, dtype=np.float32))
        self.init_pos = np.asarray(init_pos, dtype=np.float32).reshape(-1)
        self.init_vel = np.asarray(init_vel, dtype=np.float32).reshape(-1)
        self._clear()

    def _full_params(self) -> np.ndarray:
        """[tau?, delay?, local...] with the (possibly frozen) phase parameters in front."""
        head = []
        if self.phase_gn.learn_tau:
            head.append(self.phase_gn._tau)
        if self.phase_gn.learn_delay:
            head.append(self.phase_gn._delay)
        return np.concatenate([np.asarray(head, np.float32), self.params.reshape(-1)]).astype(np.float32)

    def _compute(self):
        assert self.params is not None, "set_params() first"
        D = self.num_dof
        ip = self.init_pos if self.init_pos is not None else np.zeros(D, np.float32)
        iv = self.init_vel if self.init_vel is not None else np.zeros(D, np.float32)
        it = self.init_time if self.init_time is not None else 0.0
        eng = self.engine()
        if D == 0:
            z = torch.zeros((eng.num_steps, 0), dtype=torch.float32)
            self._pos, self._vel = z, z.clone()
            return
        # one episode: pinned staging in, one launch, (pos | vel) back in one copy -> CPU tensors, which is also what
        # mp_pytorch hands to fancy_gym's get_numpy on its default device
        self._pos, self._vel = eng.trajectory_host(self._full_params(), ip, iv, it)

    def show_scaled_basis(self, plot: bool = False):
        """
        mp_pytorch's inspection helper the reference's examples call (fancy_gym/examples/mp_params_tuning.py:7): the basis
        functions times their parameter scale on 1000 times from ``delay - tau`` to ``delay + 2 tau``, evaluated by the
        device row functions (mpk_scaled_basis).  Returns ``(times [1000], basis [1000, K])`` as numpy arrays; ``plot=True``
        additionally draws them with matplotlib as upstream does.
        """
        tau, delay = float(self.phase_gn._tau0), float(self.phase_gn._delay0)
        times = np.linspace(delay - tau, delay + 2 * tau, 1000, dtype=np.float32)
        if self.duration is None:
            self.set_duration(tau, 0.01)          # any grid: the basis is evaluated at `times`, not on the plan's grid
        basis = self.engine().scaled_basis(times)
        if plot:  # pragma: no cover - needs a display
            import matplotlib.pyplot as plt
            plt.figure()
            for i in range(basis.shape[-1]):
                plt.plot(times, basis[:, i], label=f"w_basis_{i}")
            plt.grid(); plt.legend()
            plt.axvline(x=delay, linestyle="--", color="k", alpha=0.3)
            plt.axvline(x=delay + tau, linestyle="--", color="k", alpha=0.3)
            plt.show()
        return times, basis

    def learn_mp_params_from_trajs(self, times, trajs, reg: float = 1e-9, **kwargs) -> dict:
        """
        mp_pytorch's regularised least-squares fit of the parameters to demonstrated position trajectories, on the device
        (``TrajectoryEngine.fit_trajectory``: one launch for the whole batch).  ``times`` [..., N], ``trajs`` [..., N, D]; returns
        ``{"params", "init_time", "init_pos", "init_vel"}`` and, for a single demonstration, sets them on the generator as upstream
        does.  ``init_time`` / ``init_pos`` / ``init_vel`` come from ``kwargs`` when all three are given; otherwise ``init_time`` is
        ``times[..., 0]``, ``init_pos`` the first sample and ``init_vel`` the first finite difference.  The signature and that
        defaulting rule are written from recollection of mp_pytorch 0.1.x and, like the rest of the MP arithmetic, are not pinned
        against it.

        The fit is ``argmin_p |Psi p + c - trajs|^2 + reg |p|^2`` per DoF, ``reg`` absolute and > 0, on the handle's own time grid:
        the T steps of ``set_duration`` start one ``dt`` after ``init_time``.  With the three given, ``times`` must be that grid
        (N = T).  With the defaults the first sample IS the initial condition, so N = T + 1 and ``times[..., 1:]`` must be the grid of
        ``init_time = times[..., 0]``; the fit runs on the samples behind the first.  Any other grid is a ValueError: the fit inverts
        the map of that grid only.  One ``init_time`` is shared by the batch.  ProMP, ProDMP and a shared-phase DMP; a generator that
        learns tau / delay has no shared phase (ValueError: ``TrajectoryEngine.fit_trajectory`` takes them as ``phase_params``).
        """
        from .._lib import load as _lib_load
        reg = float(reg)
        if not (reg > 0.0) or not np.isfinite(reg):
            raise ValueError(f"learn_mp_params_from_trajs: reg must be a positive finite number, got {reg!r}")
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before parameters can be fitted")
        if self.learn_tau or self.learn_delay:
            raise ValueError("learn_mp_params_from_trajs: this generator learns tau / delay, so the batch has no shared phase; pass each "
                             "episode's values as phase_params to TrajectoryEngine.fit_trajectory")

        def to_np(x):
            return x.detach().cpu().numpy().astype(np.float32) if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)
        times = to_np(times)
        D = self.num_dof
        tshape = tuple(trajs.shape) if hasattr(trajs, "shape") else np.shape(trajs)
        if len(tshape) < 2 or tshape[-1] != D or tuple(times.shape) != tshape[:-1]:
            raise ValueError(f"learn_mp_params_from_trajs: trajs must be [..., T, {D}] and times [..., T], got {tshape} and "
                             f"{tuple(times.shape)}")
        given = all(kwargs.get(k) is not None for k in ("init_time", "init_pos", "init_vel"))
        N, batch = tshape[-2], tshape[:-2]
        lib = _lib_load()
        T = lib.mpk_host_times(float(self.duration), float(self.dt), None, 0)
        if N != T + (0 if given else 1):
            raise ValueError(f"learn_mp_params_from_trajs: the handle's time grid has {T} steps (duration {self.duration}, dt {self.dt}); "
                             + (f"with init_time / init_pos / init_vel given trajs needs {T} samples" if given else
                                f"without them the first sample is the initial condition and trajs needs {T + 1} samples") + f", got {N}")
        grid = np.empty(T, np.float32)
        lib.mpk_host_times(float(self.duration), float(self.dt), grid.ctypes.data, T)
        flat_t = times.reshape(-1, N)
        it = to_np(kwargs["init_time"]).reshape(-1) if given else flat_t[:, 0]
        if not np.all(it == it[0]):
            raise ValueError("learn_mp_params_from_trajs: one init_time is shared by the batch; got different values")
        it0 = np.float32(it[0])
        on_grid = flat_t if given else flat_t[:, 1:]
        if not np.allclose(on_grid, grid[None] + it0, rtol=0.0, atol=1e-3 * float(self.dt)):
            raise ValueError("learn_mp_params_from_trajs: times is not the handle's own grid for this init_time "
                             f"(linspace(0, {self.duration}, {T + 1})[1:] + {float(it0)}): the fit inverts the map of that grid only")
        if isinstance(trajs, torch.Tensor):
            y = trajs.detach().to(torch.float32).reshape(-1, N, D)
        else:
            y = torch.from_numpy(np.ascontiguousarray(np.asarray(trajs, np.float32).reshape(-1, N, D)))
        B = y.shape[0]
        if given:
            ip = torch.from_numpy(to_np(kwargs["init_pos"]).reshape(-1, D)).expand(B, D)
            iv = torch.from_numpy(to_np(kwargs["init_vel"]).reshape(-1, D)).expand(B, D)
        else:
            ip = y[:, 0, :].cpu()
            iv = ((y[:, 1, :] - y[:, 0, :]) / float(flat_t[0, 1] - flat_t[0, 0])).cpu()
            y = y[:, 1:, :]
        eng = self.engine()
        params = eng.fit_trajectory(y.to(eng.device), ip.to(eng.device), iv.to(eng.device), float(it0), reg=reg)
        out = {"params": params.reshape(*batch, -1), "init_time": torch.full(batch, float(it0)),
               "init_pos": ip.reshape(*batch, D).clone(), "init_vel": iv.reshape(*batch, D).clone()}
        if B == 1:
            self.set_params(params[0].cpu().numpy())
            self.set_initial_conditions(float(it0), ip[0].numpy(), iv[0].numpy())
        return out

    def get_traj_pos(self, **_ignored) -> torch.Tensor:
        if self._pos is None:
            self._compute()
        return self._pos

    def get_traj_vel(self, **_ignored) -> torch.Tensor:
        if self._vel is None:
            self._compute()
        return self._vel

    # ---- the probabilistic half (mp_pytorch's ProbabilisticMPInterface, ProMP / ProDMP; recollected from 0.1.x, unpinned) -------
    def set_mp_params_variances(self, params_L):
        """``params_L`` [Pl, Pl]: the lower-triangular Cholesky factor of the covariance of the Pl non-phase parameters, in the
        order ``set_params`` takes them.  None forgets it, as ``reset()`` does."""
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        if params_L is not None:
            if isinstance(params_L, torch.Tensor):
                params_L = params_L.detach().cpu().numpy()
            params_L = np.asarray(params_L, dtype=np.float32)
            Pl = self._num_local_params
            if params_L.shape == (1, Pl, Pl):
                params_L = params_L[0]
            if params_L.shape != (Pl, Pl):
                raise ValueError(f"params_L must be [{Pl}, {Pl}], got {params_L.shape}")
            params_L = np.ascontiguousarray(params_L)
        self.params_L = params_L
        self._clear()

    def _compute_std(self):
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        it = self.init_time if self.init_time is not None else 0.0
        pos_std, vel_std = self.engine().trajectory_std(self.params_L[None], it)
        # one episode, CPU tensors: what get_traj_pos hands out
        self._pos_std, self._vel_std = pos_std[0].cpu(), vel_std[0].cpu()

    def get_traj_pos_std(self, **_ignored) -> torch.Tensor:
        """[T, D]: the standard deviation of ``get_traj_pos`` under ``N(params, L L^T)`` (``TrajectoryEngine.trajectory_std``)"""
        if self._pos_std is None:
            self._compute_std()
        return self._pos_std

    def get_traj_vel_std(self, **_ignored) -> torch.Tensor:
        if self._vel_std is None:
            self._compute_std()
        return self._vel_std

    def _observations_on_grid(self, fn, times, pos, std, vel, vel_std):
        """what ``condition_on_observations`` and ``log_prob_of_observations`` hand to the engine: the observation times mapped to steps
        of the current grid (ascending; a time that is no step, or two at one step: ValueError), the rows reordered with them and
        broadcast to [1, M, D], and the stored initial conditions: (steps, pos, std, vel, vel_std, init_pos, init_vel, init_time)"""
        from .._lib import load as _lib_load

        def to_np(x):
            return x.detach().cpu().numpy().astype(np.float32) if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)
        times = np.atleast_1d(to_np(times))
        if times.ndim != 1 or times.size < 1:
            raise ValueError(f"{fn}: times must be [M] with M >= 1, got {times.shape}")
        M, D = times.size, self.num_dof
        lib = _lib_load()
        T = lib.mpk_host_times(float(self.duration), float(self.dt), None, 0)
        grid = np.empty(T, np.float32)
        lib.mpk_host_times(float(self.duration), float(self.dt), grid.ctypes.data, T)
        it = np.float32(self.init_time if self.init_time is not None else 0.0)
        grid = grid + it
        steps = np.abs(grid[None, :] - times[:, None]).argmin(axis=1)
        off = np.abs(grid[steps] - times)
        if not (off <= 1e-3 * float(self.dt)).all():
            bad = int(np.argmax(off))
            raise ValueError(f"{fn}: time {float(times[bad])} is no step of the grid (init_time {float(it)} + "
                             f"linspace(0, {self.duration}, {T + 1})[1:]; the nearest step is {float(grid[steps[bad]])})")
        order = np.argsort(steps, kind="stable")
        steps = steps[order]
        if (np.diff(steps) == 0).any():
            raise ValueError(f"{fn}: two observations at the same time; give each step once")

        def rows(x, name, full):
            if x is None:
                return None
            x = to_np(x)
            if full and x.shape != (M, D):
                raise ValueError(f"{fn}: {name} must be [{M}, {D}], got {x.shape}")
            if x.ndim == 1 and x.shape[0] == M:
                x = x[:, None]
            try:
                x = np.broadcast_to(x, (M, D))
            except ValueError:
                raise ValueError(f"{fn}: {name} does not broadcast to [{M}, {D}], got {x.shape}") from None
            return np.ascontiguousarray(x[order])[None]
        if pos is None and vel is None:
            raise ValueError(f"{fn}: pos and vel are both None: nothing is observed")
        if (pos is None) != (std is None) or (vel is None) != (vel_std is None):
            raise ValueError(f"{fn}: observed values and their standard deviations come in pairs (pos with std, "
                             "vel with vel_std)")
        yp, sp = rows(pos, "pos", True), rows(std, "std", False)
        yv, sv = rows(vel, "vel", True), rows(vel_std, "vel_std", False)
        ip = self.init_pos if self.init_pos is not None else np.zeros(D, np.float32)
        iv = self.init_vel if self.init_vel is not None else np.zeros(D, np.float32)
        return [int(s) for s in steps], yp, sp, yv, sv, ip[None], iv[None], float(it)

    def condition_on_observations(self, times, pos, std, vel=None, vel_std=None):
        """
        Condition the stored Gaussian ``N(params, L L^T)`` on observed points (``TrajectoryEngine.condition``: the ProMP operation,
        for a ProDMP with a shared phase too) and REPLACE the stored mean and factor by the posterior, so that ``get_traj_pos``,
        ``get_traj_pos_std`` and ``sample_trajectories`` see it.  ``times`` [M]: the observation times, each a step of the current
        grid (``init_time + linspace(0, duration, T + 1)[1:]``; any order, no duplicates; a time that is no step of the grid is a
        ValueError -- the kernel observes the grid's own steps).  ``pos`` [M, D] with ``std`` (a scalar, [M] or [M, D]; ``inf`` skips an
        entry, 0 is exact), and / or ``vel`` [M, D] with ``vel_std``; ``pos=None`` observes velocities only.  Returns
        ``(params, params_L)`` as stored.  Needs ``set_params`` and ``set_mp_params_variances`` first.
        """
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        assert self.params is not None, "set_params() first"
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before observations can be placed on its grid")
        if self.learn_tau or self.learn_delay:
            raise NotImplementedError("condition_on_observations: this generator learns tau / delay, so the grid's phase is not shared; "
                                      "only shared-phase generators have a conditioning kernel")
        steps, yp, sp, yv, sv, ip, iv, it = self._observations_on_grid("condition_on_observations", times, pos, std, vel, vel_std)
        mean, L = self.engine().condition(self.params.reshape(1, -1), self.params_L[None], steps, yp, sp, ip, iv, it, obs_vel=yv,
                                          obs_vel_std=sv)
        self.params = np.ascontiguousarray(mean[0].cpu().numpy().reshape(self.params.shape))
        self.params_L = np.ascontiguousarray(L[0].cpu().numpy())
        self._clear()
        return self.params, self.params_L

    def log_prob_of_observations(self, times, pos, std, vel=None, vel_std=None) -> float:
        """
        The log-likelihood of observed points under the stored Gaussian ``N(params, L L^T)`` plus observation noise
        (``TrajectoryEngine.trajectory_log_prob``, one launch), a float.  The arguments are ``condition_on_observations``'s, with its
        mapping of times to steps of the current grid; nothing stored changes.  At most 64 scalar observations (times x DoF, twice
        that with velocities).  Needs ``set_params`` and ``set_mp_params_variances`` first.
        """
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        assert self.params is not None, "set_params() first"
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before observations can be placed on its grid")
        if self.learn_tau or self.learn_delay:
            raise NotImplementedError("log_prob_of_observations: this generator learns tau / delay, so the grid's phase is not shared; "
                                      "only shared-phase generators have a likelihood kernel")
        steps, yp, sp, yv, sv, ip, iv, it = self._observations_on_grid("log_prob_of_observations", times, pos, std, vel, vel_std)
        lp = self.engine().trajectory_log_prob(self.params.reshape(1, -1), self.params_L[None], steps, yp, sp, ip, iv, it, obs_vel=yv,
                                               obs_vel_std=sv)
        return float(lp[0])

    def _given_timing_row(self, fn, phase_params):
        """what the point-wise ``_given_timing`` methods hand to the engine as ``params`` [1, P] after their common refusals: the stored
        ``[tau?, delay?, mean]`` row, its front replaced by ``phase_params`` [1, n_phase] (or [n_phase]) where given -- as
        ``log_prob_of_trajectories_given_timing`` takes them, for the one movement these methods look at"""
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        assert self.params is not None, "set_params() first"
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before the grid's steps exist")
        if not (self.learn_tau or self.learn_delay):
            raise ValueError(f"{fn}: this generator learns neither tau nor delay: the movement has its phase already; call "
                             "without _given_timing")
        row = np.array(self._full_params(), np.float32)[None]
        if phase_params is not None:
            ph = phase_params.detach().cpu().numpy() if isinstance(phase_params, torch.Tensor) else np.asarray(phase_params)
            n_phase = row.shape[1] - self.params.size
            if ph.shape == (n_phase,):
                ph = ph[None]
            if ph.shape != (1, n_phase):
                raise ValueError(f"{fn}: phase_params must be [1, {n_phase}] (the movement's tau / delay), got {ph.shape}")
            row[:, :n_phase] = np.asarray(ph, np.float32)
        return row

    def condition_on_observations_given_timing(self, times, pos, std, vel=None, vel_std=None, phase_params=None):
        """
        ``condition_on_observations`` for a generator that learns tau / delay (``TrajectoryEngine.condition_given_timing``, one
        launch): the via-points are observed at the tau / delay of ``phase_params`` [1, n_phase] -- a new movement's own speed -- or,
        without ``phase_params``, at the stored tau / delay.  The stored Gaussian is over the non-phase parameters; its mean and factor
        are REPLACED by the posterior, the stored tau / delay stay.  Returns ``(params, params_L)`` as stored.
        """
        fn = "condition_on_observations_given_timing"
        row = self._given_timing_row(fn, phase_params)                                                         # (refusals before the engine)
        steps, yp, sp, yv, sv, ip, iv, it = self._observations_on_grid(fn, times, pos, std, vel, vel_std)
        mean, L = self.engine().condition_given_timing(row, self.params_L[None], steps, yp, sp, ip, iv, it, obs_vel=yv, obs_vel_std=sv)
        n_phase = row.shape[1] - self.params.size
        self.params = np.ascontiguousarray(mean[0, n_phase:].cpu().numpy().reshape(self.params.shape))
        self.params_L = np.ascontiguousarray(L[0].cpu().numpy())
        self._clear()
        return self.params, self.params_L

    def log_prob_of_observations_given_timing(self, times, pos, std, vel=None, vel_std=None, phase_params=None) -> float:
        """
        ``log_prob_of_observations`` for a generator that learns tau / delay (``TrajectoryEngine.trajectory_log_prob_given_timing``,
        one launch), a float: the points are scored at the tau / delay of ``phase_params`` [1, n_phase] or, without it, at the stored
        ones.  Nothing stored changes.
        """
        fn = "log_prob_of_observations_given_timing"
        row = self._given_timing_row(fn, phase_params)                                                         # (refusals before the engine)
        steps, yp, sp, yv, sv, ip, iv, it = self._observations_on_grid(fn, times, pos, std, vel, vel_std)
        lp = self.engine().trajectory_log_prob_given_timing(row, self.params_L[None], steps, yp, sp, ip, iv, it, obs_vel=yv,
                                                            obs_vel_std=sv)
        return float(lp[0])

    def _std_given_timing(self, fn, phase_params):
        row = self._given_timing_row(fn, phase_params)                                                         # (refusals before the engine)
        it = self.init_time if self.init_time is not None else 0.0
        pos_std, vel_std = self.engine().trajectory_std_given_timing(row, self.params_L[None], it)
        return pos_std[0].cpu(), vel_std[0].cpu()

    def get_traj_pos_std_given_timing(self, phase_params=None) -> torch.Tensor:
        """[T, D]: ``get_traj_pos_std`` for a generator that learns tau / delay (``TrajectoryEngine.trajectory_std_given_timing``), at
        the tau / delay of ``phase_params`` [1, n_phase] or, without it, at the stored ones"""
        return self._std_given_timing("get_traj_pos_std_given_timing", phase_params)[0]

    def get_traj_vel_std_given_timing(self, phase_params=None) -> torch.Tensor:
        return self._std_given_timing("get_traj_vel_std_given_timing", phase_params)[1]

    def _demonstrations_on_grid(self, fn, kernel, pos, std, timing=None, phase_params=None):
        """what ``log_prob_of_trajectories`` and ``condition_on_trajectories`` hand to the engine after their common refusals: the stored
        mean and factor repeated per demonstration, ``pos`` as float32 [N, T, D], ``std``, the initial conditions repeated, init_time.
        ``timing`` not None: the rows are ``[tau?, delay?, mean]`` -- the stored tau / delay, or row n of ``phase_params`` [N, n_phase]"""
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        assert self.params is not None, "set_params() first"
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        if self.duration is None or self.dt is None:
            raise RuntimeError("set_duration(duration, dt) must be called before demonstrations can be placed on its grid")
        if (self.learn_tau or self.learn_delay) and timing is None:
            raise NotImplementedError(f"{fn}: this generator learns tau / delay, so the grid's phase is not shared; "
                                      f"only shared-phase generators have {kernel}")
        if timing is not None and not (self.learn_tau or self.learn_delay):
            raise ValueError(f"{fn}: this generator learns neither tau nor delay: every demonstration has its phase already; call "
                             "without _given_timing")
        D = self.num_dof
        y = pos.detach().cpu().numpy() if isinstance(pos, torch.Tensor) else np.asarray(pos)
        y = np.asarray(y, np.float32)
        if y.ndim == 2:
            y = y[None]
        if y.ndim != 3 or y.shape[2] != D:
            raise ValueError(f"{fn}: pos must be [N, T, {D}] or [T, {D}], got {y.shape}")
        N = y.shape[0]
        sd = std.detach().cpu().numpy() if isinstance(std, torch.Tensor) else np.asarray(std)
        sd = np.asarray(sd, np.float32)
        ip = self.init_pos if self.init_pos is not None else np.zeros(D, np.float32)
        iv = self.init_vel if self.init_vel is not None else np.zeros(D, np.float32)
        it = self.init_time if self.init_time is not None else 0.0
        rows = np.repeat(self.params.reshape(1, -1), N, 0)
        if timing is not None:
            rows = np.repeat(self._full_params()[None], N, 0)
            if phase_params is not None:
                ph = phase_params.detach().cpu().numpy() if isinstance(phase_params, torch.Tensor) else np.asarray(phase_params)
                n_phase = rows.shape[1] - self.params.size
                if ph.shape != (N, n_phase):
                    raise ValueError(f"{fn}: phase_params must be [{N}, {n_phase}] (tau / delay per demonstration), got {ph.shape}")
                rows[:, :n_phase] = np.asarray(ph, np.float32)
        return (rows, np.repeat(self.params_L[None], N, 0), np.ascontiguousarray(y), sd,
                np.repeat(np.asarray(ip, np.float32)[None], N, 0), np.repeat(np.asarray(iv, np.float32)[None], N, 0), float(it))

    def log_prob_of_trajectories(self, pos, std) -> torch.Tensor:
        """
        The log-likelihood of whole demonstrations under the stored Gaussian ``N(params, L L^T)`` plus observation noise
        (``TrajectoryEngine.demonstration_log_prob``, one launch for all of them): ``pos`` [N, T, D] (or [T, D]: one demonstration) on
        the current grid's T steps, ``std`` a scalar, [D], [T, D] or [N, T, D] (``inf`` removes an entry: missing samples, a prefix;
        0 is not expressible here -- ``log_prob_of_observations`` takes exact observations).  Returns [N] float64 on the CPU; nothing
        stored changes.  Needs ``set_params`` and ``set_mp_params_variances`` first.  A generator that learns tau / delay refuses
        here: ``log_prob_of_trajectories_given_timing`` is its entry point.
        """
        args = self._demonstrations_on_grid("log_prob_of_trajectories", "a likelihood kernel", pos, std)      # (refusals before the engine)
        lp = self.engine().demonstration_log_prob(*args)
        return lp.detach().cpu()

    def log_prob_of_trajectories_given_timing(self, pos, std, phase_params=None) -> torch.Tensor:
        """
        ``log_prob_of_trajectories`` for a generator that learns tau / delay
        (``TrajectoryEngine.demonstration_log_prob_given_timing``, one launch): demonstration n is scored at the tau / delay of row n
        of ``phase_params`` [N, n_phase] -- demonstrations of different durations, each at its own timing -- or, without
        ``phase_params``, every one at the stored tau / delay.  The stored Gaussian is over the non-phase parameters.
        """
        args = self._demonstrations_on_grid("log_prob_of_trajectories_given_timing", "a likelihood kernel", pos, std, "given",
                                            phase_params)                                                     # (refusals before the engine)
        lp = self.engine().demonstration_log_prob_given_timing(*args)
        return lp.detach().cpu()

    def condition_on_trajectories(self, pos, std):
        """
        Condition the stored Gaussian ``N(params, L L^T)`` on whole demonstrations (``TrajectoryEngine.condition_on_demonstration``,
        one launch for all of them) WITHOUT replacing it: ``pos`` [N, T, D] (or [T, D]: one demonstration) on the current grid's T
        steps, ``std`` a scalar, [D], [T, D] or [N, T, D] (``inf`` removes an entry: missing samples; a prefix is the rest at ``inf``;
        0 is not expressible here -- ``condition_on_observations`` takes exact observations).  Returns ``(params [N, P], params_L
        [N, Pl, Pl])`` float32 on the CPU, one posterior per demonstration, each from the stored prior -- the E-step of EM over N
        demonstrations; ``set_params`` / ``set_mp_params_variances`` with row n make posterior n the stored one.  Needs ``set_params``
        and ``set_mp_params_variances`` first.  A generator that learns tau / delay refuses here:
        ``condition_on_trajectories_given_timing`` is its entry point.
        """
        args = self._demonstrations_on_grid("condition_on_trajectories", "a conditioning kernel", pos, std)    # (refusals before the engine)
        mean, L = self.engine().condition_on_demonstration(*args)
        return mean.detach().cpu(), L.detach().cpu()

    def condition_on_trajectories_given_timing(self, pos, std, phase_params=None):
        """
        ``condition_on_trajectories`` for a generator that learns tau / delay
        (``TrajectoryEngine.condition_on_demonstration_given_timing``, one launch): demonstration n is conditioned at the tau / delay
        of row n of ``phase_params`` [N, n_phase], or, without ``phase_params``, every one at the stored tau / delay.  Returns
        ``(params [N, P], params_L [N, Pl, Pl])``: the rows of ``params`` carry those timings in front, as ``set_params`` takes them.
        """
        args = self._demonstrations_on_grid("condition_on_trajectories_given_timing", "a conditioning kernel", pos, std, "given",
                                            phase_params)                                                      # (refusals before the engine)
        mean, L = self.engine().condition_on_demonstration_given_timing(*args)
        return mean.detach().cpu(), L.detach().cpu()

    def sample_trajectories(self, num_smp: int = 1, generator: Optional[torch.Generator] = None):
        """``(pos, vel)`` [num_smp, T, D]: trajectories of parameters drawn from ``N(params, L L^T)``
        (``TrajectoryEngine.sample_trajectories``), CPU tensors"""
        if self.mp_type == "dmp":
            raise NotImplementedError("a DMP has no probabilistic interface (ProMP / ProDMP only)")
        assert self.params is not None, "set_params() first"
        if self.params_L is None:
            raise RuntimeError("set_mp_params_variances(params_L) first")
        D = self.num_dof
        ip = self.init_pos if self.init_pos is not None else np.zeros(D, np.float32)
        iv = self.init_vel if self.init_vel is not None else np.zeros(D, np.float32)
        it = self.init_time if self.init_time is not None else 0.0
        pos, vel = self.engine().sample_trajectories(self._full_params()[None], self.params_L[None], ip[None], iv[None], it,
                                                     num_samples=num_smp, generator=generator)
        return pos[0].cpu(), vel[0].cpu()


class ProMP(MPInterface):
    """'promp' (factory/trajectory_generator_factory.py:11-12)"""
    mp_type = "promp"

    def __init__(self, basis_gn, num_dof, weights_scale: float = 1.0, **kwargs):
        super().__init__(basis_gn, num_dof, weights_scale, **kwargs)
        self.has_zero_padding = isinstance(basis_gn, ZeroPaddingNormalizedRBFBasisGenerator)


class DMP(MPInterface):
    """'dmp' (factory/trajectory_generator_factory.py:13-14): one extra goal parameter per DoF"""
    mp_type = "dmp"

    def __init__(self, basis_gn, num_dof, weights_scale: float = 1.0, goal_scale: float = 1.0, alpha: float = 25,
                 **kwargs):
        self.goal_scale, self.alpha = float(goal_scale), float(alpha)
        # how the first returned sample relates to the initial condition: 'init' (default) | 'step' (include/mpk.h
        # MPK_DMP_FIRST_*; SURVEY A.6 "(?)")
        self.dmp_first_sample = kwargs.pop("dmp_first_sample", "init")
        super().__init__(basis_gn, num_dof, weights_scale, **kwargs)

    @property
    def _num_local_params(self) -> int:
        return (self.num_basis + 1) * self.num_dof

    def _engine_extra(self) -> dict:
        return dict(goal_scale=self.goal_scale, dmp_alpha=self.alpha, dmp_first_sample=self.dmp_first_sample)


class ProDMP(MPInterface):
    """'prodmp' (factory/trajectory_generator_factory.py:15-18)"""
    mp_type = "prodmp"

    def __init__(self, basis_gn, num_dof, weights_scale: float = 1.0, goal_scale: float = 1.0, **kwargs):
        assert isinstance(basis_gn, ProDMPBasisGenerator)
        self.goal_scale = float(goal_scale)
        self.auto_scale_basis = bool(kwargs.pop("auto_scale_basis", False))
        self.relative_goal = bool(kwargs.pop("relative_goal", False))
        self.disable_weights = bool(kwargs.pop("disable_weights", False))
        self.disable_goal = bool(kwargs.pop("disable_goal", False))
        # the reference passes goal_offset in box_pushing/mp_wrapper.py:77 and table_tennis/mp_wrapper.py:114; in
        # mp_pytorch <= 0.1.3 it is believed to disappear into **kwargs (SURVEY A.5 (?)): goal_offset_mode 'ignore'
        # (default) accepts and drops it, 'add' adds it to the goal (include/mpk.h MPK_GOAL_OFFSET_*)
        self.goal_offset = kwargs.pop("goal_offset", None)
        self.goal_offset_mode = kwargs.pop("goal_offset_mode", "ignore")
        # relative_goal: init_pos joins the raw goal parameter ('before_scale', default since ABI 3) or the scaled goal
        # ('after_scale') -- include/mpk.h MPK_RELGOAL_*; unpinned either way
        self.relative_goal_mode = kwargs.pop("relative_goal_mode", "before_scale")
        kwargs.pop("duration", None)   # _BB_DEFAULTS['ProDMP'] carries a stray 'duration' (registry.py:108)
        super().__init__(basis_gn, num_dof, weights_scale, **kwargs)

    @property
    def _num_local_params(self) -> int:
        k = (0 if self.disable_weights else self.num_basis) + (0 if self.disable_goal else 1)
        return k * self.num_dof

    def _engine_extra(self) -> dict:
        return dict(goal_scale=self.goal_scale, auto_scale_basis=self.auto_scale_basis,
                    relative_goal=self.relative_goal, disable_goal=self.disable_goal,
                    disable_weights=self.disable_weights, relative_goal_mode=self.relative_goal_mode,
                    goal_offset_mode=self.goal_offset_mode, goal_offset=float(self.goal_offset or 0.0))
