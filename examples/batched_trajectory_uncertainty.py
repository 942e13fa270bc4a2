#!/usr/bin/env python3
"""
What a Gaussian search distribution over movement-primitive parameters means in trajectory space, for a whole batch in one launch.

Episodic reinforcement learning over MP parameters keeps a Gaussian policy N(mean, L L^T) per context and has its Cholesky factor
(`scale_tril`) on the device.  For a fixed phase the trajectory is linear in the parameters, so the trajectory is Gaussian too and its
standard deviation at every step and DoF is the norm of the map's row times L: `TrajectoryEngine.trajectory_std` computes it on the
matrix cores without ever forming L L^T or the [B, T, D, P] intermediate (`mpk_trajectory_std`) -- what mp_pytorch's
`get_traj_pos_std` / `get_traj_vel_std` do for one distribution on the host.  Beside it, `sample_trajectories` draws parameters from
the same distributions and evaluates them in one forward launch; the spread of the samples has to fill the +-2 sigma tube.

    python examples/batched_trajectory_uncertainty.py [--envs 1024] [--samples 512] [--seed 0]

Shape: BoxPushing's ProDMP (7 DoF, 5 basis functions + goal, 100 steps).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import TrajectoryEngine  # noqa: E402


def make_engine(device=0) -> TrajectoryEngine:
    return TrajectoryEngine("prodmp", "exp", "prodmp", 7, 5, dt=0.02, duration=2.0, tau=1.5, alpha_phase=3.0,
                            basis_bandwidth_factor=2, basis_alpha=10, device=device)


def search_distributions(eng: TrajectoryEngine, envs: int, seed: int):
    """a mean and a dense lower-triangular factor per episode, as a policy head would emit them"""
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    P = eng.num_params
    mean = torch.randn((envs, P), generator=gen, device=dev)
    L = torch.tril(0.2 * torch.randn((envs, P, P), generator=gen, device=dev))
    L.diagonal(dim1=1, dim2=2).abs_().add_(0.05)
    init_pos = 2.0 * torch.rand((envs, eng.num_dof), generator=gen, device=dev) - 1.0
    init_vel = torch.zeros((envs, eng.num_dof), device=dev)
    return mean, L, init_pos, init_vel, gen


def run(envs: int = 1024, samples: int = 512, seed: int = 0, verbose: bool = True, engine: TrajectoryEngine = None):
    """returns (pos_std, the samples' empirical standard deviation, the share of sampled positions inside the +-2 sigma tube)"""
    eng = engine or make_engine()
    mean, L, init_pos, init_vel, gen = search_distributions(eng, envs, seed)
    centre = eng.trajectory(mean, init_pos, init_vel)[0]
    eng.trajectory_std(L)                                               # builds the tables of (init_time, T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pos_std, vel_std = eng.trajectory_std(L)
    torch.cuda.synchronize()
    t_std = time.perf_counter() - t0
    kernel = eng.last_kernel()
    pos, _ = eng.sample_trajectories(mean, L, init_pos, init_vel, num_samples=samples, generator=gen)
    spread = pos.std(dim=1)
    inside = float(((pos - centre[:, None]).abs() <= 2.0 * pos_std[:, None]).float().mean())
    if verbose:
        print(f"{envs} search distributions over {eng.num_params} parameters: +-2 sigma tube of {eng.num_steps} steps x {eng.num_dof} DoF "
              f"in {1e3 * t_std:.3f} ms, one launch of {kernel}")
        print("episode 0, DoF 0:   step   mean     2 sigma (trajectory_std)   2 x spread of the samples")
        for t in range(0, eng.num_steps, max(eng.num_steps // 10, 1)):
            print(f"                    {t:4d}  {float(centre[0, t, 0]):+7.3f}   {2 * float(pos_std[0, t, 0]):8.4f}"
                  f"                   {2 * float(spread[0, t, 0]):8.4f}")
        rel = float(((spread - pos_std).abs() / pos_std.clamp_min(1e-3 * float(pos_std.max()))).max())
        print(f"{samples} samples per episode: {100 * inside:.2f} % of the sampled positions lie inside the tube (a Gaussian: 95.45 %); "
              f"the samples' spread is within {100 * rel:.1f} % of trajectory_std everywhere")
    return pos_std, spread, inside


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.envs, a.samples, a.seed)
