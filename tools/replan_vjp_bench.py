#!/usr/bin/env python3
"""
Backward time of a 4-plan replanning episode on the lean path (verbose < 2) at the cfg4-like shape: ProDMP, 7 DoF, T = 100, dt = 0.02,
replanning_every = 25, condition_on_desired, SimpleReacher reward on the torque plant (profiles/r17_replan_vjp.md).  One JSON line per
batch size: device events around the four forward steps and around loss.backward().

    python tools/replan_vjp_bench.py [--tree CHECKOUT] [--option episode] [--B 4096 65536] [--rounds 30] [--warmup 8] [--label NAME]

--tree: the checkout whose fancy_gym_amd is imported (default: this one; an export of another commit with its own libmpk.so for an A/B
run in one session); --option: ``replan_gradient`` (checkouts that have it).
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--option", default=None)
ap.add_argument("--B", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--label", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fancy_gym_amd  # noqa: E402
from fancy_gym_amd import BatchedBlackBox  # noqa: E402
from fancy_gym_amd.black_box.factory import (get_basis_generator, get_controller, get_phase_generator,  # noqa: E402
                                             get_trajectory_generator)

assert os.path.abspath(fancy_gym_amd.__file__).startswith(os.path.abspath(a.tree)), fancy_gym_amd.__file__
pg, dg = 0.01 * np.array([120., 120., 120., 120., 50., 30., 10.]), 0.01 * np.array([10., 10., 10., 10., 6., 5., 3.])
for B in a.B:
    kw = dict(plant="double_integrator", reward="simple_reacher", replanning_every=25, condition_on_desired=True, verbose=1,
              steps_before_reward=99)
    if a.option:
        kw["replan_gradient"] = a.option
    phase = get_phase_generator("exp", tau=1.5, alpha_phase=3.0)
    basis = get_basis_generator("prodmp", phase, num_basis=5, basis_bandwidth_factor=3, alpha=10)
    tg = get_trajectory_generator("prodmp", 7, basis, weights_scale=0.3, goal_scale=0.3, auto_scale_basis=True, disable_goal=True)
    bb = BatchedBlackBox(tg, get_controller("motor", p_gains=pg, d_gains=dg), B, 0.02, 2.0, act_low=-1.0, act_high=1.0, **kw)
    assert bb.T == 100
    gen = torch.Generator().manual_seed(0)
    q0 = (torch.rand((B, 7), generator=gen, dtype=torch.float64) - 0.5).cuda()
    goal = (torch.rand((B, 2), generator=gen, dtype=torch.float64) * 4 - 2).cuda()
    params = [(0.5 * torch.randn((B, bb.engine.num_params), generator=gen)).cuda().requires_grad_() for _ in range(4)]
    fwd, bwd, kernels = [], [], None
    for it in range(a.warmup + a.rounds):
        bb.reset(q0, None, goal=goal)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = 0.0
        for p in params:
            loss = loss + bb.step(p, differentiable=True)["rewards"].sum()
        fk = bb.engine.last_kernel()
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        for p in params:
            p.grad = None
        if it >= a.warmup:
            fwd.append(e[0].elapsed_time(e[1]) * 1e3)
            bwd.append(e[1].elapsed_time(e[2]) * 1e3)
        kernels = (fk, bb.engine.last_kernel())
    print(json.dumps(dict(label=a.label, option=a.option, B=B, forward_us_median=round(statistics.median(fwd), 1),
                          forward_us_min=round(min(fwd), 1), backward_us_median=round(statistics.median(bwd), 1),
                          backward_us_min=round(min(bwd), 1), kernels=kernels)), flush=True)
