#!/usr/bin/env python3
"""
Device resets of the reacher envs (mpk_reacher_reset, k_reacher_reset) at the registered kwargs: SimpleReacher (2 links, goal drawn
by rejection) and HoleReacher (5 links, width and x drawn, depth 1), both with a random start.  "seeded" reseeds every episode
(seed_base + b), "continue" draws from the streams (SimpleReacher then runs its discarded goal draw too).  Captured graphs of 20
launches, median of rounds.  Beside them: the host samplers (sample_simple_reacher_starts, sample_hole_reacher_starts) per episode
on one core, and the rollouts each reset precedes (mpk_reacher_rollout at SimpleReacher-v0's shape with the reward; mpk_hole_reacher_
rollout on random smooth plans, returns only).
    python tools/reacher_reset_bench.py [B ...] [--host N]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fancy_gym_amd import RolloutSpec, TrajectoryEngine  # noqa: E402
from fancy_gym_amd.envs.classic_control import sample_hole_reacher_starts, sample_simple_reacher_starts  # noqa: E402
from tools.closed_bench import graph_time  # noqa: E402
from tools.hole_reacher_bench import plans  # noqa: E402

T = 200
LIM = float(np.float32(2 * np.pi))
KW = {"simple_reacher": dict(random_start=True, target=None),
      "hole_reacher": dict(random_start=True, hole_width=None, hole_x=None, hole_depth=1.0)}
LINKS = {"simple_reacher": 2, "hole_reacher": 5}


def host_rate(n):
    out = {}
    for name, fn in (("simple_reacher", sample_simple_reacher_starts), ("hole_reacher", sample_hole_reacher_starts)):
        t0 = time.perf_counter()
        fn(range(n), n_links=LINKS[name])
        out[name] = (time.perf_counter() - t0) / n
    return out


def main():
    args = sys.argv[1:]
    n_host = 20000
    if "--host" in args:
        n_host = int(args[args.index("--host") + 1])
        del args[args.index("--host"):args.index("--host") + 2]
    batches = [int(a) for a in args if a.isdigit()] or [4096, 65536, 262144]
    torch.cuda.set_device(0)
    engines = {n: TrajectoryEngine("promp", "linear", "zero_rbf", n, 5, dt=0.01, duration=2.0, tau=2.0, num_basis_zero_start=1,
                                   device=0) for n in (2, 5)}
    host = host_rate(n_host)
    print("| env | B | reset | us | ns / episode | host sampler, one core (s) | rollout it precedes (us) |")
    print("|---|---|---|---|---|---|---|")
    for B in batches:
        for env in ("simple_reacher", "hole_reacher"):
            n = LINKS[env]
            eng = engines[n]
            f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
            q, qd = torch.zeros((B, n), **f64), torch.zeros((B, n), **f64)
            ts, ps, done = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(B, dtype=torch.uint8, device="cuda")
            rng = torch.zeros((B, 5), dtype=torch.int64, device="cuda")
            task = torch.zeros((B, 2 if env == "simple_reacher" else 3), **f64)
            cond = (torch.empty((B, n), dtype=torch.float32, device="cuda"), torch.empty((B, n), dtype=torch.float32, device="cuda"))

            def reset(**seeding):
                eng.reacher_reset(env, q, qd, ts, ps, done, rng, task, cond=cond, **seeding, **KW[env])
            reset(seed_base=1000)
            torch.cuda.synchronize()
            # the rollout this reset precedes, on the episodes it drew
            if env == "simple_reacher":
                spec = RolloutSpec("motor", n, 0.6, 0.075, -1000.0, 1000.0, plant="double_integrator", dt=0.01)
                des = torch.zeros((B, T, n), dtype=torch.float32, device="cuda")
                q0 = q.clone()

                def roll():
                    q.copy_(q0); qd.zero_()
                    eng.reacher_rollout(spec, des, des, q, qd, task)
            else:
                spec = RolloutSpec("velocity", n, 1.0, 0.1, -LIM, LIM, plant="velocity_direct", dt=0.01)
                _, vel, _ = plans(B)
                vel = torch.as_tensor(vel, device="cuda")
                q0 = q.clone()

                def roll():
                    q.copy_(q0); qd.zero_()
                    eng.hole_reacher_rollout(spec, None, vel, q, qd, task, want_actions=False, want_rewards=False)
            roll_us = graph_time(roll) * 1e6
            for name, seeding in (("seeded", dict(seed_base=1000)), ("continue", {})):
                us = graph_time(lambda: reset(**seeding)) * 1e6
                print(f"| {env} | {B} | {name} | {us:.1f} | {us * 1e3 / B:.3f} | {host[env] * B:.3g} ({host[env] * 1e6:.1f} us / "
                      f"episode) | {roll_us:.1f} |", flush=True)
            reset(seed_base=1000)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(task).all())
            eng.poll_fault()


if __name__ == "__main__":
    main()
