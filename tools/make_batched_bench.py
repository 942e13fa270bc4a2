#!/usr/bin/env python3
"""
What BatchedVectorEnv adds on top of the launches it issues: host-clock time of one vector step (plan, rollout, last observation,
reset draw, first observation) at B episodes, for

  hand    the same sequence written by hand on a BatchedBlackBox built from the host env with typed constants, as the per-family test
          suites build it: ``step`` (observations=True: its ``obs`` is the last observation), ``reset(sample=True)``, ``observe()``
  vec     ``make_batched_vec(id, B).step(params)``
  graph   ``make_batched_vec(id, B).capture().replay()``

    python tools/make_batched_bench.py --variant hand|vec|graph --id fancy_ProDMP/HoleReacher-v0 [--batch 4096] [--rounds 9]
                                       [--steps 0] [--tree DIR]

``--tree DIR`` imports fancy_gym_amd from another checkout (the parent commit, for ``hand``).  Every round times ``--steps`` vector
steps (0: 40 for HoleReacher, 400 otherwise) between two device synchronisations; prints ONE JSON line with the per-step microseconds of
every round, their median, minimum and maximum.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["hand", "vec", "graph"], required=True)
    ap.add_argument("--id", required=True)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    import fancy_gym_amd
    from fancy_gym_amd import BatchedBlackBox, _gym

    assert torch.cuda.is_available(), "needs the GPU"
    hole = "HoleReacher" in a.id
    B, seed = a.batch, 1
    steps = a.steps or (40 if hole else 400)
    env = _gym.make(a.id)
    rng = np.random.default_rng(0)
    scale = np.geomspace(0.01, 2.0, B)[:, None] * (1.0 if hole else 50.0)
    params = torch.as_tensor((rng.standard_normal((B, env.action_space.shape[0])) * scale).astype(np.float32), device="cuda")

    if a.variant == "hand":
        lim = float(env.env.action_space.high[0])
        bb = BatchedBlackBox(env.traj_gen, env.tracking_controller, B, dt=0.01, duration=2.0, act_low=-lim, act_high=lim,
                             plant="velocity_direct" if hole else "double_integrator",
                             reward="hole_reacher" if hole else "simple_reacher", max_episode_steps=200, verbose=1, observations=True)
        bb.reset(seed=seed)
        bb.observe()

        def vector_step():
            out = bb.step(params)
            bb.reset(sample=True)
            return bb.observe(), out["rewards"]
    else:
        vec = fancy_gym_amd.make_batched_vec(a.id, B)
        vec.reset(seed=seed)
        if a.variant == "graph":
            graph = vec.capture()
            graph.actions.copy_(params)

            def vector_step():
                out = graph.replay()
                return out[0], out[1]
        else:
            def vector_step():
                out = vec.step(params)
                return out[0], out[1]

    for _ in range(max(steps // 4, 5)):
        vector_step()
    torch.cuda.synchronize()
    per_step = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            obs, rewards = vector_step()
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) / steps * 1e6)
    print(json.dumps(dict(variant=a.variant, id=a.id, batch=B, steps=steps, tree=os.path.abspath(a.tree),
                          us_per_step=[round(x, 1) for x in per_step], median=round(float(np.median(per_step)), 1),
                          min=round(min(per_step), 1), max=round(max(per_step), 1),
                          checksum=[float(obs.double().sum()), float(rewards.sum())])))


if __name__ == "__main__":
    main()
