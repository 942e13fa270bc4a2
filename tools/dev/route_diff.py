#!/usr/bin/env python3
"""
Differential check of the shared-phase route choice (plan_traj_shared / plan_episode_return, csrc/mpk_traj_launch.hip) against
another commit, without a GPU.

    tools/dev/route_diff.py [--base REV] [--work DIR] [--jobs N]

Builds tools/dev/route_stub.hip twice -- against REV's csrc (exported with `git archive`; default HEAD) and against the working
tree -- runs both sweeps (four shards each, one per MP variant), and compares the two record streams block by block (a block = one
MP variant, D, T, KP and option setting: every batch size, call kind, pointer alignment and CU count).  Blocks whose hashes differ
are dumped record by record from both builds and the differing records are counted and shown.  On the base build alone it checks the
sweep's coverage: every kernel-name literal of the base's mpk_traj_launch.hip is returned by at least one case, and the
MPK_ENOTIMPL / MPK_EINVAL exits are reached.  Exit status 0: no differing record and full coverage.
"""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STUB = os.path.join(ROOT, "tools", "dev", "route_stub.hip")
# the exits of launch_traj_shared / launch_episode_return that a sweep can reach, as the stub's summary names them
EXITS = (
    "rc=-2 err='trajectory too long for the episode-major kernel's LDS budget' name=unset",
    "rc=-2 err='' name=unset",           # a gated launch that neither k_traj_pipe nor a lane-quarter kernel takes
    "rc=-2 err='' name=set",             # a gated DMP handle
    "rc=-2 err='trajectory too long for the episode kernel's LDS budget' name=unset",
    "rc=-1 err='the validity gate belongs to the closed-loop step' name=unset",
    "rc=-1 err='internal: the episode kernel takes promp / prodmp rows' name=set",
)


def build(tree, out):
    csrc = os.path.join(tree, "fancy_gym_amd", "csrc")
    old = not os.path.exists(os.path.join(csrc, "mpk_traj_route.h"))
    # (a base from before the request struct: its launchers take argument lists)
    positional = "struct TrajRequest" not in open(os.path.join(csrc, "mpk_internal.h")).read()
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
           "-I" + os.path.join(tree, "include"), "-I" + csrc] + (["-DROUTE_OLD_ABI"] if old else []) + (["-DROUTE_POSITIONAL_CALLS"] if positional else []) + \
          [STUB, os.path.join(csrc, "mpk_traj_launch.hip"), "-o", out]
    print("[route_diff]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def sweep(binary, jobs):
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        outs = list(ex.map(lambda s: subprocess.run([binary, str(s)], check=True, capture_output=True, text=True).stdout, range(4)))
    blocks, names, exits, cases = {}, {}, {}, 0
    for out in outs:
        for line in out.splitlines():
            f = line.split("\t")
            if f[0] == "BLOCK":
                blocks[f[1]] = (int(f[2]), f[3])
            elif f[0] == "NAME":
                names[f[1]] = names.get(f[1], 0) + int(f[2])
            elif f[0] == "EXIT":
                exits[f[1]] = exits.get(f[1], 0) + int(f[2])
            elif f[0] == "CASES":
                cases += int(f[1])
    return blocks, names, exits, cases


def dump(binary, key):
    shard = ("promp", "dmp", "prodmp", "dmp_resp").index(key.split()[1])
    return subprocess.run([binary, str(shard), "--dump", key], check=True, capture_output=True, text=True).stdout.splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--work", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mpk_route_diff"))
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--show", type=int, default=5, help="differing records printed")
    a = ap.parse_args()
    base_tree = os.path.join(a.work, "base")
    os.makedirs(base_tree, exist_ok=True)
    ar = subprocess.run(["git", "-C", ROOT, "archive", a.base, "fancy_gym_amd/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", base_tree], input=ar, check=True)
    bins = {"base": os.path.join(a.work, "route_base"), "tree": os.path.join(a.work, "route_tree")}
    build(base_tree, bins["base"])
    build(ROOT, bins["tree"])
    (b_blocks, b_names, b_exits, b_cases), (t_blocks, _, _, t_cases) = sweep(bins["base"], a.jobs), sweep(bins["tree"], a.jobs)

    literals = sorted(set(re.findall(r'"(k_[a-z_]+<[^"]*>)"', open(os.path.join(base_tree, "fancy_gym_amd", "csrc", "mpk_traj_launch.hip")).read())))
    missing = [n for n in literals if n not in b_names] + [e for e in EXITS if e not in b_exits]
    differing, shown = 0, 0
    if b_cases != t_cases or set(b_blocks) != set(t_blocks):
        print(f"[route_diff] the two sweeps differ in shape: {b_cases} / {t_cases} cases, {len(b_blocks)} / {len(t_blocks)} blocks")
        differing += 1
    for key in sorted(set(b_blocks) & set(t_blocks)):
        if b_blocks[key] == t_blocks[key]:
            continue
        for lb, lt in zip(dump(bins["base"], key), dump(bins["tree"], key)):
            if lb != lt:
                differing += 1
                if shown < a.show:
                    shown += 1
                    print(f"[route_diff] {key}\n  base: {lb}\n  tree: {lt}")
    print(f"[route_diff] base {a.base}: {b_cases} cases in {len(b_blocks)} blocks")
    print(f"[route_diff] kernel names returned ({len(b_names)}; {len(literals)} literals in the base's rule): " + " ".join(sorted(b_names)))
    for e in sorted(b_exits):
        print(f"[route_diff] exit {e}: {b_exits[e]} cases")
    print(f"[route_diff] not covered: {missing if missing else 'nothing'}")
    print(f"[route_diff] differing records: {differing}")
    return 0 if differing == 0 and not missing else 1


if __name__ == "__main__":
    sys.exit(main())
