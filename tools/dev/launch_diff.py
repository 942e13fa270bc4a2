#!/usr/bin/env python3
"""
Differential check of the rollout and learned-phase launchers (launch_pd_rollout / launch_reacher_rollout, launch_phase_fused,
launch_traj_rows) against another commit at the launch boundary, without a GPU.

    tools/dev/launch_diff.py [--base REV] [--work DIR] [--jobs N] [--quick] [--ablations] [--sanitize]

Builds tools/dev/launch_rec.hip twice -- against REV's csrc (exported with `git archive`; default HEAD) and against the working
tree, host code only -- runs both sweeps (three units x eight shards, one per DoF count) and compares the two record streams block
by block (a block = one shape and option setting: every batch size, CU count and call kind).  Blocks whose hashes differ are dumped
record by record from both builds and the differing records are counted and shown.  On the base build it checks the sweep's
coverage: every kernel-name literal of the base's three units is returned by at least one case, every kernel instantiation the
base's launchers can name is launched by at least one case, and the declining exits are reached.  Exit status 0: no differing
record and full coverage (--quick: no differing record).

--ablations   both builds with -DMPK_ABLATIONS (the helper-wave rollout kernels behind "pd_helper" 1); the rollout unit only
--sanitize    the working tree's program alone with -fsanitize=address,undefined on the --quick sweep (its own main: nothing preloaded)
"""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REC = os.path.join(ROOT, "tools", "dev", "launch_rec.hip")
UNITS = ("rollout", "fused", "rows")
UNIT_FILES = ("mpk_rollout.hip", "mpk_phase_fused.hip", "mpk_traj_phase.hip")
KERNELS = r"_ZN3mpk\d+k_(pd_rollout|reacher_rollout|phase_fused|traj_phase|traj_rows)"
# instantiations the base's launchers name and no input reaches: the reward pass caps groups per wave x episodes per group at 8, and
# two links put eight episodes in a group
UNREACHABLE = ("_ZN3mpk18k_pd_rollout_tilesILi2ELb1ELi0ELi2ELb0EEEvNS_6PdArgsE", "_ZN3mpk18k_pd_rollout_tilesILi4ELb1ELi0ELi2ELb0EEEvNS_6PdArgsE",
               "_ZN3mpk18k_pd_rollout_tilesILi2ELb1ELi0ELi2ELb1EEEvNS_6PdArgsE", "_ZN3mpk18k_pd_rollout_tilesILi4ELb1ELi0ELi2ELb1EEEvNS_6PdArgsE")
# the declining exits of the three launchers, as the program's summary names them (regular expressions)
EXITS = (
    r"rc=-2 err='' name=unset",                                       # phase_fused_capable, the LDS overflow (both launchers), need > 16, D * KS > 256, the missing rows32
    r"rc=-1 err='the validity gate needs the double-integrator plant' name=unset",
    r"rc=-1 err='promp needs at least two time steps for the finite-difference velocity' name=unset",
    r"rc=-1 err='trajectory too large for the per-episode kernel's LDS budget' name=",
    # launch_traj_phase's own exits end in k_traj_rows: the program counts them by the shape that causes them
    r"k_traj_phase declined: need > 16", r"k_traj_phase declined: D \* KS > 256", r"k_traj_phase declined: rows32 missing",
    r"k_traj_phase declined: LDS overflow",
)


def build(tree, out, extra):
    csrc = os.path.join(tree, "fancy_gym_amd", "csrc")
    # (a base from before the request struct: its launchers take argument lists)
    if "struct TrajRequest" not in open(os.path.join(csrc, "mpk_internal.h")).read():
        extra = extra + ["-DLAUNCH_POSITIONAL_CALLS"]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17",
           "-ffp-contract=off", "-rdynamic", "-Wl,--unresolved-symbols=ignore-all", "-I" + os.path.join(tree, "include"), "-I" + csrc] + \
          extra + [REC, "-o", out, "-ldl"]
    print("[launch_diff]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def sweep(binary, units, jobs, quick):
    work = [(u, s) for u in units for s in range(8)]
    run = lambda w: subprocess.run([binary, w[0], str(w[1])] + (["--quick"] if quick else []), check=True, capture_output=True, text=True).stdout
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        outs = list(ex.map(run, work))
    blocks, sums, cases = {}, {"NAME": {}, "EXIT": {}, "SYM": {}}, 0
    for out in outs:
        for line in out.splitlines():
            f = line.split("\t")
            if f[0] == "BLOCK":
                blocks[f[1]] = (int(f[2]), f[3])
            elif f[0] in sums:
                sums[f[0]][f[1]] = sums[f[0]].get(f[1], 0) + int(f[2])
            elif f[0] == "CASES":
                cases += int(f[1])
    return blocks, sums, cases


def dump(binary, key):
    shard = (1, 2, 5, 7, 8, 16, 17, 64) if not key.startswith("rollout") else (1, 2, 3, 5, 7, 8, 16, 17)
    d = int(re.search(r" D=(\d+) ", key).group(1))
    return subprocess.run([binary, key.split()[0], str(shard.index(d)), "--dump", key], check=True, capture_output=True, text=True).stdout.splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--work", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mpk_launch_diff"))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--show", type=int, default=5, help="differing records printed")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ablations", action="store_true")
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.sanitize:
        binary = os.path.join(a.work, "launch_rec_san")
        build(ROOT, binary, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"])
        _, _, cases = sweep(binary, UNITS, a.jobs, True)
        print(f"[launch_diff] sanitized sweep: {cases} cases, clean")
        return 0
    base_tree = os.path.join(a.work, "base")
    os.makedirs(base_tree, exist_ok=True)
    ar = subprocess.run(["git", "-C", ROOT, "archive", a.base, "fancy_gym_amd/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", base_tree], input=ar, check=True)
    extra = ["-DMPK_ABLATIONS"] if a.ablations else []
    units = UNITS[:1] if a.ablations else UNITS
    tag = "_abl" if a.ablations else ""
    bins = {"base": os.path.join(a.work, "launch_rec_base" + tag), "tree": os.path.join(a.work, "launch_rec_tree" + tag)}
    build(base_tree, bins["base"], extra)
    build(ROOT, bins["tree"], extra)
    (b_blocks, b_sums, b_cases), (t_blocks, _, t_cases) = sweep(bins["base"], units, a.jobs, a.quick), sweep(bins["tree"], units, a.jobs, a.quick)

    literals = set()
    for f in UNIT_FILES[:len(units)]:
        literals |= set(re.findall(r'"(k_[a-z_]+<[^"]*>)"', open(os.path.join(base_tree, "fancy_gym_amd", "csrc", f)).read()))
    nm = subprocess.run(["nm", "--defined-only", bins["base"]], check=True, capture_output=True, text=True).stdout
    nameable = sorted({l.split()[-1] for l in nm.splitlines() if re.match(KERNELS, l.split()[-1])
                       and (not a.ablations or "rollout" in l.split()[-1])})
    missing = [n for n in sorted(literals) if n not in b_sums["NAME"]] + [k for k in nameable if k not in b_sums["SYM"] and k not in UNREACHABLE]
    if a.quick:
        missing = []            # (the reduced sweep leaves shapes out: it compares, the full sweep also checks its coverage)
    elif not a.ablations:
        missing += [e for e in EXITS if not any(re.match(e, x) for x in b_sums["EXIT"])]
    differing, shown = 0, 0
    if b_cases != t_cases or set(b_blocks) != set(t_blocks):
        print(f"[launch_diff] the two sweeps differ in shape: {b_cases} / {t_cases} cases, {len(b_blocks)} / {len(t_blocks)} blocks")
        differing += 1
    for key in sorted(set(b_blocks) & set(t_blocks)):
        if b_blocks[key] == t_blocks[key]:
            continue
        for lb, lt in zip(dump(bins["base"], key), dump(bins["tree"], key)):
            if lb != lt:
                differing += 1
                if shown < a.show:
                    shown += 1
                    print(f"[launch_diff] {key}\n  base: {lb}\n  tree: {lt}")
    print(f"[launch_diff] base {a.base}: {b_cases} cases in {len(b_blocks)} blocks")
    print(f"[launch_diff] kernel names returned ({len(b_sums['NAME'])}; {len(literals)} literals in the base's units): " + " ".join(sorted(b_sums["NAME"])))
    print(f"[launch_diff] kernel instantiations launched: {len(b_sums['SYM'])} of the {len(nameable)} the base's launchers can name "
          f"({len([k for k in nameable if k in UNREACHABLE])} of them reached by no input)")
    for e in sorted(b_sums["EXIT"]):
        print(f"[launch_diff] exit {e}: {b_sums['EXIT'][e]} cases")
    print(f"[launch_diff] not covered: {missing if missing else 'nothing'}")
    print(f"[launch_diff] differing records: {differing}")
    return 0 if differing == 0 and not missing else 1


if __name__ == "__main__":
    sys.exit(main())
