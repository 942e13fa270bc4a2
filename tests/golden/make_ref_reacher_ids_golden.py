#!/usr/bin/env python3
"""
Reference-generated fixture for the SETTINGS of the nine reacher MP ids (build container only: reads the reference checkout, `REF` of make_ref_config_golden.py).

With the `ast` technique of make_ref_config_golden.py (its helpers are imported, nothing of the package is, no reference text is stored):

  * registrations   the `register(id=..., entry_point=..., mp_wrapper=..., max_episode_steps=..., kwargs={...})` calls of
                    fancy_gym/envs/__init__.py for fancy/SimpleReacher-v0, fancy/LongSimpleReacher-v0, fancy/HoleReacher-v0: literal
                    arguments, the names of entry point and MP wrapper resolved to their files through the module's imports
  * `mp_config`     the class attribute of each MP wrapper, and per MP type the merge of bb_env_constructor (registry.py:284-292) with
                    the reference's own `_BB_DEFAULTS` and `nested_update`
  * env facts       `_dt` (base_reacher.py), `max_torque` / `max_vel` (base_reacher_torque.py / base_reacher_direct.py, evaluated with
                    numpy only), `steps_before_reward` (HoleReacher: the step its simple reward compares
                    `env._steps` with), and the literal defaults of the env constructors

Output: tests/golden/ref_reacher_ids.json; tests/test_batched_make_host.py compares `resolve_batched_config` with it.

    python tests/golden/make_ref_reacher_ids_golden.py [--check]      (--check: regenerate in memory and compare with the committed file)
"""
import ast
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_config_golden as G  # noqa: E402

OUT = os.path.join(HERE, "ref_reacher_ids.json")
INIT = "envs/__init__.py"
BASE_IDS = ("fancy/SimpleReacher-v0", "fancy/LongSimpleReacher-v0", "fancy/HoleReacher-v0")
MP_TYPES = ("ProMP", "DMP", "ProDMP")
# the files that hold an env class's plant constants: (file, attribute) of dt and of the action bound
PLANT_FACTS = {"SimpleReacherEnv": ("envs/classic_control/base_reacher/base_reacher_torque.py", "max_torque"),
               "HoleReacherEnv": ("envs/classic_control/base_reacher/base_reacher_direct.py", "max_vel")}
DT_AT = ("envs/classic_control/base_reacher/base_reacher.py", "_dt")


def imports(rel):
    """local name -> (file of the module, name there) for the `from .x.y import A as B` statements of package file `rel`"""
    out = {}
    pkg = os.path.dirname(rel)
    for node in G.tree(rel).body:
        if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module:
            path = os.path.join(pkg, *node.module.split("."))
            mod = path + ".py" if os.path.exists(os.path.join(G.REF, path + ".py")) else os.path.join(path, "__init__.py")
            for a in node.names:
                out[a.asname or a.name] = (mod, a.name)
    return out


def resolve(rel, name):
    """follow re-exports until the file that defines class `name`"""
    for _ in range(4):
        if any(isinstance(n, ast.ClassDef) and n.name == name for n in G.tree(rel).body):
            return rel, name
        rel, name = imports(rel)[name]
    raise KeyError(name)


def registrations():
    names = imports(INIT)
    out = {}
    for node in ast.walk(G.tree(INIT)):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "register"):
            continue
        kw = {k.arg: k.value for k in node.keywords}
        if not isinstance(kw.get("id"), ast.Constant) or kw["id"].value not in BASE_IDS:
            continue
        env_file, env_cls = resolve(*names[kw["entry_point"].id])
        wrap_file, wrap_cls = resolve(*names[kw["mp_wrapper"].id])
        out[kw["id"].value] = dict(entry_point=env_cls, entry_point_at=env_file, mp_wrapper=wrap_cls, mp_wrapper_at=wrap_file,
                                   max_episode_steps=ast.literal_eval(kw["max_episode_steps"]), kwargs=ast.literal_eval(kw["kwargs"]),
                                   at=f"{INIT}:{node.lineno}")
    assert set(out) == set(BASE_IDS), sorted(out)
    return out


def attribute(rel, name):
    """the value `self.<name> = <expression>` gives in file `rel`, evaluated with numpy only"""
    found = []
    for node in ast.walk(G.tree(rel)):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Attribute) and t.attr == name for t in node.targets):
            found.append((eval(compile(ast.Expression(node.value), f"{rel}:{name}", "eval"), {"np": np, "__builtins__": {}}), node.lineno))
    assert len(found) == 1, (rel, name, found)
    return float(found[0][0]), f"{rel}:{found[0][1]}"


def reward_step(rel):
    """the step the reward functions of HoleReacher compare `env._steps` with (`env._steps == <int>`)"""
    found = {(n.comparators[0].value, n.lineno) for n in ast.walk(G.tree(rel))
             if isinstance(n, ast.Compare) and isinstance(n.left, ast.Attribute) and n.left.attr == "_steps"
             and len(n.ops) == 1 and isinstance(n.ops[0], ast.Eq) and isinstance(n.comparators[0], ast.Constant)}
    assert len({v for v, _ in found}) == 1, (rel, found)
    value, line = sorted(found)[0]
    return value, f"{rel}:{line}"


def init_defaults(rel, cls):
    """the literal defaults of `cls.__init__`"""
    for node in G.tree(rel).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name == "__init__":
                    args = item.args.args
                    return {a.arg: ast.literal_eval(d) for a, d in zip(args[len(args) - len(item.args.defaults):], item.args.defaults)}
    raise KeyError((rel, cls))


def build():
    defaults, nested_update = G.bb_defaults_and_nested_update()
    dt, dt_at = attribute(*DT_AT)
    out = {"base": {}, "ids": {}}
    for base_id, reg in registrations().items():
        bound_file, bound_name = PLANT_FACTS[reg["entry_point"]]
        bound, bound_at = attribute(bound_file, bound_name)
        sbr, sbr_at = (G.one(reg["entry_point_at"], "steps_before_reward") if reg["entry_point"] == "SimpleReacherEnv"
                       else reward_step("envs/classic_control/hole_reacher/hr_simple_reward.py"))
        out["base"][base_id] = dict(reg, dt=dt, dt_at=dt_at, action_bound=bound, action_bound_name=bound_name, action_bound_at=bound_at,
                                    steps_before_reward=sbr, steps_before_reward_at=sbr_at,
                                    init_defaults=init_defaults(reg["entry_point_at"], reg["entry_point"]),
                                    duration=dt * reg["max_episode_steps"])
        mp_config = G.class_mp_config(reg["mp_wrapper_at"], reg["mp_wrapper"])
        for mp_type in MP_TYPES:
            # bb_env_constructor, registry.py:284-292 (these ids register no override)
            active = copy.deepcopy(mp_config.get(mp_type, {}))
            inherit = active.pop("inherit_defaults", mp_config.get("inherit_defaults", True))
            config = copy.deepcopy(defaults[mp_type]) if inherit else {}
            nested_update(config, active)
            nested_update(config, {})
            nested_update(config, {})
            ns, name = base_id.split("/")
            out["ids"][f"{ns}_{mp_type}/{name}"] = dict(base_id=base_id, mp_type=mp_type, mp_config=G.jsonable(mp_config.get(mp_type, {})),
                                                        config=G.jsonable(config))
    out["sha256"] = dict(sorted(G._read.items()))
    out["provenance"] = ("generated by tests/golden/make_ref_reacher_ids_golden.py from the reference's files with ast (no import of the "
                         "package): literal register() arguments, mp_config class attributes, the reference's _BB_DEFAULTS and "
                         "nested_update, merge order of bb_env_constructor; numpy " + np.__version__)
    return out


def main():
    text = json.dumps(build(), indent=1, sort_keys=True) + "\n"
    if "--check" in sys.argv:
        with open(OUT) as f:
            old = json.load(f)
        new = json.loads(text)
        old.pop("provenance", None); new.pop("provenance", None)
        assert old == new, "committed fixture differs from the reference"
        print("ref_reacher_ids.json matches the reference")
        return
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT, len(text), "bytes")


if __name__ == "__main__":
    main()
