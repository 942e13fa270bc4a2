"""mpk_reacher_autoreset without a GPU: include/mpk.h, the ctypes table and the built library agree on the appended entry point (ABI
still 4), the new kernel unit and the shared header are part of the build and of the source hash, the draw programs and the observation
row exist once, and the argument checks that need no device"""
import ctypes as C
import os
import re
import subprocess

import pytest

from fancy_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fancy_gym_amd", "csrc")


def read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def test_header_ctypes_table_and_library_agree_on_the_entry_point():
    hdr = read(ROOT, "include", "mpk.h")
    m = re.search(r"int mpk_reacher_autoreset\(([^;]*)\);", hdr)
    assert m, "include/mpk.h does not declare mpk_reacher_autoreset"
    n_args = len(m.group(1).split(","))
    res, args = _lib.SIGNATURES["mpk_reacher_autoreset"]
    assert res is C.c_int and len(args) == n_args == 19
    # appended: the last prototype of the header, behind everything ABI 4 already had; the version does not move
    assert hdr.rindex("int mpk_reacher_autoreset(") > hdr.rindex("mpk_last_kernel(")
    assert re.search(r"#define\s+MPK_ABI_VERSION\s+4\b", hdr) and _lib.MPK_ABI_VERSION == 4
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4 and hasattr(lib, "mpk_reacher_autoreset")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T mpk_\w+$", line)}
    assert exported == set(_lib.SIGNATURES), exported ^ set(_lib.SIGNATURES)


def test_unit_and_shared_header_are_built_and_hashed():
    assert "mpk_autoreset.hip" in _lib.KERNEL_UNITS and "mpk_reacher_env.h" in _lib.KERNEL_HEADERS
    hashed = {os.path.basename(p) for p in _lib.SOURCE_FILES}
    assert {"mpk_autoreset.hip", "mpk_reacher_env.h"} <= hashed
    assert '#include "mpk_autoreset.hip"' in read(CSRC, "mpk_kernels.hip")
    assert "k_reacher_autoreset" in read(CSRC, "mpk_autoreset.hip")


def test_draw_programs_and_observation_row_exist_once():
    """the three kernels share one text: the units include the header and define none of its functions themselves"""
    shared = read(CSRC, "mpk_reacher_env.h")
    for fn in ("draw_goal", "reset_episode", "obs_row", "obs_positions", "obs_task"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % fn, shared)) == 1, fn
        for unit in ("mpk_reset.hip", "mpk_obs.hip", "mpk_autoreset.hip"):
            text = read(CSRC, unit)
            assert '#include "mpk_reacher_env.h"' in text
            assert not re.search(r"__device__[^;{]*\b%s\(" % fn, text), (unit, fn)
    for unit in ("mpk_reset.hip", "mpk_autoreset.hip"):
        assert "reset_episode(" in read(CSRC, unit)
    for unit in ("mpk_obs.hip", "mpk_autoreset.hip"):
        assert "obs_row<" in read(CSRC, unit)
    assert "np_uniform" not in read(CSRC, "mpk_reset.hip") + read(CSRC, "mpk_autoreset.hip")


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    args = [None] * 16
    assert lib.mpk_reacher_autoreset(None, *args, 0, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()


def test_refused_configurations_without_a_device():
    from fancy_gym_amd.batched_make import make_batched_vec
    import inspect
    assert inspect.signature(make_batched_vec).parameters["partial_resets"].default is False
    from fancy_gym_amd import BatchedBlackBox, BatchedVectorEnv
    assert inspect.signature(BatchedVectorEnv.__init__).parameters["partial_resets"].default is False
    assert inspect.signature(BatchedBlackBox.reset).parameters["mask"].default is None
    for name in ("reset_done", "autoreset", "enable_partial_resets"):
        assert callable(getattr(BatchedBlackBox, name))
