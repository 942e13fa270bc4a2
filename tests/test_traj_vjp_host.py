"""mpk_trajectory_vjp without a GPU: include/mpk.h, the ctypes table and the built library agree on the appended entry point (ABI
still 4), its unit is built, hashed and part of the amalgamation, the route option exists, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

from fancy_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fancy_gym_amd", "csrc")


def read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def test_header_ctypes_table_and_library_agree_on_the_entry_point():
    hdr = read(ROOT, "include", "mpk.h")
    m = re.search(r"int mpk_trajectory_vjp\(([^;]*)\);", hdr)
    assert m, "include/mpk.h does not declare mpk_trajectory_vjp"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1] for a in args] == ["h", "g_pos", "g_vel", "init_time_shared", "g_params", "g_init_pos", "g_init_vel", "B",
                                             "stream"]
    res, argtypes = _lib.SIGNATURES["mpk_trajectory_vjp"]
    assert res is C.c_int and len(argtypes) == len(args) == 9 and argtypes[3] is C.c_double and argtypes[7] is C.c_int32
    # appended behind every earlier prototype; the version does not move
    assert hdr.rindex("int mpk_trajectory_vjp(") > hdr.rindex("int mpk_reacher_env_step(")
    assert re.search(r"#define\s+MPK_ABI_VERSION\s+4\b", hdr) and _lib.MPK_ABI_VERSION == 4
    lib = _lib.load()
    assert lib.mpk_abi_version() == 4 and hasattr(lib, "mpk_trajectory_vjp")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpk_trajectory_vjp$", out, re.M), "libmpk.so does not export mpk_trajectory_vjp"


def test_unit_is_built_hashed_and_amalgamated():
    assert "mpk_traj_vjp.hip" in _lib.KERNEL_UNITS
    assert "mpk_traj_vjp.hip" in {os.path.basename(p) for p in _lib.SOURCE_FILES}
    assert '#include "mpk_traj_vjp.hip"' in read(CSRC, "mpk_kernels.hip")


def test_route_option_and_null_handle():
    lib = _lib.load()
    assert "vjp_generic" in _lib.OPTION_KEYS and '"vjp_generic"' in read(ROOT, "include", "mpk.h")
    assert _lib.get_option("vjp_generic") == _lib.MPK_OPT_AUTO
    _lib.set_option("vjp_generic", 1)
    assert _lib.get_option("vjp_generic") == 1
    _lib.set_option("vjp_generic")
    assert lib.mpk_trajectory_vjp(None, None, None, 0.0, None, None, None, 1, None) == _lib.MPK_EINVAL
    assert "NULL handle" in _lib.last_error()
