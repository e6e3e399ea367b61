"""Builds and loads tests/cpp/libntt_driver.so: one launcher per kernel of csrc/ntt_kernels.hpp, for tests/test_gpu_ntt_kernels.py.
Test infrastructure only: nothing of libzkhip is linked into it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libntt_driver.so")
LAUNCHERS = ["twiddle", "first_table", "pass_table", "first8", "pass", "first_stages", "mid_stages"]

_lib = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libntt_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        _lib.ntt_driver_twiddle.argtypes = [vp, u, vp, vp]
        _lib.ntt_driver_first_table.argtypes = [vp, u, vp, vp]
        _lib.ntt_driver_pass_table.argtypes = [vp, u, u, u, vp, i, vp, vp]
        _lib.ntt_driver_first8.argtypes = [vp, sz, vp, vp, u, vp, vp]
        _lib.ntt_driver_pass.argtypes = [vp, vp, u, u, u, vp, vp, i, sz, vp]
        _lib.ntt_driver_first_stages.argtypes = [vp, vp, u, vp, vp]
        _lib.ntt_driver_mid_stages.argtypes = [vp, u, u, u, vp, vp]
    return _lib
