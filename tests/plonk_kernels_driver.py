"""Builds and loads tests/cpp/libplonk_kernels_driver.so: one launcher per kernel of csrc/plonk_kernels.hpp, for
tests/test_gpu_plonk_kernels.py.  Test infrastructure only: nothing of libzkhip is linked into it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libplonk_kernels_driver.so")
LAUNCHERS = ["powers", "scale_pad", "blind", "gp_ratio", "gp_top", "gp_apply", "quotient", "split", "linearise"]

_lib = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libplonk_kernels_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
        _lib.plonk_driver_stream_grid.argtypes = [sz]
        _lib.plonk_driver_powers.argtypes = [vp, vp, sz, vp, u, vp]
        _lib.plonk_driver_scale_pad.argtypes = [vp, vp, sz, sz, vp, u, vp]
        _lib.plonk_driver_blind.argtypes = [vp, sz, u, vp, vp]
        _lib.plonk_driver_gp_ratio.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp]
        _lib.plonk_driver_gp_top.argtypes = [vp, u, vp, vp]
        _lib.plonk_driver_gp_apply.argtypes = [vp, vp, sz, vp, vp, vp]
        _lib.plonk_driver_quotient.argtypes = [vp, vp, sz, u, vp, vp, vp, u, vp]
        _lib.plonk_driver_split.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, u, vp]
        _lib.plonk_driver_linearise.argtypes = [vp, vp, vp, sz, vp, u, vp]
    return _lib
