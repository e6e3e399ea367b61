"""Builds and loads tests/cpp/libdense_points_driver.so: one launcher per kernel of csrc/dense_points_kernels.hpp, each with its grid,
its segment length and its number of segments as arguments, and two wrappers for dp_pow and dp_invert, for
tests/test_gpu_dense_points_kernels.py and tests/test_dense_points_model_cpu.py.  Test infrastructure only: nothing of libzkhip is linked
into it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libdense_points_driver.so")
INVALID = 1   # hipErrorInvalidValue
LAUNCHERS = ["eval", "eval_sum", "weights", "weights_fold", "domain", "domain_fold", "pow", "invert", "constants"]

_lib = None
_constants = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libdense_points_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        _lib.dp_driver_constants.argtypes = [vp]
        _lib.dp_driver_eval.argtypes = [i, vp, sz, sz, vp, sz, sz, vp, sz, sz, u, u, u, vp]
        _lib.dp_driver_eval_sum.argtypes = [vp, u, sz, vp, sz, u, u, vp]
        _lib.dp_driver_weights.argtypes = [i, vp, sz, u, u, vp, vp, u, u, vp]
        _lib.dp_driver_weights_fold.argtypes = [vp, u, u, vp, vp, u, vp]
        _lib.dp_driver_domain.argtypes = [i, vp, sz, vp, sz, vp, sz, u, u, u, vp, vp, u, u, vp]
        _lib.dp_driver_domain_fold.argtypes = [vp, u, u, vp, u, vp]
        _lib.dp_driver_pow.argtypes = [vp, vp, u, vp, vp]
        _lib.dp_driver_invert.argtypes = [vp, u, vp, vp, vp]
    return _lib


def constants():
    """dict(lanes, chunk, max_segs, max_grid_x): DP_LANES, DP_CHUNK, DP_MAX_SEGS, DP_MAX_GRID_X of csrc/dense_points_plan.hpp"""
    global _constants
    if _constants is None:
        out = (C.c_uint32 * 4)()
        assert lib().dp_driver_constants(out) == 0
        _constants = dict(lanes=out[0], chunk=out[1], max_segs=out[2], max_grid_x=out[3])
    return _constants


def library_grid(n_points):
    """the grid_x zkhip_dense_points launches over n_points: its point blocks, capped"""
    c = constants()
    return min((n_points + c["lanes"] - 1) // c["lanes"], c["max_grid_x"])
