"""Builds and loads tests/cpp/libarith_driver.so: one launcher per primitive of the arithmetic layer (fp.hpp, fqu.hpp, g1u.hpp,
wide_acc.hpp, the reductions, mfma_fold.hpp), for tests/test_gpu_arith.py.  Test infrastructure only: nothing of libzkhip is linked
into it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libarith_driver.so")
LAUNCHERS = ["fp", "fqu", "g1u", "wide_mac", "wide_redc", "reduce", "mfma_fold", "mfma_fold_wsum"]

# operation numbers: the enums of arith_driver.hip
FP_OPS = ["add", "sub", "mul", "sqr", "neg", "dbl", "to_mont", "from_mont"]
FQU_OPS = ["from_ark", "to_ark", "mul", "weak_norm", "strong_norm", "sub4", "sub8", "sub16", "sub8_dbl", "is_zero"]
G1U_OPS = ["double_affine", "double", "madd", "madd_neg", "add", "add_quad"]
RED_OPS = ["wave", "wave2", "block", "block2"]

_lib = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libarith_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        _lib.arith_driver_op_count.argtypes = [i]
        _lib.arith_driver_fp.argtypes = [i, i, vp, vp, vp, sz, vp]
        _lib.arith_driver_fqu.argtypes = [i, vp, vp, vp, sz, vp]
        _lib.arith_driver_g1u.argtypes = [i, vp, vp, vp, sz, vp]
        _lib.arith_driver_wide_mac.argtypes = [vp, vp, sz, u, vp, vp]
        _lib.arith_driver_wide_redc.argtypes = [vp, sz, vp, vp]
        _lib.arith_driver_reduce.argtypes = [i, vp, vp, vp, vp, u, u, vp]
        _lib.arith_driver_mfma_fold.argtypes = [vp, sz, u, vp, vp, vp, u, vp]
        _lib.arith_driver_mfma_fold_wsum.argtypes = [vp, sz, u, vp, vp, u, vp, vp, u, vp]
    return _lib
