"""Builds and loads tests/cpp/libmle_kernels_driver.so: one launcher per kernel of csrc/mle_kernels.hpp (and eq_weights, eval_weights,
sum_records of csrc/multifold_kernels.hpp), each grid-stride kernel with its grid as an argument, for tests/test_gpu_mle_kernels.py and
tests/test_mle_model_cpu.py.  Test infrastructure only: nothing of libzkhip is linked into it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libmle_kernels_driver.so")
INVALID = 1   # hipErrorInvalidValue
BLOCK = 256   # MLE_BLOCK
HORNER_BLOCK = 2048   # HS_T * HS_L coefficients per workgroup of the Horner scan
LAUNCHERS = ["fold", "half_sums", "finish_sums", "fold_tail", "distinct", "elementwise", "to_bytes", "repeat", "open_step", "open_steps_small",
             "open_steps_small_batch", "horner_eval", "horner_divide", "dense_degree", "circuit_layer", "wiring_ones", "eq_weights",
             "eval_weights", "sum_records"]

_lib = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libmle_kernels_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        _lib.mle_driver_grid.argtypes = [sz, i]
        _lib.mle_driver_fold.argtypes = [vp, vp, sz, u, vp, vp, vp, u, vp]
        _lib.mle_driver_half_sums.argtypes = [vp, sz, vp, u, vp]
        _lib.mle_driver_finish_sums.argtypes = [vp, u, vp, vp]
        _lib.mle_driver_fold_tail.argtypes = [vp, u, vp, u, u, vp, vp]
        _lib.mle_driver_distinct.argtypes = [i, vp, sz, vp, sz, vp, u, vp]
        _lib.mle_driver_elementwise.argtypes = [i, vp, vp, vp, sz, vp, u, vp]
        _lib.mle_driver_to_bytes.argtypes = [vp, sz, vp, u, vp]
        _lib.mle_driver_repeat.argtypes = [vp, sz, u, sz, vp, u, vp]
        _lib.mle_driver_open_step.argtypes = [vp, sz, vp, vp, vp, u, vp]
        _lib.mle_driver_open_steps_small.argtypes = [vp, u, vp, u, vp, vp, vp, vp]
        _lib.mle_driver_open_steps_small_batch.argtypes = [vp, u, u, vp, u, vp, sz, vp, sz, vp, sz, vp, vp]
        _lib.mle_driver_horner_eval.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        _lib.mle_driver_horner_divide.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
        _lib.mle_driver_dense_degree.argtypes = [vp, sz, vp, u, vp]
        _lib.mle_driver_circuit_layer.argtypes = [vp, vp, sz, vp, u, vp]
        _lib.mle_driver_wiring_ones.argtypes = [vp, sz, u, vp, vp, u, vp]
        _lib.mle_driver_eq_weights.argtypes = [vp, u, u, vp, vp]
        _lib.mle_driver_eval_weights.argtypes = [vp, u, u, u, vp, vp, vp, vp]
        _lib.mle_driver_sum_records.argtypes = [vp, u, vp, vp]
    return _lib


def library_grid(n_items, stream):
    """the grid the library launches over n_items: mle_grid_stream (stream) or the capped mle_grid"""
    return lib().mle_driver_grid(n_items, 1 if stream else 0)
