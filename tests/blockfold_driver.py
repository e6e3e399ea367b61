"""Builds and loads tests/cpp/libblockfold_driver.so: launchers for blockfold_kernel and blockfold_shape of csrc/multifold_kernels.hpp,
for tests/test_gpu_blockfold.py and tests/test_blockfold_driver_cpu.py.  Test infrastructure only: nothing of libzkhip is linked."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zk-cryptography_amd", "csrc")
SRC = os.path.join(CPP, "blockfold_driver.hip")
LIB_PATH = os.path.join(CPP, "libblockfold_driver.so")
# compiler, architecture and flags of tests/cpp/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
# the (m, k) the library folds with: the overlapped plan at 2^19 .. 2^24 entries, single-GPU and sharded
SHAPES = [(256, 3), (512, 3), (1024, 3), (1024, 4), (1024, 5), (1024, 6), (256, 8), (256, 9), (256, 10)]
INVALID = 1   # hipErrorInvalidValue

_lib = None


def build():
    """compiles when the library is older than the driver or a csrc header"""
    deps = [SRC] + glob.glob(os.path.join(CSRC, "*.hpp"))
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps):
        subprocess.check_call([HIPCC] + FLAGS + ["-shared", "-o", LIB_PATH, SRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, u = C.c_void_p, C.c_uint
        _lib.blockfold_driver_shape.argtypes = [u, u, C.POINTER(u)]
        _lib.blockfold_driver_run.argtypes = [vp, u, u, vp, vp, vp]
    return _lib


def shape(m, k):
    """(status, {log_ow, slices, per, ny, workgroups}) of blockfold_shape(m, k)"""
    out = (C.c_uint * 5)()
    rc = lib().blockfold_driver_shape(m, k, out)
    return rc, dict(zip(("log_ow", "slices", "per", "ny", "workgroups"), out))
