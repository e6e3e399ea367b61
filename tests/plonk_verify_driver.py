"""Builds and loads tests/cpp/libplonk_verify_driver.so: launchers for the kernels of csrc/plonk_verify_kernels.hpp, for
tests/test_gpu_plonk_verify_kernels.py.  Test infrastructure only: nothing of libzkhip is linked into it.  The rule is this module's
own: compiler, flags and architecture are those of csrc/Makefile, and the library is rebuilt when the driver or a csrc header is newer."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zk-cryptography_amd", "csrc")
SRC = os.path.join(CPP, "plonk_verify_driver.hip")
LIB_PATH = os.path.join(CPP, "libplonk_verify_driver.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]

_lib = None


def build(extra_flags=()):
    deps = [SRC] + glob.glob(os.path.join(CSRC, "*.hpp"))
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps):
        subprocess.check_call([HIPCC] + FLAGS + list(extra_flags) + ["-shared", "-o", LIB_PATH, SRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz = C.c_void_p, C.c_size_t
        _lib.plonk_verify_driver_powers.argtypes = [vp, vp, sz, vp, vp]
        _lib.plonk_verify_driver_pi.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]
        _lib.plonk_verify_driver_terms_combine.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        _lib.plonk_verify_driver_check.argtypes = [vp, vp, sz, vp, vp]
    return _lib
