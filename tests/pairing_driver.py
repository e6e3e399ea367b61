"""Builds and loads tests/cpp/libpairing_driver.so: one launcher per group of operations of csrc/pairing.hpp (Fq2, Fq6, Fq12, G2, the
verifier-side G1 checks, the Miller steps), for tests/test_gpu_pairing_kernels.py.  Test infrastructure only: nothing of libzkhip is
linked into it."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zk-cryptography_amd", "csrc")
SRC = os.path.join(CPP, "pairing_driver.hip")
LIB_PATH = os.path.join(CPP, "libpairing_driver.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# compiler, flags and architecture are those of csrc/Makefile
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]

# operation codes, in the order of the enums of pairing_driver.hip (lib() checks the counts)
F2_OPS = ["add", "sub", "neg", "dbl", "conj", "mul", "sqr", "mul_fq", "mul_xi", "inverse"]
F6_OPS = ["mul", "mul_01", "mul_1", "mul_v", "inverse"]
F12_OPS = ["mul_distinct", "mul_r_is_a", "mul_r_is_b", "mul_a_is_b", "mul_all_same", "sqr", "mul_014", "inverse", "conj", "frob1", "frob2",
           "cyc_sqr", "exp_by_x", "final_exp", "is_one"]
G2_OPS = ["on_curve", "double", "madd", "mul", "in_subgroup"]
G1_OPS = ["on_curve", "in_subgroup", "mul", "mul_neg"]
ML_OPS = ["double_step", "add_step", "mul_line", "loop", "loop_prepared"]
GROUPS = [F2_OPS, F6_OPS, F12_OPS, G2_OPS, G1_OPS, ML_OPS]

_lib = None


def build():
    """a no-op when the library is newer than the driver and the csrc headers"""
    deps = [SRC] + glob.glob(os.path.join(CSRC, "*.hpp"))
    if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC] + FLAGS + ["-shared", "-o", LIB_PATH, SRC], cwd=CPP)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        _lib.pairing_driver_op_count.argtypes = [i]
        _lib.pairing_driver_prep_stride.restype = sz
        _lib.pairing_driver_f2.argtypes = [i, vp, vp, vp, sz, vp]
        _lib.pairing_driver_f6.argtypes = [i, vp, vp, vp, sz, vp]
        _lib.pairing_driver_f12.argtypes = [i, vp, vp, vp, vp, sz, vp]
        _lib.pairing_driver_g2.argtypes = [i, vp, vp, vp, vp, vp, sz, vp]
        _lib.pairing_driver_g1.argtypes = [i, vp, vp, vp, vp, sz, vp]
        _lib.pairing_driver_miller.argtypes = [i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        for g, ops in enumerate(GROUPS):
            assert _lib.pairing_driver_op_count(g) == len(ops), "pairing_driver.py and pairing_driver.hip disagree on group %d" % g
    return _lib
