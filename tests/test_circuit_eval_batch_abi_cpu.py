"""zkhip_circuit_evaluate_batch's C ABI without a GPU: the library exports the entry point with the signature the header declares,
both mirrors bind it, the refusals that need no device come back with their documented codes, and what the mirror and the header
say about the launch plan is what csrc/circuit_eval_plan.hpp holds."""
import ctypes as C
import os
import re

ERR_ARG = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from zk_cryptography_amd import _native
    _native.build()
    return C.CDLL(_native.LIB_PATH)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_point_is_exported_declared_and_bound():
    lib = _lib()
    assert hasattr(lib, "zkhip_circuit_evaluate_batch")
    header = " ".join(_read("include", "zkhip.h").split())
    assert ("int zkhip_circuit_evaluate_batch(zkhip_circuit *circuit, uint32_t n_inputs, size_t input_len, "
            "const uint64_t *const *h_layer_ptrs, size_t *h_layer_len);") in header
    assert "zkhip_circuit_evaluate_batch(" in _read("include", "zkhip.hpp")
    mirror = _read("zk-cryptography_amd", "gkr.py")
    for name in ("def evaluation_batch(self, inputs)", "def prove_inputs(circuit, inputs, max_lanes=0)", "def prove_batch(circuit, circuit_evaluations, tau)"):
        assert name in mirror, name


def test_refusals_that_need_no_circuit():
    lib = _lib()
    table = (C.c_uint64 * 8)()
    ptrs = (C.c_void_p * 3)(*[C.addressof(table)] * 3)
    lens = (C.c_size_t * 3)(7, 7, 7)
    call = lib.zkhip_circuit_evaluate_batch
    assert call(None, C.c_uint32(1), C.c_size_t(4), ptrs, lens) == ERR_ARG
    assert call(None, C.c_uint32(0), C.c_size_t(4), ptrs, lens) == ERR_ARG        # a NULL circuit before the empty batch
    assert call(None, C.c_uint32(1), C.c_size_t(4), None, None) == ERR_ARG
    assert list(lens) == [7, 7, 7] and not any(table)


def test_the_documented_widths_are_the_plan_headers():
    plan = _read("zk-cryptography_amd", "csrc", "circuit_eval_plan.hpp")
    tail_log = int(re.search(r"#define ZK_CEB_TAIL_LOG (\d+)", plan).group(1))
    chunk = int(re.search(r"constexpr uint32_t CEB_CHUNK = (\d+);", plan).group(1))
    header = _read("include", "zkhip.h")
    assert "at most 2^%d gates" % tail_log in header and "chunks of %d" % chunk in header
    assert "T = 2^%d" % tail_log in _read("DESIGN.md")
