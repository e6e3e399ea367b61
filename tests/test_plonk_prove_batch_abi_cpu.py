"""The batched PLONK prover's C ABI without a GPU: the header declares what the library exports and what PlonkProver.prove_batch passes,
and the returns that come before the key is first followed -- a NULL key, and batch = 0 next to a key pointer that is never followed (a
zeroed host block: a check that did follow it would not find a key there) -- need no device."""
import ctypes as C
import inspect
import os
import re

ERR_ARG = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from zk_cryptography_amd import _native
    _native.build()
    return C.CDLL(_native.LIB_PATH)


def _declaration(header, name):
    m = re.search(r"^(?:int|uint32_t) %s\((.*?)\);" % name, header, re.S | re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_library_and_python_agree():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for name in ("zkhip_plonk_prove_batch", "zkhip_plonk_batch_chunk"):
        assert hasattr(lib, name), name
    args = _declaration(header, "zkhip_plonk_prove_batch")
    assert args == ["zkhip_plonk_key *key", "uint32_t batch", "const uint64_t *const *h_a_ptrs", "const uint64_t *const *h_b_ptrs",
                    "const uint64_t *const *h_c_ptrs", "const uint64_t *const *h_public_ptrs", "const uint64_t *h_blinding", "uint64_t *h_points_xy",
                    "uint8_t *h_points_inf", "uint64_t *h_evals", "uint64_t *h_challenges", "int32_t *h_status"]
    assert _declaration(header, "zkhip_plonk_batch_chunk") == ["const zkhip_plonk_key *key"]
    from zk_cryptography_amd import plonk
    src = inspect.getsource(plonk.PlonkProver.prove_batch)
    call = src[src.index("zkhip_plonk_prove_batch("):]
    call = call[:call.index("\n        refused")]
    assert call.count(",") + 1 == len(args)                    # one value per declared parameter
    assert "C.c_uint32(batch)" in call and "dtype=np.int32" in src     # the batch as uint32_t, the statuses as int32_t
    sig = inspect.signature(plonk.PlonkProver.prove_batch)
    assert list(sig.parameters) == ["self", "witnesses", "blindings", "allow_failures"]
    assert sig.parameters["blindings"].default is None and sig.parameters["allow_failures"].default is False


def test_returns_that_need_no_device():
    lib = _lib()
    lib.zkhip_plonk_batch_chunk.restype = C.c_uint32
    block = (C.c_uint64 * 4096)()
    key = C.cast(block, C.c_void_p)
    out = (C.c_uint64 * 256)()
    for i in range(256):
        out[i] = 0x5A5A5A5A5A5A5A5A
    buf = C.cast(out, C.c_void_p)
    u32 = C.c_uint32
    assert lib.zkhip_plonk_prove_batch(None, u32(0), buf, buf, buf, buf, buf, buf, buf, buf, buf, buf) == ERR_ARG
    assert lib.zkhip_plonk_prove_batch(None, u32(3), buf, buf, buf, buf, buf, buf, buf, buf, buf, buf) == ERR_ARG
    assert lib.zkhip_plonk_prove_batch(key, u32(0), buf, buf, buf, buf, buf, buf, buf, buf, buf, buf) == 0
    assert lib.zkhip_plonk_prove_batch(key, u32(0), None, None, None, None, None, None, None, None, None, None) == 0
    for missing in range(2, 12):                                # every array but h_challenges (10), which may be NULL; checked before the key is followed
        if missing == 10:
            continue
        args = [key, u32(2)] + [buf] * 10
        args[missing] = None
        assert lib.zkhip_plonk_prove_batch(*args) == ERR_ARG, missing
    assert lib.zkhip_plonk_prove_batch(key, u32(65536), buf, buf, buf, buf, buf, buf, buf, buf, buf, buf) == -2
    assert lib.zkhip_plonk_batch_chunk(None) == 0
    assert not any(block) and all(v == 0x5A5A5A5A5A5A5A5A for v in out)
