"""The batched sumcheck provers' C ABI without a GPU: the library exports both entry points, and the refusals that need no device
come back with their documented codes and untouched outputs -- with a NULL context, and with NULL buffers or impossible shapes next
to a context pointer that is never followed (a zeroed host block: a check that did follow it would not find a context there)."""
import ctypes as C
import os
import re

ERR_SHAPE, ERR_ARG = -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from zk_cryptography_amd import _native
    _native.build()
    return C.CDLL(_native.LIB_PATH)


def test_both_entry_points_are_exported_and_declared():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for name in ("zkhip_sumcheck_prove_batch", "zkhip_composed_prove_batch"):
        assert hasattr(lib, name), name
        assert ("int %s(zkhip_ctx *ctx, uint32_t batch, const uint64_t *const *h_table_ptrs," % name) in header
    mirror = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    assert "zkhip_sumcheck_prove_batch(" in mirror and "zkhip_composed_prove_batch(" in mirror


def test_the_documented_chunk_is_the_kernel_headers():
    from zk_cryptography_amd.sumcheck import Sumcheck
    src = open(os.path.join(ROOT, "zk-cryptography_amd", "csrc", "sumcheck_batch_kernels.hpp")).read()
    assert int(re.search(r"constexpr uint32_t SCB_CHUNK = (\d+);", src).group(1)) == Sumcheck.BATCH_CHUNK


def test_refusals_precede_the_first_use_of_the_context_and_leave_the_outputs_alone():
    lib = _lib()
    block = (C.c_uint64 * 4096)()
    ctx = C.cast(block, C.c_void_p)
    table = (C.c_uint64 * 64)()                              # stands for a device table; nothing below reaches a launch
    B = 2
    ptrs = (C.c_void_p * (5 * B))(*[C.addressof(table)] * (5 * B))
    with_null = (C.c_void_p * (5 * B))(*([C.addressof(table)] * (5 * B - 1) + [None]))
    FILL = 0xA5A5A5A5A5A5A5A5
    outs = [(C.c_uint64 * 512)(*[FILL] * 512) for _ in range(3)]
    sums, rp, ch = outs
    claimed = (C.c_uint64 * (4 * B))()
    sz, u32 = C.c_size_t, C.c_uint32

    def basic(ctx, batch, ptrs, n, claimed, sums, rp, ch):
        return lib.zkhip_sumcheck_prove_batch(ctx, u32(batch), ptrs, sz(n), claimed, sums, rp, ch)

    def composed(ctx, batch, ptrs, k, n, rp, ch):
        return lib.zkhip_composed_prove_batch(ctx, u32(batch), ptrs, u32(k), sz(n), rp, ch)

    for cl in (None, claimed):
        assert basic(None, B, ptrs, 8, cl, sums, rp, ch) == ERR_ARG
        assert basic(ctx, B, None, 8, cl, sums, rp, ch) == ERR_ARG
        assert basic(ctx, 5 * B, with_null, 8, cl, sums, rp, ch) == ERR_ARG    # a NULL table among the batch's
        assert basic(ctx, B, ptrs, 8, cl, None, rp, ch) == ERR_ARG
        assert basic(ctx, B, ptrs, 8, cl, sums, None, ch) == ERR_ARG
        assert basic(ctx, B, ptrs, 8, cl, sums, rp, None) == ERR_ARG
        for n in (0, 3, 6, 12, (1 << 16) + 1):
            assert basic(ctx, B, ptrs, n, cl, sums, rp, ch) == ERR_SHAPE, n
        assert basic(ctx, B, ptrs, 1 << 49, cl, sums, rp, ch) == ERR_SHAPE     # more rounds than a proof may have
        assert basic(ctx, 0, ptrs, 8, cl, sums, rp, ch) == 0                   # an empty batch: nothing to do, nothing touched
    assert composed(None, B, ptrs, 2, 8, rp, ch) == ERR_ARG
    assert composed(ctx, B, None, 2, 8, rp, ch) == ERR_ARG
    assert composed(ctx, B, with_null, 5, 8, rp, ch) == ERR_ARG
    assert composed(ctx, B, ptrs, 2, 8, None, ch) == ERR_ARG
    assert composed(ctx, B, ptrs, 2, 8, rp, None) == ERR_ARG
    assert composed(ctx, B, ptrs, 0, 8, rp, ch) == ERR_ARG
    assert composed(ctx, B, ptrs, 6, 8, rp, ch) == ERR_ARG
    for n in (0, 3, 6, 12, (1 << 16) + 1):
        assert composed(ctx, B, ptrs, 2, n, rp, ch) == ERR_SHAPE, n
    assert composed(ctx, B, ptrs, 2, 1 << 49, rp, ch) == ERR_SHAPE
    assert composed(ctx, 0, ptrs, 2, 8, rp, ch) == 0
    assert composed(ctx, B, ptrs, 3, 1, rp, ch) == 0                           # one entry: no rounds, nothing delivered
    assert not any(block)
    assert all(v == FILL for o in outs for v in o)
