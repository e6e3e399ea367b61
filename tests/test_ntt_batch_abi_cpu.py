"""The batched transform's C ABI without a GPU: the library exports both entry points, and the argument checks that come before the
context is first used return their codes -- with a NULL context, and with NULL buffers or impossible shapes next to a context
pointer that is never followed (a zeroed host block: a check that did follow it would not find a context there)."""
import ctypes as C

ERR_SHAPE, ERR_ARG = -2, -4


def _lib():
    from zk_cryptography_amd import _native
    _native.build()
    return C.CDLL(_native.LIB_PATH)


def test_both_entry_points_are_exported_and_declared():
    import os
    lib = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zkhip.h")).read()
    for name in ("zkhip_domain_transform_batch", "zkhip_univariate_multiply_batch"):
        assert hasattr(lib, name), name
        assert ("int %s(zkhip_ctx *ctx, uint32_t batch," % name) in header


def test_argument_checks_precede_the_first_use_of_the_context():
    lib = _lib()
    block = (C.c_uint64 * 4096)()
    ctx = C.cast(block, C.c_void_p)
    buf = C.cast((C.c_uint64 * 64)(), C.c_void_p)           # stands for a device pointer; nothing below reaches a launch
    sz, u32 = C.c_size_t, C.c_uint32

    def transform(ctx, batch, src, src_stride, n_src, dst, dst_stride, log_n):
        return [lib.zkhip_domain_transform_batch(ctx, u32(batch), src, sz(src_stride), sz(n_src), dst, sz(dst_stride), u32(log_n), C.c_int(inv))
                for inv in (0, 1)]

    def multiply(ctx, batch, a, a_stride, na, b, b_stride, nb, out, out_stride):
        return lib.zkhip_univariate_multiply_batch(ctx, u32(batch), a, sz(a_stride), sz(na), b, sz(b_stride), sz(nb), out, sz(out_stride))

    assert transform(None, 2, buf, 4, 4, buf, 4, 2) == [ERR_ARG] * 2
    assert transform(ctx, 2, buf, 4, 4, None, 4, 2) == [ERR_ARG] * 2
    assert transform(ctx, 2, None, 4, 4, buf, 4, 2) == [ERR_ARG] * 2
    assert transform(ctx, 2, buf, 4, 4, buf, 4, 31) == [ERR_SHAPE] * 2
    assert transform(ctx, 2, buf, 5, 5, buf, 4, 2) == [ERR_SHAPE] * 2          # n_src > 2^log_n
    assert transform(ctx, 2, buf, 4, 4, buf, 3, 2) == [ERR_SHAPE] * 2          # dst_stride < 2^log_n
    assert transform(ctx, 2, buf, 2, 3, buf, 4, 2) == [ERR_SHAPE] * 2          # src_stride < n_src, batch > 1
    assert transform(ctx, 65536, buf, 4, 4, buf, 4, 2) == [ERR_SHAPE] * 2
    assert transform(ctx, 2, buf, 4, 3, buf, 4, 2) == [ERR_ARG] * 2            # in place with a short input
    assert transform(ctx, 2, buf, 4, 4, buf, 5, 2) == [ERR_ARG] * 2            # in place with two strides
    assert multiply(None, 2, buf, 4, 4, buf, 4, 4, buf, 7) == ERR_ARG
    assert multiply(ctx, 2, None, 4, 4, buf, 4, 4, buf, 7) == ERR_ARG
    assert multiply(ctx, 2, buf, 4, 4, None, 4, 4, buf, 7) == ERR_ARG
    assert multiply(ctx, 2, buf, 4, 4, buf, 4, 4, None, 7) == ERR_ARG
    assert multiply(ctx, 2, buf, 4, 0, buf, 4, 4, buf, 7) == ERR_SHAPE
    assert multiply(ctx, 2, buf, 4, 4, buf, 4, 0, buf, 7) == ERR_SHAPE
    assert multiply(ctx, 2, buf, 4, 4, buf, 4, 4, buf, 6) == ERR_SHAPE         # out_stride < na + nb - 1
    assert multiply(ctx, 65536, buf, 4, 4, buf, 4, 4, buf, 7) == ERR_SHAPE
    assert not any(block)
