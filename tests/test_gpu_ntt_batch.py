"""zkhip_domain_transform_batch / zkhip_univariate_multiply_batch: a batch equals the loop of single calls limb for limb (the single
call is pinned to the oracle by test_gpu_ntt.py), and the C oracle itself.  Every comparison is equality of packed limbs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NTT_BATCH_SCRATCH_BYTES = 256 << 20          # csrc/ntt.hip: scratch a batch call may hold; more rows run as consecutive chunks
PATTERN = 0x5A5AA5A5C3C33C3C                 # what a destination holds before a call; no transform output has four such limbs
SINGLE_SCOPES = ("ntt_first8", "ntt_pass", "ntt_first_stages", "ntt_mid_stages")


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _abi():
    from zk_cryptography_amd import _native as N
    return N, N.lib()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def patterned(elements):
    import torch
    return torch.full((elements, 4), PATTERN, dtype=torch.int64, device="cuda")


def transform_batch(handle, batch, src, src_stride, n_src, dst, dst_stride, log_n, inverse):
    N, lib = _abi()
    return lib.zkhip_domain_transform_batch(handle, C.c_uint32(batch), N.ptr(src) if src is not None else None, C.c_size_t(src_stride),
                                            C.c_size_t(n_src), N.ptr(dst) if dst is not None else None, C.c_size_t(dst_stride),
                                            C.c_uint32(log_n), C.c_int(inverse))


def singles(rows, n_src, log_n, inverse):
    """[B, n, 4]: zkhip_domain_transform of the first n_src elements of every row of the [B, m, 4] device tensor"""
    import torch
    N, lib = _abi()
    ctx = N.Context.get(0)
    out = torch.empty((rows.shape[0], 1 << log_n, 4), dtype=torch.int64, device="cuda")
    for b in range(rows.shape[0]):
        N.check(lib.zkhip_domain_transform(ctx.handle, N.ptr(rows[b]), C.c_size_t(n_src), N.ptr(out[b]), C.c_uint32(log_n), C.c_int(inverse)),
                "single transform")
    return out


def check_batch(ora, log_n, batch, n_src, seed, src_gap, dst_gap, oracle=False, single=True):
    """both directions of one shape: the rows equal the singles (and the oracle), the gaps and the tail of the destination keep the pattern"""
    import torch
    N, _ = _abi()
    ctx = N.Context.get(0)
    n = 1 << log_n
    src_stride, dst_stride, tail = n_src + src_gap, n + dst_gap, 16
    x = cuda(ora.random_fr(max(batch * src_stride, 1), seed)).view(-1, 4)       # the gaps of the source hold values too: padding is zero, not them
    rows = torch.stack([x[b * src_stride:b * src_stride + n_src] for b in range(batch)]).contiguous() if n_src else \
        torch.empty((batch, 0, 4), dtype=torch.int64, device="cuda")
    for inverse in (0, 1):
        dst = patterned(batch * dst_stride + tail)
        N.check(transform_batch(ctx.handle, batch, x, src_stride, n_src, dst, dst_stride, log_n, inverse), "transform_batch")
        body = dst[:batch * dst_stride].view(batch, dst_stride, 4)
        if single:
            assert torch.equal(body[:, :n], singles(rows, n_src, log_n, inverse)), (log_n, batch, n_src, inverse)
        if oracle:
            for b in range(batch):
                want = (ora.domain_ifft if inverse else ora.domain_fft)(host(rows[b]), n)
                assert np.array_equal(host(body[b, :n]), want), (log_n, batch, n_src, inverse, b)
        assert bool((body[:, n:] == PATTERN).all()) and bool((dst[batch * dst_stride:] == PATTERN).all()), (log_n, batch, inverse)


# ---- 1. batch equals the loop of singles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 9, 10, 11, 12, 13, 16])
def test_batch_equals_the_loop_of_singles(zk, ora, log_n):
    for batch in (1, 2, 3, 7):
        check_batch(ora, log_n, batch, 1 << log_n, 7000 + 10 * log_n + batch, 0, 0)
        check_batch(ora, log_n, batch, 1 << log_n, 7200 + 10 * log_n + batch, 3, 5)


@pytest.mark.parametrize("log_n,batch", [(3, 1), (3, 127), (3, 128), (3, 129), (10, 3)])
def test_rows_that_share_a_tile_and_the_short_last_workgroup(zk, ora, log_n, batch):
    """at 2^3 a tile holds 128 transforms: one short workgroup, one row short of full, full, full and one row; at 2^10 one row a tile"""
    check_batch(ora, log_n, batch, 1 << log_n, 7400 + batch, 0, 0)
    check_batch(ora, log_n, batch, 1 << log_n, 7600 + batch, 3, 5)


# ---- 2. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 10, 11, 12, 14])
def test_batch_matches_the_oracle(zk, ora, log_n):
    check_batch(ora, log_n, 3, 1 << log_n, 7800 + log_n, 0, 0, oracle=True, single=False)


# ---- 3. zero padding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 11, 12])
def test_short_rows_are_zero_padded(zk, ora, log_n):
    n = 1 << log_n
    for n_src in (0, 1, n // 2, n - 1):
        check_batch(ora, log_n, 3, n_src, 7900 + log_n, 3, 5, oracle=log_n == 3)


# ---- 4. in place ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [5, 11, 12])
def test_in_place_equals_out_of_place(zk, ora, log_n):
    import torch
    N, _ = _abi()
    ctx = N.Context.get(0)
    n, batch = 1 << log_n, 3
    for stride in (n, n + 5):
        x = cuda(ora.random_fr(batch * stride, 8000 + log_n))
        for inverse in (0, 1):
            want = patterned(batch * stride)
            N.check(transform_batch(ctx.handle, batch, x, stride, n, want, stride, log_n, inverse), "out of place")
            buf = x.clone()
            N.check(transform_batch(ctx.handle, batch, buf, stride, n, buf, stride, log_n, inverse), "in place")
            got, ref, src = (t.view(batch, stride, 4) for t in (buf, want, x))
            assert torch.equal(got[:, :n], ref[:, :n])
            assert torch.equal(got[:, n:], src[:, n:])              # in place the gaps keep the source's values


@pytest.mark.parametrize("log_n", [5, 11, 12])
def test_in_place_needs_whole_rows_and_one_stride(zk, ora, log_n):
    import torch
    N, _ = _abi()
    ctx = N.Context.get(0)
    n, batch = 1 << log_n, 3
    x = cuda(ora.random_fr(batch * (n + 2), 8100 + log_n))
    for inverse in (0, 1):
        for n_src, src_stride, dst_stride in ((n - 1, n, n), (0, n, n), (n, n + 1, n), (n, n, n + 2)):
            buf = x.clone()
            assert transform_batch(ctx.handle, batch, buf, src_stride, n_src, buf, dst_stride, log_n, inverse) == N.ERR_ARG
            torch.cuda.synchronize()
            assert torch.equal(buf, x)


# ---- 5. errors and the empty batch ----------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_the_empty_batch_is_ok(zk, ora):
    import torch
    from zk_cryptography_amd import distributed as D
    N, lib = _abi()
    ctx = N.Context.get(0)
    log_n, n, batch = 4, 16, 2
    x = cuda(ora.random_fr(batch * n, 8200))
    dst = patterned(batch * n)
    clean = dst.clone()
    h = ctx.handle
    cases = [
        (N.ERR_ARG, (None, batch, x, n, n, dst, n, log_n, 0)),                 # NULL context
        (N.ERR_ARG, (h, batch, x, n, n, None, n, log_n, 0)),                   # NULL destination
        (N.ERR_ARG, (h, batch, None, n, n, dst, n, log_n, 0)),                 # NULL source of n_src > 0 values
        (N.ERR_SHAPE, (h, batch, x, n, n, dst, n, 31, 0)),                     # log_n > 30
        (N.ERR_SHAPE, (h, batch, x, n + 1, n + 1, dst, n, log_n, 0)),          # n_src > 2^log_n
        (N.ERR_SHAPE, (h, batch, x, n, n, dst, n - 1, log_n, 0)),              # dst_stride < 2^log_n
        (N.ERR_SHAPE, (h, batch, x, n - 2, n - 1, dst, n, log_n, 0)),          # src_stride < n_src with batch > 1
        (N.ERR_SHAPE, (h, 65536, x, n, n, dst, n, log_n, 0)),                  # batch > 65535
    ]
    for want, args in cases:
        for inverse in (0, 1):
            assert transform_batch(*args[:-1], inverse) == want, args[1:]
    # src_stride < n_src is fine for ONE transform, as the single call has no stride at all
    one = patterned(n)
    N.check(transform_batch(h, 1, x, 0, n, one, n, log_n, 0), "batch of one")
    assert torch.equal(one, singles(x[:n].view(1, n, 4), n, log_n, 0)[0])

    def multiply(batch, a, a_stride, na, b, b_stride, nb, out, out_stride, handle=h):
        p = lambda t: N.ptr(t) if t is not None else None   # noqa: E731
        return lib.zkhip_univariate_multiply_batch(handle, C.c_uint32(batch), p(a), C.c_size_t(a_stride), C.c_size_t(na), p(b), C.c_size_t(b_stride),
                                                   C.c_size_t(nb), p(out), C.c_size_t(out_stride))
    assert multiply(2, x, 8, 0, x, 8, 8, dst, 16) == N.ERR_SHAPE               # na == 0
    assert multiply(2, x, 8, 8, x, 8, 0, dst, 16) == N.ERR_SHAPE               # nb == 0
    assert multiply(2, x, 8, 8, x, 8, 8, dst, 14) == N.ERR_SHAPE               # out_stride < na + nb - 1
    assert multiply(65536, x, 8, 8, x, 8, 8, dst, 15) == N.ERR_SHAPE
    assert multiply(2, None, 8, 8, x, 8, 8, dst, 15) == N.ERR_ARG
    assert multiply(2, x, 8, 8, None, 8, 8, dst, 15) == N.ERR_ARG
    assert multiply(2, x, 8, 8, x, 8, 8, None, 15) == N.ERR_ARG
    assert multiply(2, x, 8, 8, x, 8, 8, dst, 15, handle=None) == N.ERR_ARG
    # the workspace lent to a split-phase session: ZKHIP_ERR_BUSY, whether or not the shape would have needed scratch
    eng = D.HipSumcheckEngine(cuda(ora.random_fr(1 << 12, 8201)))
    try:
        big = cuda(ora.random_fr(2 << 12, 8202))
        assert transform_batch(h, batch, x, n, n, dst, n, log_n, 0) == N.ERR_BUSY
        assert transform_batch(h, 2, big, 1 << 12, 1 << 12, big, 1 << 12, 12, 1) == N.ERR_BUSY
        assert multiply(2, x, 8, 8, x, 8, 8, dst, 15) == N.ERR_BUSY
        torch.cuda.synchronize()
        assert np.array_equal(host(big), ora.random_fr(2 << 12, 8202))
    finally:
        eng.abort()
    # the empty batch
    assert transform_batch(h, 0, x, n, n, dst, n, log_n, 0) == N.ZKHIP_OK
    assert multiply(0, x, 8, 8, x, 8, 8, dst, 15) == N.ZKHIP_OK
    torch.cuda.synchronize()
    assert torch.equal(dst, clean)


# ---- 6. more rows than one chunk of scratch holds -------------------------------------------------------------------------------
def test_in_place_batch_across_the_chunk_bound(zk):
    import torch
    N, _ = _abi()
    ctx = N.Context.get(0)
    log_n = 12
    n = 1 << log_n
    batch = NTT_BATCH_SCRATCH_BYTES // (32 * n) + 1
    assert batch == 2049
    g = torch.Generator(device="cuda").manual_seed(86)
    x = torch.randint(0, 2 ** 62, (batch, n, 4), dtype=torch.int64, device="cuda", generator=g)      # every limb < 2^62: reduced residues
    for inverse in (0, 1):
        want = singles(x, n, log_n, inverse)
        buf = x.clone()
        N.check(transform_batch(ctx.handle, batch, buf, n, n, buf, n, log_n, inverse), "in place across chunks")
        bad = (buf != want).any(dim=2).any(dim=1).nonzero().flatten().tolist()
        assert not bad, (inverse, bad[:8], len(bad))
        del want, buf


# ---- 7. launch counts -----------------------------------------------------------------------------------------------------------
def _profiled(work, names):
    N, lib = _abi()
    ctx = N.Context.get(0)
    N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        work()
        counts = {}
        for name in names:
            cnt = C.c_uint64()
            N.check(lib.zkhip_profile_read(ctx.handle, name.encode(), None, C.byref(cnt), None), "profile_read")
            counts[name] = cnt.value
    finally:
        N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    return counts


@pytest.mark.parametrize("log_n,batch,want", [(8, 100, (1, 0, 0)), (14, 8, (0, 1, 1)), (16, 8, (0, 1, 2))])
def test_launch_count_does_not_depend_on_the_batch(zk, ora, log_n, batch, want):
    N, _ = _abi()
    ctx = N.Context.get(0)
    n = 1 << log_n
    x = cuda(ora.random_fr(batch * n, 8300 + log_n))
    dst = patterned(batch * n)
    names = ("ntt_batch_small", "ntt_batch_first8", "ntt_batch_pass") + SINGLE_SCOPES
    for inverse in (0, 1):
        N.check(transform_batch(ctx.handle, batch, x, n, n, dst, n, log_n, inverse), "warm the tables")      # table builds are not the call's launches
        counts = _profiled(lambda: N.check(transform_batch(ctx.handle, batch, x, n, n, dst, n, log_n, inverse), "transform_batch"), names)
        assert tuple(counts[k] for k in names[:3]) == want, counts
        assert all(counts[k] == 0 for k in SINGLE_SCOPES), counts


# ---- 8. the caches are the single call's ----------------------------------------------------------------------------------------
def test_batch_and_single_share_plans_in_either_order(zk, ora):
    import torch
    N, lib = _abi()
    handle = C.c_void_p()
    N.check(lib.zkhip_ctx_create(C.byref(handle), C.c_int(0), None), "ctx_create")
    try:
        for log_n, inverse, seed in ((12, 0, 8400), (13, 1, 8401)):
            n = 1 << log_n
            rows = ora.random_fr(3 * n, seed).reshape(3, n, 4)
            want = [(ora.domain_ifft if inverse else ora.domain_fft)(rows[b], n) for b in range(3)]
            x = cuda(rows.reshape(-1, 4))
            dst = torch.empty_like(x)
            torch.cuda.synchronize()
            N.check(transform_batch(handle, 3, x, n, n, dst, n, log_n, inverse), "batch first")
            N.check(lib.zkhip_ctx_synchronize(handle), "synchronize")
            for b in range(3):
                assert np.array_equal(host(dst[b * n:(b + 1) * n]), want[b]), (log_n, b)
            one = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            N.check(lib.zkhip_domain_transform(handle, N.ptr(x), C.c_size_t(n), N.ptr(one), C.c_uint32(log_n), C.c_int(inverse)), "single after")
            N.check(lib.zkhip_ctx_synchronize(handle), "synchronize")
            assert np.array_equal(host(one), want[0]), log_n
    finally:
        N.check(lib.zkhip_ctx_destroy(handle), "ctx_destroy")


# ---- 9. multiply_batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(1, 1), (37, 50), (1000, 1049), (2048, 2049), (5000, 3000)])
def test_multiply_batch(zk, ora, na, nb):
    import torch
    D = zk.DenseUnivariatePolynomial
    a = [ora.random_fr(na, 8500 + k) for k in range(3)]
    b = [ora.random_fr(nb, 8510 + k) for k in range(3)]
    got = zk.UnivariateEval.multiply_batch([D(v) for v in a], [D(v) for v in b])
    assert len(got) == 3
    for k in range(3):
        assert got[k].coefficients.shape[0] == na + nb - 1
        assert torch.equal(got[k].coefficients, zk.UnivariateEval.multiply(D(a[k]), D(b[k])).coefficients), k
        assert np.array_equal(host(got[k].coefficients), ora.univariate_multiply(a[k], b[k])), k
        if na * nb <= 40 * 60:
            assert np.array_equal(host(got[k].coefficients), ora.dense_mul(a[k], b[k])), k
    # with gaps between the rows of every operand: the gaps of the product keep what they held
    N, lib = _abi()
    ctx = N.Context.get(0)
    sa, sb, so = na + 3, nb + 2, na + nb - 1 + 5
    xa, xb = cuda(ora.random_fr(3 * sa, 8520)), cuda(ora.random_fr(3 * sb, 8521))
    for k in range(3):
        xa[k * sa:k * sa + na] = cuda(a[k])
        xb[k * sb:k * sb + nb] = cuda(b[k])
    out = patterned(3 * so + 16)
    N.check(lib.zkhip_univariate_multiply_batch(ctx.handle, C.c_uint32(3), N.ptr(xa), C.c_size_t(sa), C.c_size_t(na), N.ptr(xb), C.c_size_t(sb),
                                                C.c_size_t(nb), N.ptr(out), C.c_size_t(so)), "multiply_batch with gaps")
    body = out[:3 * so].view(3, so, 4)
    for k in range(3):
        assert torch.equal(body[k, :na + nb - 1], got[k].coefficients), k
    assert bool((body[:, na + nb - 1:] == PATTERN).all()) and bool((out[3 * so:] == PATTERN).all())


# ---- 10. the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface(zk, ora):
    x = ora.random_fr(4 * 37, 8600).reshape(4, 37, 4)
    d = zk.Domain(37)
    ev = d.fft_batch(x)
    assert tuple(ev.shape) == (4, 64, 4)
    for b in range(4):
        assert np.array_equal(host(ev[b]), ora.domain_fft(x[b], 64))
    back = host(d.ifft_batch(ev))
    assert np.array_equal(back[:, :37], x) and not back[:, 37:].any()
    with pytest.raises(AssertionError):
        d.fft_batch(ora.random_fr(2 * 65, 8601).reshape(2, 65, 4))
    D = zk.DenseUnivariatePolynomial
    p = [D(ora.random_fr(5, 8610 + k)) for k in range(3)]
    with pytest.raises(AssertionError):
        zk.UnivariateEval.multiply_batch(p, p[:2])
    with pytest.raises(AssertionError):
        zk.UnivariateEval.multiply_batch(p, [p[0], p[1], D(ora.random_fr(6, 8620))])
    assert zk.UnivariateEval.multiply_batch([], []) == []
