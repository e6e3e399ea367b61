"""GPU parity: Domain / NTT / UnivariateEval::multiply vs the CPU oracle's serial_fft restatement (bit-exact)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def dev(t):
    return t.cpu().numpy().view(np.uint64)


def test_domain_new(zk):   # domain.rs:154-168
    d = zk.Domain(10)
    assert d.size == 16
    assert zk.Fr.to_ints(d.generator) == [14788168760825820622209131888203028446852016562542525606630160374691593895118]
    assert zk.Fr.to_ints(d.group_gen_inverse) == [26753076894533791554649012143113393549300550745003194222677083919072199473480]
    assert zk.Fr.to_ints(d.group_size_inverse) == [pow(16, -1, zk.Fr.MODULUS)]


@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 9, 10, 11, 12, 14, 16, 18, 21])   # 21 = the transform size of a 2^20 x 2^20 product
def test_fft_ifft_match_oracle(zk, ora, log_n):
    n = 1 << log_n
    x = ora.random_fr(n, 70 + log_n)
    d = zk.Domain(n)
    ev = d.fft(x)
    assert np.array_equal(dev(ev), ora.domain_fft(x, n))
    assert np.array_equal(dev(d.ifft(ev)), x)
    assert np.array_equal(dev(d.ifft(x)), ora.domain_ifft(x, n))


def test_fft_pads_short_input(zk, ora):
    x = ora.random_fr(37, 5)
    d = zk.Domain(37)
    assert d.size == 64
    assert np.array_equal(dev(d.fft(x)), ora.domain_fft(x, 64))
    assert np.array_equal(dev(zk.UnivariateEval.from_coefficients(x).values), ora.domain_fft(x, 64))


def test_multiply_kats(zk):   # dense_univariate.rs:464-497 values through the NTT product
    mul = lambda a, b: zk.Fr.to_ints(dev(zk.UnivariateEval.multiply(zk.DenseUnivariatePolynomial(zk.Fr.from_ints(a)),
                                                                    zk.DenseUnivariatePolynomial(zk.Fr.from_ints(b))).coefficients))
    assert mul([1, 3, 2], [3, 2]) == [3, 11, 12, 4]
    assert mul([6, 5, 3], [5, 4, 2]) == [30, 49, 47, 22, 6]
    assert mul([1, 3, 2], [3]) == [3, 9, 6]
    assert mul([7], [6]) == [42]


@pytest.mark.parametrize("na,nb", [(1, 1), (37, 50), (1000, 1049), (5000, 3000), (1 << 14, 1 << 14)])
def test_multiply_matches_oracle(zk, ora, na, nb):
    a, b = ora.random_fr(na, 11), ora.random_fr(nb, 12)
    got = dev(zk.UnivariateEval.multiply(zk.DenseUnivariatePolynomial(a), zk.DenseUnivariatePolynomial(b)).coefficients)
    assert np.array_equal(got, ora.univariate_multiply(a, b))
    if na * nb <= 40 * 60:
        assert np.array_equal(got, ora.dense_mul(a, b))


def test_multiply_2_20_evaluation_identity(zk, ora):
    """SURVEY 2a size (2 x 2^20 coefficients -> 2^21-point transforms): (a*b)(z) == a(z) * b(z) at a random z,
    with the three evaluations done by the oracle's Horner-free restatement on the downloaded coefficients."""
    import torch
    n = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    b = torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    c = zk.UnivariateEval.multiply(zk.DenseUnivariatePolynomial(a), zk.DenseUnivariatePolynomial(b)).coefficients
    assert c.shape[0] == 2 * n - 1
    R = zk.Fr.MODULUS
    z = 0x1234567890ABCDEF1234567890ABCDEF % R

    def horner(t):   # python ints over a strided sample would not be an identity; evaluate fully but vectorised by chunks
        ints = zk.Fr.to_ints(t.cpu().numpy().view(np.uint64))
        acc = 0
        for v in reversed(ints):
            acc = (acc * z + v) % R
        return acc
    # keep the CPU side affordable: check the identity on the low 2^12 x 2^12 sub-product instead of 2^20
    m = 1 << 12
    c_small = zk.UnivariateEval.multiply(zk.DenseUnivariatePolynomial(a[:m].clone()), zk.DenseUnivariatePolynomial(b[:m].clone())).coefficients
    assert horner(c_small) == horner(a[:m]) * horner(b[:m]) % R
    # and tie the big product to the small one: the lowest m coefficients of a*b depend only on a[:m], b[:m]
    assert torch.equal(c[:m], c_small[:m])
    # iNTT(NTT(x)) == x at the full 2^21 size
    d = zk.Domain(2 * n)
    x = torch.cat([a, b])
    assert torch.equal(d.ifft(d.fft(x)), x)


# ---- DenseUnivariatePolynomial::{evaluate, degree, Mul} on device coefficients (dense_univariate.rs) --------------
def test_dense_polynomial_evaluation_degree_multiplication(ora):
    import zk_cryptography_amd as zk
    F = zk.Fr.from_ints
    D = zk.DenseUnivariatePolynomial
    ints = lambda p: zk.Fr.to_ints(p.coefficients.cpu().numpy().view(np.uint64)) if len(p) else []   # noqa: E731
    assert zk.Fr.to_ints(D(F([5, 2, 4])).evaluate(zk.Fr.from_int(2))) == [25]                  # :425-433
    assert zk.Fr.to_ints(D(F([5, 2, 0, 0, 0, 0, 4])).evaluate(zk.Fr.from_int(2))) == [265]     # :185-188
    assert D(F([1, 3, 2])).degree() == 2 and D(F([1, 3, 0, 0])).degree() == 1 and D(F([0, 0])).degree() == 0
    assert ints(D(F([1, 3, 2])) * D(F([3, 2]))) == [3, 11, 12, 4]                               # :464-477
    assert ints(D(F([6, 5, 3])) * D(F([5, 4, 2]))) == [30, 49, 47, 22, 6]                       # :479-497
    assert ints(D(F([1, 3, 2])) * D(F([3]))) == [3, 9, 6]                                        # :500-509
    assert ints(D(F([1, 3, 2, 0, 0])) * D(F([3, 2, 0]))) == [3, 11, 12, 4]                       # degree() ignores zero leading coefficients
    assert ints(D(F([1, 3, 2])) * zk.Fr.from_int(3)) == [3, 9, 6] and ints(D(F([1, 3, 2])) * zk.Fr.from_int(0)) == []


@pytest.mark.parametrize("n", [1, 7, 2048, 2049, 100000])
def test_dense_evaluate_matches_oracle(ora, n):
    import zk_cryptography_amd as zk
    coeffs, z = ora.random_fr(n, 900 + n), ora.random_fr(1, 901 + n)[0]
    got = zk.DenseUnivariatePolynomial(coeffs).evaluate(z)
    ci, zi, acc = zk.Fr.to_ints(coeffs), zk.Fr.to_ints(z)[0], 0
    for c in reversed(ci):
        acc = (acc * zi + c) % zk.Fr.MODULUS
    assert zk.Fr.to_ints(got) == [acc]
    if n <= 2049:
        assert np.array_equal(got, ora.dense_evaluate(coeffs, z))


# ---- every pass plan, the gather's and the last pass's edges, the caches, the aliasing rule ----------------------------------------
# A transform of >= 2^12 points is the first eight stages and then passes (s0, T) spread evenly: one pass at 12..15, two at 16..22,
# three from 23 on (the table in profiles/ntt/NOTES.md; each kernel alone: tests/test_gpu_ntt_kernels.py).
@pytest.mark.parametrize("log_n", [3, 4, 6, 7, 8, 13, 15, 17, 19])
def test_fft_ifft_match_oracle_remaining_plans(zk, ora, log_n):
    n = 1 << log_n
    x = ora.random_fr(n, 170 + log_n)
    d = zk.Domain(n)
    ev = d.fft(x)
    assert np.array_equal(dev(ev), ora.domain_fft(x, n))
    assert np.array_equal(dev(d.ifft(ev)), x)
    assert np.array_equal(dev(d.ifft(x)), ora.domain_ifft(x, n))


GEOMETRIC_A = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [11, 12, 16, 19, 20, 22, 23])
def test_transform_of_a_geometric_sequence_closed_form(zk, ora, log_n, inverse):
    """x[j] = a^j transforms to (a^n - 1) / (a w^i - 1): every output is checked multiplicatively (oracle/ntt.c), three products per
    index, so 2^22 -- (8,7)(15,7), the coset transforms of a 2^20-row PLONK proof -- and 2^23 -- the smallest plan of three passes --
    are affordable.  The input is dense, every butterfly sees generic operands and all expected outputs are distinct.  Up to 2^19 the
    oracle's transform compares the same outputs, so the two references vouch for each other."""
    n = 1 << log_n
    a = GEOMETRIC_A % zk.Fr.MODULUS
    assert pow(a, n, zk.Fr.MODULUS) != 1
    am = ora.fr_from_ints([a])[0]
    x = ora.fr_powers(am, n)
    d = zk.Domain(n)
    got = dev(d.ifft(x) if inverse else d.fft(x))
    assert ora.ntt_geometric_mismatches(got, am, inverse) == (0, n)
    if log_n <= 19:
        assert np.array_equal(got, ora.domain_ifft(x, n) if inverse else ora.domain_fft(x, n))


@pytest.mark.parametrize("log_n", [22, 23])
def test_dense_random_round_trip_large(zk, log_n):
    import torch
    n = 1 << log_n
    g = torch.Generator(device="cuda").manual_seed(40 + log_n)
    x = torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)     # < 2^254 < r: valid residues
    d = zk.Domain(n)
    assert torch.equal(d.ifft(d.fft(x)), x)
    assert torch.equal(d.fft(d.ifft(x)), x)


# n_src in {0, 1, 2047, 2049, n/2, n - 1}; at 2^11, just below the switch to the >= 2^12-point kernels, 2049 does not fit and 2047 is n - 1
@pytest.mark.parametrize("log_n,n_srcs", [(11, (0, 1, 1024, 2047)), (12, (0, 1, 2047, 2049, 2048, 4095)),
                                          (16, (0, 1, 2047, 2049, 32768, 65535))])
def test_short_input_is_zero_padded(zk, ora, log_n, n_srcs):
    n = 1 << log_n
    x = ora.random_fr(n, 270 + log_n)
    d = zk.Domain(n)
    for n_src in n_srcs:
        assert np.array_equal(dev(d.fft(x[:n_src])), ora.domain_fft(x[:n_src], n)), n_src
        assert np.array_equal(dev(d.ifft(x[:n_src])), ora.domain_ifft(x[:n_src], n)), n_src


@pytest.mark.parametrize("na,nb", [(1000, 1050), (4096, 2), (8191, 2), (2048, 2049), (1, 5000), (5000, 1), (4097, 4096)])
def test_multiply_cuts(zk, ora, na, nb):
    """products whose length na + nb - 1 is one past a tile (2049), one past a pass block (4097) and the whole transform (8192)"""
    a, b = ora.random_fr(na, 21), ora.random_fr(nb, 22)
    got = dev(zk.UnivariateEval.multiply(zk.DenseUnivariatePolynomial(a), zk.DenseUnivariatePolynomial(b)).coefficients)
    assert got.shape[0] == na + nb - 1
    assert np.array_equal(got, ora.univariate_multiply(a, b))


def _abi():
    import ctypes as C
    from zk_cryptography_amd import _native as N
    return C, N, N.lib()


@pytest.mark.parametrize("log_n", [11, 12, 16])
def test_in_place_equals_out_of_place(zk, ora, log_n):
    import torch
    C, N, lib = _abi()
    n = 1 << log_n
    x = torch.from_numpy(ora.random_fr(n, 370 + log_n).view(np.int64)).cuda()
    d = zk.Domain(n)
    ctx = N.Context.get(0)
    for inverse in (0, 1):
        want = d.ifft(x) if inverse else d.fft(x)
        buf = x.clone()
        N.check(lib.zkhip_ntt(ctx.handle, N.ptr(buf), C.c_uint32(log_n), C.c_int(inverse)), "ntt")
        assert torch.equal(buf, want)
        buf = x.clone()
        N.check(lib.zkhip_domain_transform(ctx.handle, N.ptr(buf), C.c_size_t(n), N.ptr(buf), C.c_uint32(log_n), C.c_int(inverse)), "in place")
        assert torch.equal(buf, want)


@pytest.mark.parametrize("log_n", [11, 12])
def test_in_place_needs_the_whole_input(zk, ora, log_n):
    """one aliasing rule on both sides of the 2^12 switch: d_dst == d_src with n_src < 2^log_n is ZKHIP_ERR_ARG and writes nothing"""
    import torch
    C, N, lib = _abi()
    n = 1 << log_n
    x = torch.from_numpy(ora.random_fr(n, 470 + log_n).view(np.int64)).cuda()
    ctx = N.Context.get(0)
    for inverse in (0, 1):
        for n_src in (0, 1, n - 1):
            buf = x.clone()
            st = lib.zkhip_domain_transform(ctx.handle, N.ptr(buf), C.c_size_t(n_src), N.ptr(buf), C.c_uint32(log_n), C.c_int(inverse))
            assert st == N.ERR_ARG, (n_src, st)
            torch.cuda.synchronize()
            assert torch.equal(buf, x)


def test_plan_and_twiddle_caches_interleaved(zk, ora):
    """two sizes and both directions through one context's caches, the first repeated at the end; then a context created afterwards"""
    import torch
    C, N, lib = _abi()
    steps = [(12, 0), (12, 1), (16, 0), (13, 1), (12, 0)]
    xs = {k: ora.random_fr(1 << k, 570 + k) for k in (12, 13, 16)}
    want = {(k, inv): (ora.domain_ifft if inv else ora.domain_fft)(xs[k], 1 << k) for k, inv in set(steps)}

    def run(handle):
        for k, inv in steps:
            src = torch.from_numpy(xs[k].view(np.int64)).cuda()
            dst = torch.empty_like(src)
            torch.cuda.synchronize()                   # the uploads are done before a context on another stream reads them
            N.check(lib.zkhip_domain_transform(handle, N.ptr(src), C.c_size_t(1 << k), N.ptr(dst), C.c_uint32(k), C.c_int(inv)), "transform")
            N.check(lib.zkhip_ctx_synchronize(handle), "synchronize")
            assert np.array_equal(dev(dst), want[(k, inv)]), (k, inv)

    first = C.c_void_p()
    N.check(lib.zkhip_ctx_create(C.byref(first), C.c_int(0), None), "ctx_create")
    try:
        run(first)
        second = C.c_void_p()
        N.check(lib.zkhip_ctx_create(C.byref(second), C.c_int(0), None), "ctx_create")
        try:
            run(second)
            run(first)
        finally:
            N.check(lib.zkhip_ctx_destroy(second), "ctx_destroy")
    finally:
        N.check(lib.zkhip_ctx_destroy(first), "ctx_destroy")
