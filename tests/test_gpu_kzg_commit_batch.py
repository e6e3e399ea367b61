"""GPU parity of MultilinearKZG.commitment_batch / UnivariateKZG.commitment_batch (zkhip_kzg_commit_polys): a batch of polynomials
against one SRS equals, limb for limb, the single commitments, and commit == p(tau) * G from the CPU oracle (which never touches the
code under test) -- on the short route (a table, at most 2^12 scalars), on the bucket route with plain points and with the table, across
every chunk edge of the planner, with mixed lengths, skewed scalars, identity points, and beside work in flight."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _native():
    from zk_cryptography_amd import _native as N
    return N


def _same_points(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.infinity == w.infinity, b
        if not w.infinity:
            assert np.array_equal(g.xy, w.xy), b


def _p_tau_g(ora, scalars, tau):
    """p(tau) * G as (xy, inf), p(tau) from the oracle's multilinear evaluation"""
    p_tau = ora.fr_to_ints(ora.mle_evaluation(np.ascontiguousarray(scalars), tau))[0]
    a = ora.g1_to_affine(ora.g1_mul_int(ora.g1_generator(), p_tau))
    return a[:12].copy(), bool(a[12])


def _is(got, want_xy, want_inf):
    assert got.infinity == want_inf
    if not want_inf:
        assert np.array_equal(got.xy, want_xy)


def _raw(zk, srs, tensors, lens, table=None, points=True, require_equal_len=False, ptrs=None):
    """zkhip_kzg_commit_polys as it stands in the header -> (status, xy [B, 12], inf [B]); the outputs start as SENTINEL"""
    N = _native()
    b = len(lens)
    xy = np.full((max(b, 1), 12), SENTINEL, dtype=np.uint64)
    inf = np.full(max(b, 1), 0xA5, dtype=np.uint8)
    if ptrs is None:
        ptrs = [t.data_ptr() if n else None for t, n in zip(tensors, lens)]
    parr = (C.c_void_p * max(b, 1))(*ptrs)
    larr = (C.c_size_t * max(b, 1))(*[int(n) for n in lens])
    ctx = N.Context.get(srs.powers_of_tau_in_g1.device.index)
    vp = C.c_void_p
    st = N.lib().zkhip_kzg_commit_polys(ctx.handle, N.ptr(srs.powers_of_tau_in_g1) if points else None, N.ptr(table) if table is not None else None,
                                        N.ptr(srs.inf), C.c_size_t(len(srs)), C.c_uint32(b), parr, larr, C.c_int(1 if require_equal_len else 0),
                                        xy.ctypes.data_as(vp), inf.ctypes.data_as(vp))
    return st, xy, inf


def _untouched(xy, inf):
    return bool((xy == SENTINEL).all() and (inf == 0xA5).all())


def _as_points(zk, xy, inf, b):
    return [zk.G1Affine(xy[j], inf[j]) for j in range(b)]


def _plan(n_points, lens, with_table):
    """zkhip_commit_polys_plan_info -> (route, [polynomials per chunk])"""
    N = _native()
    b = len(lens)
    route, n_chunks = C.c_uint32(0), C.c_uint32(0)
    counts = (C.c_uint32 * max(b, 1))()
    st = N.lib().zkhip_commit_polys_plan_info(C.c_size_t(n_points), (C.c_size_t * max(b, 1))(*lens), C.c_uint32(b), C.c_int(1 if with_table else 0),
                                              C.byref(route), C.byref(n_chunks), counts, None)
    assert st == 0
    return route.value, list(counts[:n_chunks.value])


ROUTE_SINGLE, ROUTE_SHORT, ROUTE_BUCKET = 0, 1, 2


# ---- 1. reference data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precompute", [False, True])
def test_commitment_batch_reference_data(zk, ora, precompute):   # multilinear_kzg.rs:133-148 data, in a batch with two random polynomials
    vals = [0, 7, 0, 5, 0, 7, 4, 9]
    tau = zk.Fr.from_ints([2, 3, 4])
    srs = zk.TrustedSetup.setup(tau)
    if precompute:
        srs.precompute()
    tables = [zk.Fr.from_ints(vals), ora.random_fr(8, 7101), ora.random_fr(8, 7102)]
    got = zk.MultilinearKZG.commitment_batch([zk.Multilinear(t) for t in tables], srs)
    assert len(got) == 3
    x, y = got[0].coords()
    assert x == 0x16ad11e5d15f77c1143b1697344911b9c590110fdd8dd09df2e58bfd757269169deefe8be3544d4e049fb3776fb0bcfb
    assert y == 0x0f5c8be5f27fc19eee337785e43d18414a8ff04995230f04509800252164cf47887a4a1864f18288652196af6272e7f6
    for g, t in zip(got, tables):
        _is(g, *_p_tau_g(ora, t, tau))
    # the plain points through the bucket route, too (the mirror of an SRS this small always commits against its table)
    st, xy, inf = _raw(zk, srs, [zk.Multilinear(t).evaluations for t in tables], [8, 8, 8], require_equal_len=True)
    assert st == 0
    _same_points(_as_points(zk, xy, inf, 3), got)


# ---- 2. every route and every chunk edge, against single commits ----------------------------------------------------------------------
_CASES = {}


def _case(zk, ora, log_n):
    """(tau, srs, the polynomials' host tables, the polynomials, their single commitments), once per size"""
    if log_n not in _CASES:
        n = 1 << log_n
        tau = ora.random_fr(log_n, 7200 + log_n)
        srs = zk.TrustedSetup.setup(tau)
        host = [ora.random_fr(n, 7300 + 100 * log_n + b) for b in range(65)]
        polys = [zk.Multilinear(t) for t in host]
        singles = [zk.MultilinearKZG.commitment(p, srs) for p in polys]
        _CASES[log_n] = (tau, srs, host, polys, singles)
    return _CASES[log_n]


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("log_n", [3, 8, 12, 13, 14])
def test_commitment_batch_matches_single_commits(zk, ora, log_n, table):
    n = 1 << log_n
    tau, srs, host, polys, singles = _case(zk, ora, log_n)
    batches = [1, 2, 3, 5, 64, 65]
    route, chunks = _plan(n, [n] * 65, table)
    assert sum(chunks) == 65
    if route == ROUTE_BUCKET and chunks[0] < 64:
        batches += [chunks[0], chunks[0] + 1]              # the planner's chunk and one polynomial more, whatever that is
    # every route this size has is taken by one of the batches: the short route (its chunk of 64 and one more at 2^3) while the batch
    # is small, the bucket route beyond, single commits for one polynomial (and for two against a table above 2^12)
    routes = {_plan(n, [n] * b, table)[0] for b in batches}
    want = {ROUTE_SINGLE, ROUTE_BUCKET} if not table or log_n > 12 else {ROUTE_SINGLE, ROUTE_SHORT} if log_n == 3 else {ROUTE_SINGLE, ROUTE_SHORT, ROUTE_BUCKET}
    assert routes == want
    if table and log_n == 3:
        assert (route, chunks) == (ROUTE_SHORT, [64, 1])
    if table:
        srs_t = zk.TrustedSetup(srs.powers_of_tau_in_g1, srs.inf).precompute()
    for b in batches:
        if table:
            got = zk.MultilinearKZG.commitment_batch(polys[:b], srs_t)
        else:       # the plain points (the mirror gives an SRS of at most 2^12 points its table on first use)
            st, xy, inf = _raw(zk, srs, [p.evaluations for p in polys[:b]], [n] * b, require_equal_len=True)
            assert st == 0
            got = _as_points(zk, xy, inf, b)
        _same_points(got, singles[:b])
    if not table:   # and the mirror with the table choice of the single call
        _same_points(zk.MultilinearKZG.commitment_batch(polys[:3], srs), singles[:3])
    if log_n in (8, 12, 13):
        for b in (0, 64):
            _is(singles[b], *_p_tau_g(ora, host[b], tau))


# ---- 3. mixed lengths, univariate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
def test_commitment_batch_mixed_lengths_univariate(zk, ora, table):
    srs = zk.UnivariateKZG.generate_srs(ora.random_fr(1, 7400)[0], (1 << 14) - 1)
    assert len(srs) == 1 << 14
    if table:
        srs.precompute()
    lens = [0, 1, 5, 300, 4096, 4097, 9000, 16384]
    route, chunks = _plan(1 << 14, lens, table)
    assert route == ROUTE_BUCKET and sum(chunks) == 7          # short and long polynomials in one batch: problems of 1 and 2^14 entries share a pass
    coeffs = ora.random_fr(1 << 14, 7401)
    polys = [zk.DenseUnivariatePolynomial(np.ascontiguousarray(coeffs[(3 * k) % 7:(3 * k) % 7 + n])) for k, n in enumerate(lens)]
    singles = [zk.UnivariateKZG.commitment(p, srs) for p in polys]
    assert singles[0].infinity
    for order in (list(range(8)), list(range(7, -1, -1))):
        got = zk.UnivariateKZG.commitment_batch([polys[k] for k in order], srs)
        _same_points(got, [singles[k] for k in order])
        assert got[order.index(0)].infinity and not got[order.index(0)].xy.any()
    if table:
        # two polynomials against a table run as commits in flight; the second is the larger one: the first ends before it begins
        assert _plan(1 << 14, [4097, 16384], True) == (ROUTE_SINGLE, [1, 1])
        _same_points(zk.UnivariateKZG.commitment_batch([polys[5], polys[7]], srs), [singles[5], singles[7]])


def test_commitment_batch_short_route_mixed_lengths(zk, ora):
    """the short route with several lengths in one chunk (a launch pair per length), some of them repeated and out of order"""
    tau = ora.random_fr(1, 7410)
    srs = zk.UnivariateKZG.generate_srs(tau[0], 4095)
    lens = [4096, 1, 300, 1000, 0, 17, 300, 2000, 64, 1]
    assert _plan(4096, lens, True)[0] == ROUTE_SHORT
    coeffs = ora.random_fr(4096 + 16, 7411)
    polys = [zk.DenseUnivariatePolynomial(np.ascontiguousarray(coeffs[k:k + n])) for k, n in enumerate(lens)]
    singles = [zk.UnivariateKZG.commitment(p, srs) for p in polys]
    _same_points(zk.UnivariateKZG.commitment_batch(polys, srs), singles)
    # p(tau) * G for two of them: Horner over the integers, the product from the oracle
    t = ora.fr_to_ints(tau)[0]
    for k in (2, 8):
        p_tau = 0
        for c in reversed(ora.fr_to_ints(np.ascontiguousarray(coeffs[k:k + lens[k]]))):
            p_tau = (p_tau * t + c) % R
        want = ora.g1_to_affine(ora.g1_mul_int(ora.g1_generator(), p_tau))
        _is(singles[k], want[:12].copy(), bool(want[12]))


def test_commitment_batch_short_route_launches_per_length(zk, ora):
    """the short route's launch shape: one plane-sums and one reduce launch per distinct non-zero length of the chunk and nothing of the
    single call's or the bucket pipeline's, where the loop of single commitments is one short-path call per non-empty polynomial"""
    from test_gpu_kzg_open_batch import _profiled
    srs = zk.UnivariateKZG.generate_srs(ora.random_fr(1, 7420)[0], 255)
    lens = [17, 1, 256, 17, 0, 256]
    assert len(srs) == 256 and _plan(256, lens, True)[0] == ROUTE_SHORT
    coeffs = ora.random_fr(256 + 8, 7421)
    polys = [zk.DenseUnivariatePolynomial(np.ascontiguousarray(coeffs[k:k + n])) for k, n in enumerate(lens)]
    zk.UnivariateKZG.commitment(polys[0], srs)           # builds the table: its launches are not counted below
    names = ("commit_polys_planes", "commit_polys_reduce", "msm_small", "msm_accumulate")
    got, c_batch = _profiled(lambda: zk.UnivariateKZG.commitment_batch(polys, srs), names)
    singles, c_loop = _profiled(lambda: [zk.UnivariateKZG.commitment(p, srs) for p in polys], names)
    assert c_batch == {"commit_polys_planes": 3, "commit_polys_reduce": 3, "msm_small": 0, "msm_accumulate": 0}
    assert c_loop == {"commit_polys_planes": 0, "commit_polys_reduce": 0, "msm_small": 5, "msm_accumulate": 0}
    _same_points(got, singles)
    for g, w in zip(got, singles):
        assert np.array_equal(g.xy, w.xy)
    assert got[4].infinity and not got[4].xy.any()


# ---- 4. skewed scalars and shared structure ----------------------------------------------------------------------------------------------
def _skewed(zk, ora, kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return zk.Fr.from_ints([0] * n)
    if kind == "ones":
        return zk.Fr.from_ints([1] * n)
    if kind == "bits":
        return zk.Fr.from_ints([int(v) for v in rng.integers(0, 2, n)])
    if kind == "minus_one":
        return zk.Fr.from_ints([R - 1] * n)
    return ora.random_fr(n, seed)


@pytest.mark.parametrize("table", [False, True])
def test_commitment_batch_skewed_scalars(zk, ora, table):
    n = 1 << 13
    tau, srs = _case(zk, ora, 13)[:2]
    srs = zk.TrustedSetup(srs.powers_of_tau_in_g1, srs.inf)
    if table:
        srs.precompute()
    for kinds in (("zero", "ones", "bits", "minus_one"), ("bits", "bits", "uniform", "zero"), ("zero", "zero", "zero", "zero")):
        host = [_skewed(zk, ora, k, n, 7500 + j) for j, k in enumerate(kinds)]
        polys = [zk.Multilinear(t) for t in host]
        assert _plan(n, [n] * 4, table) == (ROUTE_BUCKET, [4])
        got = zk.MultilinearKZG.commitment_batch(polys, srs)
        _same_points(got, [zk.MultilinearKZG.commitment(p, srs) for p in polys])
        for g, t in zip(got, host):
            _is(g, *_p_tau_g(ora, t, tau))
    # the same device pointer twice
    p, q = zk.Multilinear(ora.random_fr(n, 7510)), zk.Multilinear(ora.random_fr(n, 7511))
    got = zk.MultilinearKZG.commitment_batch([p, q, p, p], srs)
    sp, sq = zk.MultilinearKZG.commitment(p, srs), zk.MultilinearKZG.commitment(q, srs)
    _same_points(got, [sp, sq, sp, sp])


@pytest.mark.parametrize("log_n,table", [(4, False), (4, True), (13, False), (13, True)])
def test_commitment_batch_srs_with_identity_points(zk, ora, log_n, table):
    """tau = (0, 1, 2, ...) makes eq-scalars that are 0, so SRS points that are the identity (test_srs_with_identity_points_and_zero_scalars):
    their flags belong to the POINTS -- index i of every polynomial of the batch, not position i of the pass."""
    n = 1 << log_n
    tau = zk.Fr.from_ints(list(range(log_n)))
    srs = zk.TrustedSetup.setup(tau)
    assert 0 < int(srs.inf.sum().item()) < n
    if table:
        srs.precompute()
    host = [ora.random_fr(n, 7600 + b) for b in range(4)]
    polys = [zk.Multilinear(t) for t in host]
    if table or log_n > 12:
        got = zk.MultilinearKZG.commitment_batch(polys, srs)
    else:
        st, xy, inf = _raw(zk, srs, [p.evaluations for p in polys], [n] * 4, require_equal_len=True)
        assert st == 0
        got = _as_points(zk, xy, inf, 4)
    _same_points(got, [zk.MultilinearKZG.commitment(p, srs) for p in polys])
    for g, t in zip(got, host):
        _is(g, *_p_tau_g(ora, t, tau))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_commitment_batch_refusals(zk, ora):
    N = _native()
    n = 1 << 13
    tau, srs, host, polys, singles = _case(zk, ora, 13)
    srs_t = zk.TrustedSetup(srs.powers_of_tau_in_g1, srs.inf).precompute()
    short = zk.Multilinear(ora.random_fr(n // 2, 7700))
    ev = [p.evaluations for p in polys[:3]]
    # one polynomial of the wrong length among good ones: the single call's AssertionError, nothing written
    with pytest.raises(AssertionError):
        zk.MultilinearKZG.commitment_batch([polys[0], short, polys[1]], srs)
    st, xy, inf = _raw(zk, srs, [ev[0], short.evaluations, ev[1]], [n, n // 2, n], require_equal_len=True)
    assert st == N.ERR_SHAPE and _untouched(xy, inf)
    # longer than the SRS (univariate): the single call's IndexError
    usrs = zk.UnivariateKZG.generate_srs(ora.random_fr(1, 7701)[0], 99)
    long_poly = zk.DenseUnivariatePolynomial(ora.random_fr(101, 7702))
    ok_poly = zk.DenseUnivariatePolynomial(ora.random_fr(100, 7703))
    with pytest.raises(IndexError):
        zk.UnivariateKZG.commitment(long_poly, usrs)
    with pytest.raises(IndexError):
        zk.UnivariateKZG.commitment_batch([ok_poly, long_poly], usrs)
    st, xy, inf = _raw(zk, usrs, [ok_poly.coefficients, long_poly.coefficients], [100, 101])
    assert st == N.ERR_INDEX and _untouched(xy, inf)
    # a null pointer in the table of pointers
    st, xy, inf = _raw(zk, srs, ev, [n] * 3, ptrs=[ev[0].data_ptr(), None, ev[2].data_ptr()])
    assert st == N.ERR_ARG and _untouched(xy, inf)
    # both or neither of points / table
    st, xy, inf = _raw(zk, srs, ev, [n] * 3, table=srs_t.table, points=True)
    assert st == N.ERR_ARG and _untouched(xy, inf)
    st, xy, inf = _raw(zk, srs, ev, [n] * 3, table=None, points=False)
    assert st == N.ERR_ARG and _untouched(xy, inf)
    # a table built for another size
    other = zk.TrustedSetup.setup(ora.random_fr(12, 7704)).precompute()
    st, xy, inf = _raw(zk, srs, ev, [n] * 3, table=other.table, points=False)
    assert st == N.ERR_ARG and _untouched(xy, inf)
    # a commit in flight holds the workspace: busy, nothing written; after wait() the same call succeeds
    pending = zk.MultilinearKZG.commitment_begin(polys[3], srs)
    st, xy, inf = _raw(zk, srs, ev, [n] * 3, require_equal_len=True)
    assert st == N.ERR_BUSY and _untouched(xy, inf)
    with pytest.raises(N.ZkhipError):
        zk.MultilinearKZG.commitment_batch(polys[:3], srs)
    _same_points([pending.wait()], [singles[3]])
    _same_points(zk.MultilinearKZG.commitment_batch(polys[:3], srs), singles[:3])
    # nothing to do
    assert zk.MultilinearKZG.commitment_batch([], srs) == [] and zk.UnivariateKZG.commitment_batch([], usrs) == []
    st, xy, inf = _raw(zk, srs, [], [])
    assert st == 0 and _untouched(xy, inf)
    # only empty polynomials: identities, without a launch
    empty = zk.DenseUnivariatePolynomial(ora.random_fr(4, 7705)[:0])
    got = zk.UnivariateKZG.commitment_batch([empty, empty], usrs)
    assert all(g.infinity and not g.xy.any() for g in got)


# ---- 6. beside work in flight --------------------------------------------------------------------------------------------------------------
def test_commitment_batch_beside_work_in_flight(zk, ora):
    import gkr_cases as G
    tau, srs, host, polys, singles = _case(zk, ora, 13)
    table = ora.random_fr(1 << 12, 7800)
    sc = zk.Sumcheck(zk.Multilinear(table))
    sc.poly_sum()
    layers = G.random_circuit(4)
    cir = zk.Circuit.from_tuples(layers)
    inputs = [ora.random_fr(16, 7810 + b) for b in range(3)]
    gkr_proofs = zk.GKRProtocol.prove_batch(cir, [cir.evaluation(i) for i in inputs], max_lanes=2)      # a result from before
    ticket = sc.prove_begin()                                                                           # a proof in flight
    got = zk.MultilinearKZG.commitment_batch(polys[:3], srs)
    proof, challenges = ticket.wait()
    _same_points(got, singles[:3])
    s, rp, ch = ora.sumcheck_prove(table)
    assert np.array_equal(proof.sum, s) and np.array_equal(proof.univariate_poly, rp) and np.array_equal(challenges, ch)
    for b in range(3):
        assert G.gkr_proof_mismatches(ora, gkr_proofs[b], ora.gkr_prove(layers, ora.circuit_evaluation(layers, inputs[b]))) == []
