"""GPU parity of zkhip_dense_points and its mirrors: DenseUnivariatePolynomial.evaluate([m, 4]) / evaluate_batch against the oracle's
Horner and, limb for limb, against the single call; interpolate / interpolate_batch against a Lagrange model in Python integers
(tests/dense_points_model.py) and, at the large sizes, by uniqueness; both sides of the segment decision; every stride combination;
the refusals; both ops beside a commit and a proof in flight; and shamir secret sharing on top.  Every raw call writes into a buffer
filled with a pattern, with a wider out_stride, and the padding is checked to be untouched.  Section 9 takes the plans the small
shapes above never select: a batch and a cut together, segments of several staged chunks, and a batch of interpolations that the entry
point runs as two chunks of jobs (the kernels alone, at chosen grids and cuts: tests/test_gpu_dense_points_kernels.py)."""
import ctypes as C
import itertools
import os
import time

import numpy as np
import pytest

import tables as T
from dense_points_model import R, horner, lagrange_coefficients, lagrange_coefficients_many, root_of_unity

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
EVALUATE, INTERPOLATE = 0, 1
PAD = 3                                     # elements of padding behind every output row


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


@pytest.fixture(scope="module")
def N():
    from zk_cryptography_amd import _native
    return _native


def plan_info(N, op, batch, n_in, n_x):
    info = (C.c_uint32 * 8)()
    assert N.lib().zkhip_dense_points_plan_info(op, batch, n_in, n_x, info) == N.ZKHIP_OK
    return dict(regime=info[0], segs=info[1], lanes=info[2], launches=info[3], scratch=info[4] + (info[5] << 32), L=info[6], chunk=info[7])


def dev(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def raw(N, op, ins, xs, n_out, batch=None, in_stride=None, x_stride=None, expect=None):
    """zkhip_dense_points on host arrays `ins` ([B, n_in, 4] or [n_in, 4] shared) and `xs` ([B, n_x, 4] or [n_x, 4] shared) -> [B, n_out, 4];
    the output rows are n_out + PAD apart, pre-filled, and the padding is checked"""
    import torch
    ins, xs = np.asarray(ins, dtype=np.uint64), np.asarray(xs, dtype=np.uint64)
    B = batch if batch is not None else (ins.shape[0] if ins.ndim == 3 else xs.shape[0] if xs.ndim == 3 else 1)
    n_in, n_x = ins.shape[-2], xs.shape[-2]
    d_in, d_x = dev(ins.reshape(-1, 4)), dev(xs.reshape(-1, 4))
    stride = n_out + PAD
    out = torch.from_numpy(np.full((max(B, 1) * stride, 4), FILL).view(np.int64)).cuda()
    ctx = N.Context.get(0)
    st = N.lib().zkhip_dense_points(ctx.handle, op, B, d_in.data_ptr(), (n_in if ins.ndim == 3 else 0) if in_stride is None else in_stride, n_in,
                                    d_x.data_ptr(), (n_x if xs.ndim == 3 else 0) if x_stride is None else x_stride, n_x, out.data_ptr(), stride)
    got = host(out).reshape(max(B, 1), stride, 4)
    if expect is not None:
        assert st == expect, st
        return got
    assert st == N.ZKHIP_OK, st
    assert (got[:, n_out:] == FILL).all(), "the padding of a wider out_stride was written"
    return got[:B, :n_out]


def oracle_values(ora, coeffs, xs):
    """ora.dense_evaluate at every point; many points of a long polynomial on a few threads (the oracle is C behind ctypes, which
    releases the interpreter's lock: 4096 points of 4096 coefficients take 17 s on one thread)"""
    if len(xs) == 0:
        return np.empty((0, 4), dtype=np.uint64)
    if len(xs) * len(coeffs) < 1 << 20:
        return np.stack([ora.dense_evaluate(coeffs, x) for x in xs])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return np.stack(list(pool.map(lambda x: ora.dense_evaluate(coeffs, x), xs, chunksize=32)))


_POINTS = {}


def points(n_x):
    """n_x points with 0, 1 and r - 1 among them (as far as they fit): made once per size"""
    if n_x not in _POINTS:
        p = T.fill("uniform_r", n_x, 31000 + n_x)
        for k, v in enumerate((0, 1, R - 1)[:n_x]):
            p[(k * 7) % n_x if n_x > 21 else k] = T.stored(v)
        _POINTS[n_x] = p
    return _POINTS[n_x]


# ---- 1. evaluation against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_x", [1, 63, 64, 65, 255, 256, 257])
def test_every_value_is_the_oracles(N, ora, n_x):
    L = plan_info(N, EVALUATE, 1, 1, n_x)["L"]
    xs = points(n_x)
    for k, n_in in enumerate((0, 1, 2, L - 1, L, L + 1)):
        kind = T.FILLS_ARITH[k % len(T.FILLS_ARITH)]
        coeffs = T.fill(kind, n_in, 32000 + n_in) if n_in else np.empty((0, 4), dtype=np.uint64)
        got = raw(N, EVALUATE, coeffs, xs, n_x)[0]
        assert np.array_equal(got, oracle_values(ora, coeffs, xs)), (n_in, kind)


@pytest.mark.parametrize("kind", T.FILLS_ARITH)
def test_every_fill_of_the_coefficients(N, ora, kind):
    L = plan_info(N, EVALUATE, 1, 1, 65)["L"]
    coeffs, xs = T.fill(kind, L + 1, 32500), points(65)
    assert np.array_equal(raw(N, EVALUATE, coeffs, xs, 65)[0], oracle_values(ora, coeffs, xs))


def test_both_sides_of_the_segment_decision(N, ora):
    n_in = 1 << 14
    coeffs = ora.random_fr(n_in, 33000)
    cut = plan_info(N, EVALUATE, 1, n_in, 3)
    assert cut["segs"] > 1 and cut["launches"] == 2 and cut["scratch"] >= cut["segs"] * 3 * 32
    xs = points(3)
    assert np.array_equal(raw(N, EVALUATE, coeffs, xs, 3)[0], oracle_values(ora, coeffs, xs))
    # a shorter last segment: the coefficients are no multiple of the segment
    odd = plan_info(N, EVALUATE, 1, n_in - 300, 3)
    assert odd["segs"] > 1
    assert np.array_equal(raw(N, EVALUATE, coeffs[:n_in - 300], xs, 3)[0], oracle_values(ora, coeffs[:n_in - 300], xs))
    B, n_x = 64, 4096
    whole = plan_info(N, EVALUATE, B, n_in, n_x)
    assert whole["segs"] == 1 and whole["launches"] == 1
    xs = T.fill("uniform_r", n_x, 33001)
    got = raw(N, EVALUATE, coeffs, xs, n_x, batch=B)
    assert (got == got[0]).all()                                            # one polynomial, one set of points: B equal rows
    pick = [0, 1, 255, 256, 257, n_x - 1]
    assert np.array_equal(got[B - 1][pick], oracle_values(ora, coeffs, xs[pick]))


# ---- 2. evaluation against the single call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3, 64])
def test_the_batch_is_the_single_calls_at_every_stride_combination(zk, N, ora, B):
    n_in, m = 37, 5
    polys = [T.fill(T.FILLS_ARITH[b % 4], n_in, 34000 + b) for b in range(B)]
    pts = T.fill("uniform_r", B * m, 34100).reshape(B, m, 4)
    dpolys = [zk.DenseUnivariatePolynomial(p) for p in polys]
    single = {}                                                              # (polynomial, row of points) -> the m single calls
    for b, c in sorted({(b, b) for b in range(B)} | {(b, 0) for b in range(B)} | {(0, c) for c in range(B)}):
        single[b, c] = np.stack([dpolys[b].evaluate(pts[c, k]) for k in range(m)])
    # neither stride zero: polynomial b at its own points
    own = np.stack([single[b, b] for b in range(B)])
    assert np.array_equal(raw(N, EVALUATE, np.stack(polys), pts, m), own)
    assert np.array_equal(zk.DenseUnivariatePolynomial.evaluate_batch(dpolys, pts), own)
    # x_stride == 0: every polynomial at the points of row 0
    shared = np.stack([single[b, 0] for b in range(B)])
    assert np.array_equal(raw(N, EVALUATE, np.stack(polys), pts[0], m), shared)
    assert np.array_equal(zk.DenseUnivariatePolynomial.evaluate_batch(dpolys, pts[0]), shared)
    # in_stride == 0: polynomial 0 at every job's points
    assert np.array_equal(raw(N, EVALUATE, polys[0], pts, m), np.stack([single[0, c] for c in range(B)]))
    # the 2-D form of evaluate: numpy in, numpy out; a device tensor in, a device tensor out
    for b in range(min(B, 2)):
        got = dpolys[b].evaluate(pts[b])
        assert isinstance(got, np.ndarray) and got.shape == (m, 4) and np.array_equal(got, single[b, b])
        got = dpolys[b].evaluate(dev(pts[b]))
        assert got.is_cuda and np.array_equal(host(got), single[b, b])
        assert np.array_equal(dpolys[b].evaluate(pts[b, :1]), single[b, b][:1])      # m = 1 through the 2-D form
    assert np.array_equal(single[0, 0], oracle_values(ora, polys[0], pts[0]))


def test_the_empty_polynomial_and_no_points(zk):
    empty = zk.DenseUnivariatePolynomial(np.empty((0, 4), dtype=np.uint64))
    assert not empty.evaluate(points(5)).any()
    p = zk.DenseUnivariatePolynomial(T.fill("uniform_r", 9, 34500))
    assert p.evaluate(np.empty((0, 4), dtype=np.uint64)).shape == (0, 4)


# ---- 3. interpolation against the model ----------------------------------------------------------------------------------------------
def nodes(n, seed, special=True):
    """n distinct nodes, as ints; with 0, 1 and powers of the transform domain's generator among them"""
    first = []
    if special:
        w = root_of_unity(1 << max((n - 1).bit_length(), 1))
        first = list(dict.fromkeys([0, 1, w, pow(w, 3, R), pow(w, n - 1, R)]))[:n]
    drawn = [x for x in dict.fromkeys(T.canonical(T.fill("uniform_r", n + 8, seed))) if x not in first]
    xs = first + drawn[:n - len(first)]
    assert len(xs) == n and len(set(xs)) == n
    return xs


_MODEL = {}


def model_case(ora, n):
    """(xs, ys per kind, model coefficients per kind) at n nodes: computed once, shared"""
    if n not in _MODEL:
        xs = nodes(n, 35000 + n)
        low = T.canonical(T.fill("uniform_r", max(n - 2, 1), 35500 + n)) if n >= 3 else None
        ys = {"zero": [0] * n}
        for kind in T.FILLS_ARITH:
            ys[kind] = T.canonical(T.fill(kind, n, 35600 + n))
        if low is not None:                                                 # sampled from a polynomial of degree n - 3
            ys["low_degree"] = [horner(low, x) for x in xs]
        _MODEL[n] = (xs, ys, dict(zip(ys, lagrange_coefficients_many(xs, list(ys.values())))))
    return _MODEL[n]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 17, 63, 64, 65, 255, 256, 257, 512])
def test_the_coefficients_are_the_models(zk, N, ora, n):
    xs, ys, want = model_case(ora, n)
    X = ora.fr_from_ints(xs)
    for kind, y in ys.items():
        got = raw(N, INTERPOLATE, ora.fr_from_ints(y), X, n)[0]
        assert np.array_equal(got, ora.fr_from_ints(want[kind])), kind
        if kind == "zero":
            assert not got.any()
        if kind == "low_degree":
            assert not got[n - 2:].any() and want[kind][n - 3] != 0
    poly = zk.DenseUnivariatePolynomial.interpolate(ora.fr_from_ints(ys["uniform_r"]), X)                  # the mirror, the reference's argument order
    assert len(poly) == n and np.array_equal(host(poly.coefficients), ora.fr_from_ints(want["uniform_r"]))
    zero = zk.DenseUnivariatePolynomial.interpolate(ora.fr_from_ints(ys["zero"]), X)
    assert len(zero) == n and zero.degree() == 0 and not zero.evaluate(X[0]).any()


# ---- 4. large sizes, by uniqueness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(1 << 10) + 1, 1 << 12, 1 << 14])
def test_the_interpolant_returns_the_values_at_the_nodes(zk, N, ora, n):
    info = plan_info(N, INTERPOLATE, 1, n, n)
    assert info["regime"] == 2 and (n < (1 << 14) or info["segs"] > 1)
    X = ora.fr_from_ints(nodes(n, 36000 + n))
    Y = T.fill("uniform_r", n, 36100 + n)
    poly = zk.DenseUnivariatePolynomial.interpolate(Y, X)
    coeffs = host(poly.coefficients)
    assert coeffs.shape == (n, 4)
    pick = list(range(n)) if n < (1 << 14) else list(range(0, n, n // 256))    # at 2^14: 256 nodes through the oracle
    assert np.array_equal(oracle_values(ora, coeffs, X[pick]), Y[pick])
    if n == 1 << 14:                                                        # all nodes through the evaluation op, pinned against the oracle above
        assert np.array_equal(poly.evaluate(X), Y)


# ---- 5. interpolation in batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 257])
def test_a_batch_of_interpolations_is_the_single_calls(zk, N, ora, n):
    Bmax = 64
    Xs = np.stack([ora.fr_from_ints(nodes(n, 37000 + 100 * n + b, special=b % 2 == 0)) for b in range(Bmax)])
    Ys = np.stack([T.fill(T.FILLS_ARITH[b % 4], n, 37500 + 100 * n + b) for b in range(Bmax)])
    own = np.stack([host(zk.DenseUnivariatePolynomial.interpolate(Ys[b], Xs[b]).coefficients) for b in range(Bmax)])
    shared = np.stack([host(zk.DenseUnivariatePolynomial.interpolate(Ys[b], Xs[0]).coefficients) for b in range(Bmax)])
    for B in (1, 2, 3, 64):
        assert np.array_equal(host(zk.DenseUnivariatePolynomial.interpolate_batch(Ys[:B], Xs[:B])), own[:B]), B
        assert np.array_equal(host(zk.DenseUnivariatePolynomial.interpolate_batch(Ys[:B], Xs[0])), shared[:B]), B
        assert np.array_equal(raw(N, INTERPOLATE, Ys[:B], Xs[:B], n), own[:B]), B
        assert np.array_equal(raw(N, INTERPOLATE, Ys[:B], Xs[0], n), shared[:B]), B


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------
def test_repeated_nodes_and_refusals(zk, N, ora):
    n = 9
    ctx = N.Context.get(0)
    X = ora.fr_from_ints(nodes(n, 38000))
    Y = T.fill("uniform_r", n, 38001)
    bad = X.copy()
    bad[7] = bad[3]
    with pytest.raises(ValueError):
        zk.DenseUnivariatePolynomial.interpolate(Y, bad)
    with pytest.raises(AssertionError):
        zk.DenseUnivariatePolynomial.interpolate(Y[:-1], X)
    assert N.lib().zkhip_last_hip_error(ctx.handle) == 0
    # only one job of three repeats a node
    for which in range(3):
        Xs = np.stack([X, X, X])
        Xs[which] = bad
        raw(N, INTERPOLATE, np.stack([Y, Y, Y]), Xs, n, expect=N.ERR_ARG)
    raw(N, INTERPOLATE, Y, bad, n, batch=3, expect=N.ERR_ARG)                # shared nodes
    # a repeat across two segments' worth of nodes
    big = ora.fr_from_ints(nodes(600, 38002))
    big[599] = big[2]
    raw(N, INTERPOLATE, T.fill("uniform_r", 600, 38003), big, 600, expect=N.ERR_ARG)
    assert N.lib().zkhip_last_hip_error(ctx.handle) == 0
    # shapes
    import torch
    a, b, c = (torch.zeros((40, 4), dtype=torch.int64, device="cuda") for _ in range(3))
    call = lambda op, batch, i, n_in, x, n_x, o: N.lib().zkhip_dense_points(ctx.handle, op, batch, i.data_ptr(), n_in, n_in, x.data_ptr(), n_x, n_x,  # noqa: E731
                                                                          o.data_ptr(), max(n_in, n_x))
    assert call(INTERPOLATE, 1, a, 8, b, 9, c) == N.ERR_SHAPE
    assert call(INTERPOLATE, 1, a, (1 << 14) + 1, b, (1 << 14) + 1, c) == N.ERR_SHAPE
    for op in (EVALUATE, INTERPOLATE):
        assert call(op, 65536, a, 8, b, 8, c) == N.ERR_SHAPE
        assert call(op, 1, a, 8, b, 8, a) == N.ERR_ARG                       # d_out == d_in
        assert call(op, 1, a, 8, b, 8, b) == N.ERR_ARG                       # d_out == d_x
        assert call(op, 0, a, 8, b, 8, c) == N.ZKHIP_OK
    assert not c.any().item()
    assert N.lib().zkhip_last_hip_error(ctx.handle) == 0
    # and the context still serves
    assert np.array_equal(raw(N, INTERPOLATE, Y, X, n)[0], ora.fr_from_ints(lagrange_coefficients(ora.fr_to_ints(X), ora.fr_to_ints(Y))))


# ---- 7. beside a holder -----------------------------------------------------------------------------------------------------------------
def _both_ops(N, ora):
    coeffs, xs = ora.random_fr(300, 39000), points(65)
    X, Y = ora.fr_from_ints(nodes(300, 39001)), T.fill("uniform_r", 300, 39002)
    return raw(N, EVALUATE, coeffs, xs, 65)[0], raw(N, INTERPOLATE, Y, X, 300)[0]


def test_beside_a_commit_in_flight_both_ops_serve(zk, N, ora):
    idle = _both_ops(N, ora)
    srs = zk.TrustedSetup.setup(ora.random_fr(10, 39100))
    poly = zk.Multilinear(ora.random_fr(1 << 10, 39101))
    want_commit = zk.MultilinearKZG.commitment(poly, srs)
    pending = zk.MultilinearKZG.commitment_begin(poly, srs)
    try:
        beside = _both_ops(N, ora)
    finally:
        got_commit = pending.wait()
    assert got_commit == want_commit
    assert np.array_equal(beside[0], idle[0]) and np.array_equal(beside[1], idle[1])


def test_beside_a_proof_in_flight_both_ops_serve(zk, N, ora):
    idle = _both_ops(N, ora)
    table = zk.Multilinear(ora.random_fr(1 << 12, 39200))
    sc = zk.Sumcheck(table)
    sc.poly_sum()
    want, want_ch = sc.prove()
    sc2 = zk.Sumcheck(table)
    sc2.poly_sum()
    pending = sc2.prove_begin()
    try:
        beside = _both_ops(N, ora)
    finally:
        got, got_ch = pending.wait()
    assert np.array_equal(got.sum, want.sum) and np.array_equal(got.univariate_poly, want.univariate_poly) and np.array_equal(got_ch, want_ch)
    assert np.array_equal(beside[0], idle[0]) and np.array_equal(beside[1], idle[1])


# ---- 8. shamir ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secret,threshold,total", [(123, 3, 5), (102057, 17, 40)])
def test_shamir_shares_reconstruct_the_secret(zk, ora, secret, threshold, total):
    randoms = T.fill("uniform_r", threshold - 1, 40000 + threshold)
    shares = zk.shamir.create_shares(secret, threshold, total, randoms=randoms)
    assert len(shares) == total and zk.Fr.to_ints(np.stack([x for x, _y in shares])) == list(range(1, total + 1))
    # the shares are the model's polynomial through (0, secret), (i, randoms[i - 1]) at 1 .. total
    coeffs = lagrange_coefficients(list(range(threshold)), [secret] + T.canonical(randoms))
    assert zk.Fr.to_ints(np.stack([y for _x, y in shares])) == [horner(coeffs, i) for i in range(1, total + 1)]
    assert zk.Fr.to_ints(zk.shamir.reconstruct_secret(shares[:threshold], 0)) == [secret]
    subsets = list(itertools.combinations(range(total), threshold)) if total <= 5 else [tuple(range(total - threshold, total)), tuple(range(1, 2 * threshold, 2)),
                                                                                      tuple(sorted((7 * k + 3) % total for k in range(threshold)))]
    for sub in subsets:
        assert len(set(sub)) == threshold
        assert zk.Fr.to_ints(zk.shamir.reconstruct_secret([shares[i] for i in sub], zk.Fr.from_int(0))) == [secret], sub
    drawn = zk.shamir.create_shares(secret, threshold, total)                  # randoms drawn on the host
    assert zk.Fr.to_ints(zk.shamir.reconstruct_secret(drawn[-threshold:], 0)) == [secret]


def test_shamir_batches_are_the_loop(zk, ora):
    B, threshold, total = 64, 5, 9
    secrets_ = T.fill("uniform_r", B, 41000)
    randoms = T.fill("uniform_r", B * (threshold - 1), 41001).reshape(B, threshold - 1, 4)
    xs, ys = zk.shamir.create_shares_batch(list(secrets_), threshold, total, randoms)
    assert xs.shape == (total, 4) and ys.shape == (B, total, 4)
    for b in range(B):
        loop = zk.shamir.create_shares(secrets_[b], threshold, total, randoms=randoms[b])
        assert np.array_equal(np.stack([y for _x, y in loop]), ys[b]) and np.array_equal(np.stack([x for x, _y in loop]), xs)
    pick = [8, 1, 4, 6, 2]
    got = zk.shamir.reconstruct_secret_batch(xs[pick], ys[:, pick], 0)
    assert np.array_equal(got, secrets_)
    for b in range(B):
        assert np.array_equal(zk.shamir.reconstruct_secret([(xs[i], ys[b, i]) for i in pick], 0), got[b])


# ---- 9. plans the small shapes never select ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_in,n_x", [(3, 600, 5), (2, 769, 257)])
def test_evaluation_with_a_batch_and_a_cut_together(N, ora, B, n_in, n_x):
    """records at (job * segs + seg) * n_x + p with job > 0 and seg > 0 at once, at every stride combination"""
    info = plan_info(N, EVALUATE, B, n_in, n_x)
    assert info["segs"] > 1 and info["launches"] == 2, info
    polys = np.stack([T.fill(T.FILLS_ARITH[b % 4], n_in, 42000 + b) for b in range(B)])
    pts = np.stack([np.roll(points(n_x), b, axis=0) for b in range(B)])
    pts[1:, n_x // 2] = T.fill("uniform_r", B - 1, 42100)                    # the jobs' points differ in more than their order
    value = {(b, c): oracle_values(ora, polys[b], pts[c]) for b, c in {(b, b) for b in range(B)} | {(b, 0) for b in range(B)} | {(0, c) for c in range(B)}}
    assert np.array_equal(raw(N, EVALUATE, polys, pts, n_x), np.stack([value[b, b] for b in range(B)]))
    assert np.array_equal(raw(N, EVALUATE, polys, pts[0], n_x), np.stack([value[b, 0] for b in range(B)]))          # x_stride == 0
    assert np.array_equal(raw(N, EVALUATE, polys[0], pts, n_x), np.stack([value[0, c] for c in range(B)]))          # in_stride == 0
    assert np.array_equal(raw(N, EVALUATE, polys[0], pts[0], n_x, batch=B), np.stack([value[0, 0]] * B))            # both
    assert not np.array_equal(value[1, 1], value[0, 0]) and not np.array_equal(value[1, 0], value[0, 0])


def test_evaluation_segments_of_more_than_one_chunk(N, ora):
    """20000 coefficients at 3 points: segments of two staged chunks, a last segment of one partial chunk, x^lo with lo up to 19968"""
    n_in = 20000
    info = plan_info(N, EVALUATE, 1, n_in, 3)
    assert info["segs"] > 1 and -(-n_in // info["segs"]) > info["L"], info   # a segment is at least the mean: more than one chunk
    assert n_in % info["L"] and info["segs"] <= 64
    xs = points(3)
    for kind in ("uniform_r", "top"):
        coeffs = T.fill(kind, n_in, 42200)
        assert np.array_equal(raw(N, EVALUATE, coeffs, xs, 3)[0], oracle_values(ora, coeffs, xs)), kind


def test_interpolation_in_two_chunks(N, ora):
    """n = 65, B = 65535: the entry point runs the batch as two launch chains and offsets d_in, d_x and d_out by the chunk's first job.
    The values of job b are row b % 7 of seven rows (and its nodes row b % 5 of five) and seven is coprime to the chunk's length, so a
    second chunk that starts at a wrong job -- 4 * ch.first * in_stride dropped, say, or x_stride, or out_stride -- reads or writes
    rows that differ from the right ones; every output row is compared with the model's coefficients for its (b % 5, b % 7).  Then a
    repeated node in the LAST job only (second chunk) and in job 0 only (first chunk).  The rows are built and compared on the device:
    136 MB per buffer."""
    import torch
    t0 = time.perf_counter()
    n, B = 65, 65535
    info = plan_info(N, INTERPOLATE, B, n, n)
    chunk = info["chunk"]
    assert info["regime"] == 2 and 0 < chunk < B and chunk % 7 and chunk % 5, info
    ctx = N.Context.get(0)
    lib = N.lib()
    xs5 = [nodes(n, 43000 + k, special=k % 2 == 0) for k in range(5)]
    ys7 = [T.canonical(T.fill(("uniform_r", "top", "limb_edges")[k % 3], n, 43100 + k)) for k in range(7)]   # seven DISTINCT rows
    want35 = np.stack([ora.fr_from_ints(c) for k in range(5) for c in lagrange_coefficients_many(xs5[k], ys7)])   # row 7 k5 + k7
    assert len({w.tobytes() for w in want35}) == 35
    b = torch.arange(B, device="cuda")
    d_Y = dev(np.stack([ora.fr_from_ints(y) for y in ys7])).reshape(7, n, 4)[b % 7].contiguous()
    d_X = dev(np.stack([ora.fr_from_ints(x) for x in xs5])).reshape(5, n, 4)[b % 5].contiguous()
    d_want = dev(want35).reshape(35, n, 4)
    stride = n + PAD
    fill = int(np.array([FILL]).view(np.int64)[0])
    out = torch.empty((B, stride, 4), dtype=torch.int64, device="cuda")

    def call(x_stride):
        out.fill_(fill)
        torch.cuda.synchronize()                                             # torch's stream wrote the buffers; the library has its own
        st = lib.zkhip_dense_points(ctx.handle, INTERPOLATE, B, d_Y.data_ptr(), n, n, d_X.data_ptr(), x_stride, n, out.data_ptr(), stride)
        assert lib.zkhip_last_hip_error(ctx.handle) == 0
        return st

    def rows_are(which):
        assert bool((out[:, n:] == fill).all()), "the padding of a wider out_stride was written"
        bad = (out[:, :n] != d_want[which]).any(dim=2).any(dim=1).nonzero()
        assert not len(bad), "%d rows differ, the first is job %d (the chunk holds %d jobs)" % (len(bad), int(bad[0]), chunk)

    assert call(0) == N.ZKHIP_OK                                             # shared nodes: row 0 of d_X
    rows_are(b % 7)
    assert call(n) == N.ZKHIP_OK                                             # nodes of the job's own
    own = (b % 5) * 7 + b % 7
    rows_are(own)
    for job in (B - 1, 0):
        kept = d_X[job, 7].clone()
        d_X[job, 7] = d_X[job, 3]
        assert call(n) == N.ERR_ARG, job
        d_X[job, 7] = kept
    assert call(n) == N.ZKHIP_OK
    rows_are(own)
    print("interpolation in two chunks (B = %d, chunk %d): %.2f s" % (B, chunk, time.perf_counter() - t0))
