"""No GPU: the stage models of tests/dense_points_model.py (what tests/test_gpu_dense_points_kernels.py judges the kernels of
csrc/dense_points_kernels.hpp with) held to each other and to the CPU oracle before any of them judges a kernel -- the folded (Num, Den)
records are the Lagrange model's polynomial at every domain point, the summed evaluation records are Horner and the oracle's
dense_evaluate, the weights' records multiply to D_i, at every cut and with nodes on the transform domain; records of a coarse cut are the
combined records of a finer one, which is how the GPU test derives them -- and the refusals of tests/cpp/dense_points_driver.hip, which
come before a device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_points_driver as DRV  # noqa: E402
import dense_points_model as M  # noqa: E402
import tables as T  # noqa: E402

R = M.R
SEGS = [1, 2, 3, 64]


def cuts(n):
    """(seg_len, segs) with segs of SEGS and no empty segment, as far as n allows; and one cut with two empty segments"""
    if n == 0:
        return [(1, 1), (1, 3)]
    out = []
    for segs in SEGS:
        seg_len = -(-n // segs)
        if -(-n // seg_len) == segs:
            out.append((seg_len, segs))
    return out + [(max(n, 1), 3)]


def distinct_nodes(n, seed, on_domain=(), N=None):
    """n distinct nodes with 0, 1 and r - 1 among them; on_domain: {index: exponent of the domain's generator}"""
    xs = list(dict.fromkeys([0, 1, R - 1] + T.canonical(T.fill("uniform_r", n + 8, seed))))[:n]
    w = M.root_of_unity(N) if N else None
    for i, e in dict(on_domain).items():
        xs[i] = pow(w, e, R)
    assert len(set(xs)) == n
    return xs


def test_model_constants_and_inverse():
    assert M.R == T.R and M.invert(0) == 0 and M.invert(1) == 1
    for d in (2, R - 1, 0x1234567 << 200):
        assert d * M.invert(d) % R == 1
    assert [M.segment(10, 4, s) for s in range(4)] == [(0, 4), (4, 8), (8, 10), (10, 10)]


@pytest.mark.parametrize("kind", T.FILLS_ARITH)
@pytest.mark.parametrize("n", [0, 1, 7, 64, 127])
def test_summed_evaluation_records_are_horner_and_the_oracle(ora, kind, n):
    limbs = T.fill(kind, n, 51000 + n) if n else np.empty((0, 4), dtype=np.uint64)
    coeffs = T.canonical(limbs) if n else []
    xs = [0, 1, R - 1, 2] + T.canonical(T.fill("uniform_r", 3, 51001))
    want = [M.horner(coeffs, x) for x in xs]
    assert want == [sum(c * pow(x, k, R) for k, c in enumerate(coeffs)) % R for x in xs]
    if n:
        X = ora.fr_from_ints(xs)
        assert [ora.fr_to_ints(ora.dense_evaluate(limbs, X[p]))[0] for p in range(len(xs))] == want
    for seg_len, segs in cuts(n):
        rec = M.eval_records(coeffs, xs, seg_len, segs)
        assert len(rec) == segs and all(len(r) == len(xs) for r in rec)
        assert [sum(r[p] for r in rec) % R for p in range(len(xs))] == want, (seg_len, segs)
        for seg, r in enumerate(rec):
            lo, hi = M.segment(n, seg_len, seg)
            if lo == hi:
                assert r == [0] * len(xs)
            elif lo > 0:
                assert r[0] == 0 and r[1] == sum(coeffs[lo:hi]) % R           # x = 0 and x = 1 in a segment with lo > 0


@pytest.mark.parametrize("n", [1, 2, 3, 9, 64, 127])
def test_weight_records_multiply_to_the_weights(n):
    xs = distinct_nodes(n, 52000 + n)
    D = M.weights(xs)
    assert D == [np.prod([1] + [(xs[i] - xs[j]) % R for j in range(n) if j != i], dtype=object) % R for i in range(n)]
    assert all(d * v % R == 1 for d, v in zip(D, M.weights_inv(xs)))
    for seg_len, segs in cuts(n):
        rec = M.weight_records(xs, seg_len, segs)
        prod = [1] * n
        for seg, r in enumerate(rec):
            if M.segment(n, seg_len, seg)[0] == M.segment(n, seg_len, seg)[1]:
                assert r == [1] * n
            prod = [a * b % R for a, b in zip(prod, r)]
        assert prod == D, (seg_len, segs)
    if n >= 3:                                                              # a repeated node: both weights vanish, and their inverses by the convention
        xs[n - 1] = xs[1]
        D = M.weights(xs)
        assert [i for i, d in enumerate(D) if d == 0] == [1, n - 1]
        assert [i for i, v in enumerate(M.weights_inv(xs)) if v == 0] == [1, n - 1]


def placements(n, N):
    """the nodes' places on the domain: none, one in the last place, two far apart, two neighbours, and (n == N) all, permuted"""
    out = [{}, {n - 1: 5 % N}]
    if n >= 4:
        out += [{2: 1, n - 2: N - 1}, {2: 3 % N, 3: N // 2 + 1}]
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17, 64, 127])
def test_folded_records_are_the_interpolant_on_the_domain(ora, n):
    N = 1 << (n - 1).bit_length()
    w = M.root_of_unity(N)
    assert N == 1 or ora.fr_to_ints(ora.fr_get_root_of_unity(N)) == [w]
    zs = [pow(w, t, R) for t in range(N)]
    cases = [distinct_nodes(n, 53000 + n + q, pl, N) if not any(e in (0, N // 2) for e in pl.values()) else None for q, pl in enumerate(placements(n, N))]
    if n == N:
        cases.append([zs[(5 * t + 3) % N] for t in range(N)])               # every node on the domain
    for q, xs in enumerate(c for c in cases if c is not None):
        ys = T.canonical(T.fill(T.FILLS_ARITH[q % 4], n, 53500 + n))
        winv = M.weights_inv(xs)
        coeffs = M.lagrange_coefficients(xs, ys)
        want = [M.horner(coeffs, z) for z in zs]
        for i, x in enumerate(xs):
            if x in zs:
                assert want[zs.index(x)] == ys[i]
        fine = None
        for seg_len, segs in cuts(n):
            rec = M.domain_records(xs, ys, winv, N, seg_len, segs)
            assert len(rec) == segs and all(len(r) == N for r in rec)
            folded = M.domain_fold(rec)
            assert [num for num, _den in folded] == want, (q, seg_len, segs)
            assert [den for _num, den in folded] == [np.prod([(z - x) % R for x in xs], dtype=object) % R for z in zs]
            for seg, r in enumerate(rec):
                lo, hi = M.segment(n, seg_len, seg)
                if lo == hi:
                    assert r == [(0, 1)] * N
                for t, (_num, den) in enumerate(r):
                    assert (den == 0) == (zs[t] in xs[lo:hi])
            if segs == 64:
                fine = rec
        if fine is not None:                                                # a coarse cut's records are the finer cut's, combined in order
            seg_len = -(-n // 64)
            for group in (2, 3):
                coarse = M.domain_records(xs, ys, winv, N, group * seg_len, -(-64 // group))
                assert coarse == [M.domain_fold(fine[g:g + group]) for g in range(0, 64, group)]
                wf = M.weight_records(xs, seg_len, 64)
                wc = M.weight_records(xs, group * seg_len, -(-64 // group))
                assert wc == [[np.prod([r[i] for r in wf[g:g + group]], dtype=object) % R for i in range(n)] for g in range(0, 64, group)]


@pytest.mark.parametrize("n", [1, 2, 5, 17, 64])
def test_a_rotated_problem_has_rotated_records(n):
    """what the GPU test gives its second and third job at the large sizes: the first job's problem moved by a power of the domain's
    generator, whose records follow from the first job's"""
    N = 1 << (n - 1).bit_length()
    xs = distinct_nodes(n, 54000 + n)
    ys = T.canonical(T.fill("top", n, 54500 + n))
    winv = M.weights_inv(xs)
    for k, c in ((1, 3), (N - 1, R - 2), (5 % N, ys[0] or 7)):
        xr, yr, wr = M.rotate_problem(xs, ys, winv, N, k, c)
        assert wr == M.weights_inv(xr) and len(set(xr)) == n
        g = pow(M.root_of_unity(N), k, R)
        p, pr = M.lagrange_coefficients(xs, ys), M.lagrange_coefficients(xr, yr)
        assert pr == [c * a * pow(g, -i, R) % R for i, a in enumerate(p)]      # c P(X / g)
        for seg_len, segs in cuts(n):
            direct = M.domain_records(xr, yr, wr, N, seg_len, segs)
            assert M.rotate_domain_records(M.domain_records(xs, ys, winv, N, seg_len, segs), N, n, k, c, seg_len) == direct, (k, seg_len, segs)


# ---- the driver: built for gfx950, refusals before a device is touched ----------------------------------------
@pytest.fixture(scope="module")
def L():
    return DRV.lib()


def test_driver_builds_and_reports_the_plans_constants(L):
    assert os.path.exists(DRV.LIB_PATH)
    assert all(hasattr(L, "dp_driver_" + name) for name in DRV.LAUNCHERS)
    c = DRV.constants()
    assert c["lanes"] >= 64 and c["chunk"] >= 1 and c["max_segs"] >= 2 and c["max_grid_x"] >= 1
    assert [DRV.library_grid(n) for n in (1, c["lanes"], c["lanes"] + 1, c["lanes"] * c["max_grid_x"] + 1)] == [1, 1, 2, c["max_grid_x"]]
    assert L.dp_driver_constants(None) == DRV.INVALID


def test_driver_refuses_null_pointers_zero_grids_and_bad_shapes(L):
    p, z = 4096, None                                                    # `p` is never dereferenced: the refusal comes first
    ch = DRV.constants()["chunk"]
    big_x, big_yz, many = (1 << 32) // DRV.constants()["lanes"], 65536, (1 << 14) + 1
    calls = [
        # eval: null pointers; zero and oversized grids; seg_len zero, below a chunk, no multiple; no points; !record with segments or a short stride
        L.dp_driver_eval(0, z, 8, 8, p, 8, 8, p, 8, ch, 1, 1, 1, z), L.dp_driver_eval(0, p, 8, 8, z, 8, 8, p, 8, ch, 1, 1, 1, z),
        L.dp_driver_eval(1, p, 8, 8, p, 8, 8, z, 8, ch, 1, 1, 1, z), L.dp_driver_eval(0, p, 8, 8, p, 8, 8, p, 8, ch, 0, 1, 1, z),
        L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch, 1, 0, 1, z), L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch, 1, 1, 0, z),
        L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch, big_x, 1, 1, z), L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch, 1, big_yz, 1, z),
        L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch, 1, 1, big_yz, z), L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, 0, 1, 1, 1, z),
        L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch - 1, 1, 1, 1, z), L.dp_driver_eval(1, p, 8, 8, p, 8, 8, p, 8, ch + 1, 1, 1, 1, z),
        L.dp_driver_eval(0, p, 8, 8, p, 8, 0, p, 8, ch, 1, 1, 1, z), L.dp_driver_eval(0, p, 8, 8, p, 8, 8, p, 8, ch, 1, 2, 1, z),
        L.dp_driver_eval(0, p, 8, 8, p, 8, 8, p, 7, ch, 1, 1, 1, z),
        L.dp_driver_eval_sum(z, 2, 8, p, 8, 1, 1, z), L.dp_driver_eval_sum(p, 2, 8, z, 8, 1, 1, z), L.dp_driver_eval_sum(p, 0, 8, p, 8, 1, 1, z),
        L.dp_driver_eval_sum(p, 2, 0, p, 8, 1, 1, z), L.dp_driver_eval_sum(p, 2, 8, p, 7, 1, 1, z), L.dp_driver_eval_sum(p, 2, 8, p, 8, 0, 1, z),
        L.dp_driver_eval_sum(p, 2, 8, p, 8, big_x, 1, z), L.dp_driver_eval_sum(p, 2, 8, p, 8, 1, 0, z), L.dp_driver_eval_sum(p, 2, 8, p, 8, 1, big_yz, z),
        # weights: n of 0 and above 2^14; seg_len; !record with segments
        L.dp_driver_weights(1, z, 8, 8, ch, p, p, 1, 1, z), L.dp_driver_weights(1, p, 8, 8, ch, z, p, 1, 1, z), L.dp_driver_weights(0, p, 8, 8, ch, p, z, 1, 1, z),
        L.dp_driver_weights(1, p, 8, 0, ch, p, p, 1, 1, z), L.dp_driver_weights(1, p, 8, many, ch, p, p, 1, 1, z),
        L.dp_driver_weights(1, p, 8, 8, 0, p, p, 1, 1, z), L.dp_driver_weights(1, p, 8, 8, ch + 1, p, p, 1, 1, z),
        L.dp_driver_weights(1, p, 8, 8, ch, p, p, 0, 1, z), L.dp_driver_weights(1, p, 8, 8, ch, p, p, 1, 0, z),
        L.dp_driver_weights(1, p, 8, 8, ch, p, p, big_yz, 1, z), L.dp_driver_weights(1, p, 8, 8, ch, p, p, 1, big_yz, z),
        L.dp_driver_weights(0, p, 8, 8, ch, p, p, 2, 1, z),
        L.dp_driver_weights_fold(z, 2, 8, p, p, 1, z), L.dp_driver_weights_fold(p, 2, 8, z, p, 1, z), L.dp_driver_weights_fold(p, 2, 8, p, z, 1, z),
        L.dp_driver_weights_fold(p, 0, 8, p, p, 1, z), L.dp_driver_weights_fold(p, 2, 0, p, p, 1, z), L.dp_driver_weights_fold(p, 2, many, p, p, 1, z),
        L.dp_driver_weights_fold(p, 2, 8, p, p, 0, z), L.dp_driver_weights_fold(p, 2, 8, p, p, big_yz, z),
        # domain: every pointer; n; log_N above 14; seg_len; grids; !record with segments
        L.dp_driver_domain(1, z, 8, p, 8, p, 8, 8, 3, ch, p, p, 1, 1, z), L.dp_driver_domain(1, p, 8, z, 8, p, 8, 8, 3, ch, p, p, 1, 1, z),
        L.dp_driver_domain(1, p, 8, p, 8, z, 8, 8, 3, ch, p, p, 1, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, z, p, 1, 1, z),
        L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, p, z, 1, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 0, 3, ch, p, p, 1, 1, z),
        L.dp_driver_domain(1, p, 8, p, 8, p, 8, many, 14, ch, p, p, 1, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 15, ch, p, p, 1, 1, z),
        L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, 0, p, p, 1, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, 3 * ch // 2, p, p, 1, 1, z),
        L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, p, p, 0, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, p, p, 1, 0, z),
        L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, p, p, big_yz, 1, z), L.dp_driver_domain(1, p, 8, p, 8, p, 8, 8, 3, ch, p, p, 1, big_yz, z),
        L.dp_driver_domain(0, p, 8, p, 8, p, 8, 8, 3, ch, p, p, 2, 1, z),
        L.dp_driver_domain_fold(z, 2, 8, p, 1, z), L.dp_driver_domain_fold(p, 2, 8, z, 1, z), L.dp_driver_domain_fold(p, 0, 8, p, 1, z),
        L.dp_driver_domain_fold(p, 2, 0, p, 1, z), L.dp_driver_domain_fold(p, 2, many, p, 1, z), L.dp_driver_domain_fold(p, 2, 8, p, 0, z),
        L.dp_driver_domain_fold(p, 2, 8, p, big_yz, z),
        L.dp_driver_pow(z, p, 4, p, z), L.dp_driver_pow(p, z, 4, p, z), L.dp_driver_pow(p, p, 4, z, z), L.dp_driver_pow(p, p, 0, p, z),
        L.dp_driver_pow(p, p, 4097, p, z),
        L.dp_driver_invert(z, 4, p, p, z), L.dp_driver_invert(p, 4, z, p, z), L.dp_driver_invert(p, 4, p, z, z), L.dp_driver_invert(p, 0, p, p, z),
        L.dp_driver_invert(p, many, p, p, z),
    ]
    assert calls == [DRV.INVALID] * len(calls)
