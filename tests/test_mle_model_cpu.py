"""No GPU: tests/mle_model.py (the integer model that tests/test_gpu_mle_kernels.py judges the kernels of csrc/mle_kernels.hpp with)
against the CPU oracle, on random tables and on every fill of tests/tables.py -- the two check each other before either judges a kernel --
and the refusals of tests/cpp/mle_kernels_driver.hip, which come before a device is touched."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mle_kernels_driver as DRV  # noqa: E402
import mle_model as M  # noqa: E402
import tables as T  # noqa: E402

R = T.R
KINDS = ["random"] + T.FILLS
SPECIAL = [0, 1, R - 1]


def table(ora, kind, n, seed):
    return ora.random_fr(n, seed) if kind == "random" else T.fill(kind, n, seed)


def points(ora, k, seed, special=None):
    """k random points; `special` replaces the first, the middle and the last one"""
    pts = M.unpack(ora.random_fr(k, seed))
    if special is not None:
        pts[0] = pts[k // 2] = pts[-1] = special
    return pts


def eq(table_limbs, ints):
    return np.array_equal(np.asarray(table_limbs, dtype=np.uint64).reshape(-1, 4), M.pack(ints))


def test_pack_and_unpack_are_the_conversions_of_the_package(ora):
    from zk_cryptography_amd import Fr
    vals = [0, 1, 2, R - 1, R - 2, (1 << 254) + 5, random.Random(1).randrange(R)]
    assert np.array_equal(M.pack(vals), Fr.from_ints(vals)) and np.array_equal(M.pack(vals), ora.fr_from_ints(vals))
    a = T.fill("top", 16, 3)
    assert M.unpack(a) == Fr.to_ints(a) == ora.fr_to_ints(a)


@pytest.mark.parametrize("kind", KINDS)
def test_fold_every_variable(ora, kind):
    a = table(ora, kind, 32, 11)
    t = M.unpack(a)
    for r in points(ora, 2, 12) + SPECIAL:
        for var in range(5):
            want = ora.mle_partial_evaluation(a, M.pack([r])[0], var)
            assert eq(want, M.fold(t, r, 4 - var)), (r, var)


def test_fold_partner_index_is_the_pair_list_of_the_reference():
    """pick_pairs_with_random_index: for variable k of n entries, (i, i + n >> (k + 1)) for every i whose bit is clear, in order"""
    for log_n in range(1, 7):
        n = 1 << log_n
        for var in range(log_n):
            half = n >> (var + 1)
            lows = [i for i in range(n) if not i & half]
            assert [M.fold_lo_index(j, log_n - 1 - var) for j in range(n // 2)] == lows


@pytest.mark.parametrize("kind", KINDS)
def test_half_sums_and_fold_tail(ora, kind):
    a = table(ora, kind, 64, 21)
    t = M.unpack(a)
    assert eq(ora.mle_half_sums(a), list(M.half_sums(t)))
    assert M.half_sums(t[:1]) == (0, t[0])                              # what the kernels do with one entry: an empty lower half
    for special in [None] + SPECIAL:
        pts = points(ora, 6, 22, special)
        assert eq(ora.mle_evaluation(a, M.pack(pts)), M.fold_tail(t, pts))
        assert eq(ora.mle_partial_evaluations(a, M.pack(pts[:4]), [0] * 4), M.fold_tail(t, pts[:4]))
    assert M.fold_tail(t, []) == t


@pytest.mark.parametrize("kind", KINDS)
def test_distinct_repeat_and_bytes(ora, kind):
    a, b = table(ora, kind, 4, 31), table(ora, "random" if kind == "random" else T.rotation(T.FILLS, kind, 2)[1], 16, 32)
    ta, tb = M.unpack(a), M.unpack(b)
    for x, y, tx, ty in ((a, b, ta, tb), (b, a, tb, ta), (a[:1], b, ta[:1], tb), (b, a[:1], tb, ta[:1])):
        assert eq(ora.mle_add_distinct(x, y), M.distinct(tx, ty, False))
        assert eq(ora.mle_mul_distinct(x, y), M.distinct(tx, ty, True))
    for v in (0, 1, 3):
        assert eq(ora.mle_add_to_front(b, v), M.repeat(tb, 0, len(tb) * 2 << v))
        assert eq(ora.mle_add_to_back(b, v), M.repeat(tb, v, len(tb) << v))
    assert ora.mle_to_bytes(b) == M.to_bytes(tb)
    assert M.to_bytes([0, R - 1]) == bytes(32) + (R - 1).to_bytes(32, "big")


@pytest.mark.parametrize("kind", KINDS)
def test_elementwise(ora, kind):
    a, b = table(ora, kind, 8, 41), table(ora, "random" if kind == "random" else T.rotation(T.FILLS, kind, 3)[2], 8, 42)
    ta, tb = M.unpack(a), M.unpack(b)
    assert eq([ora.fr_add(x, y) for x, y in zip(a, b)], M.elementwise(0, ta, tb))
    assert eq([ora.fr_sub(x, y) for x, y in zip(a, b)], M.elementwise(1, ta, tb))
    assert M.elementwise(1, ta, ta) == [0] * 8 and M.elementwise(0, ta, [(R - v) % R for v in ta]) == [0] * 8
    for s in SPECIAL + [tb[0]]:
        assert eq([ora.fr_mul(x, M.pack([s])[0]) for x in a], M.elementwise(2, ta, scalar=s))


@pytest.mark.parametrize("kind", KINDS)
def test_open_steps(ora, kind):
    """the oracle's kzg_open keeps its quotients to itself: the rounds are held to what defines them -- the quotient is f(1, .) - f(0, .),
    the remainder the table folded at the point, the last remainder the evaluation"""
    a = table(ora, kind, 32, 51)
    t = M.unpack(a)
    for special in [None] + SPECIAL:
        pts = points(ora, 5, 52, special)
        quotients, rems = M.open_steps(t, pts)
        assert len(quotients) == 31 and [len(x) for x in rems] == [16, 8, 4, 2, 1]
        cur, off = a, 0
        for i, z in enumerate(pts):
            h = len(cur) // 2
            assert eq([ora.fr_sub(cur[j + h], cur[j]) for j in range(h)], quotients[off:off + h])
            cur = ora.mle_partial_evaluation(cur, M.pack([z])[0], 0)
            assert eq(cur, rems[i])
            off += h
        assert eq(ora.mle_evaluation(a, M.pack(pts)), rems[-1])
        assert M.open_step(t, pts[0]) == (quotients[:16], rems[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 9, 40])
def test_horner_suffix(ora, kind, n):
    c = table(ora, kind, n, 61)
    t = M.unpack(c)
    n = len(t)                                                           # (the two-halves fills give an even length)
    for z in points(ora, 1, 62) + SPECIAL:
        v = M.horner_suffix(t, z)
        assert eq(ora.dense_evaluate(c, M.pack([z])[0]), v[:1])
        assert v[0] == sum(x * pow(z, i, R) for i, x in enumerate(t)) % R
        if n > 1 and t[-1]:
            q, rem = ora.dense_divide(c, M.pack([-z, 1]))                # (p(x) - p(z)) / (x - z) has the quotient of p(x) / (x - z)
            assert eq(q, v[1:]) and eq(rem, v[:1] if v[0] else [])
        nz = {i: x for i, x in enumerate(t) if x}
        assert M.horner_suffix_sparse(nz, z, range(n)) == v


def test_dense_degree():
    assert M.dense_degree([]) == 0 and M.dense_degree([0, 0, 0]) == 0 and M.dense_degree([5, 0, 0]) == 0
    assert M.dense_degree([0, 5, 0, R, 0]) == 1 and M.dense_degree([0] * 9 + [1]) == 9


def test_circuit_tables(ora):
    layers = [[("mul", 0, 1)], [("add", 0, 3), ("mul", 2, 1)], [("mul", 1, 1), ("add", 0, 7), ("add", 6, 5), ("mul", 3, 4)]]
    inp = T.fill("uniform_r", 8, 71)
    ev = ora.circuit_evaluation(layers, inp)                             # output layer first, the input last
    cur = M.unpack(inp)
    for k in (2, 1, 0):
        cur = M.circuit_layer(cur, [(0 if g[0] == "add" else 1, g[1], g[2]) for g in layers[k]])
        assert eq(ev[k], cur)
    for k in (1, 2):
        add, mul = ora.circuit_add_mult_mle(layers, k)
        w_add, w_mul = M.wiring_ones([(0 if g[0] == "add" else 1, g[1], g[2]) for g in layers[k]], k + 1, ora.gkr_mle_size(k))
        assert eq(add, w_add) and eq(mul, w_mul)


@pytest.mark.parametrize("kind", ["random", "uniform_r", "top", "limb_edges", "one_hot"])
def test_eq_tables_weigh_a_table_to_its_evaluation(ora, kind):
    a = table(ora, kind, 128, 81)
    t = M.unpack(a)
    for special in [None] + SPECIAL:
        pts = points(ora, 7, 82, special)
        want = M.unpack(ora.mle_evaluation(a, M.pack(pts)))[0]
        assert sum(w * x for w, x in zip(M.eq_table(pts), t)) % R == want
        for k1, s in ((2, 2), (3, 0), (1, 6), (4, 1)):
            k2 = 7 - k1
            w1, wa, wb = M.eval_weights(pts, k1, k2, s)
            assert len(w1) == 1 << k1 and len(wa) == 1 << (k2 - s) and len(wb) == 1 << s
            m, inv = 1 << k2, pow(M.W_FACTOR, -1, R)
            got = sum(w1[b] * inv * wa[j >> s] * wb[j & ((1 << s) - 1)] * t[b * m + j] for b in range(1 << k1) for j in range(m)) % R
            assert got == want
        assert M.eq_weights(pts, 2, 3) == [w * M.W_FACTOR % R for w in M.eq_table(pts[2:5])]
    assert M.sum_records(t) == M.unpack(ora.mle_sum(a))[0]


def test_weight_factor_is_the_constant_of_the_kernels():
    """eq_weights_kernel and eval_weights_kernel start their products from these eight words: the stored form of 2^32"""
    words = [0xcaaf6b13, 0x355094ea, 0x69a568ef, 0xf6b10cb3, 0x40cc3869, 0xe2c926a6, 0xed269aad, 0x736a6d3b]
    assert T.to_int(T.stored(1 << 32)) == sum(w << (32 * i) for i, w in enumerate(words))
    assert [M.evaluation_split(l) for l in (17, 18, 22)] == [(4, 13, 6), (5, 13, 6), (8, 14, 7)]


# ---- the driver: built for gfx950, refusals before a device is touched ----------------------------------------
@pytest.fixture(scope="module")
def L():
    return DRV.lib()


def test_driver_builds_and_knows_the_library_grids(L):
    assert os.path.exists(DRV.LIB_PATH)
    assert L.mle_driver_block() == DRV.BLOCK and L.mle_driver_horner_block() == DRV.HORNER_BLOCK and L.mle_driver_tail_n() == 4096
    assert all(hasattr(L, "mle_driver_" + name) for name in DRV.LAUNCHERS)
    assert [DRV.library_grid(n, False) for n in (0, 1, 256, 257, 1 << 19, (1 << 19) + 1, 1 << 30)] == [1, 1, 1, 2, 2048, 2048, 2048]
    assert [DRV.library_grid(n, True) for n in (0, 1, 257, 1 << 22, (1 << 22) + 1, 1 << 30)] == [1, 1, 2, 16384, 16384, 16384]


def test_driver_refuses_null_pointers_and_bad_shapes(L):
    p, z = 4096, None                                                    # `p` is never dereferenced: the refusal comes first
    calls = [
        L.mle_driver_fold(z, p, 4, 0, p, z, z, 1, z), L.mle_driver_fold(p, p, 4, 0, p, p, z, 1, z), L.mle_driver_fold(p, p, 4, 0, z, z, z, 1, z),
        L.mle_driver_fold(p, p, 3, 0, p, z, z, 1, z), L.mle_driver_fold(p, p, 4, 3, p, z, z, 1, z), L.mle_driver_fold(p, p, 4, 0, p, z, z, 0, z),
        L.mle_driver_half_sums(p, 0, p, 1, z), L.mle_driver_half_sums(p, 8, z, 1, z), L.mle_driver_finish_sums(p, 0, p, z),
        L.mle_driver_fold_tail(p, 8192, p, 0, 1, p, z), L.mle_driver_fold_tail(p, 8, p, 0, 4, p, z), L.mle_driver_fold_tail(p, 8, p, 47, 2, p, z),
        L.mle_driver_distinct(0, p, 0, p, 4, p, 1, z), L.mle_driver_distinct(1, p, 4, z, 4, p, 1, z),
        L.mle_driver_elementwise(3, p, p, p, 4, p, 1, z), L.mle_driver_elementwise(0, p, z, p, 4, p, 1, z),
        L.mle_driver_elementwise(2, p, p, z, 4, p, 1, z), L.mle_driver_elementwise(1, p, p, z, 0, p, 1, z),
        L.mle_driver_to_bytes(p, 4, z, 1, z), L.mle_driver_to_bytes(p, 4, p, (1 << 20) + 1, z),
        L.mle_driver_repeat(p, 3, 0, 8, p, 1, z), L.mle_driver_repeat(p, 4, 1, 9, p, 1, z), L.mle_driver_repeat(p, 4, 41, 8, p, 1, z),
        L.mle_driver_open_step(p, 6, p, p, p, 1, z), L.mle_driver_open_step(p, 8, z, p, p, 1, z),
        L.mle_driver_open_steps_small(p, 8192, p, 1, p, p, p, z), L.mle_driver_open_steps_small(p, 8, p, 4, p, p, p, z),
        L.mle_driver_open_steps_small(p, 8, p, 0, p, p, p, z),
        L.mle_driver_open_steps_small_batch(p, 0, 8, p, 3, p, 7, p, 4, p, 2, p, z),
        L.mle_driver_open_steps_small_batch(p, 2, 8, p, 3, p, 6, p, 4, p, 2, p, z),
        L.mle_driver_open_steps_small_batch(p, 2, 8, p, 3, p, 7, p, 3, p, 2, p, z),
        L.mle_driver_open_steps_small_batch(p, 2, 8, p, 3, p, 7, p, 4, p, 2, z, z),
        L.mle_driver_horner_eval(p, 0, p, p, p, p, z), L.mle_driver_horner_eval(p, 8, p, p, p, z, z), L.mle_driver_horner_eval(p, 1 << 31, p, p, p, p, z),
        L.mle_driver_horner_divide(p, 8, z, p, p, p, p, z), L.mle_driver_horner_divide(p, 0, p, p, p, p, p, z),
        L.mle_driver_dense_degree(p, 0, p, 1, z), L.mle_driver_dense_degree(p, 8, z, 1, z),
        L.mle_driver_circuit_layer(p, z, 4, p, 1, z), L.mle_driver_wiring_ones(p, 4, 14, p, p, 1, z), L.mle_driver_wiring_ones(p, 0, 2, p, p, 1, z),
        L.mle_driver_eq_weights(p, 0, 0, p, z), L.mle_driver_eq_weights(p, 0, 10, p, z), L.mle_driver_eq_weights(p, 46, 3, p, z),
        L.mle_driver_eval_weights(p, 0, 8, 4, p, p, p, z), L.mle_driver_eval_weights(p, 4, 8, 9, p, p, p, z),
        L.mle_driver_eval_weights(p, 8, 41, 20, p, p, p, z), L.mle_driver_sum_records(p, 0, p, z), L.mle_driver_sum_records(z, 4, p, z),
    ]
    assert calls == [DRV.INVALID] * len(calls)
