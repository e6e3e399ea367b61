"""GPU: every operation of csrc/pairing.hpp on its own, against the independent model tests/pairing_model.py, bit for bit.

test_gpu_pairing.py and test_gpu_kzg_verify.py reach this code end to end on well-behaved pairs, which catches a formula that is wrong
everywhere.  Here each operation is launched through tests/cpp/pairing_driver.hip, one element per lane, on the inputs where a formula
can be wrong somewhere: zero, one, minus one, elements of the embedded subfields, components 0, 1, p - 1, the Montgomery constants, the
five aliasing forms of f12_mul, accumulators that meet the point they add or its inverse with Z != 1, and points of order 3, 11, 13 and
23 (tests/pairing_cases.py; tests/test_pairing_cases_cpu.py proves that they drive the subgroup checks through the doubling and inverse
branches).  No tolerance: every comparison is equality of Montgomery limbs with the packed canonical integers of the model, so an
unreduced result fails too; where a result has no unique expected limbs (Jacobian coordinates, x^-1 checked as x x^-1 = 1) every limb
vector is checked to be below p before it is used.  Every output buffer is pre-filled with a pattern and carries one guard element
that must keep it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_cases as PC  # noqa: E402
import pairing_driver as DRV  # noqa: E402

pytestmark = pytest.mark.gpu
PM, M = PC.PM, PC.M
P, R = PC.P, PC.R
MONT = (1 << 384) % P
MONT_INV = pow(MONT, -1, P)
PATTERN = 0x5A5A5A5A5A5A5A5A
FLAG_PATTERN = 0x5A5A5A5A
# Fq components every pool draws from: the ends of the range, the middle, a high power of two and the two Montgomery constants
EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 380, MONT, MONT * MONT % P]
F2_ZERO, F2_ONE = (0, 0), (1, 0)
ZERO12 = [F2_ZERO] * 6


def op(group, name):
    return group.index(name)


# ---- plumbing: python ints <-> device tensors of Montgomery limbs ------------------------------------------------------------------
def pack(rows):
    """rows of canonical ints -> uint64 [n, 6 len(row)] Montgomery limbs, with integers only"""
    raw = b"".join((v % P * MONT % P).to_bytes(48, "little") for row in rows for v in row)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(rows), -1).copy()


def dev(rows):
    import torch
    return torch.from_numpy(pack(rows).view(np.int64)).cuda()


def dev_scalars(ks):
    """canonical 256-bit scalars as 8 x u32, NOT Montgomery"""
    import torch
    raw = b"".join(int(k).to_bytes(32, "little") for k in ks)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int32).reshape(len(ks), 8).copy()).cuda()


def outbuf(n, words):
    """n elements and one guard, all pattern"""
    import torch
    return torch.full((n + 1, words), PATTERN, dtype=torch.int64, device="cuda")


def flagbuf(n):
    import torch
    return torch.full((n + 1,), FLAG_PATTERN, dtype=torch.int32, device="cuda")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def launched(status):
    assert status == 0, "launcher returned hipError %d" % status


def limbs_of(buf, what):
    """the n output rows as uint64, after the guard behind them was seen untouched"""
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[-1] == np.uint64(PATTERN)).all(), what + ": the element behind the output was written"
    return got[:-1]


def check(buf, want_rows, what):
    """all of `want_rows`, bit for bit (so every limb vector is the canonical one, below p), and the guard untouched"""
    got = limbs_of(buf, what)
    exp = pack(want_rows)
    assert got.shape == exp.shape, what
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        raise AssertionError("%s: %d of %d elements differ, the first at index %d" % (what, len(bad), len(want_rows), bad[0]))


def ints_of(buf, what):
    """output rows -> rows of canonical ints; a limb vector that is not below p is a failure"""
    rows = []
    for i, row in enumerate(limbs_of(buf, what)):
        vals = []
        for k in range(0, len(row), 6):
            v = int.from_bytes(row[k: k + 6].tobytes(), "little")
            assert v < P, "%s: element %d holds an unreduced limb vector" % (what, i)
            vals.append(v * MONT_INV % P)
        rows.append(vals)
    return rows


def flags_of(buf, what):
    got = buf.cpu().numpy().view(np.uint32)
    assert got[-1] == FLAG_PATTERN, what + ": the flag behind the output was written"
    return [int(v) for v in got[:-1]]


# ---- the model's side: Fq2 tuples, Fq6 as the even w-coefficients, Fq12 in the w-basis ---------------------------------------------------
def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def flat2(a):
    return [a[0], a[1]]


def tower(a):
    """w-basis Fq12 -> the device's 12 ints"""
    return PM.f12_to_tower(a)


def f6_embed(c):
    """(c0, c1, c2) of Fq6 = Fq2[v] -> Fq12, v = w^2"""
    return [c[0], F2_ZERO, c[1], F2_ZERO, c[2], F2_ZERO]


def f6_row(c):
    return flat2(c[0]) + flat2(c[1]) + flat2(c[2])


def f6_of(a, what):
    assert a[1] == a[3] == a[5] == F2_ZERO, what
    return (a[0], a[2], a[4])


def f12_add(a, b):
    return [PM.f2_add(x, y) for x, y in zip(a, b)]


def f12_neg(a):
    return [f2_neg(x) for x in a]


def rows_to_f12(rows):
    return [PC.f12_from_tower(r) for r in rows]


def rng_fq(rng):
    return int.from_bytes(rng.bytes(48), "little") % P


def f2_pool(rng, n_random):
    return [(a, b) for a in EDGE for b in EDGE] + [(rng_fq(rng), rng_fq(rng)) for _ in range(n_random)]


def f12_pool(rng):
    """zero, one, minus one, the embedded subfields, each of the six positions alone, xi and its inverse, all components p - 1, random"""
    r2 = lambda: (rng_fq(rng), rng_fq(rng))          # noqa: E731
    one, top = PM.f12_one(), (P - 1, P - 1)
    pool = [ZERO12, one, f12_neg(one)]
    pool += [[(e, 0)] + [F2_ZERO] * 5 for e in EDGE[2:]]                                   # Fq
    pool += [[c] + [F2_ZERO] * 5 for c in ((0, 1), (0, P - 1), top, (MONT, P - 2), r2())]  # Fq2
    pool += [[PM.XI] + [F2_ZERO] * 5, [PM.XI_INV] + [F2_ZERO] * 5]
    pool += [f6_embed(c) for c in ((F2_ONE, F2_ONE, F2_ONE), (top, top, top), (F2_ZERO, F2_ONE, F2_ZERO), (r2(), r2(), r2()))]     # Fq6
    for k in range(6):                                                                      # one non-zero coefficient
        for c in (F2_ONE, (0, 1), top, r2()):
            pool.append([c if j == k else F2_ZERO for j in range(6)])
    pool.append([top] * 6)
    pool += [[r2() for _ in range(6)] for _ in range(4)]
    return pool


def pairs_of(pool, n):
    """n pairs of pool elements: every element meets zero, one, minus one and itself, the rest is a fixed shuffle"""
    m, out = len(pool), []
    for i in range(m):
        out += [(pool[i], pool[0]), (pool[1], pool[i]), (pool[i], pool[2]), (pool[i], pool[i])]
    k = 0
    while len(out) < n:
        out.append((pool[(5 * k + 3) % m], pool[(11 * k + 7) % m]))
        k += 1
    return out[:n]


def run_f12(name, a_rows, b_rows=None):
    n = len(a_rows)
    a, b = dev(a_rows), None if b_rows is None else dev(b_rows)
    out = outbuf(n, 72)
    launched(DRV.lib().pairing_driver_f12(op(DRV.F12_OPS, name), ptr(a), ptr(b), ptr(out), None, n, stream()))
    return out


# ---- Fq2 -------------------------------------------------------------------------------------------------------------------------
def test_fq2_operations():
    rng = np.random.default_rng(2)
    pool = f2_pool(rng, 28)                                      # 128 elements
    n = len(pool)
    b_pool = [pool[(37 * i + 11) % n] for i in range(n)]         # 37 is prime to 128: every element appears once on each side
    a, b = dev([flat2(x) for x in pool]), dev([flat2(x) for x in b_pool])
    sqr = lambda x: PM.f2_mul(x, x)                              # noqa: E731
    model = {"add": PM.f2_add, "sub": PM.f2_sub, "neg": lambda x, y: f2_neg(x), "dbl": lambda x, y: PM.f2_add(x, x),
             "conj": lambda x, y: (x[0], (-x[1]) % P), "mul": PM.f2_mul, "sqr": lambda x, y: sqr(x),
             "mul_fq": lambda x, y: PM.f2_scale(x, y[0]), "mul_xi": lambda x, y: PM.f2_mul(x, PM.XI)}
    for name, f in model.items():
        out = outbuf(n, 12)
        launched(DRV.lib().pairing_driver_f2(op(DRV.F2_OPS, name), ptr(a), ptr(b), ptr(out), n, stream()))
        check(out, [flat2(f(x, y)) for x, y in zip(pool, b_pool)], "f2 " + name)
    out = outbuf(n, 12)
    launched(DRV.lib().pairing_driver_f2(op(DRV.F2_OPS, "inverse"), ptr(a), None, ptr(out), n, stream()))
    inv = ints_of(out, "f2 inverse")
    assert pool[0] == F2_ZERO
    for x, y in zip(pool, inv):
        # Fermat: the inverse of zero is zero (g2_to_affine never asks for it, and this is what it would get)
        assert PM.f2_mul(x, tuple(y)) == (F2_ZERO if x == F2_ZERO else F2_ONE), x
    # the same input object may be the operand twice: x * x and x - x through the binary forms
    for name, want in (("mul", [flat2(sqr(x)) for x in pool]), ("sub", [[0, 0]] * n), ("add", [flat2(PM.f2_add(x, x)) for x in pool])):
        out = outbuf(n, 12)
        launched(DRV.lib().pairing_driver_f2(op(DRV.F2_OPS, name), ptr(a), ptr(a), ptr(out), n, stream()))
        check(out, want, "f2 %s of an element with itself" % name)


# ---- Fq6 -------------------------------------------------------------------------------------------------------------------------
def test_fq6_operations():
    rng = np.random.default_rng(6)
    comp = [F2_ZERO, F2_ONE, (0, 1), (P - 1, P - 1), (P - 1, 0), PM.XI, PM.XI_INV, (MONT, (P + 1) // 2), (1 << 380, P - 2)]
    pool = [(a, b, c) for a in comp[:4] for b in comp[:4] for c in comp[:4]]                       # 64 structured
    pool += [(comp[(i + 4) % 9], comp[(2 * i + 5) % 9], comp[(3 * i + 6) % 9]) for i in range(32)]
    pool += [tuple((rng_fq(rng), rng_fq(rng)) for _ in range(3)) for _ in range(32)]               # 128 in all
    n = len(pool)
    b_pool = [pool[(37 * i + 11) % n] for i in range(n)]
    a, b = dev([f6_row(x) for x in pool]), dev([f6_row(x) for x in b_pool])
    mul = lambda x, y: f6_of(PM.f12_mul(f6_embed(x), f6_embed(y)), "a product of Fq6 elements left Fq6")     # noqa: E731
    model = {"mul": mul, "mul_01": lambda x, y: mul(x, (y[0], y[1], F2_ZERO)), "mul_1": lambda x, y: mul(x, (F2_ZERO, y[1], F2_ZERO)),
             "mul_v": lambda x, y: mul(x, (F2_ZERO, F2_ONE, F2_ZERO))}
    for name, f in model.items():
        out = outbuf(n, 36)
        launched(DRV.lib().pairing_driver_f6(op(DRV.F6_OPS, name), ptr(a), ptr(b), ptr(out), n, stream()))
        check(out, [f6_row(f(x, y)) for x, y in zip(pool, b_pool)], "f6 " + name)
    out = outbuf(n, 36)
    launched(DRV.lib().pairing_driver_f6(op(DRV.F6_OPS, "inverse"), ptr(a), None, ptr(out), n, stream()))
    inv = ints_of(out, "f6 inverse")
    zero6, one6 = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)
    assert pool[0] == zero6
    for x, y in zip(pool, inv):
        y6 = ((y[0], y[1]), (y[2], y[3]), (y[4], y[5]))
        assert mul(x, y6) == (zero6 if x == zero6 else one6), x


# ---- Fq12: products, squares, inverses ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f12_elems():
    return f12_pool(np.random.default_rng(12))


def test_f12_mul_in_all_five_aliasing_forms(f12_elems):
    pairs = pairs_of(f12_elems, 256)
    a_rows, b_rows = [tower(x) for x, _ in pairs], [tower(y) for _, y in pairs]
    want = [tower(PM.f12_mul(x, y)) for x, y in pairs]
    for name in ("mul_distinct", "mul_r_is_a", "mul_r_is_b"):
        check(run_f12(name, a_rows, b_rows), want, "f12_mul, form " + name)
    elems = f12_elems
    rows = [tower(x) for x in elems]
    squares = [tower(PM.f12_mul(x, x)) for x in elems]
    for name in ("mul_a_is_b", "mul_all_same", "sqr"):
        check(run_f12(name, rows), squares, "f12 square, form " + name)


def test_f12_mul_014_equals_the_dense_product(f12_elems):
    rng = np.random.default_rng(14)
    r2 = lambda: (rng_fq(rng), rng_fq(rng))          # noqa: E731
    top = (P - 1, P - 1)
    lines = [(r2(), r2(), r2()), (F2_ZERO, r2(), r2()), (r2(), F2_ZERO, r2()), (r2(), r2(), F2_ZERO), (F2_ZERO, F2_ZERO, r2()),
             (F2_ZERO, r2(), F2_ZERO), (r2(), F2_ZERO, F2_ZERO), (F2_ZERO, F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO, F2_ZERO), (top, top, top),
             (F2_ONE, F2_ONE, F2_ONE), ((0, 1), (0, P - 1), (MONT, 0))]
    cases = [(x, lines[(i + j) % len(lines)]) for i, x in enumerate(f12_elems) for j in range(4)][:256]
    # c0 + c1 v + c4 v w in the w-basis: positions 0, 2 and 3
    sparse = [[c0, F2_ZERO, c1, c4, F2_ZERO, F2_ZERO] for _, (c0, c1, c4) in cases]
    want = [tower(PM.f12_mul(x, s)) for (x, _), s in zip(cases, sparse)]
    check(run_f12("mul_014", [tower(x) for x, _ in cases], [tower(s) for s in sparse]), want, "f12_mul_014")


def test_f12_inverse_conj_and_is_one(f12_elems):
    rows = [tower(x) for x in f12_elems]
    n = len(rows)
    inv = rows_to_f12(ints_of(run_f12("inverse", rows), "f12_inverse"))
    one = PM.f12_one()
    assert f12_elems[0] == ZERO12
    for x, y in zip(f12_elems, inv):
        assert PM.f12_mul(x, y) == (ZERO12 if x == ZERO12 else one)        # the inverse of zero is zero
    check(run_f12("conj", rows), [tower(PC.f12_conj(x)) for x in f12_elems], "f12_conj")
    flag = flagbuf(n)
    a = dev(rows)
    launched(DRV.lib().pairing_driver_f12(op(DRV.F12_OPS, "is_one"), ptr(a), None, None, ptr(flag), n, stream()))
    got = flags_of(flag, "f12_is_one")
    assert got == [1 if x == one else 0 for x in f12_elems] and 1 <= sum(got) < n


# ---- Frobenius -------------------------------------------------------------------------------------------------------------------------
def test_frobenius_maps(f12_elems):
    elems = f12_elems
    rows = [tower(x) for x in elems]
    f1 = rows_to_f12(ints_of(run_f12("frob1", rows), "f12_frobenius<1>"))
    f2 = rows_to_f12(ints_of(run_f12("frob2", rows), "f12_frobenius<2>"))
    # against the model's plain powers on a handful: a dense random element, all components p - 1, and one element per odd position
    # (each has its own constant) -- the powers are the cost of this test
    picks = [len(elems) - 1, len(elems) - 5] + [next(i for i, x in enumerate(elems) if x[k] != F2_ZERO and sum(c != F2_ZERO for c in x) == 1)
                                                for k in (1, 3, 5)]
    for i in picks:
        assert f1[i] == PM.f12_pow(elems[i], P), i
        assert f2[i] == PM.f12_pow(elems[i], P * P), i
    # the rest: both maps are ring homomorphisms, against the device's own product (pinned above) and the exact sum
    pairs = pairs_of(elems, 192)
    index = {id(x): i for i, x in enumerate(elems)}
    prod = rows_to_f12(ints_of(run_f12("mul_distinct", [tower(x) for x, _ in pairs], [tower(y) for _, y in pairs]), "f12_mul"))
    sums = [f12_add(x, y) for x, y in pairs]
    for name, imgs in (("frob1", f1), ("frob2", f2)):
        fa, fb = [imgs[index[id(x)]] for x, _ in pairs], [imgs[index[id(y)]] for _, y in pairs]
        check(run_f12(name, [tower(x) for x in prod]), [r for r in ints_of(run_f12("mul_distinct", [tower(x) for x in fa], [tower(y) for y in fb]),
                                                                                   name)], name + " is multiplicative")
        check(run_f12(name, [tower(s) for s in sums]), [tower(f12_add(x, y)) for x, y in zip(fa, fb)], name + " is additive")
    # the p^2 map is the p map twice, and six times the p^2 map is the identity
    check(run_f12("frob1", [tower(x) for x in f1]), [tower(x) for x in f2], "frobenius<1> twice")
    cur = elems
    for _ in range(6):
        cur = rows_to_f12(ints_of(run_f12("frob2", [tower(x) for x in cur]), "frobenius<2>"))
    assert cur == elems


# ---- the cyclotomic subgroup ----------------------------------------------------------------------------------------------------------
def test_cyclotomic_squaring_and_exp_by_x():
    cyc = PC.cyclotomic_elements()
    rows = [tower(x) for x in cyc]
    want = [tower(PM.f12_mul(x, x)) for x in cyc]
    check(run_f12("cyc_sqr", rows), want, "f12_cyclotomic_sqr against the model's square")
    check(run_f12("sqr", rows), want, "f12_sqr on the same elements")
    # the negative control: outside the subgroup the Granger-Scott formulas are NOT a square, so the comparison above can tell
    ctl = PC.not_cyclotomic()
    got = ints_of(run_f12("cyc_sqr", [tower(ctl)]), "f12_cyclotomic_sqr")[0]
    assert got != tower(PM.f12_mul(ctl, ctl))
    check(run_f12("sqr", [tower(ctl)]), [tower(PM.f12_mul(ctl, ctl))], "f12_sqr of the control")
    # a^x, x < 0: a^|x| conjugated
    check(run_f12("exp_by_x", rows), [tower(PC.f12_conj(PM.f12_pow(x, PM.X_ABS))) for x in cyc], "f12_exp_by_x")


def test_final_exponentiation():
    rng = np.random.default_rng(99)
    r2 = lambda: (rng_fq(rng), rng_fq(rng))          # noqa: E731
    in_fq6 = f6_embed((r2(), r2(), r2()))
    elems = [PM.f12_one(), in_fq6, PM.miller_loop(M.G1, PM.G2), PM.miller_loop(M.g1_mul(M.G1, 7), PM.g2_mul(PM.G2, R - 3)),
             [r2() for _ in range(6)]]
    want = [PM.f12_pow(x, PM.FINAL_EXP) for x in elems]
    assert want[0] == want[1] == PM.f12_one() and want[2] != PM.f12_one()        # Fq6* is killed by p^6 - 1
    check(run_f12("final_exp", [tower(x) for x in elems]), [tower(x) for x in want], "final_exponentiation")


# ---- G2 ----------------------------------------------------------------------------------------------------------------------------
def g2_row(q):
    return flat2(q[0]) + flat2(q[1])


def jac_row(q, z):
    """(x z^2, y z^3, z): the affine point under another Z"""
    z2 = PM.f2_mul(z, z)
    return flat2(PM.f2_mul(q[0], z2)) + flat2(PM.f2_mul(q[1], PM.f2_mul(z2, z))) + flat2(z)


def jac_to_affine(row, identity):
    x, y, z = (row[0], row[1]), (row[2], row[3]), (row[4], row[5])
    assert (z == F2_ZERO) == bool(identity), "the identity flag and Z disagree"
    if z == F2_ZERO:
        return None
    zi = PM.f2_inv(z)
    zi2 = PM.f2_mul(zi, zi)
    return PM.f2_mul(x, zi2), PM.f2_mul(y, PM.f2_mul(zi2, zi))


def run_g2(name, a_rows, b_rows=None, ks=None, out_words=0):
    n = len(a_rows)
    a, b = dev(a_rows), None if b_rows is None else dev(b_rows)
    k = None if ks is None else dev_scalars(ks)
    out = outbuf(n, out_words) if out_words else None
    flag = flagbuf(n)
    launched(DRV.lib().pairing_driver_g2(op(DRV.G2_OPS, name), ptr(a), ptr(b), ptr(k), ptr(out), ptr(flag), n, stream()))
    return out, flags_of(flag, "g2 " + name)


@pytest.fixture(scope="module")
def g2_points():
    small = PC.g2_small_order_points()
    return {"gen": PM.G2, "five": PM.g2_mul(PM.G2, 5), "big": PM.g2_mul(PM.G2, 0x1234567890ABCDEF ** 3 % R), 13: small[13], 23: small[23],
            "stray": PC.twist_not_in_subgroup()}


def test_g2_double_and_madd(g2_points):
    rng = np.random.default_rng(22)
    r2 = lambda: (rng_fq(rng), rng_fq(rng))          # noqa: E731
    pts = list(g2_points.values())
    identity = flat2((5, 6)) + flat2((7, 8)) + [0, 0]                     # Z = 0 with stale X, Y: they must not matter
    # doubling: the identity, Z = 1, Z != 1
    acc_rows, want = [identity], [None]
    for q in pts:
        for z in (F2_ONE, r2(), (0, P - 1)):
            acc_rows.append(jac_row(q, z))
            want.append(PM.g2_add(q, q))
    out, ident = run_g2("double", acc_rows, out_words=36)
    got = [jac_to_affine(r, f) for r, f in zip(ints_of(out, "g2_double"), ident)]
    assert got == want
    # mixed addition, the four cases: identity accumulator; generic; acc == q (doubling) and acc == -q (identity out), both under Z != 1
    # so that the collision shows in the projective comparison only, not in equal limbs
    acc_rows, q_rows, want = [], [], []
    for i, q in enumerate(pts):
        other = pts[(i + 1) % len(pts)]
        for acc, z in ((None, None), (other, F2_ONE), (other, r2()), (q, r2()), (q, (P - 1, 0)), (PM.g2_neg(q), r2()), (PM.g2_neg(q), (0, 1)),
                       (q, F2_ONE), (PM.g2_neg(q), F2_ONE), (PM.g2_add(q, q), r2())):
            acc_rows.append(identity if acc is None else jac_row(acc, z))
            q_rows.append(g2_row(q))
            want.append(PM.g2_add(acc, q))
    out, ident = run_g2("madd", acc_rows, q_rows, out_words=36)
    got = [jac_to_affine(r, f) for r, f in zip(ints_of(out, "g2_madd"), ident)]
    assert got == want
    assert sum(w is None for w in want) == 3 * len(pts)


def test_g2_mul_subgroup_and_curve_checks(g2_points):
    rng = np.random.default_rng(23)
    scalars = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(2)]
    names = ["five", 13, 23]
    a_rows = [g2_row(g2_points[nm]) for nm in names for _ in scalars]
    ks = [k for _ in names for k in scalars]
    want = [PM.g2_mul_raw(g2_points[nm], k) for nm in names for k in scalars]
    out, finite = run_g2("mul", a_rows, ks=ks, out_words=24)
    assert finite == [0 if w is None else 1 for w in want]
    check(out, [[0] * 4 if w is None else g2_row(w) for w in want], "g2_mul<8> then g2_to_affine")
    # membership: true inside the subgroup, false for the orders 13 and 23 and for the large-order point the suite always used
    order = ["gen", "five", "big", 13, 23, "stray"]
    _, got = run_g2("in_subgroup", [g2_row(g2_points[nm]) for nm in order])
    assert got == [1, 1, 1, 0, 0, 0]
    off = [PC.off_twist(), (PM.G2[0], PM.f2_add(PM.G2[1], F2_ONE)), (PM.f2_add(PM.G2[0], (0, 1)), PM.G2[1])]
    _, got = run_g2("on_curve", [g2_row(g2_points[nm]) for nm in order] + [g2_row(q) for q in off])
    assert got == [1] * 6 + [0] * 3


# ---- G1, the verifier's side ---------------------------------------------------------------------------------------------------------
def run_g1(name, a_rows, ks=None):
    n = len(a_rows)
    a = dev(a_rows)
    k = None if ks is None else dev_scalars(ks)
    out = outbuf(n, 12) if ks is not None else None
    flag = flagbuf(n)
    launched(DRV.lib().pairing_driver_g1(op(DRV.G1_OPS, name), ptr(a), ptr(k), ptr(out), ptr(flag), n, stream()))
    return out, flags_of(flag, "g1 " + name)


def test_g1_mul_subgroup_and_curve_checks():
    rng = np.random.default_rng(31)
    small = PC.g1_small_order_points()
    pts = {"gen": M.G1, "five": M.g1_mul(M.G1, 5), "big": M.g1_mul(M.G1, 0xFEDCBA9876543210 ** 3 % R), 3: small[3], 11: small[11],
           "stray": PC.g1_not_in_subgroup()}
    scalars = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(2)]
    names = ["gen", "five", 3, 11]
    a_rows = [list(pts[nm]) for nm in names for _ in scalars]
    ks = [k for _ in names for k in scalars]
    plain = [PC.g1_mul_raw(pts[nm], k) for nm in names for k in scalars]
    for name, want in (("mul", plain), ("mul_neg", [PC.g1_neg(w) for w in plain])):
        out, finite = run_g1(name, a_rows, ks)
        assert finite == [0 if w is None else 1 for w in want], name
        check(out, [[0, 0] if w is None else list(w) for w in want], "g1_" + name)
    order = ["gen", "five", "big", 3, 11, "stray"]
    _, got = run_g1("in_subgroup", [list(pts[nm]) for nm in order])
    assert got == [1, 1, 1, 0, 0, 0]
    off = [(1, 1), (M.G1[0], (M.G1[1] + 1) % P), ((M.G1[0] + 1) % P, M.G1[1])]
    _, got = run_g1("on_curve", [list(pts[nm]) for nm in order] + [list(p) for p in off])
    assert got == [1] * 6 + [0] * 3


# ---- Miller steps and the loop ------------------------------------------------------------------------------------------------------
def run_miller(name, n, p=None, q=None, t=None, f=None, out_words=72, want_t=False, prep=None):
    out_t = outbuf(n, 36) if want_t else None
    out = outbuf(n, out_words)
    launched(DRV.lib().pairing_driver_miller(op(DRV.ML_OPS, name), ptr(p), ptr(q), ptr(t), ptr(f), ptr(out_t), ptr(out), ptr(prep), n, stream()))
    return out_t, out


def proj_row(q, z):
    """homogeneous projective (x z, y z, z)"""
    return flat2(PM.f2_mul(q[0], z)) + flat2(PM.f2_mul(q[1], z)) + flat2(z)


def proj_to_affine(row):
    x, y, z = (row[0], row[1]), (row[2], row[3]), (row[4], row[5])
    zi = PM.f2_inv(z)
    return PM.f2_mul(x, zi), PM.f2_mul(y, zi)


def test_miller_steps_and_line_product(g2_points, f12_elems):
    rng = np.random.default_rng(41)
    r2 = lambda: (rng_fq(rng), rng_fq(rng))          # noqa: E731
    qs = [g2_points["gen"], g2_points["five"], g2_points["big"]]
    cases = [(q, z) for q in qs for z in (F2_ONE, r2(), (0, P - 1))]
    n = len(cases)
    t = dev([proj_row(q, z) for q, z in cases])
    t2, lines_d = run_miller("double_step", n, t=t, out_words=36, want_t=True)
    doubled = ints_of(t2, "g2_double_step T")
    assert [proj_to_affine(r) for r in doubled] == [PM.g2_add(q, q) for q, _ in cases]
    # T = 2 Q (as the step left it, Z != 1) plus Q
    qd = dev([g2_row(q) for q, _ in cases])
    t3, lines_a = run_miller("add_step", n, q=qd, t=dev(doubled), out_words=36, want_t=True)
    assert [proj_to_affine(r) for r in ints_of(t3, "g2_add_step T")] == [PM.g2_add(PM.g2_add(q, q), q) for q, _ in cases]
    # f12_mul_line: f * (c0 + c1 px v + c2 py v w) with the device's own lines and with degenerate ones
    top = (P - 1, P - 1)
    lines = [tuple((r[2 * k], r[2 * k + 1]) for k in range(3)) for r in ints_of(lines_d, "doubling line") + ints_of(lines_a, "addition line")]
    lines = [(l[0], l[1], l[2]) for l in lines] + [(F2_ZERO, F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO, F2_ZERO), (F2_ZERO, top, F2_ZERO), (top, top, top)]
    g1s = [M.G1, M.g1_mul(M.G1, R - 1), PC.G1_ORDER_3, (P - 1, 1)]             # f12_mul_line does not ask for a curve point
    cases = [(f12_elems[(7 * i + 3) % len(f12_elems)], l, g1s[i % 4]) for i, l in enumerate(lines)]
    sparse = [[l[0], F2_ZERO, PM.f2_scale(l[1], p[0]), PM.f2_scale(l[2], p[1]), F2_ZERO, F2_ZERO] for _, l, p in cases]
    _, out = run_miller("mul_line", len(cases), p=dev([list(p) for _, _, p in cases]), t=dev([f6_row(l) for _, l, _ in cases]),
                        f=dev([tower(x) for x, _, _ in cases]))
    check(out, [tower(PM.f12_mul(x, s)) for (x, _, _), s in zip(cases, sparse)], "f12_mul_line")


def test_miller_loop_both_forms_and_the_pairing():
    import torch
    k = 0x0123456789ABCDEF ** 4 % R
    pairs = [(M.G1, PM.G2), (M.g1_mul(M.G1, 2), PM.g2_mul(PM.G2, 2)), (M.g1_mul(M.G1, R - 1), PM.g2_mul(PM.G2, R - 1)),
             (M.g1_mul(M.G1, k), PM.g2_mul(PM.G2, k * k % R))]
    n = len(pairs)
    p, q = dev([list(a) for a, _ in pairs]), dev([g2_row(b) for _, b in pairs])
    _, on_the_way = run_miller("loop", n, p=p, q=q)
    stride = DRV.lib().pairing_driver_prep_stride()
    n_lines = DRV.lib().pairing_driver_lines()
    assert stride == 36 * n_lines + 8
    prep = torch.full((n + 1, stride), PATTERN, dtype=torch.int64, device="cuda")
    _, prepared = run_miller("loop_prepared", n, p=p, q=q, prep=prep)
    f_way, f_prep = limbs_of(on_the_way, "miller_loop"), limbs_of(prepared, "miller_loop from prepared lines")
    # the same lines give the same value, limb for limb: a line the prepare loop wrote differently would change it
    assert np.array_equal(f_way, f_prep)
    lines = limbs_of(prep, "prepared lines")
    assert (lines[:, 36 * n_lines] == n_lines).all() and (lines[:, 36 * n_lines + 1:] == np.uint64(PATTERN)).all()
    # the first two prepared lines are the doubling step at (Q, 1) and the addition step after it (|x| = 0b1101...), limb for limb
    t2, l0 = run_miller("double_step", n, t=dev([proj_row(b, F2_ONE) for _, b in pairs]), out_words=36, want_t=True)
    _, l1 = run_miller("add_step", n, q=q, t=dev(ints_of(t2, "T")), out_words=36, want_t=True)
    assert np.array_equal(lines[:, :36], limbs_of(l0, "line 0")) and np.array_equal(lines[:, 36:72], limbs_of(l1, "line 1"))
    # raw Miller values differ from the model's by subfield factors; after the final exponentiation they are the pairing
    gt = run_f12("final_exp", ints_of(on_the_way, "miller_loop"))
    check(gt, [tower(PM.pairing(a, b)) for a, b in pairs], "final_exponentiation(miller_loop(P, Q))")


# ---- the launchers refuse what they cannot run --------------------------------------------------------------------------------------------
def test_a_refused_call_launches_nothing():
    a, out = dev([[1, 2]]), outbuf(1, 12)
    L = DRV.lib()
    assert L.pairing_driver_f2(len(DRV.F2_OPS), ptr(a), ptr(a), ptr(out), 1, stream()) != 0
    assert L.pairing_driver_f2(0, ptr(a), None, ptr(out), 1, stream()) != 0
    assert L.pairing_driver_f2(0, ptr(a), ptr(a), ptr(out), 0, stream()) != 0
    assert L.pairing_driver_f2(0, ptr(a), ptr(a), ptr(out), 1 << 20, stream()) != 0
    assert (out.cpu().numpy().view(np.uint64) == np.uint64(PATTERN)).all()
