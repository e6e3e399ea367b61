"""Edge inputs of the BLS12-381 verifier stack, built with the independent model (tests/pairing_model.py) only: points off the curves,
points of the curves outside the order-r subgroups -- of large order and of the small orders 3, 11 (E(Fq)) and 13, 23 (the twist
E'(Fq2)) -- and elements of Fq12 inside and outside the cyclotomic subgroup.  Shared by test_gpu_pairing.py, test_gpu_kzg_verify.py,
test_gpu_pairing_kernels.py and test_pairing_cases_cpu.py, which proves on the CPU that the inputs are what they are named.

A point of small order matters to the device code because its subgroup check is a plain MSB-first double-and-add by r: over such a
point the accumulator keeps meeting q and -q, which is the only way into the doubling and inverse branches of g1_madd / g2_madd."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_model as PM  # noqa: E402

M = PM.M
P, R = PM.P, PM.R
X = -PM.X_ABS                                                            # the curve parameter, x < 0
H1 = (X - 1) ** 2 // 3                                                   # #E(Fq) = H1 r
H2 = (X ** 8 - 4 * X ** 7 + 5 * X ** 6 - 4 * X ** 4 + 6 * X ** 3 - 4 * X ** 2 - 4 * X + 13) // 9     # #E'(Fq2) = H2 r
assert (X - 1) ** 2 % 3 == 0 and H1 % (3 * 121) == 0 and H2 % (13 * 13 * 23 * 23) == 0
CYCLOTOMIC_ORDER = P ** 4 - P ** 2 + 1                                    # the order of the cyclotomic subgroup of Fq12*
EASY_EXP = (P ** 6 - 1) * (P ** 2 + 1)                                    # the easy part of the final exponentiation maps into it


# ---- off the curve / outside the subgroup, of large order (what test_gpu_pairing.py always used) -------------------------------------
def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = PM.f2_mul(r, a)
        a = PM.f2_mul(a, a)
        e >>= 1
    return r


def off_twist():
    q = ((1, 0), (1, 0))                          # 1 != 1 + 4 (u + 1)
    assert not PM.g2_on_curve(q)
    return q


@functools.lru_cache(maxsize=None)
def twist_not_in_subgroup():
    """a point of the twist E'(Fq2) outside the order-r subgroup: try x = i, i + 1, ... until x^3 + b is a square in Fq2"""
    for i in range(1, 200):
        x = (i, 1)
        rhs = PM.f2_add(PM.f2_mul(PM.f2_mul(x, x), x), PM.B2)
        # sqrt in Fq2 (p = 3 mod 4): a = rhs, alpha = a^((p-3)/4) ...
        a = rhs
        a1 = f2_pow(a, (P - 3) // 4)
        alpha = PM.f2_mul(a1, PM.f2_mul(a1, a))
        x0 = PM.f2_mul(a1, a)
        if alpha == ((P - 1) % P, 0):
            y = PM.f2_mul((0, 1), x0)
        else:
            b = f2_pow(PM.f2_add((1, 0), alpha), (P - 1) // 2)
            y = PM.f2_mul(b, x0)
        if PM.f2_mul(y, y) != rhs:
            continue
        q = (x, y)
        if PM.g2_mul_raw(q, R) is not None:
            return q
    raise AssertionError("no point found")


def g1_mul_raw(pt, k):
    """k * pt without reducing k mod r"""
    acc = None
    while k:
        if k & 1:
            acc = M.g1_add(acc, pt)
        pt = M.g1_add(pt, pt)
        k >>= 1
    return acc


@functools.lru_cache(maxsize=None)
def g1_not_in_subgroup():
    for x in range(1, 100):
        rhs = (x ** 3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs and g1_mul_raw((x, y), R) is not None:
            return x, y
    raise AssertionError("no point found")


# ---- points of small order ---------------------------------------------------------------------------------------------------------
def g1_on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def g1_neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


G1_ORDER_3 = (0, 2)


@functools.lru_cache(maxsize=None)
def g1_order_11():
    """The whole cofactor but 11^2 times a point outside the subgroup.  The 11-Sylow subgroup of E(Fq) is not cyclic, so dividing out a
    single 11 gives the identity."""
    pt = g1_mul_raw(g1_not_in_subgroup(), H1 * R // 121)
    assert pt is not None
    return pt


@functools.lru_cache(maxsize=None)
def g2_small_order(q):
    assert q in (13, 23)
    pt = PM.g2_mul_raw(twist_not_in_subgroup(), H2 * R // (q * q))
    assert pt is not None
    return pt


def g1_small_order_points():
    return {3: G1_ORDER_3, 11: g1_order_11()}


def g2_small_order_points():
    return {13: g2_small_order(13), 23: g2_small_order(23)}


def walk_r(pt, add, neg):
    """What an MSB-first double-and-add by r does over `pt`: (times the accumulator equals pt when pt is to be added -- the doubling
    branch of a mixed addition --, times it equals -pt -- the inverse branch --, the result)."""
    acc, same, inverse = None, 0, 0
    for bit in bin(R)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            if acc is not None and acc == pt:
                same += 1
            elif acc is not None and acc == neg(pt):
                inverse += 1
            acc = add(acc, pt)
    return same, inverse, acc


def walk_r_g1(pt):
    return walk_r(pt, M.g1_add, g1_neg)


def walk_r_g2(pt):
    return walk_r(pt, PM.g2_add, PM.g2_neg)


# ---- Fq12: the model's w-basis (six Fq2 coefficients of w^0 .. w^5) and the tower order of the device ---------------------------------------
TOWER_ORDER = (0, 2, 4, 1, 3, 5)                  # tower slot k (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) holds the coefficient of w^TOWER_ORDER[k]


def f12_from_tower(t):
    """12 canonical ints in arkworks order -> the model's w-basis element"""
    a = [None] * 6
    for slot, k in enumerate(TOWER_ORDER):
        a[k] = (t[2 * slot] % P, t[2 * slot + 1] % P)
    return a


def f12_conj(a):
    """a^(p^6): w -> -w"""
    return [c if k % 2 == 0 else ((-c[0]) % P, (-c[1]) % P) for k, c in enumerate(a)]


def f12_random(rng):
    return [(int.from_bytes(rng.bytes(48), "little") % P, int.from_bytes(rng.bytes(48), "little") % P) for _ in range(6)]


@functools.lru_cache(maxsize=None)
def gt_generator():
    """e(G1, G2), w-basis"""
    return PM.pairing(M.G1, PM.G2)


@functools.lru_cache(maxsize=None)
def cyclotomic_elements():
    """Elements of the cyclotomic subgroup: 1, e(G1, G2), its conjugate (= inverse) and three random elements raised to the easy part."""
    import numpy as np
    rng = np.random.default_rng(381)
    e = gt_generator()
    return [PM.f12_one(), e, f12_conj(e)] + [PM.f12_pow(f12_random(rng), EASY_EXP) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def not_cyclotomic():
    """the negative control: a random element of Fq12, outside the cyclotomic subgroup"""
    import numpy as np
    return f12_random(np.random.default_rng(12))
