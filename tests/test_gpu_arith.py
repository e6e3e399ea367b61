"""GPU: the arithmetic layer under every kernel, one primitive at a time, at its extreme inputs, against python integers.

The provers and the MSM are compared with the oracle on uniformly random field elements, which never reach a carry chain whose limbs
equal the modulus over a prefix (probability 2^-192 for the Fq borrow handover), an FqU operand at the edge of its lazy-reduction
bound, two different encodings of one x in the group law's branch test, or a matrix-core column at +-2^27.  Here every primitive of
fp.hpp, fqu.hpp, g1u.hpp, wide_acc.hpp, the DPP reductions and mfma_fold.hpp is launched alone through tests/cpp/arith_driver.hip on
inputs built for those places.  The reference is python `int`, `%` and the affine g1_add / g1_mul of tests/golden/model.py; values go
to the device as raw limbs and come back as raw limbs, so no conversion of the library takes part.  Every comparison is == on limbs
or on integers; every output buffer carries a guard behind it.  Each input set is checked on the CPU against the precondition its
primitive documents before anything is sent to the device (the _check_* functions): no case is filtered at run time.
"""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import arith_driver as DRV  # noqa: E402
import model  # noqa: E402

pytestmark = pytest.mark.gpu

R_FR, P_FQ, G1 = model.R, model.P, model.G1
PATTERN32 = 0x5A5A5A5A


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def limbs32(v, n32):
    assert 0 <= v < 1 << (32 * n32)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n32)]


def to_dev(rows, width):
    """list of limb lists -> int32 tensor [n, width] on the device"""
    import torch
    a = np.array(rows, dtype=np.uint32).reshape(-1, width)
    return torch.from_numpy(a.view(np.int32)).cuda()


def ints_to_dev(vals, n32):
    import torch
    raw = b"".join(v.to_bytes(4 * n32, "little") for v in vals)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int32).reshape(-1, n32).copy()).cuda()


def outbuf(n, width):
    """n rows and one guard row, all pattern"""
    import torch
    return torch.full((n + 1, width), PATTERN32, dtype=torch.int32, device="cuda")


def rows_of(buf, what):
    """the rows a kernel wrote as python ints per limb; the guard row must still hold the pattern"""
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[-1] == np.uint32(PATTERN32)).all(), what + ": the row behind the output was written"
    return got[:-1]


def value32(row):
    return sum(int(x) << (32 * i) for i, x in enumerate(row))


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def launched(status):
    assert status == 0, "launcher returned hipError %d" % status


def compare_ints(got_rows, want, what):
    got = [value32(r) for r in got_rows]
    assert len(got) == len(want), what
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d items differ, the first at index %d: got %#x, want %#x" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# ---- 1. Fr and Fq ---------------------------------------------------------------------------------------------------------------
class Field:
    def __init__(self, name, p, n32, index):
        self.name, self.p, self.n32, self.index = name, p, n32, index
        self.R = 1 << (32 * n32)
        self.Rinv = pow(self.R, -1, p)


FR = Field("Fr", R_FR, 8, 0)
FQ = Field("Fq", P_FQ, 12, 1)


def edge_set(F):
    """Canonical stored values at the edges of the carry and borrow chains.  The last family is the canonical neighbour of "limbs
    below position i all ones, limbs above p's" (that value itself is >= p: limb i is decremented to bring it under p; the value
    itself is reached as a SUM a + b by chain_sum_pairs)."""
    p, n = F.p, F.n32
    pl = limbs32(p, n)
    E = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.R % p, F.R * F.R % p]
    for i in range(1, n):
        E += [(1 << (32 * i)) - 1, 1 << (32 * i)]
    for i in range(n):                                           # p with exactly one limb decremented
        assert pl[i] > 0
        E.append(p - (1 << (32 * i)))
    for i in range(1, n):                                        # p's limbs above i, limb i one less, all ones below
        E.append(((p >> (32 * i)) << (32 * i)) - 1)
    return E


def split_sum(s, p, rng, k):
    """k pairs (a, b) of canonical values with a + b == s (s < 2p - 1)"""
    lo, hi = max(0, s - (p - 1)), min(s, p - 1)
    assert lo <= hi
    picks = [lo, hi, (lo + hi) // 2] + [rng.randrange(lo, hi + 1) for _ in range(k)]
    return [(a, s - a) for a in picks[:k]]


def chain_sum_pairs(F, rng):
    """pairs whose SUM, before the conditional subtraction, has p's limbs above a position and an extreme below it"""
    p, n = F.p, F.n32
    out = []
    for i in range(1, n):
        hi_part, p_lo = (p >> (32 * i)) << (32 * i), p % (1 << (32 * i))
        for x in (0, p_lo - 1, p_lo, p_lo + 1, (1 << (32 * i)) - 1):
            out += split_sum(hi_part + x, p, rng, 3)
    return out


def fq_handover_pairs(rng):
    """the limb-5 / limb-6 borrow handover of sub_to_chain12: the high halves of a + b and p compare equal, the low half decides"""
    p_hi, p_lo = P_FQ >> 192, P_FQ % (1 << 192)
    out = []
    for x in (0, p_lo - 1, p_lo, p_lo + 1, (1 << 192) - 1):
        out += split_sum((p_hi << 192) + x, P_FQ, rng, 5)
    return out


def cond_sub_pairs(F, rng):
    p = F.p
    avals = [2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 32, (1 << 32) - 1, F.R % p, 1 << (32 * (F.n32 - 1))]
    avals += [rng.randrange(2, p) for _ in range(10)]
    return [(a, b) for a in avals for b in (p - a - 1, p - a, p - a + 1)]


_FP_CASES = {}


def fp_pairs(F):
    if F.name not in _FP_CASES:
        rng = random.Random(0xA117 + F.index)
        E = edge_set(F)
        pairs = [(a, b) for a in E for b in E]
        pairs += cond_sub_pairs(F, rng) + chain_sum_pairs(F, rng)
        if F is FQ:
            pairs += fq_handover_pairs(rng)
        pairs += [(rng.randrange(F.p), rng.randrange(F.p)) for _ in range(300)]
        _check_fp_pairs(F, pairs)
        _FP_CASES[F.name] = pairs
    return _FP_CASES[F.name]


def _check_fp_pairs(F, pairs):
    """CPU only: `< p` is the contract of every Fp operation"""
    assert all(0 <= a < F.p and 0 <= b < F.p for a, b in pairs)
    if F is FQ:                                                  # the handover case is really there, on both sides
        p_hi, p_lo = P_FQ >> 192, P_FQ % (1 << 192)
        lows = {(a + b) % (1 << 192) for a, b in pairs if (a + b) >> 192 == p_hi}
        assert {0, p_lo - 1, p_lo, p_lo + 1, (1 << 192) - 1} <= lows


FP_REF = {
    "add": lambda F, a, b: (a + b) % F.p,
    "sub": lambda F, a, b: (a - b) % F.p,
    "mul": lambda F, a, b: a * b * F.Rinv % F.p,
    "sqr": lambda F, a, b: a * a * F.Rinv % F.p,
    "neg": lambda F, a, b: -a % F.p,
    "dbl": lambda F, a, b: 2 * a % F.p,
    "to_mont": lambda F, a, b: a * F.R % F.p,
    "from_mont": lambda F, a, b: a * F.Rinv % F.p,
}


@pytest.mark.parametrize("op", DRV.FP_OPS)
@pytest.mark.parametrize("F", [FR, FQ], ids=lambda F: F.name)
def test_fp_edges(F, op):
    """Fr and Fq: every operation over E x E (E = edge_set), the conditional-subtraction pairs b in {p - a - 1, p - a, p - a + 1}, sums
    with p's limbs over a prefix (for Fq the limb-5/6 handover of sub_to_chain12) and 300 random pairs; unary operations take a"""
    pairs = fp_pairs(F)
    n = len(pairs)
    a, b, out = ints_to_dev([x for x, _ in pairs], F.n32), ints_to_dev([y for _, y in pairs], F.n32), outbuf(n, F.n32)
    launched(DRV.lib().arith_driver_fp(F.index, DRV.FP_OPS.index(op), ptr(a), ptr(b), ptr(out), n, stream()))
    compare_ints(rows_of(out, op), [FP_REF[op](F, x, y) for x, y in pairs], "%s %s" % (F.name, op))


# ---- 2. FqU ---------------------------------------------------------------------------------------------------------------------
W28, NL = 28, 14
MASK28 = (1 << W28) - 1
WEAK = (1 << W28) + 16                       # limbs 0..12 of a weakly normalised element are below this
R392 = 1 << 392
PINV392 = pow(P_FQ, -1, R392)
L295 = int(2 ** 29.5)                        # floor(2^29.5): the largest limb a multiplier input may carry
C_IN, C_OUT = pow(2, 400, P_FQ), pow(2, 384, P_FQ)


def strong(v):
    """the normalised limbs of a value"""
    assert 0 <= v < 1 << (W28 * 13 + 32)
    return [(v >> (W28 * i)) & MASK28 for i in range(13)] + [v >> (W28 * 13)]


def value28(l):
    return sum(int(x) << (W28 * i) for i, x in enumerate(l[:NL]))


def lift(l, idx, c):
    """another encoding of the same value: c units of limb idx + 1 moved down into limb idx"""
    l = list(l)
    assert l[idx + 1] >= c
    l[idx] += c << W28
    l[idx + 1] -= c
    return l


def weakest(v):
    """the weak encoding of v with as many limbs as the value allows above 2^28: limb i takes 2^28 from limb i + 1 wherever it is
    below 16 and the next one is not zero"""
    l = strong(v)
    for i in range(13):
        if l[i] < 16 and l[i + 1] > 0:
            l = lift(l, i, 1)
    return l


def full_limbs(limb, below):
    """limbs 0..12 all `limb`, the top limb the largest that keeps the value below `below`"""
    low = sum(limb << (W28 * i) for i in range(13))
    top = (below - 1 - low) >> (W28 * 13)
    assert top >= 0
    return [limb] * 13 + [top]


def is_weak(l):
    return all(x < WEAK for x in l[:13])


def fqu_dev(encs):
    return to_dev([list(l) + [0, 0] for l in encs], 16)


def mont392(a, b):
    """the integer fqu_mul returns for integer operands: (a b + m p) / 2^392 with the one m < 2^392 that makes it divide"""
    ab = a * b
    m = -ab * PINV392 % R392
    return (ab + m * P_FQ) >> 392


def run_fqu(op, a_encs, b_encs=None, width=16):
    n = len(a_encs)
    a = ints_to_dev([value32(l) for l in a_encs], 12) if op == "from_ark" else fqu_dev(a_encs)
    b = fqu_dev(b_encs) if b_encs is not None else None
    out = outbuf(n, width)
    launched(DRV.lib().arith_driver_fqu(DRV.FQU_OPS.index(op), ptr(a), ptr(b), ptr(out), n, stream()))
    rows = rows_of(out, op)
    if width == 16:
        assert not rows[:, 14:].any(), op + ": pad words"
    return [[int(x) for x in r[:NL]] if width == 16 else [int(x) for x in r] for r in rows]


def mixed_encodings(vals):
    """every value in its strong form, in the weakest form the value allows, and with 2^28 more in one limb (legal for a multiplier
    input, not weak) wherever the next limb can give it"""
    out = []
    for v in vals:
        s = strong(v)
        out += [s, weakest(v)]
        out += [lift(s, idx, 1) for idx in (0, 6, 12) if s[idx + 1] >= 1]
    return out


def test_fqu_ark_round_trip():
    """fqu_from_ark: the exact integer mont392(a, 2^400 mod p), normalised; fqu_to_ark of that: a again.  Over the Fq edge set."""
    E = sorted(set(edge_set(FQ)))
    assert all(0 <= v < P_FQ for v in E)
    got = run_fqu("from_ark", [limbs32(v, 12) for v in E])
    for v, l in zip(E, got):
        assert l == strong(mont392(v, C_IN)), hex(v)
        assert value28(l) % P_FQ == v * 256 % P_FQ and value28(l) < 2 * P_FQ
    back = run_fqu("to_ark", got, width=12)
    compare_ints(back, E, "to_ark(from_ark)")


def test_fqu_to_ark_lazy_inputs():
    """fqu_to_ark on value t p + v, t = 0..31 (its bound is value < 32 p), v over the edge set, in the weakest encoding"""
    E = sorted(set(edge_set(FQ)))
    encs, want = [], []
    for k, v in enumerate(E):
        for t in {0, 31, k % 32}:
            encs.append(weakest(t * P_FQ + v))
            want.append(v * pow(256, -1, P_FQ) % P_FQ)
    assert all(value28(l) < 32 * P_FQ and is_weak(l) for l in encs)
    compare_ints(run_fqu("to_ark", encs, width=12), want, "to_ark")


def fqu_mul_cases():
    """(a, b, inside): `inside` when value(a) value(b) < 2^392 p, the condition under which (a b + m p) / 2^392 < 2p holds for every
    m < 2^392 -- the contract of fqu_mul.  2^392 p = 2520.2 p^2."""
    p = P_FQ
    e64, e50, e39 = full_limbs(L295, 64 * p), full_limbs(L295, 50 * p), full_limbs(L295, 39 * p)
    cases = [(e50, e50), (e64, e39), (e39, e64), (e64, e64)]
    mixed = mixed_encodings(sorted(set(edge_set(FQ))))
    rng = random.Random(77)
    for k, l in enumerate(mixed):
        cases += [(l, mixed[(7 * k + 3) % len(mixed)]), (e64, l), (l, e39)]
    cases += [(strong(rng.randrange(2 * p)), weakest(rng.randrange(14 * p))) for _ in range(200)]
    return [(a, b, value28(a) * value28(b) < R392 * p) for a, b in cases]


def test_fqu_mul_contract_edge():
    """fqu_mul at the edge of its contract: every limb floor(2^29.5); value just under 64 p against just under 39 p, and 50 p against
    50 p (64 x 39 = 2496 and 50 x 50 = 2500, against 2520.2 = 2^392 / p); the Fq edge set in mixed weak / strong encodings.  The
    result is the exact integer (a b + m p) / 2^392, its limbs 0..12 < 2^28, its value < 2p and = a b 2^-392 (mod p).

    The pair with BOTH values just under 64 p is kept: there the result is still exact and normalised, but Montgomery reduction gives
    (a b + m p) / 2^392 = 2.42 p for it (python integers, not a measurement of the kernel), and up to 64^2 / 2520.2 + 1 = 2.63 p for
    such values in general: `value < 2p` cannot hold for 64 p x 64 p, whatever the multiplier does.  fqu.hpp claimed it; its contract
    now says value(a) value(b) < 2^392 p.  The group law's largest pair is 18 p x 18 p."""
    cases = fqu_mul_cases()
    for a, b, _ in cases:                                        # CPU: limb and value bounds of a multiplier input
        assert all(x <= L295 for x in a + b) and value28(a) < 64 * P_FQ and value28(b) < 64 * P_FQ
    assert sum(1 for _, _, inside in cases if not inside) == 1   # 64 p x 64 p alone
    got = run_fqu("mul", [a for a, _, _ in cases], [b for _, b, _ in cases])
    for (a, b, inside), l in zip(cases, got):
        va, vb = value28(a), value28(b)
        assert l == strong(mont392(va, vb)), (a, b)
        assert all(x < 1 << W28 for x in l[:13])
        assert value28(l) * R392 % P_FQ == va * vb % P_FQ
        if inside:
            assert value28(l) < 2 * P_FQ
        else:
            assert value28(l) * R392 < va * vb + R392 * P_FQ    # what the reduction guarantees: a b / 2^392 + p


def norm_inputs():
    rng = random.Random(5)
    ins = [[0] * NL, strong(P_FQ), full_limbs(WEAK - 1, 14 * P_FQ), full_limbs(L295, 64 * P_FQ)]
    ins.append([1 << W28] + [MASK28] * 12 + [5])                 # one carry rippling through all 13 limbs
    ins.append([WEAK - 1] + [MASK28] * 12 + [5])
    ins.append([0xFFFFFFFF] + [0xFFFFFFF0] * 12 + [7])           # the largest limbs whose carries still fit 32 bits
    ins += [[rng.randrange(1 << 31) for _ in range(13)] + [rng.randrange(1 << 20)] for _ in range(100)]
    return ins


def test_fqu_weak_norm():
    """value kept exactly, limbs 0..12 < 2^28 + 16, for limbs up to 0xFFFFFFFF (its carries are taken in parallel, so no sum wraps)"""
    ins = norm_inputs() + [[0xFFFFFFFF] * 13 + [3]]
    assert all(l[13] + (l[12] >> 28) < 1 << 32 for l in ins)
    for l_in, l in zip(ins, run_fqu("weak_norm", ins)):
        assert value28(l) == value28(l_in) and is_weak(l), l_in


def test_fqu_strong_norm():
    """value kept exactly, limbs 0..12 < 2^28: the carries ripple.  Inputs up to what its callers give and beyond: any limbs whose
    running carry fits 32 bits."""
    ins = norm_inputs()
    for l in ins:
        c = 0
        for x in l:
            assert x + c < 1 << 32
            c = (x + c) >> 28
    for l_in, l in zip(ins, run_fqu("strong_norm", ins)):
        assert l == strong(value28(l_in)), l_in


def sub_cases(K):
    p, rng = P_FQ, random.Random(K)
    b_edge = full_limbs(WEAK - 1, (K - 1) * p)                   # just under (K - 1) p, every limb 2^28 + 15
    a_set = [[0] * NL, strong(p - 1), full_limbs(L295, 64 * p), full_limbs(WEAK - 1, 14 * p), strong(rng.randrange(2 * p))]
    b_set = [b_edge, [0] * NL, strong((K - 1) * p - 1), weakest(rng.randrange((K - 1) * p))]
    b_set += [weakest(t * p + v) for t in range(K - 1) for v in (0, 1, p - 1)]
    return [(a, b) for a in a_set for b in b_set]


@pytest.mark.parametrize("K", [4, 8, 16])
def test_fqu_sub(K):
    """fqu_sub<K>: value(a) + K p - value(b) AS INTEGERS (no limb wrapped) and weakly normalised, for b just under (K - 1) p with every
    limb at 2^28 + 15, and a from zero to every limb floor(2^29.5)"""
    cases = sub_cases(K)
    assert all(is_weak(b) and value28(b) < (K - 1) * P_FQ and all(x <= L295 for x in a) for a, b in cases)
    got = run_fqu("sub%d" % K, [a for a, _ in cases], [b for _, b in cases])
    for (a, b), l in zip(cases, got):
        assert value28(l) == value28(a) + K * P_FQ - value28(b), (a, b)
        assert is_weak(l)


def test_fqu_sub_group_law_shapes():
    """the two shapes the group law passes: fqu_sub<8>(x, fqu_dbl(s)) with s normalised and every limb 2^28 - 1 -- limbs 2^29 - 2, which
    only the 2^29 lift of the 8 p constant dominates -- and fqu_sub<16>(q, x3) with x3 just under 14 p, every limb 2^28 + 15"""
    p, rng = P_FQ, random.Random(9)
    s_edge = full_limbs(MASK28, 2 * p)
    xs = [[0] * NL, strong(rng.randrange(2 * p)), full_limbs(MASK28, 2 * p)]
    ss = [s_edge, strong(2 * p - 1), strong(rng.randrange(2 * p)), [0] * NL]
    cases = [(x, s) for x in xs for s in ss]
    assert all(all(v < 1 << W28 for v in s[:13]) and value28(s) < 2 * p for _, s in cases)
    for (x, s), l in zip(cases, run_fqu("sub8_dbl", [x for x, _ in cases], [s for _, s in cases])):
        assert value28(l) == value28(x) + 8 * p - 2 * value28(s) and is_weak(l), (x, s)
    x3 = full_limbs(WEAK - 1, 14 * p)
    qs = [[0] * NL, strong(2 * p - 1), full_limbs(MASK28, 2 * p)]
    for q, l in zip(qs, run_fqu("sub16", qs, [x3] * len(qs))):
        assert value28(l) == value28(q) + 16 * p - value28(x3) and is_weak(l), q


def is_zero_cases():
    """(encoding, expected).  Multiples t p, t = 0..31, strong and in encodings that carry excess in the limbs (weak: + 15 x 2^28 in
    a limb; lazy: limbs up to 2^31); zero itself has one encoding only.  Non-multiples: t p +- 1; t p + j 2^28, whose low limb is
    that of t p, so the filter passes them and fqu_equals_multiple decides; values whose low limb gives t >= 32."""
    p, cases = P_FQ, []
    pinv28 = pow(p, -1, 1 << W28)
    for t in range(32):
        s = strong(t * p)
        cases.append((s, True))
        if t:
            cases.append((lift(s, 0, 15), True))
            cases.append((lift(lift(lift(s, 12, 15), 5, 15), 9, 1), True))
            lazy = s
            for idx in range(13):
                lazy = lift(lazy, idx, min(7, lazy[idx + 1]))
            cases.append((lazy, True))
            cases.append((strong(t * p - 1), False))
        cases.append((strong(t * p + 1), False))
        for j in (1, 2, 3, 1 << 28, (1 << 300) + 5):
            s = strong(t * p + (j << W28))
            cases.append((s, False))
            if s[4] >= 9:
                cases.append((lift(s, 3, 9), False))
        v = t * p + 12345                                        # low limb test gives t >= 32
        cases.append((strong(v), False))
    return cases, pinv28


def test_fqu_is_zero_mod_p():
    cases, pinv28 = is_zero_cases()
    slow_false, far_false = 0, 0
    for l, want in cases:                                        # CPU: the bounds of the function, and that every path is taken
        v = value28(l)
        assert v < 32 * P_FQ and (v % P_FQ == 0) == want
        c = 0
        for x in l:
            assert x + c < 1 << 32                               # fqu_strong_norm inside the exact test
            c = (x + c) >> 28
        t = (l[0] & MASK28) * pinv28 & MASK28
        slow_false += (not want) and t < 32
        far_false += (not want) and t >= 32
    assert slow_false >= 32 * 5 and far_false >= 32
    got = run_fqu("is_zero", [l for l, _ in cases], width=1)
    bad = [(i, cases[i][0]) for i in range(len(cases)) if bool(got[i][0]) != cases[i][1] or got[i][0] > 1]
    assert not bad, "%d of %d wrong, the first: case %d %s" % (len(bad), len(cases), bad[0][0], bad[0][1])


# ---- 3. the group law -----------------------------------------------------------------------------------------------------------
def M(v):
    return v * R392 % P_FQ


def neg_pt(pt):
    return None if pt is None else (pt[0], -pt[1] % P_FQ)


_MULT = {}


def mult(k):
    if k not in _MULT:
        _MULT[k] = model.g1_mul(G1, k)
    return _MULT[k]


ID_XYZZ = [[0] * NL] * 4


def enc_xyzz(pt, z, i=13, j=5, tz=1, tzz=1):
    """an XYZZ encoding of an affine point: (x z^2 + i p, y z^3 + j p, z^2 + tz p, z^3 + tzz p) in Montgomery form, every coordinate
    in the weakest encoding its value allows.  i = 13, j = 5: X just under 14 p, Y just under 6 p."""
    if pt is None:
        return ID_XYZZ
    zz, zzz = z * z % P_FQ, z * z * z % P_FQ
    return [weakest(M(pt[0] * zz) + i * P_FQ), weakest(M(pt[1] * zzz) + j * P_FQ), weakest(M(zz) + tz * P_FQ), weakest(M(zzz) + tzz * P_FQ)]


def enc_xyzz_full_x(pt, seed):
    """an encoding whose X has EVERY limb at the weak maximum 2^28 + 15 and a value just under 14 p: X is chosen first, zz = X / x
    follows (the top limb goes down until zz is a square, p = 3 mod 4), then z, zzz and Y"""
    X = full_limbs(WEAK - 1, 14 * P_FQ)
    X[13] -= seed
    while True:
        zz = value28(X) * pow(R392, -1, P_FQ) * pow(pt[0], -1, P_FQ) % P_FQ
        z = pow(zz, (P_FQ + 1) // 4, P_FQ)
        if z * z % P_FQ == zz:
            break
        X[13] -= 1
    zzz = z * z * z % P_FQ
    return [X, weakest(M(pt[1] * zzz) + 5 * P_FQ), weakest(M(zz) + P_FQ), weakest(M(zzz) + P_FQ)]


def enc_affine(pt, tx=1, ty=1):
    return [weakest(M(pt[0]) + tx * P_FQ), weakest(M(pt[1]) + ty * P_FQ)]


def xyzz_dev(encs):
    return to_dev([list(c) + [0, 0] for e in encs for c in e], 64)


def affine_dev(encs):
    return to_dev([list(c) + [0, 0] for e in encs for c in e], 32)


def run_g1u(op, a_encs, b_encs=None):
    n = len(a_encs)
    a = affine_dev(a_encs) if op == "double_affine" else xyzz_dev(a_encs)
    b = None if b_encs is None else affine_dev(b_encs) if op.startswith("madd") else xyzz_dev(b_encs)
    out = outbuf(n, 64)
    launched(DRV.lib().arith_driver_g1u(DRV.G1U_OPS.index(op), ptr(a), ptr(b), ptr(out), n, stream()))
    rows = rows_of(out, op)
    res = []
    for r in rows:
        coords = [[int(x) for x in r[16 * c:16 * c + 14]] for c in range(4)]
        assert not any(r[16 * c + 14] or r[16 * c + 15] for c in range(4)), op + ": pad words"
        res.append(coords)
    return res


def _check_xyzz_input(e):
    """CPU: the stored invariants every group operation is written against, and the point really on the curve"""
    X, Y, ZZ, ZZZ = (value28(c) for c in e)
    assert all(is_weak(c) for c in e)
    if not any(any(c) for c in e):
        return None
    assert X < 14 * P_FQ and Y < 6 * P_FQ and ZZ < 2 * P_FQ and ZZZ < 2 * P_FQ and ZZ % P_FQ
    assert pow(ZZ, 3, P_FQ) == ZZZ * ZZZ * R392 % P_FQ                   # zz^3 = zzz^2, in Montgomery form
    pt = (X * pow(ZZ, -1, P_FQ) % P_FQ, Y * pow(ZZZ, -1, P_FQ) % P_FQ)
    assert model.on_curve(pt)
    return pt


def check_xyzz_output(e, want, what):
    """the affine point after host normalisation equals the model's, and the stored invariants hold: X < 14 p, Y < 6 p, ZZ and ZZZ <
    2 p, limbs weak, the identity all-zero limbs"""
    X, Y, ZZ, ZZZ = (value28(c) for c in e)
    assert all(is_weak(c) for c in e), what + ": limbs not weak"
    if want is None:
        assert not any(any(c) for c in e), what + ": the identity is all-zero limbs"
        return
    assert any(e[2]) and ZZ % P_FQ, what + ": identity returned"
    assert X < 14 * P_FQ and Y < 6 * P_FQ and ZZ < 2 * P_FQ and ZZZ < 2 * P_FQ, what + ": stored bounds"
    assert pow(ZZ, 3, P_FQ) == ZZZ * ZZZ * R392 % P_FQ, what + ": zz^3 != zzz^2"
    got = (X * pow(ZZ, -1, P_FQ) % P_FQ, Y * pow(ZZZ, -1, P_FQ) % P_FQ)
    assert got == want, what + ": wrong point"


def add_cases():
    """(name, a, b) as XYZZ encodings.  The equal and the opposite points use different z and different multiples of p, so that no
    coordinate of the two operands has equal limbs."""
    z = [0x1234567 + 977 * k for k in range(12)]
    P3, P5, P7 = mult(3), mult(5), mult(7)
    cases = [
        ("generic", enc_xyzz(P3, z[0]), enc_xyzz(P5, z[1])),
        ("generic small multiples", enc_xyzz(P5, z[2], 0, 0, 0, 0), enc_xyzz(P7, z[3], 2, 1, 0, 1)),
        ("generic full X", enc_xyzz_full_x(P3, 0), enc_xyzz_full_x(P7, 3)),
        ("P + P", enc_xyzz(P3, z[4]), enc_xyzz(P3, z[5], 6, 2, 0, 1)),
        ("P + P full X", enc_xyzz_full_x(P5, 0), enc_xyzz(P5, z[6], 1, 0, 1, 0)),
        ("P + (-P)", enc_xyzz(P3, z[7]), enc_xyzz(neg_pt(P3), z[8], 4, 3, 1, 0)),
        ("P + (-P) full X", enc_xyzz(neg_pt(P7), z[9], 0, 5, 0, 0), enc_xyzz_full_x(P7, 1)),
        ("identity + P", ID_XYZZ, enc_xyzz(P5, z[10])),
        ("P + identity", enc_xyzz(P5, z[11]), ID_XYZZ),
        ("identity + identity", ID_XYZZ, ID_XYZZ),
    ]
    for name, a, b in cases:
        if name.startswith("P + "):
            assert all(ca != cb for ca, cb in zip(a, b)), name
    return cases


_G1U = {}


def g1u_add_round():
    """g1u_add over add_cases(), once per session: (cases, device outputs, expected affine points)"""
    if "add" not in _G1U:
        cases = add_cases()
        want = [model.g1_add(_check_xyzz_input(a), _check_xyzz_input(b)) for _, a, b in cases]
        _G1U["add"] = (cases, run_g1u("add", [a for _, a, _ in cases], [b for _, _, b in cases]), want)
    return _G1U["add"]


def test_g1u_add():
    cases, got, want = g1u_add_round()
    assert sum(w is None for w in want) == 3
    for (name, _, _), e, w in zip(cases, got, want):
        check_xyzz_output(e, w, "g1u_add " + name)


def test_g1u_bounds_closed_under_the_law():
    """the outputs of g1u_add, raw, as inputs of a second operation: each added to its neighbour, each doubled, each added to ITSELF as
    g1u_add's other operand (the doubling branch, entered with equal limbs this time), and an affine point added to each"""
    cases, got, want = g1u_add_round()
    n = len(got)
    nxt = [got[(i + 1) % n] for i in range(n)]
    for i, e in enumerate(run_g1u("add", got, nxt)):
        check_xyzz_output(e, model.g1_add(want[i], want[(i + 1) % n]), "second add %d" % i)
    for i, e in enumerate(run_g1u("double", got)):
        check_xyzz_output(e, model.g1_add(want[i], want[i]), "second double %d" % i)
    for i, e in enumerate(run_g1u("add", got, got)):
        check_xyzz_output(e, model.g1_add(want[i], want[i]), "second add to itself %d" % i)
    aff = [enc_affine(mult(8))] * n
    third = run_g1u("madd", got, aff)
    for i, e in enumerate(third):
        check_xyzz_output(e, model.g1_add(want[i], mult(8)), "second madd %d" % i)
    for i, e in enumerate(run_g1u("double", third)):                 # and once more
        check_xyzz_output(e, model.g1_mul(model.g1_add(want[i], mult(8)), 2), "third double %d" % i)


def test_g1u_double():
    z = 0x7654321
    pts = [mult(k) for k in (1, 2, 3, 11)]
    encs = [enc_xyzz(pt, z + k) for k, pt in enumerate(pts)] + [enc_xyzz(pts[1], z, 0, 0, 0, 0), enc_xyzz_full_x(pts[3], 0), ID_XYZZ]
    want = [model.g1_add(q, q) for q in (_check_xyzz_input(e) for e in encs)]
    assert want[-1] is None
    for i, e in enumerate(run_g1u("double", encs)):
        check_xyzz_output(e, want[i], "g1u_double %d" % i)


def test_g1u_double_affine():
    """affine x, y in encodings up to just under 4 p (its documented bound; the MSM passes < 2 p)"""
    pts = [mult(k) for k in (1, 2, 9)]
    encs = [enc_affine(pt, tx, ty) for pt in pts for tx, ty in ((0, 0), (1, 1), (3, 3), (0, 3))]
    for e in encs:
        assert all(is_weak(c) and value28(c) < 4 * P_FQ for c in e)
    want = [model.g1_add(pt, pt) for pt in pts for _ in range(4)]
    for i, e in enumerate(run_g1u("double_affine", encs)):
        check_xyzz_output(e, want[i], "g1u_double_affine %d" % i)


@pytest.mark.parametrize("neg", [False, True], ids=["plus", "minus"])
def test_g1u_madd(neg):
    """acc +- affine point: generic, the same point (through g1u_double_affine) and the opposite point with the accumulator in an
    encoding that shares no limbs with the affine operand, the identity accumulator (with `neg`: the stored point is (x, 4p - y, 1, 1))"""
    z = [0x2468ACE + 31 * k for k in range(8)]
    P3, P4 = mult(3), mult(4)
    same, opp = (neg_pt(P4), P4) if neg else (P4, neg_pt(P4))      # accumulators for which +-P4 doubles / cancels
    cases = [
        ("generic", enc_xyzz(P3, z[0]), enc_affine(P4)),
        ("generic full X", enc_xyzz_full_x(P3, 2), enc_affine(P4, 0, 1)),
        ("same point", enc_xyzz(same, z[1]), enc_affine(P4, 1, 1)),
        ("same point full X", enc_xyzz_full_x(same, 0), enc_affine(P4, 0, 0)),
        ("opposite point", enc_xyzz(opp, z[2]), enc_affine(P4, 1, 0)),
        ("opposite point small multiples", enc_xyzz(opp, z[3], 0, 0, 0, 0), enc_affine(P4, 1, 1)),
        ("identity accumulator", ID_XYZZ, enc_affine(P4, 1, 1)),
        ("identity accumulator, x < p", ID_XYZZ, enc_affine(P3, 0, 1)),
    ]
    for _, _, b in cases:
        assert all(is_weak(c) and value28(c) < 2 * P_FQ for c in b)
    sign = neg_pt if neg else (lambda q: q)
    want = []
    for name, a, b in cases:
        bpt = (value28(b[0]) * pow(R392, -1, P_FQ) % P_FQ, value28(b[1]) * pow(R392, -1, P_FQ) % P_FQ)
        assert model.on_curve(bpt)
        want.append(model.g1_add(_check_xyzz_input(a), sign(bpt)))
    assert [w is None for w in want] == [False, False, False, False, True, True, False, False]
    got = run_g1u("madd_neg" if neg else "madd", [a for _, a, _ in cases], [b for _, _, b in cases])
    for (name, _, _), e, w in zip(cases, got, want):
        check_xyzz_output(e, w, "g1u_madd %s" % name)
    for i, e in enumerate(run_g1u("double", got)):                   # closed under the law
        check_xyzz_output(e, model.g1_add(want[i], want[i]), "double after madd %d" % i)


def quad_waves():
    """waves of 16 quads.  Wave 0: neighbouring quads take different branches (generic, double, cancel, a identity, b identity, both
    identity, in turn).  One further wave per early-return branch, every quad of it in that branch."""
    kinds = ["generic", "double", "cancel", "a_id", "b_id", "both_id"]

    def pair(kind, q):
        z1, z2 = 0x13579B + 11 * q, 0xFDB975 + 7 * q
        A, B = mult(2 + q % 5), mult(9 + q % 3)
        if kind == "generic":
            return (enc_xyzz_full_x(A, q), enc_xyzz(B, z2, 13 - q % 4, 5 - q % 3)) if q % 2 else (enc_xyzz(A, z1), enc_xyzz(B, z2, q % 14, q % 6, 0, 1))
        if kind == "double":
            return enc_xyzz(A, z1), enc_xyzz(A, z2, q % 13, q % 5, 0, 1)
        if kind == "cancel":
            return enc_xyzz(A, z1, q % 13, q % 5, 1, 0), enc_xyzz(neg_pt(A), z2)
        if kind == "a_id":
            return ID_XYZZ, enc_xyzz(B, z2)
        if kind == "b_id":
            return enc_xyzz(A, z1), ID_XYZZ
        return ID_XYZZ, ID_XYZZ

    waves = [[pair(kinds[q % 6], q) for q in range(16)]]
    for kind in ["double", "cancel", "a_id", "b_id", "both_id", "generic"]:
        waves.append([pair(kind, q) for q in range(16)])
    return [pr for w in waves for pr in w]


def test_g1u_add_quad():
    """g1u_add_quad: whole waves, the four lanes of a quad hold the same pair and must return the same limbs -- the limbs g1u_add gives
    are not required, the point and the stored invariants are"""
    quads = quad_waves()
    want = [model.g1_add(_check_xyzz_input(a), _check_xyzz_input(b)) for a, b in quads]
    a = [a for a, _ in quads for _ in range(4)]
    b = [b for _, b in quads for _ in range(4)]
    assert len(a) % 64 == 0
    got = run_g1u("add_quad", a, b)
    for q in range(len(quads)):
        lanes = got[4 * q:4 * q + 4]
        assert all(lane == lanes[0] for lane in lanes), "quad %d of wave %d: its lanes differ" % (q % 16, q // 16)
        check_xyzz_output(lanes[0], want[q], "g1u_add_quad wave %d quad %d" % (q // 16, q % 16))
    again = run_g1u("add_quad", got, got[4:] + got[:4])                   # the outputs as inputs: quad q + quad q + 1
    for q in range(len(quads)):
        lanes = again[4 * q:4 * q + 4]
        assert all(lane == lanes[0] for lane in lanes)
        check_xyzz_output(lanes[0], model.g1_add(want[q], want[(q + 1) % len(quads)]), "second g1u_add_quad %d" % q)


# ---- 4. the unreduced accumulator -----------------------------------------------------------------------------------------------
R288_INV = pow(1 << 288, -1, R_FR)
# The largest number of products a caller gives one WideAcc before wide_reduce:
#   multifold_kernel<64, 4, true>   per = 2^k / waves = 64 at k = 8 (4 waves), 7 (2), 6 (1); k <= MF_MAX_LOGK = 8    (zkhip.hip)
#   multifold_kernel<16>            per = 2^k / (4 waves) <= 4                                                      (zkhip.hip)
#   blockfold_kernel                per <= 4                                                          (blockfold_shape)
#   composed_fold2_kernel           4
#   composed_round_wide2_kernel     ceil(pairs / (grid * 256)) <= 256: work <= MLE_MAX_GRID * MLE_BLOCK * 256     (composed.hip)
#   composed_cross2_kernel          ceil(per / 64) with per = m / grid: 6 below m = 1024; m / 16384 when ZKHIP_CROSS_VALU=1 sends a
#                                   large stage to it, 1024 at m = 2^24, the largest m the override covers        (composed.hip)
# 1024 is also what x < 2^520 (the comment of wide_redc) admits: 1024 (r - 1)^2 < 2^520.
WIDE_MAX_TERMS = 1024
WIDE_TERMS = [1, 2, 255, 256, 1024, WIDE_MAX_TERMS]


def fr_dev(vals):
    return ints_to_dev(vals, 8)


@pytest.mark.parametrize("terms", sorted(set(WIDE_TERMS)))
def test_wide_acc_mac_reduce(terms):
    """WideAcc::mac over N products, then wide_reduce: (sum w t) 2^-288 mod r on the stored integers.  Lanes: all stored r - 1 (the
    largest columns and carry counts), all zero, alternating r - 1 / 0 and r - 1 / 1, random"""
    rng = random.Random(terms)
    r = R_FR
    lanes = [([r - 1] * terms, [r - 1] * terms), ([0] * terms, [0] * terms),
             ([(r - 1) * (j & 1) for j in range(terms)], [r - 1] * terms),
             ([r - 1 if j & 1 else 1 for j in range(terms)], [1 if j & 1 else r - 1 for j in range(terms)])]
    lanes += [([rng.randrange(r) for _ in range(terms)], [rng.randrange(r) for _ in range(terms)]) for _ in range(4)]
    assert all(0 <= v < r for w, t in lanes for v in w + t)
    assert all(sum(a * b for a, b in zip(w, t)) < 1 << 520 for w, t in lanes)
    n = len(lanes)
    w = fr_dev([lanes[i][0][j] for j in range(terms) for i in range(n)])
    t = fr_dev([lanes[i][1][j] for j in range(terms) for i in range(n)])
    out = outbuf(n, 8)
    launched(DRV.lib().arith_driver_wide_mac(ptr(w), ptr(t), n, terms, ptr(out), stream()))
    compare_ints(rows_of(out, "wide"), [sum(a * b for a, b in zip(wl, tl)) * R288_INV % r for wl, tl in lanes], "wide_reduce, %d terms" % terms)


def test_wide_redc_alone():
    """wide_redc on 17 limbs: the largest x its bound admits (2^520 - 1), zero, x = r + h 2^288 (every one of the nine multipliers m is
    0xFFFFFFFF: x + (2^288 - 1) r = 0 mod 2^288 needs x = r there), the largest sum 1024 products give, and random x < 2^520"""
    rng = random.Random(3)
    r = R_FR
    xs = [(1 << 520) - 1, 0, r, r + (((1 << 232) - 1) << 288), 1024 * (r - 1) ** 2, 1 << 519, (1 << 288) - 1, 1 << 288]
    xs += [rng.randrange(1 << 520) for _ in range(56)]
    assert all(0 <= x < 1 << 520 for x in xs)
    for x in (xs[2], xs[3]):                                       # CPU: the nine multipliers of these two
        v = x
        for i in range(9):
            m = -(v >> (32 * i)) % (1 << 32)
            assert m == 0xFFFFFFFF
            v += m * r << (32 * i)
    xin = ints_to_dev(xs, 17)
    out = outbuf(len(xs), 8)
    launched(DRV.lib().arith_driver_wide_redc(ptr(xin), len(xs), ptr(out), stream()))
    compare_ints(rows_of(out, "redc"), [x * R288_INV % r for x in xs], "wide_redc")


# ---- 5. the reductions ----------------------------------------------------------------------------------------------------------
def run_reduce(op, block, grid, a_vals, b_vals=None):
    """a_vals, b_vals: numpy uint32 [grid * block, 8]; returns what every thread got, as object arrays of python ints"""
    import torch
    a = torch.from_numpy(a_vals.view(np.int32)).cuda()
    b = torch.from_numpy(b_vals.view(np.int32)).cuda() if b_vals is not None else None
    n = block * grid
    oa = outbuf(n, 8)
    ob = outbuf(n, 8) if b_vals is not None else None
    launched(DRV.lib().arith_driver_reduce(DRV.RED_OPS.index(op), ptr(a), ptr(b), ptr(oa), ptr(ob), block, grid, stream()))
    return rows_of(oa, op), (rows_of(ob, op) if ob is not None else None)


def fr_rows(vals):
    return np.array([limbs32(v, 8) for v in vals], dtype=np.uint32)


def expect_rows(got, want_rows, what):
    if not np.array_equal(got, want_rows):
        bad = np.nonzero((got != want_rows).any(axis=1))[0]
        raise AssertionError("%s: %d of %d threads differ, the first is thread %d" % (what, len(bad), len(got), bad[0]))


def one_hot(block, values):
    """block workgroups of `block` lanes: workgroup i holds values[i] in lane i and zero elsewhere"""
    a = np.zeros((block * block, 8), dtype=np.uint32)
    rows = fr_rows(values)
    a[np.arange(block) * block + np.arange(block)] = rows
    return a, rows


@pytest.mark.parametrize("block", [64, 128, 256, 1024])
def test_reductions_one_hot(block):
    """a single non-zero value in lane i, for every i of the block: a lane dropped by a DPP row mask is a missing term.  The wave
    forms return the sum to every lane of the wave, the block forms to thread 0.  The two-sum forms get their second value in
    lane block - 1 - i."""
    rng = random.Random(block)
    va = [rng.randrange(1, R_FR) for _ in range(block)]
    vb = [rng.randrange(1, R_FR) for _ in range(block)]
    a, rows_a = one_hot(block, va)
    b, rows_b = one_hot(block, vb[::-1])
    b = b.reshape(block, block, 8)[::-1].reshape(block * block, 8).copy()      # workgroup i: vb[i] in lane block - 1 - i
    rows_b = fr_rows(vb)
    wave_of = np.arange(block) // 64

    def wave_want(rows, hot_lane):
        w = np.zeros((block, block, 8), dtype=np.uint32)
        for i in range(block):
            w[i, wave_of == hot_lane[i] // 64] = rows[i]
        return w.reshape(block * block, 8)

    hot_a, hot_b = np.arange(block), block - 1 - np.arange(block)
    got, _ = run_reduce("wave", block, block, a)
    expect_rows(got, wave_want(rows_a, hot_a), "wave_reduce_fr")
    ga, gb = run_reduce("wave2", block, block, a, b)
    expect_rows(ga, wave_want(rows_a, hot_a), "wave_reduce_fr2, first sum")
    expect_rows(gb, wave_want(rows_b, hot_b), "wave_reduce_fr2, second sum")
    got, _ = run_reduce("block", block, block, a)
    expect_rows(got[::block], rows_a, "block_reduce_fr, thread 0")
    ga, gb = run_reduce("block2", block, block, a, b)
    expect_rows(ga[::block], rows_a, "block_reduce_fr2, first sum, thread 0")
    expect_rows(gb[::block], rows_b, "block_reduce_fr2, second sum, thread 0")


@pytest.mark.parametrize("block", [64, 128, 256, 1024])
def test_reductions_dense(block):
    """workgroup 0: every lane r - 1, so every addition reduces (the second sum: every lane 1); workgroups 1 and 2: distinct random
    values per lane, the two sums from unrelated data"""
    rng = random.Random(1000 + block)
    r = R_FR
    va = [r - 1] * block + [rng.randrange(r) for _ in range(2 * block)]
    vb = [1] * block + [rng.randrange(r) for _ in range(2 * block)]
    assert all(0 <= v < r for v in va + vb)
    a, b = fr_rows(va), fr_rows(vb)

    def sums(vals, width):
        return [sum(vals[k:k + width]) % r for k in range(0, len(vals), width)]

    def per_wave(vals):
        return np.repeat(fr_rows(sums(vals, 64)), 64, axis=0)

    got, _ = run_reduce("wave", block, 3, a)
    expect_rows(got, per_wave(va), "wave_reduce_fr")
    ga, gb = run_reduce("wave2", block, 3, a, b)
    expect_rows(ga, per_wave(va), "wave_reduce_fr2, first sum")
    expect_rows(gb, per_wave(vb), "wave_reduce_fr2, second sum")
    got, _ = run_reduce("block", block, 3, a)
    expect_rows(got[::block], fr_rows(sums(va, block)), "block_reduce_fr, thread 0")
    ga, gb = run_reduce("block2", block, 3, a, b)
    expect_rows(ga[::block], fr_rows(sums(va, block)), "block_reduce_fr2, first sum, thread 0")
    expect_rows(gb[::block], fr_rows(sums(vb, block)), "block_reduce_fr2, second sum, thread 0")


# ---- Part B: the k-variable fold on the matrix cores, alone ---------------------------------------------------------------------
M_TOP = ((R_FR >> 192) << 192) - 1                       # the largest canonical value whose low 24 bytes are 0xFF (fed as +127)
W_NEG = int.from_bytes(bytes([0x80] + [0x7F] * 30 + [0x73]), "little")     # signed base-256 digits: -128 thirty-one times, then 116
W_POS = int.from_bytes(bytes([0x7F] * 31 + [0x73]), "little")              # +127 thirty-one times, then 115
R256_INV = pow(1 << 256, -1, R_FR)


def _digits(w):
    """the signed digits multifold_mfma_kernel recodes a weight into"""
    s = w + int.from_bytes(bytes([0x80] * 32), "little")
    assert s < 1 << 256
    return [(b ^ 0x80) - 256 * ((b ^ 0x80) >> 7) for b in s.to_bytes(32, "little")]


def fold_cases(m, k, rng):
    """(name, weights[2^k], table[2^k][m]) as stored integers"""
    nt = 1 << k
    rnd_w = [rng.randrange(R_FR) for _ in range(nt)]
    rnd_t = [[rng.randrange(R_FR) for _ in range(m)] for _ in range(nt)]
    by_out = [M_TOP if j & 1 else 0 for j in range(m)]
    by_out_64 = [M_TOP if (j >> 5) & 1 else 0 for j in range(m)]
    return [
        ("w -128, T 0x00 (fed -128)", [W_NEG] * nt, [[0] * m] * nt),
        ("w -128, T M (fed +127)", [W_NEG] * nt, [[M_TOP] * m] * nt),
        ("w +127, T M", [W_POS] * nt, [[M_TOP] * m] * nt),
        ("w +127, T 0x00", [W_POS] * nt, [[0] * m] * nt),
        ("w alternating, T alternating by term", [W_NEG if b & 1 else W_POS for b in range(nt)], [[0 if b & 1 else M_TOP] * m for b in range(nt)]),
        ("w random, T alternating by output", rnd_w, [by_out if b & 2 else by_out_64 for b in range(nt)]),
        ("w zero, T random", [0] * nt, rnd_t),
        ("w -128 / zero, T alternating by output", [W_NEG if b & 1 else 0 for b in range(nt)], [by_out] * nt),
        ("w random, T random", rnd_w, rnd_t),
    ]


def fold_reference(weights, table, m):
    memo = {}
    out = []
    for j in range(m):
        key = tuple(row[j] for row in table)
        if key not in memo:
            memo[key] = sum(w * t for w, t in zip(weights, key)) * R288_INV % R_FR
        out.append(memo[key])
    return out


@pytest.mark.parametrize("k", [4, 7, 8])
@pytest.mark.parametrize("m", [256, 512])
def test_mfma_fold_alone(m, k):
    """multifold_mfma_kernel<4, 4> on m = 256 (one workgroup of four tiles) and 512 outputs, k = 4 (one chunk of 16 terms), 7 (a full
    chunk of 128) and 8 (two chunks: kc_lds adds up across them), rot 0, 1, 3, 9.  Weights whose signed digits are all -128 or all +127
    against table bytes all 0x00 (fed as -128) or 0xFF (+127) drive every int32 column to 2^k x 32 x 128 x 128 = 2^27 at k = 8, either
    sign.  out[j] = (sum_b W_b T[b m + j]) 2^-288 mod r on the stored integers; partials[tile] = the sum of its 64 outputs."""
    import torch
    assert _digits(W_NEG) == [-128] * 31 + [116] and _digits(W_POS) == [127] * 31 + [115]
    assert M_TOP < R_FR and M_TOP.to_bytes(32, "little")[:24] == b"\xff" * 24
    rng = random.Random(100 * m + k)
    for name, weights, table in fold_cases(m, k, rng):
        assert all(0 <= v < R_FR for v in weights) and all(0 <= v < R_FR for row in {id(r): r for r in table}.values() for v in row)
        want = fold_reference(weights, table, m)
        want_part = [sum(want[t:t + 64]) % R_FR for t in range(0, m, 64)]
        d_in, d_w = fr_dev([v for row in table for v in row]), fr_dev(weights)
        for rot in (0, 1, 3, 9):
            out, part = outbuf(m, 8), outbuf(m // 64, 8)
            launched(DRV.lib().arith_driver_mfma_fold(ptr(d_in), m, k, ptr(d_w), ptr(out), ptr(part), rot, stream()))
            compare_ints(rows_of(out, name), want, "fold m=%d k=%d rot=%d, %s" % (m, k, rot, name))
            compare_ints(rows_of(part, name), want_part, "fold partials m=%d k=%d rot=%d, %s" % (m, k, rot, name))
        del d_in, d_w
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", [4, 8])
def test_mfma_fold_wsum(k):
    """multifold_mfma_kernel<4, 4, true>: nothing but the records, record[tile] = sum over its 64 outputs of out[j] wa[j >> s] wb[j &
    (2^s - 1)] (Montgomery products), out_s = 3 and 0"""
    m = 512
    rng = random.Random(k)
    for name, weights, table in fold_cases(m, k, rng)[-3:] + fold_cases(m, k, rng)[:2]:
        out = fold_reference(weights, table, m)
        d_in, d_w = fr_dev([v for row in table for v in row]), fr_dev(weights)
        for s, rot in ((3, 1), (0, 9)):
            wa = [rng.randrange(R_FR) for _ in range(m >> s)]
            wb = [rng.randrange(R_FR) for _ in range(1 << s)]
            wa[0], wb[-1] = R_FR - 1, R_FR - 1
            eq = [wa[j >> s] * wb[j & ((1 << s) - 1)] * R256_INV % R_FR for j in range(m)]
            want = [sum(out[j] * eq[j] * R256_INV % R_FR for j in range(t, t + 64)) % R_FR for t in range(0, m, 64)]
            rec, d_wa, d_wb = outbuf(m // 64, 8), fr_dev(wa), fr_dev(wb)
            launched(DRV.lib().arith_driver_mfma_fold_wsum(ptr(d_in), m, k, ptr(d_w), ptr(rec), rot, ptr(d_wa), ptr(d_wb), s, stream()))
            compare_ints(rows_of(rec, name), want, "fold records k=%d out_s=%d, %s" % (k, s, name))
