"""csrc/affine_step.hpp on the GPU against python integers: (t + d * D) mod r from the table of digit multiples T_k = D * 2^(28 k) mod r,
one triple per row of 16 lanes (tests/cpp/affine_step_driver.hip), bit for bit.

The integer model below takes the routine's own steps -- ten digits of 28 bits, carry-free columns, the quotient word from the top of
the columns and floor(2^288 / r), the generate / propagate carries, two conditional subtractions -- and asserts, for the very inputs
of this file, the bounds the routine's comment derives: columns below 2^64, the quotient word below 2^32, no overflow where the
high words move one lane up, and a remainder below 2 r (the second subtraction never fires).  A changed digit width or reciprocal
fails here before it can pass on the GPU by luck."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_step_driver as DRV  # noqa: E402

pytestmark = pytest.mark.gpu

P = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BITS, DIGITS = 28, 10
MU = (1 << 288) // P
M32 = (1 << 32) - 1


def digits(d):
    return [(d >> (BITS * k)) & ((1 << BITS) - 1) for k in range(DIGITS)]


def model(t, D, d):
    """-> (result, facts): the routine step by step"""
    assert 0 <= t < P and 0 <= D < P and 0 <= d < (1 << 256)
    dg = digits(d)
    assert sum(dk << (BITS * k) for k, dk in enumerate(dg)) == d
    T = [(D << (BITS * k)) % P for k in range(DIGITS)]
    col = [((t >> (32 * j)) & M32) + sum(dg[k] * ((T[k] >> (32 * j)) & M32) for k in range(DIGITS)) for j in range(8)] + [0]
    assert max(col) < 1 << 64
    S = sum(c << (32 * j) for j, c in enumerate(col))
    assert S % P == (t + d * D) % P
    hprev = [0] + [c >> 32 for c in col[:8]]
    top = col[7] + hprev[7]
    assert top < 1 << 64 and S // (1 << 224) - 3 < top <= S // (1 << 224)
    a96 = (top >> 32) * (MU & M32) + (((top & M32) * (MU & M32)) >> 32)
    assert MU >> 32 == 2 and a96 + 2 * top < 1 << 64
    q = (a96 + 2 * top) >> 32
    assert q == (top * MU) >> 64 and q < 1 << 32 and S // P - 1 <= q <= S // P
    n = [(((1 << 256) - P) >> (32 * j)) & M32 for j in range(8)] + [0]
    g = [q * n[j] + (col[j] & M32) + hprev[j] for j in range(9)]
    assert max(g) < 1 << 64
    w = [((g[j] & M32) + (g[j - 1] >> 32 if j else 0)) for j in range(9)]
    gen = [x >> 32 for x in w]
    w = [x & M32 for x in w]
    prop = [int(x == M32) for x in w[:8]] + [0]
    cin, c = [], 0
    for j in range(9):
        cin.append(c)
        c = gen[j] | (prop[j] & c)
    limbs = [(w[j] + cin[j]) & M32 for j in range(8)]
    R = sum(x << (32 * j) for j, x in enumerate(limbs))
    assert R == S - q * P and R < 2 * P
    first = R >= P
    if first:
        R -= P
    assert R < P                        # the second subtraction is margin
    return R, {"carried_through": sum(p_ & c_ for p_, c_ in zip(prop, cin)), "corrected": first, "q": q}


def _cases():
    rng = random.Random(2841)
    vals = [0, 1, P - 1, P - 2, (1 << 255) % P, (P - 1) // 2]
    ds = [0, 1, P - 1, P, 2 * P, 2 * P + 1, (1 << 256) - 1, (1 << 256) - 2, 1 << 255, (1 << 252) - 1, P + 1, 2 * P - 1,
          sum(((1 << BITS) - 1) << (BITS * k) for k in range(0, DIGITS - 1, 2)), sum(1 << (BITS * k) for k in range(DIGITS))]
    out = [("grid", t, D, d) for t in vals for D in vals for d in ds]
    for k in range(DIGITS):                                   # a single digit set: its least and its greatest value
        top = (1 << min(BITS, 256 - BITS * k)) - 1
        for D in (1, P - 1, rng.randrange(P)):
            for t in (0, P - 1):
                out.append(("digit", t, D, 1 << (BITS * k)))
                out.append(("digit", t, D, top << (BITS * k)))
    # a carry that travels through limbs of 0xFFFFFFFF.  D = 1 makes S = t + d; t = 2^224 - 1 and d = 1 is the plain long chain ...
    out.append(("carry", (1 << 224) - 1, 1, 1))
    out.append(("carry", (1 << 224) - 1, 1, (1 << 32) + 1))
    # ... and with a quotient: results with runs of zero limbs, which are either untouched zeros or 0xFFFFFFFF plus a carry
    for _ in range(600):
        lo_run, hi_run = sorted((rng.randrange(0, 7), rng.randrange(1, 8)))
        r_want = rng.randrange(P)
        for j in range(lo_run, hi_run + 1):
            r_want &= ~(M32 << (32 * j))
        D = rng.choice([1, 1, rng.randrange(P)])
        d = rng.randrange(1 << 256)
        out.append(("carry", (r_want - d * D) % P, D, d))
    for _ in range(4096):
        out.append(("random", rng.randrange(P), rng.randrange(P), rng.randrange(1 << 256)))
    return out


def _words(xs):
    return np.array([[(x >> (32 * i)) & M32 for i in range(8)] for x in xs], dtype=np.uint32)


@pytest.fixture(scope="module")
def run():
    """every case through the model and through one launch: (kind, t, D, d, want, facts, got) per case"""
    import torch
    cases = _cases()
    modelled = [model(t, D, d) for _, t, D, d in cases]
    pad = (-len(cases)) % 16
    t = _words([c[1] for c in cases] + [0] * pad)
    D = _words([c[2] for c in cases] + [0] * pad)
    d = _words([c[3] for c in cases] + [0] * pad)
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in (t, D, d)]
    out = torch.full((len(t), 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = DRV.lib().affine_step_driver(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(t), out.data_ptr())
    assert rc == 0
    got = out.cpu().numpy().view(np.uint32)
    ints = [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in got]
    return [(c[0], c[1], c[2], c[3], m[0], m[1], g) for c, m, g in zip(cases, modelled, ints)]


def test_model_is_the_field_operation(run):
    """what the model returns is t + (d mod r) * D mod r, the value the Montgomery product gave"""
    for _, t, D, d, want, _, _ in run:
        assert want == (t + (d % P) * D) % P


def test_inputs_reach_the_edges(run):
    """the inputs of this file do contain what they are meant to: carries through full limbs, with and without a quotient, and
    remainders that need the subtraction"""
    through = [f for kind, *_, f, _ in run if kind == "carry" and f["carried_through"]]
    assert len(through) >= 20 and any(f["carried_through"] >= 3 for f in through) and any(f["q"] > 0 for f in through)
    assert sum(f["corrected"] for *_, f, _ in run) >= 50
    assert any(f["q"] == 0 for *_, f, _ in run) and max(f["q"] for *_, f, _ in run) > 1 << 31


@pytest.mark.parametrize("kind", ["grid", "digit", "carry", "random"])
def test_affine_step(run, kind):
    bad = [(hex(t), hex(D), hex(d), hex(want), hex(got)) for k, t, D, d, want, _, got in run if k == kind and got != want]
    assert not bad, (len(bad), bad[:3])


def test_corrected_triples(run):
    """the triples whose remainder was at or above r before the subtraction"""
    sel = [(want, got) for *_, want, f, got in run if f["corrected"]]
    assert sel and all(w == g for w, g in sel)
