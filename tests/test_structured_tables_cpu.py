"""The fills of tests/tables.py (full-range, extreme and structured tables) on the CPU: the generators keep their contracts, the C oracle
and the independent python-int model (tests/golden/model.py) give the same proofs on every fill, and the zero-coefficient cases the GPU
tests rely on have the shape they are meant to have.  A GPU mismatch on these tables (tests/test_gpu_structured_tables.py) is therefore a
finding about the HIP path, not about the oracle."""
import os
import sys

import numpy as np
import pytest

import tables as T
from gkr_cases import random_circuit, scrambled_circuit

HERE = os.path.dirname(os.path.abspath(__file__))
R = T.R


@pytest.fixture(scope="module")
def model():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import model as m
    return m


# ---- the generators ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.FILLS)
@pytest.mark.parametrize("n", [1, 2, 64, 1 << 12])
def test_every_element_is_below_r(kind, n):
    a = T.fill(kind, n, 5)
    assert a.shape == (n, 4) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    assert T.below_r(a).all()
    assert all(T.to_int(row) < R for row in a[:64])                                  # ... and by python ints, not by below_r()
    assert np.array_equal(a, T.fill(kind, n, 5))                                     # seeded
    if kind not in ("stored_max", "zero", "one", "minus_one") and n >= 64:
        assert not np.array_equal(a, T.fill(kind, n, 6))


def test_arithmetic_fills_reach_what_random_fr_cannot(ora):
    n = 1 << 12
    assert T.at_least_2_254(T.fill("top", n, 1)).all()
    assert min(T.to_int(row) for row in T.fill("top", 256, 2)) >= 1 << 254
    assert T.at_least_2_254(T.fill("uniform_r", n, 1)).mean() > 0.35                 # 1 - 2^254 / r = 0.448 of the field
    assert all(T.to_int(row) == R - 1 for row in T.fill("stored_max", 8, 0))
    e = T.fill("limb_edges", n, 1)
    halves = np.concatenate([e & np.uint64(0xFFFFFFFF), e >> np.uint64(32)]).reshape(-1)
    assert set(int(v) for v in np.unique(halves)) == {0, 1, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF}
    for col in range(4):                                                             # every value in every low position (the top limb must stay < r's)
        lo = set(int(v) for v in np.unique(e[:, col] & np.uint64(0xFFFFFFFF)))
        assert lo == {0, 1, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF}
    # why this file exists: the suite's usual source of tables never leaves [0, 2^254)
    assert not T.at_least_2_254(ora.random_fr(1 << 16, 3)).any()


def test_shape_fills_hold_what_they_say(ora):
    n = 256
    assert T.canonical(T.fill("zero", 4, 0)) == [0] * 4
    assert T.canonical(T.fill("one", 4, 0)) == [1] * 4
    assert T.canonical(T.fill("minus_one", 4, 0)) == [R - 1] * 4
    assert set(T.canonical(T.fill("bits", n, 1))) == {0, 1}
    b = T.canonical(T.fill("bytes", 1 << 12, 1))
    assert max(b) == 255 and min(b) == 0
    h = T.canonical(T.fill("one_hot", n, 1))
    assert sum(1 for v in h if v) == 1
    assert {T.canonical(T.fill("one_hot", n, s)).index(max(T.canonical(T.fill("one_hot", n, s)))) for s in range(8)} != {0}
    c = T.canonical(T.fill("halves_cancel", n, 1))
    assert all((x + y) % R == 0 for x, y in zip(c[:n // 2], c[n // 2:])) and any(c)
    q = T.canonical(T.fill("halves_equal", n, 1))
    assert q[:n // 2] == q[n // 2:] and len(set(q)) == n // 2
    for kind in T.FILLS:                                                             # canonical() is the oracle's own conversion
        a = T.fill(kind, 16, 9)
        assert T.canonical(a) == ora.fr_to_ints(a)
        assert np.array_equal(ora.fr_from_ints(T.canonical(a)), a)
    z = np.zeros((3, 4), dtype=np.uint64)
    assert np.array_equal(T.negate(z), z)
    u = T.fill("limb_edges", 64, 4)
    assert [(-v) % R for v in T.canonical(u)] == T.canonical(T.negate(u))


# ---- oracle == model on every fill ----------------------------------------------------------------------------------------------------
LOGS = [1, 3, 6]


def _kinds_for(kind, count):
    return T.rotation(T.FILLS, kind, count)


@pytest.mark.parametrize("kind", T.FILLS)
def test_sumcheck_oracle_equals_model(ora, model, kind):
    for log_n in LOGS:
        ev = T.fill(kind, 1 << log_n, 100 + log_n)
        s, rp, ch = ora.sumcheck_prove(ev)
        ms, mrp, mch = model.sumcheck_prove(T.canonical(ev))
        assert ora.fr_to_ints(s) == [ms]
        assert [ora.fr_to_ints(r) for r in rp] == mrp and ora.fr_to_ints(ch) == mch
        assert ora.sumcheck_verify(ev, s, rp)
        rp2, ch2 = T.sumcheck_with_claimed_sum(ora, ev, s)                           # the round-by-round restatement the GPU tests use
        assert np.array_equal(rp2, rp) and np.array_equal(ch2, ch)
        rp0, ch0 = T.sumcheck_with_claimed_sum(ora, ev, np.zeros(4, dtype=np.uint64))
        assert np.array_equal(rp0[0], rp[0]) and (np.array_equal(ch0, ch) == (ms == 0))


@pytest.mark.parametrize("kind", T.FILLS)
def test_composed_oracle_equals_model(ora, model, kind):
    for log_n in LOGS:
        for k in (2, 3, 5):
            for kinds in (_kinds_for(kind, k), [kind] * k):
                t = np.stack([T.fill(f, 1 << log_n, 200 + 10 * log_n + q) for q, f in enumerate(kinds)])
                rp, ch = ora.composed_prove(t)
                mrp, mch = model.composed_prove([T.canonical(x) for x in t])
                assert [ora.fr_to_ints(r) for r in rp] == mrp and ora.fr_to_ints(ch) == mch, (log_n, kinds)
                assert ora.fr_to_ints(ora.composed_sum(t)) == [model.product_sums([T.canonical(x) for x in t])]


@pytest.mark.parametrize("kind", T.FILLS)
def test_multi_composed_oracle_equals_model(ora, model, kind):
    for log_n in LOGS:
        for sizes in ([2, 2], [2, 1], [1, 1]):
            kinds = _kinds_for(kind, sum(sizes))
            flat = np.stack([T.fill(f, 1 << log_n, 300 + 10 * log_n + q) for q, f in enumerate(kinds)])
            ints = [T.canonical(x) for x in flat]
            terms, at = [], 0
            for k in sizes:
                terms.append(ints[at:at + k])
                at += k
            s = ora.multi_composed_sum(flat, sizes)
            assert ora.fr_to_ints(s) == [model.multi_composed_sum(terms)]
            for partial in (True, False):
                rps, ch = ora.multi_composed_prove(flat, sizes, s, partial)
                mrps, mch = model.multi_composed_prove(terms, ora.fr_to_ints(s)[0], partial)
                assert [p.monomials() for p in rps] == mrps and ora.fr_to_ints(ch) == mch, (log_n, sizes, partial)
                assert ora.multi_composed_proof_bytes(rps) == model.proof_bytes(mrps)


def _gkr_same(ora, proof, want):
    """an oracle GkrProof against the model's dict"""
    if proof.n_proofs != len(want["layers"]) or ora.fr_to_ints(np.array(proof.w0[0:8], dtype=np.uint64)) != want["w0"]:
        return False
    for k, lp in enumerate(want["layers"]):
        s, rps, wb, wc = proof.layer(k)
        got = (ora.fr_to_ints(s)[0], [p.monomials() for p in rps], ora.fr_to_ints(proof.layer_challenges(k)), ora.fr_to_ints(wb)[0], ora.fr_to_ints(wc)[0])
        if got != (lp["sum"], lp["rps"], lp["challenges"], lp["wb"], lp["wc"]):
            return False
    return True


@pytest.mark.parametrize("kind", T.FILLS)
@pytest.mark.parametrize("depth", [3, 4])
def test_gkr_oracle_equals_model(ora, model, kind, depth):
    inp = T.fill(kind, 1 << depth, 400 + depth)
    for layers in (random_circuit(depth), scrambled_circuit(depth, 40 + depth)):
        ev = ora.circuit_evaluation(layers, inp)
        mev = model.circuit_evaluation(layers, T.canonical(inp))
        assert [ora.fr_to_ints(e) for e in ev] == mev
        want = model.gkr_prove(layers, mev)
        dense, sparse = ora.gkr_prove(layers, ev), ora.gkr_prove_sparse(layers, ev)
        assert _gkr_same(ora, dense, want) and _gkr_same(ora, sparse, want)
        assert dense.fields() == sparse.fields()
        assert ora.gkr_verify(layers, inp, dense)
        assert model.gkr_verify(layers, T.canonical(inp), want)


# ---- the zero-coefficient families of the GPU tests, on the oracle's proof alone ---------------------------------------------------
ZERO_COEFF_LOG = 15


@pytest.mark.parametrize("family,want_lens,zero_sum", [
    ("linear", [2] * ZERO_COEFF_LOG, False),
    ("first_round", [2] + [3] * (ZERO_COEFF_LOG - 1), False),
    ("zero_sum", [2] * ZERO_COEFF_LOG, True),
])
def test_zero_coefficient_families_have_their_shape(ora, family, want_lens, zero_sum):
    flat = T.zero_coeff_tables(family, ZERO_COEFF_LOG)
    s = ora.multi_composed_sum(flat, [2, 2])
    assert (ora.fr_to_ints(s) == [0]) == zero_sum
    rps, ch = ora.multi_composed_prove(flat, [2, 2], s, True)
    assert [p.len for p in rps] == want_lens
    assert [[w for c, w in p.monomials()] for p in rps] == [[0, 1, 2][:l] for l in want_lens]
    assert all(c != 0 for p in rps for c, w in p.monomials())
    if zero_sum:
        (c0, _), (c1, _) = rps[0].monomials()
        assert (2 * c0 + c1) % R == 0                                                # p(0) + p(1) = 0


def test_cancelling_terms_keep_their_zero_coefficients(ora, model):
    flat = T.cancelling_tables(12)
    s = ora.multi_composed_sum(flat, [2, 2])
    assert ora.fr_to_ints(s) == [0]
    rps, ch = ora.multi_composed_prove(flat, [2, 2], s, True)
    assert [p.monomials() for p in rps] == [[(0, 0), (0, 1)]] * 12
    small = T.cancelling_tables(4)
    ints = [T.canonical(x) for x in small]
    mrps, mch = model.multi_composed_prove([ints[:2], ints[2:]], 0, True)
    orps, och = ora.multi_composed_prove(small, [2, 2], ora.fr_from_ints([0])[0], True)
    assert [p.monomials() for p in orps] == mrps == [[(0, 0), (0, 1)]] * 4 and ora.fr_to_ints(och) == mch
