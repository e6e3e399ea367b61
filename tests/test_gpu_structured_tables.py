"""GPU parity on the tables of tests/tables.py: the provers, the Multilinear operations and Domain.fft / ifft on full-range, extreme and
structured inputs, bit for bit against the CPU oracle on the same limbs.

Every other GPU parity test draws its tables from oracle.random_fr (stored values below 2^254) or from 62-bit limbs: the kernels that
stream the CALLER's table -- the sums passes, the first fold, the composed first round in all its forms, the GKR layer tables, the one-pass
evaluation -- never read a stored value in [2^254, r), a limb of 0 or 0xFFFFFFFF, a constant table or one whose sums vanish.  Those are the
kernels with lazy reductions and unreduced accumulators.  tests/test_structured_tables_cpu.py holds the oracle to the independent
python-int model on every fill used here, so a mismatch in this file is a finding about the HIP path.

Forms that only an environment switch reaches run in a child process each (fresh process: the overrides are read once), one after
another: this file run as a program is that child."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tables as T
from gkr_cases import gkr_proof_mismatches, random_circuit, scrambled_circuit
from test_gpu_sumcheck import ENQUEUE_ORDER, ENQUEUE_ORDER_OVERLAPPED, _enqueue_order, _unsummed

pytestmark = pytest.mark.gpu

LARGE = T.FILLS_ARITH + ["bits", "zero"]                      # from 2^19 entries on: the oracle takes its seconds there
DIAGONAL = ["stored_max", "zero", "one", "minus_one"]        # every factor of a product the same constant table
ZERO = np.zeros(4, dtype=np.uint64)


def _param_id(v):
    return "x".join(str(e) for e in v) if isinstance(v, list) else str(v)


def fills_for(log_n):
    return T.FILLS if log_n < 19 else LARGE


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _same(*pairs):
    return all(np.array_equal(a, b) for a, b in pairs)


# ---- Sumcheck -----------------------------------------------------------------------------------------------------------------------
def sumcheck_mismatches(zk, ora, ev):
    """poly_sum() + prove() against the oracle's proof, and prove() alone (the transcript absorbs the default sum, zero) against the
    oracle's rounds restated on that claimed sum"""
    bad = []
    s, rp, och = ora.sumcheck_prove(ev)
    sc = zk.Sumcheck(zk.Multilinear(ev))
    sc.poly_sum()
    proof, ch = sc.prove()
    if not _same((proof.sum, s), (proof.univariate_poly, rp), (ch, och), (sc.sum, s)):
        bad.append("poly_sum + prove")
    proof, ch = zk.Sumcheck(zk.Multilinear(ev)).prove()
    rp0, ch0 = T.sumcheck_with_claimed_sum(ora, ev, ZERO)
    if not _same((proof.sum, ZERO), (proof.univariate_poly, rp0), (ch, ch0)):
        bad.append("prove without poly_sum")
    return bad


def plan_names(zk, ora, ev):
    """the launch scopes of one proof whose every sum the library derives itself, in host enqueue order; the proof is the oracle's"""
    (proof, ch), names = _enqueue_order(zk, _unsummed(zk, ev).prove)
    s, rp, och = ora.sumcheck_prove(ev)
    assert _same((proof.sum, s), (proof.univariate_poly, rp), (ch, och))
    return names


@pytest.mark.parametrize("log_n,kind", [(l, k) for l in sorted(ENQUEUE_ORDER) for k in fills_for(l)])
def test_sumcheck_prove(zk, ora, log_n, kind):
    """2^10: the serial kernel alone; 2^11: one stage; 2^19: two stages; 2^21: the first fold in the matrix-core form"""
    assert sumcheck_mismatches(zk, ora, T.fill(kind, 1 << log_n, 1000 + log_n)) == []


@pytest.mark.parametrize("log_n", sorted(ENQUEUE_ORDER))
def test_sumcheck_structured_tables_take_their_plan(zk, ora, log_n):
    for kind in ("top", "zero"):
        names = plan_names(zk, ora, T.fill(kind, 1 << log_n, 1100 + log_n))
        print(log_n, kind, names)
        assert set(names) == set(ENQUEUE_ORDER[log_n])


def _run_child(job, env, timeout):
    """This file as a program in a process of its own with `env` set -> what the job returned"""
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(job)], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit("a child of %s hung: nothing more is started on this device\n%s" % (os.path.basename(__file__), (e.stdout or b"").decode()[-3000:]), 1)
    text = out.stdout.decode()
    if out.returncode < 0 or out.returncode in (134, 139):
        pytest.exit("a child of %s was killed (%d): nothing more is started on this device\n%s" % (os.path.basename(__file__), out.returncode, text[-3000:]), 1)
    assert out.returncode == 0, text[-3000:]
    return json.loads(text.strip().splitlines()[-1])


def test_sumcheck_prove_in_the_overlapped_plan():
    """ZKHIP_OVERLAP_MIN_LOG=19: fine_sums, coarse_sums, blockfold, multifold and multifold_valu read the caller's table at 2^19 / 2^20"""
    got = _run_child({"overlapped": [19, 20]}, {"ZKHIP_OVERLAP_MIN_LOG": "19"}, 300)
    print(got)
    assert got["bad"] == []
    for log_n in ("19", "20"):
        assert set(got["names"][log_n]) == set(ENQUEUE_ORDER_OVERLAPPED[log_n])


def _job_overlapped(zk, ora, logs):
    bad, names = [], {}
    for log_n in logs:
        for kind in LARGE:
            bad += ["%d %s: %s" % (log_n, kind, b) for b in sumcheck_mismatches(zk, ora, T.fill(kind, 1 << log_n, 1000 + log_n))]
        names[str(log_n)] = plan_names(zk, ora, T.fill("top", 1 << log_n, 1100 + log_n))
    return {"bad": bad, "names": names}


# ---- ComposedSumcheck ---------------------------------------------------------------------------------------------------------------
def composed_cases(k, pool):
    """(label, the fill of each of the k tables): table q of case i takes pool[(i + q) % len], and the diagonals the pool holds"""
    return [(lead, T.rotation(pool, lead, k)) for lead in pool] + [("all_" + d, [d] * k) for d in DIAGONAL if d in pool]


def composed_mismatch(zk, ora, k, log_n, kinds):
    t = np.stack([T.fill(f, 1 << log_n, 2000 + 100 * k + 10 * log_n + q) for q, f in enumerate(kinds)])
    poly = zk.ComposedMultilinear(list(t))
    proof, ch = zk.ComposedSumcheck(poly).prove()
    rp, och = ora.composed_prove(t)
    return not _same((proof.round_polys, rp), (ch, och), (zk.ComposedSumcheck.calculate_poly_sum(poly), ora.composed_sum(t)))


COMPOSED_IN_PROCESS = [(1, 10), (2, 12), (3, 9), (4, 10), (5, 13), (2, 18), (3, 16)]   # (2, 18): the stage form; (3, 16): across CMP_TSPLIT_MAX


@pytest.mark.parametrize("k,log_n,label,kinds", [(k, l, label, kinds) for k, l in COMPOSED_IN_PROCESS for label, kinds in composed_cases(k, T.FILLS)],
                         ids=_param_id)
def test_composed_prove(zk, ora, k, log_n, label, kinds):
    assert not composed_mismatch(zk, ora, k, log_n, kinds)


def composed_scopes(zk, ora, k, log_n, kinds):
    """the launch scopes of one ComposedSumcheck proof (the library's profile); the proof is the oracle's"""
    t = np.stack([T.fill(f, 1 << log_n, 2000 + 100 * k + 10 * log_n + q) for q, f in enumerate(kinds)])
    (proof, ch), names = _enqueue_order(zk, zk.ComposedSumcheck(zk.ComposedMultilinear(list(t))).prove)
    rp, och = ora.composed_prove(t)
    assert _same((proof.round_polys, rp), (ch, och))
    return sorted(set(names))


def _job_composed(zk, ora, cases):
    bad = ["%d x 2^%d %s" % (k, log_n, label) for k, log_n, pool in cases for label, kinds in composed_cases(k, pool)
           if composed_mismatch(zk, ora, k, log_n, kinds)]
    return {"bad": bad, "scopes": {"%d x 2^%d" % (k, log_n): composed_scopes(zk, ora, k, log_n, T.rotation(pool, pool[0], k)) for k, log_n, pool in cases}}


STAGE_SCOPES = {"composed_cross2", "composed_stage_close", "composed_fold2"}
# switches, cases (tables, log2 of the entries, fills), and per case the launch scopes that must / must not appear
COMPOSED_FORMS = {
    # composed_round_wide2_kernel from CMP_WIDE_MIN_WORK pairs on (the oracle takes seconds per proof there: three fills), and the round form
    "round_form": ({"ZKHIP_STAGE": "0"}, [(2, 21, ["top", "stored_max", "bits"]), (2, 16, T.FILLS)], {"composed_round"}, STAGE_SCOPES),
    "stage_form_at_its_smallest": ({"ZKHIP_STAGE": "1"}, [(2, 16, T.FILLS)], STAGE_SCOPES, set()),
    "cross_sums_on_the_valu": ({"ZKHIP_STAGE": "1", "ZKHIP_CROSS_VALU": "1"}, [(2, 16, T.FILLS)], STAGE_SCOPES, set()),        # composed_cross2_kernel
    "round_dot": ({"ZKHIP_ROUND_DOT_MIN_LOG": "8"}, [(5, 12, T.FILLS)], {"composed_round"}, set()),                              # every round on the matrix cores
    "round_dot_two_workgroups": ({"ZKHIP_ROUND_DOT_MIN_LOG": "8", "ZKHIP_ROUND_GRID": "2"}, [(5, 12, T.FILLS)], {"composed_round"}, set()),
    "round_by_round": ({"ZKHIP_PIPE": "0"}, [(2, 14, T.FILLS), (5, 10, T.FILLS)], {"composed_round"}, {"composed_pipe_round"}),
}


@pytest.mark.parametrize("form", sorted(COMPOSED_FORMS))
def test_composed_prove_forced_forms(form):
    env, cases, must, never = COMPOSED_FORMS[form]
    got = _run_child({"composed": cases}, env, 600)
    print(got)
    assert got["bad"] == []
    for case, scopes in got["scopes"].items():
        assert must <= set(scopes) and not never & set(scopes), (case, scopes)


def test_composed_default_form_of_two_tables_at_2_18_is_the_stage_form(zk, ora):
    assert STAGE_SCOPES <= set(composed_scopes(zk, ora, 2, 18, ["top", "stored_max"]))


# ---- MultiComposedSumcheckProver ----------------------------------------------------------------------------------------------------
def multi_mismatches(zk, ora, flat, sizes, want_lens=None):
    """calculate_poly_sum, prove_partial and prove on the tables flat [sum(sizes), n, 4]: to_bytes(), monomials(), challenges, claimed sum"""
    bad, terms, at = [], [], 0
    for k in sizes:
        terms.append(zk.ComposedMultilinear([zk.Multilinear(t) for t in flat[at:at + k]]))
        at += k
    s = ora.multi_composed_sum(flat, sizes)
    if not np.array_equal(zk.MultiComposedSumcheckProver.calculate_poly_sum(terms), s):
        bad.append("sum")
    for partial in (True, False):
        proof, ch = (zk.MultiComposedSumcheckProver.prove_partial if partial else zk.MultiComposedSumcheckProver.prove)(terms, s)
        orps, och = ora.multi_composed_prove(flat, sizes, s, partial)
        ok = proof.to_bytes() == ora.multi_composed_proof_bytes(orps) and [p.monomials() for p in proof.round_polys] == [o.monomials() for o in orps]
        if not (ok and _same((ch, och), (proof.sum, s))):
            bad.append("prove_partial" if partial else "prove")
        if want_lens is not None and [len(p.monomials()) for p in proof.round_polys] != want_lens:
            bad.append("monomials per round")
    return bad


def multi_tables(sizes, log_n, lead):
    kinds = T.rotation(T.FILLS, lead, sum(sizes))
    return np.stack([T.fill(f, 1 << log_n, 3000 + 10 * log_n + q) for q, f in enumerate(kinds)])


MULTI_IN_PROCESS = [([2, 2], 18), ([2, 3], 10), ([1, 5], 8), ([2, 2, 1, 1], 9)]


@pytest.mark.parametrize("sizes,log_n,lead", [(s, l, lead) for s, l in MULTI_IN_PROCESS for lead in T.FILLS], ids=_param_id)
def test_multi_composed_prove(zk, ora, sizes, log_n, lead):
    assert multi_mismatches(zk, ora, multi_tables(sizes, log_n, lead), sizes) == []


@pytest.mark.parametrize("family", sorted(T.ZERO_COEFF_FAMILIES))
def test_multi_composed_zero_coefficients_are_dropped(zk, ora, family):
    """sparse_univariate.rs:55 in the stage form, the pipelined closing kernels and the LDS tail: 2^18 entries, 18 rounds"""
    assert multi_mismatches(zk, ora, T.zero_coeff_tables(family, 18), [2, 2], T.zero_coeff_lens(family, 18)) == []


@pytest.mark.parametrize("log_n", [12, 18])
def test_multi_composed_cancelling_terms_keep_their_zeros(zk, ora, log_n):
    flat = T.cancelling_tables(log_n)
    assert multi_mismatches(zk, ora, flat, [2, 2], [2] * log_n) == []
    terms = [zk.ComposedMultilinear([zk.Multilinear(t) for t in flat[:2]]), zk.ComposedMultilinear([zk.Multilinear(t) for t in flat[2:]])]
    proof, ch = zk.MultiComposedSumcheckProver.prove_partial(terms, ZERO)
    assert [p.monomials() for p in proof.round_polys] == [[(0, 0), (0, 1)]] * log_n


def _job_multi(zk, ora, cases):
    bad = []
    for sizes, log_n in cases:
        for lead in T.FILLS:
            bad += ["%s 2^%d %s: %s" % (sizes, log_n, lead, b) for b in multi_mismatches(zk, ora, multi_tables(sizes, log_n, lead), sizes)]
        for family in sorted(T.ZERO_COEFF_FAMILIES):
            got = multi_mismatches(zk, ora, T.zero_coeff_tables(family, log_n), [2, 2], T.zero_coeff_lens(family, log_n))
            bad += ["%s 2^%d %s: %s" % (sizes, log_n, family, b) for b in got]
    return {"bad": bad}


def test_multi_composed_prove_in_the_stage_form_at_its_smallest():
    """ZKHIP_STAGE=1: the stage form from 2^15 entries on -- every fill and the three zero-coefficient families of
    tests/test_structured_tables_cpu.py at the size that file pins them at"""
    assert _run_child({"multi": [([2, 2], 15)]}, {"ZKHIP_STAGE": "1"}, 600)["bad"] == []


# ---- GKR ----------------------------------------------------------------------------------------------------------------------------
GKR_DEPTHS = [6, 10, 12]                                      # 6: against the dense prover and its verifier; 10, 12: the sparse restatement


def _gkr_layers(depth, which):
    return random_circuit(depth) if which == "random" else scrambled_circuit(depth, 50 + depth)


@functools.lru_cache(maxsize=16)
def _gkr_case(depth, which, kind):
    """(layers, input, the oracle's evaluation, the oracle's proof): computed once, shared by the tests whose batches hold this input"""
    from oracle import oracle as ora
    layers = _gkr_layers(depth, which)
    inp = T.fill(kind, 1 << depth, 4000 + depth)
    ev = ora.circuit_evaluation(layers, inp)
    return layers, inp, ev, (ora.gkr_prove if depth == 6 else ora.gkr_prove_sparse)(layers, ev)


@functools.lru_cache(maxsize=None)
def _gkr_circuit(depth, which):
    import zk_cryptography_amd as zk
    return zk.Circuit.from_tuples(_gkr_layers(depth, which))


@pytest.mark.parametrize("depth,kind", [(d, k) for d in GKR_DEPTHS for k in T.FILLS])
def test_gkr_prove(zk, ora, depth, kind):
    """Inputs from every fill (real inputs are small integers and bits; all-zero: every layer sum 0, every round polynomial vanishing):
    prove, the sharded prover's sessions on one rank, and a batch of three inputs of different fills"""
    from test_gpu_gkr import _to_oracle_proof
    for which in ("random", "scrambled"):
        circuit = _gkr_circuit(depth, which)
        batch = [_gkr_case(depth, which, k) for k in T.rotation(T.FILLS, kind, 3)]
        layers, inp, want_ev, want = batch[0]
        ev = circuit.evaluation(inp)
        assert all(np.array_equal(a.cpu().numpy().view(np.uint64), b) for a, b in zip(ev, want_ev)), which
        proof = zk.GKRProtocol.prove(circuit, ev)
        assert gkr_proof_mismatches(ora, proof, want) == [], which
        assert gkr_proof_mismatches(ora, zk.GKRProtocol.prove_sharded(circuit, ev, use_stages=True), want) == [], which
        if depth == 6:
            assert ora.gkr_verify(layers, inp, want) and ora.gkr_verify(layers, inp, _to_oracle_proof(zk, ora, proof)), which
        proofs = zk.GKRProtocol.prove_batch(circuit, [ev] + [circuit.evaluation(c[1]) for c in batch[1:]])
        assert [gkr_proof_mismatches(ora, p, c[3]) for p, c in zip(proofs, batch)] == [[], [], []], which


# ---- Multilinear --------------------------------------------------------------------------------------------------------------------
ML_FILLS = T.FILLS_ARITH + ["bits", "halves_cancel"]
SPECIAL_POINTS = [0, 1, T.R - 1]


def _points(count, seed, special=None, at=()):
    """`count` full-range random points, those at the positions `at` replaced by the value `special`"""
    pts = T.fill("uniform_r", count, seed)
    for j in at:
        pts[j % count] = T.stored(special)
    return pts


@pytest.mark.parametrize("log_n,kind", [(l, k) for l in (10, 11, 13, 16) for k in ML_FILLS])
def test_partial_evaluation(zk, ora, log_n, kind):
    a = T.fill(kind, 1 << log_n, 5000 + log_n)
    poly = zk.Multilinear(a)
    points = [T.fill("top", 1, 51)[0], T.fill("uniform_r", 1, 52)[0]] + [T.stored(v) for v in SPECIAL_POINTS]
    for k in sorted({0, 1, log_n // 2, log_n - 1}):
        for j, r in enumerate(points):
            assert np.array_equal(poly.partial_evaluation(r, k).to_numpy(), ora.mle_partial_evaluation(a, r, k)), (k, j)


@pytest.mark.parametrize("log_n,kind", [(l, k) for l in (11, 15, 19) for k in ML_FILLS])
def test_half_sums_and_sum(zk, ora, log_n, kind):
    a = T.fill(kind, 1 << log_n, 5100 + log_n)
    poly = zk.Multilinear(a)
    assert np.array_equal(poly.split_poly_into_two_and_sum_each_part().to_numpy(), ora.mle_half_sums(a))
    assert np.array_equal(poly.sum_over_the_boolean_hypercube(), ora.mle_sum(a))


@pytest.mark.parametrize("log_n,kind", [(l, k) for l in (12, 17, 19) for k in ML_FILLS])
def test_evaluation(zk, ora, log_n, kind):
    """either side of 2^17, where `evaluation` becomes one pass over the caller's table"""
    a = T.fill(kind, 1 << log_n, 5200 + log_n)
    poly = zk.Multilinear(a)
    cases = [_points(log_n, 61)] + [_points(log_n, 62 + i, v, (0, 7, 8, log_n - 1)) for i, v in enumerate(SPECIAL_POINTS)]
    cases += [np.tile(T.stored(v), (log_n, 1)) for v in SPECIAL_POINTS]
    for j, pts in enumerate(cases):
        assert np.array_equal(poly.evaluation(pts), ora.mle_evaluation(a, pts)), j


@pytest.mark.parametrize("kind", ML_FILLS)
def test_partial_evaluations_of_the_leading_variables(zk, ora, kind):
    a = T.fill(kind, 1 << 12, 5300)
    poly = zk.Multilinear(a)
    for k in (1, 5, 12):
        for j, pts in enumerate([_points(k, 71)] + [_points(k, 72 + i, v, (0, k // 2, k - 1)) for i, v in enumerate(SPECIAL_POINTS)]):
            got = poly.partial_evaluations(pts, [0] * k).to_numpy().reshape(-1, 4)
            assert np.array_equal(got, ora.mle_partial_evaluations(a, pts, [0] * k)), (k, j)


# ---- Domain.fft / ifft --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,kind", [(l, k) for l in (10, 12, 14, 16) for k in T.FILLS_ARITH + ["zero", "one_hot"]])
def test_domain_fft_ifft(zk, ora, log_n, kind):
    """the kernel-level NTT tests feed full-range values; Domain's own path only ever got oracle.random_fr"""
    n = 1 << log_n
    x = T.fill(kind, n, 6000 + log_n)
    d = zk.Domain(n)
    assert np.array_equal(d.fft(x).cpu().numpy().view(np.uint64), ora.domain_fft(x, n))
    assert np.array_equal(d.ifft(x).cpu().numpy().view(np.uint64), ora.domain_ifft(x, n))


# ---- the child ----------------------------------------------------------------------------------------------------------------------
JOBS = {"overlapped": _job_overlapped, "composed": _job_composed, "multi": _job_multi}

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import zk_cryptography_amd
    from oracle import oracle
    oracle.lib()
    (name, arg), = json.loads(sys.argv[1]).items()
    print(json.dumps(JOBS[name](zk_cryptography_amd, oracle, arg)))
