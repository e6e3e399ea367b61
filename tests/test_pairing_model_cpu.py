"""CPU: the independent pairing model (tests/pairing_model.py) pinned on the group laws and on the reference's own KZG verdicts
(kzg/src/multilinear_kzg.rs:132-197, kzg/src/univariate_kzg.rs:111-150), entirely in python."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_model as PM  # noqa: E402

M = PM.M


def test_g2_generator_on_twist_and_of_order_r():
    assert PM.g2_on_curve(PM.G2)
    assert PM.g2_mul_raw(PM.G2, PM.R) is None
    assert PM.g2_mul_raw(PM.G2, PM.R - 1) == PM.g2_neg(PM.G2)


def test_bilinear_of_order_r_and_non_degenerate():
    a, b = 0x1234567, 0xABCDEF01
    e = PM.pairing(M.G1, PM.G2)
    assert not PM.gt_is_one(e)
    assert PM.gt_is_one(PM.f12_pow(e, PM.R))
    assert PM.pairing(M.g1_mul(M.G1, a), PM.g2_mul(PM.G2, b)) == PM.f12_pow(e, a * b)
    assert PM.gt_is_one(PM.pairing(None, PM.G2)) and PM.gt_is_one(PM.pairing(M.G1, None))


def test_exact_hard_part_identity():
    x, p, r = -PM.X_ABS, PM.P, PM.R
    assert (x - 1) ** 2 % 3 == 0
    assert ((x - 1) ** 2 // 3) * (x + p) * (x * x + p * p - 1) + 1 == (p ** 4 - p ** 2 + 1) // r
    assert (p ** 4 - p ** 2 + 1) % r == 0


def _ml_case(vals, prover, verifier):
    vals = [v % PM.R for v in vals]
    srs = M.multilinear_srs(prover)
    commit = M.commit(vals, srs, True)
    evaluation, proofs = M.kzg_open(vals, verifier, srs)
    return commit, evaluation, proofs


def test_kzg_1_verdict():                  # multilinear_kzg.rs:132-155
    commit, ev, proofs = _ml_case([0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    assert PM.multilinear_verify(commit, [5, 9, 6], ev, proofs, PM.multilinear_srs_g2([2, 3, 4])) is True


def test_kzg_2_verdicts():                 # multilinear_kzg.rs:157-197
    vals = [0, 0, 0, 2, 0, 0, 10, 12, 0, -12, 4, -6, 0, -12, 14, 4]
    commit, ev, proofs = _ml_case(vals, [12, 9, 28, 40], [54, 90, 76, 160])
    z = [54, 90, 76, 160]
    assert PM.multilinear_verify(commit, z, ev, proofs, PM.multilinear_srs_g2([12, 9, 28, 40])) is True
    assert PM.multilinear_verify(commit, z, ev, proofs, PM.multilinear_srs_g2([12, 19, 28, 40])) is False


def _uv_case():
    srs = M.univariate_srs(10, 4)
    coeffs = [1, 2, 3, 4, 5]
    commit = M.commit(coeffs, srs, False)
    ev, proof = M.univariate_open(coeffs, 2, srs)
    return commit, ev, proof, PM.univariate_srs_g2(10, 4)


def test_univariate_kzg_verdict():         # univariate_kzg.rs:111-129
    commit, ev, proof, g2 = _uv_case()
    assert PM.univariate_verify(commit, 2, ev, proof, g2) is True


def test_univariate_kzg_invalid_opening_verdict():   # univariate_kzg.rs:131-150
    commit, ev, proof, g2 = _uv_case()
    assert PM.univariate_verify(commit, 4, ev, proof, g2) is False


def test_rewritten_check_agrees_with_the_reference_form():
    """e(C - vG1 + sum z_i pi_i, G2) * prod e(-pi_i, tau_i G2) == 1, the form the device computes, on the kzg_1 data"""
    commit, ev, proofs = _ml_case([0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    z, g2 = [5, 9, 6], PM.multilinear_srs_g2([2, 3, 4])
    acc = M.g1_add(commit, M.g1_mul(M.G1, (-ev) % PM.R))
    for zi, pi in zip(z, proofs):
        acc = M.g1_add(acc, M.g1_mul(pi, zi))
    pairs = [(acc, PM.G2)] + [(None if pi is None else (pi[0], (-pi[1]) % PM.P), t) for pi, t in zip(proofs, g2)]
    assert PM.gt_is_one(PM.multi_pairing(pairs))
