"""GPU: MultilinearKZG::verify / UnivariateKZG::verify through the pairing kernels -- the reference's own KZG tests with their
verify calls and expected booleans (kzg/src/multilinear_kzg.rs:132-197, kzg/src/univariate_kzg.rs:111-150), open -> verify round
trips, single tampers, and batches that must return exactly the verdicts of single calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
PM, M = PC.PM, PC.M

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _ml(zk, vals, prover, verifier):
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints(prover), g2=True)
    poly = zk.Multilinear(zk.Fr.from_ints(vals))
    commit = zk.MultilinearKZG.commitment(poly, srs)
    proof = zk.MultilinearKZG.open(poly, zk.Fr.from_ints(verifier), srs)
    return srs, commit, proof


def test_kzg_1(zk):                        # multilinear_kzg.rs:132-155
    srs, commit, proof = _ml(zk, [0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    assert zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([5, 9, 6]), proof, srs) is True


def test_kzg_2(zk):                        # multilinear_kzg.rs:157-197
    vals = [0, 0, 0, 2, 0, 0, 10, 12, 0, -12, 4, -6, 0, -12, 14, 4]
    srs, commit, proof = _ml(zk, vals, [12, 9, 28, 40], [54, 90, 76, 160])
    tampered = zk.TrustedSetup.setup(zk.Fr.from_ints([12, 19, 28, 40]), g2=True)
    pts = zk.Fr.from_ints([54, 90, 76, 160])
    assert zk.MultilinearKZG.verify(commit, pts, proof, srs) is True
    assert zk.MultilinearKZG.verify(commit, pts, proof, tampered) is False


def _uv(zk, z_open):
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(10), 4, g2=True)
    poly = zk.DenseUnivariatePolynomial(zk.Fr.from_ints([1, 2, 3, 4, 5]))
    commit = zk.UnivariateKZG.commitment(poly, srs)
    proof = zk.UnivariateKZG.open(poly, zk.Fr.from_int(z_open), srs)
    return srs, commit, proof


def test_univariate_kzg(zk):               # univariate_kzg.rs:111-129
    srs, commit, proof = _uv(zk, 2)
    assert zk.UnivariateKZG.verify(commit, zk.Fr.from_int(2), proof, srs) is True


def test_univariate_kzg_invalid_opening(zk):   # univariate_kzg.rs:131-150
    srs, commit, proof = _uv(zk, 2)
    assert zk.UnivariateKZG.verify(commit, zk.Fr.from_int(4), proof, srs) is False


def test_verify_needs_the_g2_half(zk):
    srs1 = zk.TrustedSetup.setup(zk.Fr.from_ints([2, 3, 4]))
    _, commit, proof = _ml(zk, [0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    with pytest.raises(ValueError):
        zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([5, 9, 6]), proof, srs1)


@pytest.mark.parametrize("nv", [2, 3, 5, 8, 12, 16, 20])
def test_multilinear_round_trip_and_tampers(zk, nv):
    rng = np.random.default_rng(nv)
    tau = zk.Fr.random(nv, 100 + nv)
    z = zk.Fr.random(nv, 200 + nv)
    vals = zk.Fr.random(1 << nv, 300 + nv)
    srs = zk.TrustedSetup.setup(tau, g2=True)
    poly = zk.Multilinear(vals)
    commit = zk.MultilinearKZG.commitment(poly, srs)
    proof = zk.MultilinearKZG.open(poly, z, srs)
    V = zk.MultilinearKZG.verify
    assert V(commit, z, proof, srs)
    # evaluation
    bad = zk.MultilinearKZGProof(zk.Fr.from_int(zk.Fr.to_ints(proof.evaluation)[0] + 1), proof.proofs)
    assert not V(commit, z, bad, srs)
    # one proof point
    i = int(rng.integers(nv))
    swapped = list(proof.proofs)
    swapped[i] = commit
    assert not V(commit, z, zk.MultilinearKZGProof(proof.evaluation, swapped), srs)
    # commitment
    assert not V(proof.proofs[0], z, proof, srs)
    # one verifier point
    z2 = z.copy()
    z2[i] = zk.Fr.from_int(zk.Fr.to_ints(z[i])[0] + 1)
    assert not V(commit, z2, proof, srs)
    # a G2 half from another tau
    other = zk.TrustedSetup.setup(zk.Fr.random(nv, 999), g2=True)
    assert not V(commit, z, proof, other)


def test_constant_polynomial_and_tau_equal_to_z(zk):
    nv = 4
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints([3, 5, 7, 11]), g2=True)
    poly = zk.Multilinear(zk.Fr.from_ints([42] * 16))
    commit = zk.MultilinearKZG.commitment(poly, srs)
    proof = zk.MultilinearKZG.open(poly, zk.Fr.from_ints([1, 2, 3, 4]), srs)
    assert all(p.infinity for p in proof.proofs)
    assert zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([1, 2, 3, 4]), proof, srs)
    # tau_i = z_i
    tau = [6, 0, 8, 9]
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints(tau), g2=True)
    poly = zk.Multilinear(zk.Fr.random(1 << nv, 4))
    commit = zk.MultilinearKZG.commitment(poly, srs)
    proof = zk.MultilinearKZG.open(poly, zk.Fr.from_ints(tau), srs)
    assert zk.MultilinearKZG.verify(commit, zk.Fr.from_ints(tau), proof, srs)


def test_shape_and_invalid_points(zk):
    srs, commit, proof = _ml(zk, [0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    with pytest.raises(AssertionError):
        zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([5, 9]), proof, srs)
    with pytest.raises(AssertionError):
        zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([5, 9, 6]), zk.MultilinearKZGProof(proof.evaluation, proof.proofs[:2]), srs)
    off = zk.G1Affine(np.array(list(commit.xy[:6]) + [1, 0, 0, 0, 0, 0], dtype=np.uint64), False)
    with pytest.raises(ValueError):
        zk.MultilinearKZG.verify(off, zk.Fr.from_ints([5, 9, 6]), proof, srs)
    with pytest.raises(ValueError):
        zk.MultilinearKZG.verify(commit, zk.Fr.from_ints([5, 9, 6]), zk.MultilinearKZGProof(proof.evaluation, [off] + proof.proofs[1:]), srs)


def test_multilinear_batch_matches_single_calls(zk):
    nv, B = 6, 256
    srs = zk.TrustedSetup.setup(zk.Fr.random(nv, 1), g2=True)
    base = []
    for k in range(4):
        poly = zk.Multilinear(zk.Fr.random(1 << nv, 10 + k))
        z = zk.Fr.random(nv, 20 + k)
        base.append((zk.MultilinearKZG.commitment(poly, srs), z, zk.MultilinearKZG.open(poly, z, srs)))
    rng = np.random.default_rng(3)
    commits, points, proofs = [], [], []
    for b in range(B):
        c, z, p = base[b % 4]
        kind = int(rng.integers(4))
        if kind == 1:
            p = zk.MultilinearKZGProof(zk.Fr.from_int(zk.Fr.to_ints(p.evaluation)[0] + b), p.proofs)
        elif kind == 2:
            c = base[(b + 1) % 4][0]
        elif kind == 3:
            z = base[(b + 2) % 4][1]
        commits.append(c), points.append(z), proofs.append(p)
    got = zk.MultilinearKZG.verify_batch(commits, points, proofs, srs)
    singles = np.array([zk.MultilinearKZG.verify(c, z, p, srs) for c, z, p in zip(commits, points, proofs)])
    assert got.dtype == bool and got.shape == (B,)
    assert np.array_equal(got, singles)
    assert 0 < got.sum() < B


def test_univariate_round_trip_tampers_and_batch(zk):
    tau = zk.Fr.random(1, 77)[0]
    srs = zk.UnivariateKZG.generate_srs(tau, 15, g2=True)
    other = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(5), 15, g2=True)
    V = zk.UnivariateKZG.verify
    items = []
    for k in range(4):
        poly = zk.DenseUnivariatePolynomial(zk.Fr.random(16, 50 + k))
        z = zk.Fr.random(1, 60 + k)[0]
        c = zk.UnivariateKZG.commitment(poly, srs)
        p = zk.UnivariateKZG.open(poly, z, srs)
        assert V(c, z, p, srs)
        assert not V(c, z, zk.UnivariateKZGProof(zk.Fr.from_int(zk.Fr.to_ints(p.evaluation)[0] + 1), p.proof), srs)
        assert not V(c, z, zk.UnivariateKZGProof(p.evaluation, c), srs)
        assert not V(p.proof, z, p, srs)
        assert not V(c, zk.Fr.from_int(zk.Fr.to_ints(z)[0] + 1), p, srs)
        assert not V(c, z, p, other)
        items.append((c, z, p))
    # constant polynomial: the quotient is zero (proof at infinity)
    poly = zk.DenseUnivariatePolynomial(zk.Fr.from_ints([9]))
    c = zk.UnivariateKZG.commitment(poly, srs)
    p = zk.UnivariateKZG.open(poly, zk.Fr.from_int(3), srs)
    assert V(c, zk.Fr.from_int(3), p, srs)
    # z = tau
    poly = zk.DenseUnivariatePolynomial(zk.Fr.random(8, 5))
    c = zk.UnivariateKZG.commitment(poly, srs)
    p = zk.UnivariateKZG.open(poly, tau, srs)
    assert V(c, tau, p, srs)
    # batch of 256 mixed
    rng = np.random.default_rng(9)
    cs, zs, ps = [], [], []
    for b in range(256):
        c, z, p = items[b % 4]
        kind = int(rng.integers(3))
        if kind == 1:
            z = items[(b + 1) % 4][1]
        elif kind == 2:
            p = items[(b + 1) % 4][2]
        cs.append(c), zs.append(z), ps.append(p)
    got = zk.UnivariateKZG.verify_batch(cs, zs, ps, srs)
    singles = np.array([V(c, z, p, srs) for c, z, p in zip(cs, zs, ps)])
    assert np.array_equal(got, singles)
    assert 0 < got.sum() < 256
    # an SRS with a G2 half of one point has no powers_of_tau_in_g2[1]
    short = zk.UnivariateKZG.generate_srs(tau, 0, g2=True)
    with pytest.raises(IndexError):
        V(c, tau, p, short)


# ---- the verifiers at edge inputs: points of small order, colliding terms, limb vectors that are not field elements --------------------
def _fq_limbs(v):
    m = v * (1 << 384) % PM.P
    return [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def _g1(zk, pt):
    if pt is None:
        return zk.G1Affine(np.zeros(12, dtype=np.uint64), True)
    return zk.G1Affine(np.array(_fq_limbs(pt[0]) + _fq_limbs(pt[1]), dtype=np.uint64), False)


def _plus(limbs, modulus):
    """the same residue under a second encoding: the limb integer plus the modulus"""
    n = len(limbs)
    v = sum(int(w) << (64 * k) for k, w in enumerate(limbs)) + modulus
    assert v < 1 << (64 * n)
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(n)], dtype=np.uint64)


def _g1_plus_p(zk, point, coord):
    xy = point.xy.copy()
    xy[6 * coord: 6 * coord + 6] = _plus(xy[6 * coord: 6 * coord + 6], PM.P)
    return zk.G1Affine(xy, point.infinity)


def _srs_with_g2(zk, srs, index, words):
    """the SRS with G2 point `index` replaced by the 24 limbs `words`"""
    xy = srs.powers_of_tau_in_g2.cpu().numpy().view(np.uint64).copy()
    xy[index] = words
    return zk.TrustedSetup(srs.powers_of_tau_in_g1, srs.inf, xy, srs.g2_inf.cpu().numpy())


def _g2_limbs(q):
    (x0, x1), (y0, y1) = q
    return np.array(_fq_limbs(x0) + _fq_limbs(x1) + _fq_limbs(y0) + _fq_limbs(y1), dtype=np.uint64)


R_LIMBS = np.array([(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)      # the limbs of r itself


@pytest.fixture(scope="module")
def opening3(zk):
    """a valid opening with three variables"""
    srs, commit, proof = _ml(zk, [0, 7, 0, 5, 0, 7, 4, 9], [2, 3, 4], [5, 9, 6])
    z = zk.Fr.from_ints([5, 9, 6])
    assert zk.MultilinearKZG.verify(commit, z, proof, srs) is True
    return srs, commit, z, proof


def test_small_order_points_are_refused_by_the_verifiers(zk, opening3):
    srs, commit, z, proof = opening3
    V = zk.MultilinearKZG.verify
    for pt in PC.g1_small_order_points().values():
        bad = _g1(zk, pt)
        with pytest.raises(ValueError):
            V(bad, z, proof, srs)
        for i in range(3):
            with pytest.raises(ValueError):
                V(commit, z, zk.MultilinearKZGProof(proof.evaluation, proof.proofs[:i] + [bad] + proof.proofs[i + 1:]), srs)
    for q in PC.g2_small_order_points().values():
        with pytest.raises(ValueError):
            V(commit, z, proof, _srs_with_g2(zk, srs, 1, _g2_limbs(q)))
    assert V(commit, z, proof, srs) is True
    usrs, ucommit, uproof = _uv(zk, 2)
    U = zk.UnivariateKZG.verify
    for pt in PC.g1_small_order_points().values():
        with pytest.raises(ValueError):
            U(_g1(zk, pt), zk.Fr.from_int(2), uproof, usrs)
        with pytest.raises(ValueError):
            U(ucommit, zk.Fr.from_int(2), zk.UnivariateKZGProof(uproof.evaluation, _g1(zk, pt)), usrs)
    for q in PC.g2_small_order_points().values():
        with pytest.raises(ValueError):
            U(ucommit, zk.Fr.from_int(2), uproof, _srs_with_g2(zk, usrs, 1, _g2_limbs(q)))
    assert U(ucommit, zk.Fr.from_int(2), uproof, usrs) is True


def _raw_verify_batch(zk, commits, points, proofs, srs, prepared):
    """zkhip_kzg_verify_batch itself -> (status, h_ok): the mirror class raises on an error and drops the verdicts"""
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd.polynomial import _fr_host
    b, nv = len(commits), len(proofs[0].proofs)
    cxy = np.stack([c.xy for c in commits])
    cinf = np.array([1 if c.infinity else 0 for c in commits], dtype=np.uint8)
    flat = [q for p in proofs for q in p.proofs]
    pxy = np.stack([q.xy for q in flat])
    pinf = np.array([1 if q.infinity else 0 for q in flat], dtype=np.uint8)
    ev = np.stack([np.asarray(p.evaluation, dtype=np.uint64).reshape(4) for p in proofs])
    z = np.concatenate([np.asarray(_fr_host(v), dtype=np.uint64).reshape(nv, 4) for v in points])
    ok = np.full(b, 0x5A, dtype=np.uint8)
    prep = srs.prepared_lines(False) if prepared else None
    ctx = N.Context.get(srs.powers_of_tau_in_g2.device.index)
    vp = C.c_void_p
    st = N.lib().zkhip_kzg_verify_batch(ctx.handle, C.c_size_t(b), C.c_uint32(nv), cxy.ctypes.data_as(vp), cinf.ctypes.data_as(vp),
                                        ev.ctypes.data_as(vp), z.ctypes.data_as(vp), pxy.ctypes.data_as(vp), pinf.ctypes.data_as(vp),
                                        N.ptr(srs.powers_of_tau_in_g2), N.ptr(srs.g2_inf), C.c_size_t(nv), N.ptr(prep) if prepared else None,
                                        ok.ctypes.data_as(vp))
    return st, [int(v) for v in ok]


def test_one_bad_element_in_a_batch_of_four(zk, opening3):
    """include/zkhip.h: ZKHIP_ERR_ARG, h_ok = 0 for the opening that holds the refused input, and every other opening's verdict as a
    call without it returns it"""
    from zk_cryptography_amd import _native as N
    srs, commit, z, proof = opening3
    wrong = zk.MultilinearKZGProof(zk.Fr.from_int(zk.Fr.to_ints(proof.evaluation)[0] + 1), proof.proofs)     # valid input, verdict 0
    order11 = _g1(zk, PC.g1_order_11())
    unreduced_eval = zk.MultilinearKZGProof(R_LIMBS.copy(), proof.proofs)
    bads = [(order11, proof), (commit, zk.MultilinearKZGProof(proof.evaluation, [proof.proofs[0], order11, proof.proofs[2]])),
            (_g1_plus_p(zk, commit, 0), proof), (commit, unreduced_eval)]
    for prepared in (True, False):
        st, ok = _raw_verify_batch(zk, [commit] * 4, [z] * 4, [proof, wrong, proof, wrong], srs, prepared)
        assert st == N.ZKHIP_OK and ok == [1, 0, 1, 0]
        for slot, (c, p) in enumerate(bads):
            commits, proofs = [commit] * 4, [proof, wrong, proof, wrong]
            commits[slot], proofs[slot] = c, p
            st, ok = _raw_verify_batch(zk, commits, [z] * 4, proofs, srs, prepared)
            assert st == N.ERR_ARG, (prepared, slot)
            assert ok == [0 if k == slot else v for k, v in enumerate([1, 0, 1, 0])], (prepared, slot)
            with pytest.raises(ValueError):
                zk.MultilinearKZG.verify_batch(commits, [z] * 4, proofs, srs)
    # a refused SRS point, prepared inside the call: no verdict stands
    stray = _srs_with_g2(zk, srs, 2, _g2_limbs(PC.g2_small_order(23)))
    st, ok = _raw_verify_batch(zk, [commit] * 4, [z] * 4, [proof] * 4, stray, False)
    assert st == N.ERR_ARG and ok == [0, 0, 0, 0]


def test_commitment_that_collides_with_the_evaluation_term(zk, opening3):
    """C = -v G1: the term C - v G1 adds -v G1 to itself, g1_madd's doubling branch.  The verdict is the model's, on the same data."""
    srs, commit, z, proof = opening3
    v = zk.Fr.to_ints(proof.evaluation)[0]
    assert v not in (0, 1)
    proofs = [None if q.infinity else q.coords() for q in proof.proofs]
    srs_g2 = PM.multilinear_srs_g2([2, 3, 4])
    wants = []
    for c in (M.g1_mul(M.G1, (-v) % R), M.g1_mul(M.G1, v), commit.coords()):       # doubling; inverse (the term is the identity); the true one
        wants.append(PM.multilinear_verify(c, [5, 9, 6], v, proofs, srs_g2))
        assert zk.MultilinearKZG.verify(_g1(zk, c), z, proof, srs) is wants[-1]
    assert wants == [False, False, True]


def test_unreduced_encodings_are_refused(zk, opening3):
    """c + p is the same residue and would satisfy the curve equation; v + r would multiply to the same point.  Each has one accepted
    encoding: ValueError (ZKHIP_ERR_ARG), as the PLONK verifier refuses them."""
    srs, commit, z, proof = opening3
    V = zk.MultilinearKZG.verify
    with pytest.raises(ValueError):
        V(_g1_plus_p(zk, commit, 0), z, proof, srs)                                             # the commitment's x
    with pytest.raises(ValueError):
        V(commit, z, zk.MultilinearKZGProof(proof.evaluation, [proof.proofs[0], _g1_plus_p(zk, proof.proofs[1], 1)] + proof.proofs[2:]), srs)
    g2 = srs.powers_of_tau_in_g2.cpu().numpy().view(np.uint64)[1].copy()
    g2[6:12] = _plus(g2[6:12], PM.P)                                                            # an SRS point's x.c1
    with pytest.raises(ValueError):
        V(commit, z, proof, _srs_with_g2(zk, srs, 1, g2))
    ev = np.asarray(proof.evaluation, dtype=np.uint64).reshape(4)
    for limbs in (_plus(ev, R), R_LIMBS.copy()):                                                # v + r, and r itself
        with pytest.raises(ValueError):
            V(commit, z, zk.MultilinearKZGProof(limbs, proof.proofs), srs)
    for limbs in (_plus(np.asarray(z[1], dtype=np.uint64).reshape(4), R), R_LIMBS.copy()):
        z2 = z.copy()
        z2[1] = limbs
        with pytest.raises(ValueError):
            V(commit, z2, proof, srs)
    assert V(commit, z, proof, srs) is True
    usrs, ucommit, uproof = _uv(zk, 2)
    U = zk.UnivariateKZG.verify
    two = zk.Fr.from_int(2)
    with pytest.raises(ValueError):
        U(_g1_plus_p(zk, ucommit, 1), two, uproof, usrs)
    with pytest.raises(ValueError):
        U(ucommit, two, zk.UnivariateKZGProof(uproof.evaluation, _g1_plus_p(zk, uproof.proof, 0)), usrs)
    with pytest.raises(ValueError):
        U(ucommit, two, zk.UnivariateKZGProof(_plus(np.asarray(uproof.evaluation, dtype=np.uint64).reshape(4), R), uproof.proof), usrs)
    with pytest.raises(ValueError):
        U(ucommit, _plus(np.asarray(two, dtype=np.uint64).reshape(4), R), uproof, usrs)
    assert U(ucommit, two, uproof, usrs) is True


def test_coordinates_of_a_point_at_infinity_are_not_read(zk):
    """a constant polynomial's proofs are all the identity: whatever their coordinate words hold, unreduced limbs included"""
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints([3, 5, 7]), g2=True)
    poly = zk.Multilinear(zk.Fr.from_ints([42] * 8))
    commit = zk.MultilinearKZG.commitment(poly, srs)
    z = zk.Fr.from_ints([1, 2, 3])
    proof = zk.MultilinearKZG.open(poly, z, srs)
    assert all(p.infinity for p in proof.proofs)
    full = np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    junk = zk.MultilinearKZGProof(proof.evaluation, [zk.G1Affine(full, True) for _ in proof.proofs])
    assert zk.MultilinearKZG.verify(commit, z, junk, srs) is True
    g2 = np.full(24, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    at_inf = zk.TrustedSetup.setup(zk.Fr.from_ints([3, 0, 7]), g2=True)                      # tau_1 = 0: that G2 point is the identity
    assert at_inf.g2_points()[1].infinity
    poly = zk.Multilinear(zk.Fr.random(8, 4))
    commit = zk.MultilinearKZG.commitment(poly, at_inf)
    proof = zk.MultilinearKZG.open(poly, z, at_inf)
    want = zk.MultilinearKZG.verify(commit, z, proof, at_inf)
    assert zk.MultilinearKZG.verify(commit, z, proof, _srs_with_g2(zk, at_inf, 1, g2)) is want
