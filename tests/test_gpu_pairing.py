"""GPU parity: the BLS12-381 pairing, the G2 SRS and the prepared lines (csrc/pairing.hip) against the independent python model
tests/pairing_model.py, bit for bit on the GT encoding (f^((p^12 - 1) / r) exactly)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_cases as PC  # noqa: E402
import pairing_model as PM  # noqa: E402
from pairing_cases import g1_not_in_subgroup as _g1_not_in_subgroup  # noqa: E402
from pairing_cases import off_twist as _off_twist  # noqa: E402
from pairing_cases import twist_not_in_subgroup as _twist_not_in_subgroup  # noqa: E402

pytestmark = pytest.mark.gpu

M = PM.M
RMONT = 1 << 384


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _limbs(v):
    m = v * RMONT % PM.P
    return [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def g1(zk, pt):
    if pt is None:
        return zk.G1Affine(np.zeros(12, dtype=np.uint64), True)
    return zk.G1Affine(np.array(_limbs(pt[0]) + _limbs(pt[1]), dtype=np.uint64), False)


def g2(zk, q):
    if q is None:
        return zk.G2Affine(np.zeros(24, dtype=np.uint64), True)
    (x0, x1), (y0, y1) = q
    return zk.G2Affine(np.array(_limbs(x0) + _limbs(x1) + _limbs(y0) + _limbs(y1), dtype=np.uint64), False)


def _pairs():
    pts = [(M.g1_mul(M.G1, 3), PM.g2_mul(PM.G2, 5)), (M.G1, PM.G2), (None, PM.G2), (M.G1, None), (None, None),
           (M.g1_mul(M.G1, 0xDEADBEEF12345), PM.g2_mul(PM.G2, 77)), (M.g1_mul(M.G1, PM.R - 1), PM.G2),
           (M.g1_mul(M.G1, 2), PM.g2_mul(PM.G2, PM.R - 9))]
    return pts


def test_pairing_matches_model_bit_for_bit(zk):
    pairs = _pairs()
    got = zk.pairing([g1(zk, p) for p, _ in pairs], [g2(zk, q) for _, q in pairs])
    for k, (p, q) in enumerate(pairs):
        want = PM.f12_to_tower(PM.pairing(p, q))
        assert zk.gt_ints(got[k]) == want, k


def test_pairing_bilinear_on_device(zk):
    rng = np.random.default_rng(5)
    a, b = int(rng.integers(1, 1 << 62)) ** 3 % PM.R, int(rng.integers(1, 1 << 62)) ** 3 % PM.R
    p, q = M.g1_mul(M.G1, 11), PM.g2_mul(PM.G2, 13)
    got = zk.pairing([g1(zk, M.g1_mul(p, a)), g1(zk, M.g1_mul(p, a * b)), g1(zk, p)],
                     [g2(zk, PM.g2_mul(q, b)), g2(zk, q), g2(zk, PM.g2_mul(q, a * b))])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])
    one = zk.gt_ints(zk.pairing([g1(zk, None)], [g2(zk, q)])[0])
    assert one == [1] + [0] * 11
    assert zk.gt_ints(got[0]) != one


def test_prepared_path_equals_unprepared(zk):
    from zk_cryptography_amd import kzg as K
    pairs = _pairs()
    g1s, g2s = [g1(zk, p) for p, _ in pairs], [g2(zk, q) for _, q in pairs]
    prep = K.g2_prepare(g2s)
    assert np.array_equal(zk.pairing(g1s, prepared=prep), zk.pairing(g1s, g2s))


def test_g2_srs_matches_model(zk):
    tau = [5, 9, 6, PM.R - 2]
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints(tau), g2=True)
    want = PM.multilinear_srs_g2(tau)
    got = srs.g2_points()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert not g.infinity and g.coords() == w
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(10), 4, g2=True)
    want = PM.univariate_srs_g2(10, 4)
    assert [g.coords() for g in srs.g2_points()] == want
    # tau_i = 0 gives the point at infinity
    assert zk.TrustedSetup.setup(zk.Fr.from_ints([0, 3]), g2=True).g2_points()[0].infinity
    # the default setup does no G2 work
    assert zk.TrustedSetup.setup(zk.Fr.from_ints(tau)).powers_of_tau_in_g2 is None


def test_invalid_inputs_are_refused(zk):
    from zk_cryptography_amd import kzg as K
    bad2 = [g2(zk, _off_twist()), g2(zk, _twist_not_in_subgroup())]
    for q in bad2:
        with pytest.raises(ValueError):
            zk.pairing([g1(zk, M.G1)], [q])
        with pytest.raises(ValueError):
            K.g2_prepare([q])
    bad1 = [g1(zk, (1, 1)), g1(zk, _g1_not_in_subgroup())]
    for p in bad1:
        with pytest.raises(ValueError):
            zk.pairing([p], [g2(zk, PM.G2)])
    with pytest.raises(AssertionError):
        zk.pairing([g1(zk, M.G1)] * 2, [g2(zk, PM.G2)])


def _plus_p(limbs):
    """the same residue under a second encoding: the limb integer plus p (p < 2^381, so it still fits six words)"""
    v = sum(int(w) << (64 * k) for k, w in enumerate(limbs)) + PM.P
    assert v < 1 << 384
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def _unreduced(zk, point, coord):
    """`point` (zk.G1Affine / zk.G2Affine) with coordinate number `coord` stored as c + p"""
    xy = point.xy.copy()
    xy[6 * coord: 6 * coord + 6] = _plus_p(xy[6 * coord: 6 * coord + 6])
    return type(point)(xy, point.infinity)


def test_small_order_points_are_refused(zk):
    """points of order 3 and 11 on E(Fq), 13 and 23 on the twist: on the curve, and what walks the subgroup check through the doubling
    and inverse branches of the mixed additions (tests/test_pairing_cases_cpu.py)"""
    from zk_cryptography_amd import kzg as K
    for pt in PC.g1_small_order_points().values():
        with pytest.raises(ValueError):
            zk.pairing([g1(zk, pt)], [g2(zk, PM.G2)])
        with pytest.raises(ValueError):                       # in a batch, whatever its place
            zk.pairing([g1(zk, M.G1), g1(zk, pt), g1(zk, None)], [g2(zk, PM.G2)] * 3)
    for q in PC.g2_small_order_points().values():
        with pytest.raises(ValueError):
            zk.pairing([g1(zk, M.G1)], [g2(zk, q)])
        with pytest.raises(ValueError):
            K.g2_prepare([g2(zk, PM.G2), g2(zk, q)])


def test_unreduced_coordinates_are_refused(zk):
    """x + p is the same residue as x and would pass the curve equation: refused, so that every point has one accepted encoding"""
    from zk_cryptography_amd import kzg as K
    p, q = g1(zk, M.g1_mul(M.G1, 3)), g2(zk, PM.g2_mul(PM.G2, 5))
    want = zk.pairing([p], [q])
    for coord in range(2):
        with pytest.raises(ValueError):
            zk.pairing([_unreduced(zk, p, coord)], [q])
        with pytest.raises(ValueError):
            zk.pairing([_unreduced(zk, p, coord)], prepared=K.g2_prepare([q]))
    for coord in range(4):
        with pytest.raises(ValueError):
            zk.pairing([p], [_unreduced(zk, q, coord)])
        with pytest.raises(ValueError):
            K.g2_prepare([_unreduced(zk, q, coord)])
    full = np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)       # 2^384 - 1: far outside what the field product is stated for
    with pytest.raises(ValueError):
        zk.pairing([zk.G1Affine(full, False)], [q])
    # the coordinates of a point flagged at infinity are ignored: still the neutral element, still no error
    one = [1] + [0] * 11
    assert zk.gt_ints(zk.pairing([zk.G1Affine(full, True)], [q])[0]) == one
    assert zk.gt_ints(zk.pairing([p], [zk.G2Affine(np.concatenate([full, full]), True)])[0]) == one
    K.g2_prepare([zk.G2Affine(np.concatenate([full, full]), True)])
    assert np.array_equal(zk.pairing([p], [q]), want)
