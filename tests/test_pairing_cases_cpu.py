"""CPU: the edge inputs of tests/pairing_cases.py are what the GPU tests take them for.  A point named "of order 13" that was the
identity, or a "cyclotomic" element that was not, would let test_gpu_pairing_kernels.py pass without reaching the branch it is there for."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_cases as PC  # noqa: E402

PM, M = PC.PM, PC.M


@pytest.mark.parametrize("order", [3, 11])
def test_g1_small_order_points(order):
    pt = PC.g1_small_order_points()[order]
    assert pt is not None and PC.g1_on_curve(pt)
    assert PC.g1_mul_raw(pt, order) is None                         # killed by its order, and the order is prime: exactly that order
    assert PC.g1_mul_raw(pt, 1) == pt
    assert PC.g1_mul_raw(pt, PC.R) is not None                      # so not in the subgroup of order r


@pytest.mark.parametrize("order", [13, 23])
def test_g2_small_order_points(order):
    pt = PC.g2_small_order_points()[order]
    assert pt is not None and PM.g2_on_curve(pt)
    assert PM.g2_mul_raw(pt, order) is None
    assert PM.g2_mul_raw(pt, 1) == pt
    assert PM.g2_mul_raw(pt, PC.R) is not None


def test_single_cofactor_division_is_not_enough():
    """why the constructions divide by 11^2 and q^2: the Sylow subgroups are not cyclic, a single division gives the identity"""
    assert PC.g1_mul_raw(PC.g1_not_in_subgroup(), PC.H1 * PC.R // 11) is None
    assert PM.g2_mul_raw(PC.twist_not_in_subgroup(), PC.H2 * PC.R // 13) is None


@pytest.mark.parametrize("order", [3, 11, 13, 23])
def test_walking_r_over_a_small_order_point_meets_both_branches(order):
    """the double-and-add of g1_in_subgroup / g2_in_subgroup reaches acc == q (doubling) and acc == -q (inverse) on these points"""
    if order in (3, 11):
        pt = PC.g1_small_order_points()[order]
        same, inverse, end = PC.walk_r_g1(pt)
        assert end == PC.g1_mul_raw(pt, PC.R % order)
    else:
        pt = PC.g2_small_order_points()[order]
        same, inverse, end = PC.walk_r_g2(pt)
        assert end == PM.g2_mul_raw(pt, PC.R % order)
    assert same > 0 and inverse > 0, (order, same, inverse)
    assert end is not None


def test_large_order_points_never_collide():
    """the two points the suite used before are outside the subgroup too, but walk r without a single collision"""
    assert PC.walk_r_g1(PC.g1_not_in_subgroup())[:2] == (0, 0)
    assert PC.walk_r_g2(PC.twist_not_in_subgroup())[:2] == (0, 0)


def test_cyclotomic_inputs_and_the_negative_control():
    one = PM.f12_one()
    elems = PC.cyclotomic_elements()
    assert elems[0] == one and len(elems) == 6
    assert len({tuple(e) for e in elems}) == 6
    for e in elems:
        assert PM.f12_pow(e, PC.CYCLOTOMIC_ORDER) == one
        assert PM.f12_mul(e, PC.f12_conj(e)) == one                  # unitary: the inverse is the conjugate, what f12_exp_by_x relies on
    assert PM.f12_pow(PC.not_cyclotomic(), PC.CYCLOTOMIC_ORDER) != one


def test_tower_order_round_trip():
    import numpy as np
    a = PC.f12_random(np.random.default_rng(1))
    assert PC.f12_from_tower(PM.f12_to_tower(a)) == a
    assert PM.f12_pow(a, PC.P ** 6) == PC.f12_conj(a)
