"""GPU: the kernels of csrc/plonk_verify_kernels.hpp alone, through tests/plonk_verify_driver.py (nothing of libzkhip linked).

The PI pass against python integers: PI(zeta) of an evaluation-form column is the barycentric sum, and the column's own entry where
zeta is a root of unity -- which is what `to_coefficient_poly(..).evaluate` gives (checked here at n = 4 and 64, where the model's
quadratic route is cheap).  Sizes: n = 4 is shorter than one lane's run of eight rows, 1024 fills one workgroup, 2048 needs two, 4096
four.  The roots of unity taken for zeta sit at the edges of a lane's run (rows 7 and 8), of the column (0, 1, n - 1).

The term and combine kernels against the model's group law: the twenty terms of a proof with scalars 0, 1, r - 1 and random ones, a
point at infinity among them, and a proof whose terms cancel to the identity."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402
import plonk_verify_driver as D  # noqa: E402
from test_gpu_plonk import from_affine, point_outside_the_subgroup, to_affine  # noqa: E402

pytestmark = pytest.mark.gpu
M, R = PL.M, PL.R
P = M.P
TERMS = 20
RUN = 8                                     # consecutive rows of one lane of the PI pass
VP = C.c_void_p


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


@pytest.fixture(scope="module")
def drv():
    lib = D.lib()
    assert lib.plonk_verify_driver_terms() == TERMS and lib.plonk_verify_driver_pi_rows() == 1024 and lib.plonk_verify_driver_pi_run() == RUN
    return lib


def dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def pi_reference(column, w, zeta):
    """PI(zeta) in python integers"""
    n = len(column)
    if pow(zeta, n, R) == 1:
        return column[w.index(zeta)]
    s = sum(c * wi % R * pow((zeta - wi) % R, -1, R) for c, wi in zip(column, w) if c) % R
    return (pow(zeta, n, R) - 1) * pow(n, -1, R) % R * s % R


def test_the_reference_formula_is_the_coefficient_form_evaluated():
    rng = random.Random(3)
    for n in (4, 8, 64):
        w = PL.roots_of_unity(n)
        column = [rng.randrange(R) for _ in range(n)]
        poly = PL.to_coefficient_poly(column, n)
        for zeta in (rng.randrange(R), 0, w[0], w[1], w[n - 1]):
            assert pi_reference(column, w, zeta) == poly.evaluate(zeta)


@pytest.mark.parametrize("n", [4, 1024, 2048, 4096])
def test_pi_pass_against_python_integers(zk, drv, n):
    import torch
    rng = random.Random(n)
    w = PL.roots_of_unity(n)
    omega = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    assert drv.plonk_verify_driver_powers(zk.Fr.from_ints([w[1]]).ctypes.data_as(VP), zk.Fr.from_ints([1]).ctypes.data_as(VP), n, omega.data_ptr(), None) == 0
    assert zk.Fr.to_ints(host(omega, np.uint64)) == w
    columns = [[0] * n, [R - 1] * n, [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]]
    d_columns = [dev(zk.Fr.from_ints(c)) for c in columns]
    roots = [i for i in (0, 1, RUN - 1, RUN, n - 1) if i < n]
    zetas = [rng.randrange(R), 0] + [w[i] for i in roots] + [rng.randrange(R)]
    n_blocks = (n + 1023) // 1024
    cases = [([z], [k]) for z in zetas for k in range(4)]                        # B = 1: every zeta with every column
    cases += [(zetas[i:i + 3], [(i + j) % 4 for j in range(3)]) for i in range(len(zetas) - 2)]      # B = 3: different zetas and columns
    cases.append(([zetas[2], zetas[2], zetas[0]], [2, 3, 2]))                   # two proofs at one root of unity
    for zs, ks in cases:
        B = len(zs)
        ptrs = dev(np.array([d_columns[k].data_ptr() for k in ks], dtype=np.uint64))
        factors = [(pow(z, n, R) - 1) * pow(n, -1, R) % R for z in zs]
        d_z, d_f = dev(zk.Fr.from_ints(zs)), dev(zk.Fr.from_ints(factors))
        partial = torch.full((B * n_blocks, 4), -1, dtype=torch.int64, device="cuda")
        hit = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        out = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        st = drv.plonk_verify_driver_pi(ptrs.data_ptr(), omega.data_ptr(), d_z.data_ptr(), d_f.data_ptr(), n, B, partial.data_ptr(), hit.data_ptr(),
                                        out.data_ptr(), None)
        assert st == 0
        got = zk.Fr.to_ints(host(out, np.uint64))
        assert got == [pi_reference(columns[k], w, z) for z, k in zip(zs, ks)], (zs, ks)


def run_terms(zk, drv, vk, proofs_points, scalars):
    """vk: 8 model points; proofs_points: B lists of 9 model points; scalars: B lists of 20 ints -> (right, left) per proof, -left check, bad"""
    import torch
    B = len(proofs_points)

    def arrays(points):
        objs = [to_affine(zk, p) for p in points]
        return np.stack([o.xy for o in objs]), np.array([1 if o.infinity else 0 for o in objs], dtype=np.uint8)
    vxy, vinf = arrays(vk)
    pxy, pinf = arrays([p for pts in proofs_points for p in pts])
    sc = zk.Fr.from_ints([s for row in scalars for s in row])
    d = [dev(a) for a in (vxy, vinf, pxy, pinf, sc)]
    terms = torch.zeros((B * TERMS, 24), dtype=torch.int64, device="cuda")
    bad = torch.full((B * TERMS,), 9, dtype=torch.uint8, device="cuda")
    pair_xy, out_xy = (torch.zeros((B, 2, 12), dtype=torch.int64, device="cuda") for _ in range(2))
    pair_inf, out_inf = (torch.full((B, 2), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
    st = drv.plonk_verify_driver_terms_combine(*[t.data_ptr() for t in d], B, terms.data_ptr(), bad.data_ptr(), pair_xy.data_ptr(), pair_inf.data_ptr(),
                                               out_xy.data_ptr(), out_inf.data_ptr(), None)
    assert st == 0
    oxy, oinf, qxy, qinf = host(out_xy, np.uint64), host(out_inf, np.uint8), host(pair_xy, np.uint64), host(pair_inf, np.uint8)
    res = []
    for b in range(B):
        right, left = (None if oinf[b, k] else from_affine(zk.G1Affine(oxy[b, k], 0)) for k in range(2))
        for k in range(2):
            if oinf[b, k]:
                assert not oxy[b, k].any() and not qxy[b, k].any()              # infinity flag set, coordinates zero
        assert list(qinf[b]) == list(oinf[b])
        assert (None if qinf[b, 0] else from_affine(zk.G1Affine(qxy[b, 0], 0))) == right       # `right` goes to the pairing as it is,
        neg_left = None if left is None else (left[0], (P - left[1]) % P)                      # `left` negated
        assert (None if qinf[b, 1] else from_affine(zk.G1Affine(qxy[b, 1], 0))) == neg_left
        res.append((right, left))
    return res, host(bad, np.uint8).reshape(B, TERMS)


# term j -> its point: vk 0..7, then the proof's points as, bs, cs, acc, tl, tm, th, wz, wzw, then G, then wz, wzw again
def term_point(vk, pts, j):
    return vk[j] if j < 8 else M.G1 if j == 17 else pts[j - 8] if j < 17 else pts[j - 11]


def model_sums(vk, pts, scalars):
    sc = list(scalars)
    sc[4] = sc[18] = 1                                                          # q_c and the left W_zeta: added as they are
    right = left = None
    for j in range(TERMS):
        t = PL.g1_mul(term_point(vk, pts, j), sc[j])
        if j < 18:
            right = M.g1_add(right, t)
        else:
            left = M.g1_add(left, t)
    return right, left


@pytest.mark.parametrize("B", [1, 5])
def test_terms_and_combine_against_the_group_law(zk, drv, B):
    rng = random.Random(40 + B)
    pt = lambda: PL.g1_mul(M.G1, rng.randrange(1, R))
    vk = [pt() for _ in range(8)]
    vk[6] = None                                                                # a key commitment at infinity (a zero column)
    proofs, scalars = [], []
    for b in range(B):
        pts = [pt() for _ in range(9)]
        sc = [rng.randrange(R) for _ in range(TERMS)]
        if b == 0:
            sc[0], sc[1], sc[2], sc[8], sc[17], sc[19] = 0, 1, R - 1, R - 1, 0, 1     # the scalars at their edges
            pts[5] = None                                                        # a proof point at infinity among the terms
        if b == B - 1 and B > 1:
            # terms that cancel: right = s (A - A) and left = W - W with every other scalar zero
            sc = [0] * TERMS
            pts[1] = pts[0]
            sc[8], sc[9] = 5, R - 5
            pts[7] = None                                                        # left: W_zeta at infinity, mu = 0
        proofs.append(pts)
        scalars.append(sc)
    if B > 1:
        # the q_c term is always added once: give the cancelling proof -q_c through the generator's scalar
        k = rng.randrange(1, R)
        vk[4] = PL.g1_mul(M.G1, k)
        scalars[B - 1][17] = (R - k) % R
    got, bad = run_terms(zk, drv, vk, proofs, scalars)
    assert not bad.any()
    for b in range(B):
        assert got[b] == model_sums(vk, proofs[b], scalars[b]), b
    if B > 1:
        assert got[B - 1] == (None, None)


def test_terms_flag_invalid_points_and_combine_gives_identities(zk, drv):
    rng = random.Random(7)
    pt = lambda: PL.g1_mul(M.G1, rng.randrange(1, R))
    vk = [pt() for _ in range(8)]
    good = [pt() for _ in range(9)]
    x, y = good[2]
    off_curve = list(good)
    off_curve[2] = (x, (y + 1) % P)
    stray = list(good)
    stray[8] = point_outside_the_subgroup()
    sc = [[rng.randrange(R) for _ in range(TERMS)] for _ in range(3)]
    got, bad = run_terms(zk, drv, vk, [off_curve, good, stray], sc)
    want = np.zeros((3, TERMS), dtype=np.uint8)
    want[0, 10] = 1                                                             # cs: term 10
    want[2, 16] = want[2, 19] = 1                                               # w_zeta_omega: terms 16 and 19
    assert np.array_equal(bad, want)
    assert got[0] == (None, None) and got[2] == (None, None)
    assert got[1] == model_sums(vk, good, sc[1])
