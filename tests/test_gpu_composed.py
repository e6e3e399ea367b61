"""GPU parity: composed and multi-composed sumcheck provers vs the CPU oracle (round polynomials, challenges,
proof bytes bit-exact).  Names follow sumcheck/src/composed/*.rs and composed_multilinear.rs tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def F(zk, v):
    return zk.Fr.from_ints(v)


def test_composed_multilinear_evaluation(zk):   # composed_multilinear.rs:134-155
    polys = zk.ComposedMultilinear([F(zk, [0, 1, 2, 3]), F(zk, [0, 0, 0, 1])])
    assert polys.evaluation(F(zk, [2, 3])) == 42
    assert polys.partial_evaluation(F(zk, [2])[0], 0).evaluation(F(zk, [3])) == 42
    assert polys.n_vars() == 2 and polys.max_degree() == 2


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def test_element_wise_product_and_add(zk):   # composed_multilinear.rs:159-184
    polys = zk.ComposedMultilinear([F(zk, [0, 1, 2, 3]), F(zk, [0, 0, 0, 1])])
    assert zk.Fr.to_ints(_host(polys.element_wise_product())) == [0, 0, 0, 3]
    assert zk.Fr.to_ints(_host(polys.element_wise_add())) == [0, 1, 2, 4]


@pytest.mark.parametrize("k,log_n", [(1, 0), (2, 3), (3, 12), (5, 16), (11, 10)])
def test_element_wise_random_matches_host_arithmetic(zk, ora, k, log_n):
    """Any number of tables (the reference's fold over `polys` has no cap): 11 tables take two launches."""
    n = 1 << log_n
    tabs = [ora.random_fr(n, 6100 + 17 * k + q) for q in range(k)]
    polys = zk.ComposedMultilinear(tabs)
    R = zk.Fr.MODULUS
    ints = [zk.Fr.to_ints(t) for t in tabs]            # python integers: an independent check of the kernels' field arithmetic
    prod, add = list(ints[0]), list(ints[0])
    for t in ints[1:]:
        prod = [a * b % R for a, b in zip(prod, t)]
        add = [(a + b) % R for a, b in zip(add, t)]
    assert zk.Fr.to_ints(_host(polys.element_wise_product())) == prod
    assert zk.Fr.to_ints(_host(polys.element_wise_add())) == add
    # sum_over_boolean_hypercube (sumcheck/src/utils.rs:45-51) = the sum of the product vector
    if k <= 5:
        assert zk.Fr.to_ints(zk.ComposedSumcheck.calculate_poly_sum(polys))[0] == sum(prod) % R


def test_sum_calculation(zk):   # composed_sumcheck.rs:108-140, multi_composed_sumcheck.rs:195-214
    cs = zk.ComposedSumcheck.calculate_poly_sum
    assert zk.Fr.to_ints(cs(zk.ComposedMultilinear([F(zk, [0, 1, 2, 3]), F(zk, [0, 0, 0, 1])]))) == [3]
    assert zk.Fr.to_ints(cs(zk.ComposedMultilinear([F(zk, [3, 3, 5, 5]), F(zk, [0, 0, 0, 1])]))) == [5]
    assert zk.Fr.to_ints(cs(zk.ComposedMultilinear([F(zk, [0, 1, 2, 3])]))) == [6]
    assert zk.Fr.to_ints(cs(zk.ComposedMultilinear([F(zk, [0, 0, 0, 2, 2, 2, 2, 4])]))) == [12]
    ms = zk.MultiComposedSumcheckProver.calculate_poly_sum
    assert zk.Fr.to_ints(ms([zk.ComposedMultilinear([F(zk, [0, 1, 2, 3])]), zk.ComposedMultilinear([F(zk, [0, 0, 0, 1])])])) == [7]
    assert zk.Fr.to_ints(ms([zk.ComposedMultilinear([F(zk, [0, 0, 0, 2])]), zk.ComposedMultilinear([F(zk, [0, 3, 0, 3])])])) == [8]


COMPOSED_CASES = [
    [[3, 3, 5, 5], [0, 0, 0, 1]],
    [[0, 0, 2, 7, 3, 3, 6, 11]],
    [[0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]],
    [[1, 3, 5, 7, 2, 4, 6, 8, 3, 5, 7, 9, 4, 6, 8, 10]],
]


@pytest.mark.parametrize("tables", COMPOSED_CASES)
def test_sum_check_proof(zk, ora, tables):   # composed_sumcheck.rs:143-241
    t = np.stack([F(zk, v) for v in tables])
    proof, ch = zk.ComposedSumcheck(zk.ComposedMultilinear(list(t))).prove()
    rp, och = ora.composed_prove(t)
    assert np.array_equal(proof.round_polys, rp) and np.array_equal(ch, och)
    assert ora.composed_verify(t, ora.composed_sum(t), proof.round_polys)


@pytest.mark.parametrize("k,log_n", [(1, 1), (2, 5), (2, 12), (3, 9), (5, 8), (5, 13), (4, 10),
                                     (2, 20), (3, 18), (2, 21), (2, 22), (5, 20)])   # (2, 20) .. (2, 22): grids above the workgroup cap (grid-stride rounds); (2, 21) / (2, 22): one / two rounds on the unreduced K = 2 sums; (5, 20): the first round's last factor on the matrix cores (composed_dot.hpp), four steps per workgroup
def test_composed_prove_random(zk, ora, k, log_n):   # benches: 2 and 5 tables (composed_sumcheck_benchmark.rs)
    t = np.stack([ora.random_fr(1 << log_n, 900 + 10 * k + q) for q in range(k)])
    poly = zk.ComposedMultilinear(list(t))
    proof, ch = zk.ComposedSumcheck(poly).prove()
    rp, och = ora.composed_prove(t)
    assert np.array_equal(proof.round_polys, rp)
    assert np.array_equal(ch, och)
    assert np.array_equal(zk.ComposedSumcheck.calculate_poly_sum(poly), ora.composed_sum(t))


def _gkr_example(zk, ora):   # multi_composed_sumcheck.rs:266-311
    add_i, mul_i = F(zk, [4, 4, 7, 7, 4, 4, 7, 9]), F(zk, [3, 3, 3, 4, 3, 3, 5, 6])
    w_b, w_c = zk.Multilinear(F(zk, [0, 4])), zk.Multilinear(F(zk, [0, 3]))
    two = F(zk, [2])[0]
    lhs = [zk.Multilinear(add_i).partial_evaluation(two, 0), w_b.add_distinct(w_c)]
    rhs = [zk.Multilinear(mul_i).partial_evaluation(two, 0), w_b.mul_distinct(w_c)]
    return [lhs, rhs]


def _multi_cases(zk, ora):
    p1, p2 = F(zk, [0, 0, 0, 2]), F(zk, [0, 3, 0, 3])
    mk = lambda tabs: [zk.Multilinear(t) for t in tabs]
    return [[mk([p1]), mk([p2])], [mk([p1]), mk([p2]), mk([p2])], [mk([p1, p2]), mk([p2, p1])], _gkr_example(zk, ora)]


def _check_multi(zk, ora, terms, partial):
    poly = [zk.ComposedMultilinear(t) for t in terms]
    flat = np.stack([m.to_numpy() for t in terms for m in t])
    sizes = [len(t) for t in terms]
    s = zk.MultiComposedSumcheckProver.calculate_poly_sum(poly)
    assert np.array_equal(s, ora.multi_composed_sum(flat, sizes))
    fn = zk.MultiComposedSumcheckProver.prove_partial if partial else zk.MultiComposedSumcheckProver.prove
    proof, ch = fn(poly, s)
    orps, och = ora.multi_composed_prove(flat, sizes, s, partial=partial)
    assert [rp.monomials() for rp in proof.round_polys] == [o.monomials() for o in orps]
    assert proof.to_bytes() == ora.multi_composed_proof_bytes(orps)
    assert np.array_equal(ch, och)
    return flat, sizes, s, orps


@pytest.mark.parametrize("stage", ["0", "1"])
def test_composed_forms_forced(stage):
    """Large claims of two-table terms take two rounds per pass by default (csrc/composed_stage.hpp, cross sums on the matrix cores);
    ZKHIP_STAGE=0 forces the round form (its unreduced K = 2 kernel is otherwise idle), ZKHIP_STAGE=1 the stage form from 2^15 entries on
    (the VALU cross sums below 2^12 indices per block): both must give the oracle's proof."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys; sys.path.insert(0, %r)
import numpy as np
import zk_cryptography_amd as zk
from oracle import oracle as ora
for k, log_n in ((2, 21), (2, 16)):
    t = np.stack([ora.random_fr(1 << log_n, 4000 + 10 * log_n + q) for q in range(k)])
    proof, ch = zk.ComposedSumcheck(zk.ComposedMultilinear(list(t))).prove()
    rp, och = ora.composed_prove(t)
    assert np.array_equal(proof.round_polys, rp) and np.array_equal(ch, och), (k, log_n)
flat = np.stack([ora.random_fr(1 << 17, 4500 + q) for q in range(4)])
s = ora.multi_composed_sum(flat, [2, 2])
terms = [zk.ComposedMultilinear([zk.Multilinear(flat[0]), zk.Multilinear(flat[1])]), zk.ComposedMultilinear([zk.Multilinear(flat[2]), zk.Multilinear(flat[3])])]
proof, ch = zk.MultiComposedSumcheckProver.prove_partial(terms, s)
orps, och = ora.multi_composed_prove(flat, [2, 2], s, partial=True)
assert proof.to_bytes() == ora.multi_composed_proof_bytes(orps) and np.array_equal(ch, och)
print("forms ok")
""" % root
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZKHIP_STAGE=stage), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "forms ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("partial", [False, True])
def test_multi_composed_sumcheck_proof(zk, ora, case, partial):   # multi_composed_sumcheck.rs:217-311
    flat, sizes, s, orps = _check_multi(zk, ora, _multi_cases(zk, ora)[case], partial)
    if not partial:
        assert ora.multi_composed_verify(flat, sizes, s, orps) == 1


@pytest.mark.parametrize("sizes,log_n", [([2, 3], 8), ([2, 2], 12), ([1, 5], 6), ([3], 10), ([2, 2, 1, 1], 7), ([2, 2], 20)])
@pytest.mark.parametrize("partial", [False, True])
def test_multi_composed_random(zk, ora, sizes, log_n, partial):   # bench shape: 2 + 3 tables x 2^8
    terms, seed = [], 1000
    for k in sizes:
        terms.append([zk.Multilinear(ora.random_fr(1 << log_n, seed + q)) for q in range(k)])
        seed += 17
    _check_multi(zk, ora, terms, partial)


def test_multi_composed_zero_coefficient_semantics(zk, ora):
    # a term whose round polynomial has vanishing coefficients (dropped at interpolation, sparse_univariate.rs:55)
    # next to one that cancels it (zero kept after addition, :159-203)
    R = zk.Fr.MODULUS
    a = zk.Multilinear(F(zk, [1, 2, 3, 4]))
    neg_a = zk.Multilinear(F(zk, [R - 1, R - 2, R - 3, R - 4]))
    const = zk.Multilinear(F(zk, [5, 5, 5, 5]))
    _check_multi(zk, ora, [[a], [neg_a]], True)
    _check_multi(zk, ora, [[const], [a]], True)
    _check_multi(zk, ora, [[const, const], [neg_a]], False)


@pytest.mark.parametrize("grid", [None, "2"])
def test_five_table_rounds_on_the_matrix_cores_at_every_size(grid):
    """composed_round_dot_kernel (K = 5: the last factor of every index as a byte GEMM, csrc/composed_dot.hpp) serves rounds of >= 2^18
    output pairs by default.  Here the prover tests above run once more in a process where it takes every round of >= 256 pairs
    (ZKHIP_ROUND_DOT_MIN_LOG=8), first and folding rounds, one step per workgroup and -- with two workgroups per round -- up to eight:
    bit-identical to the oracle and the golden vectors."""
    import os, subprocess, sys
    env = dict(os.environ, ZKHIP_ROUND_DOT_MIN_LOG="8")
    if grid:
        env["ZKHIP_ROUND_GRID"] = grid
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_composed.py"), os.path.join(here, "test_golden.py"), "-m", "gpu", "-x", "-q",
                          "-k", "(test_composed_prove_random and 5-) or test_multi_composed_random or test_hip_path_reproduces_golden or test_sum_check_proof"],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert out.returncode == 0, out.stdout.decode()[-3000:]


# ---- the two byte-GEMM kernels at their per-workgroup limit ---------------------------------------------------------------------------
# composed_round_dot_kernel and composed_cross2_mfma_kernel feed bytes as u - 128 to int8 MFMAs and rebuild the unsigned sums
# sum ua ub = G + 128 UA + 128 UB - 16384 J in 32 bits, for at most 65536 indices per workgroup.  The production grids give a workgroup
# 4096 indices and random bytes, so a true sum never has its top bit set.  Here one workgroup takes all 65536 and the operand bytes are 0xFF:
# M = ((r >> 192) << 192) - 1 has 24 low bytes of 0xFF as a STORED value, every byte-product sum of the 24 x 24 low positions is
# 65536 x 255^2 = 4 261 478 400 > 2^31, and with all-zero tables every fed byte is -128: G = +2^30 and the true sums are 0.
_LIMIT_CHILD = """
import sys; sys.path.insert(0, %(root)r)
import numpy as np
import zk_cryptography_amd as zk
from oracle import oracle as ora
R = zk.Fr.MODULUS
M = ((R >> 192) << 192) - 1
ONE = (1 << 256) %% R                               # the stored form of 1
n = 1 << 18
def const(v, count=n):                              # `count` entries with the STORED value v: raw limbs, canonical
    assert 0 <= v < R
    return np.tile(np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64), (count, 1))
def quarters(*parts):
    return np.concatenate(parts)
rnd = lambda seed: ora.random_fr(n // 4, seed)
tables = %(tables)s
t = np.stack(tables)
assert t.shape == (%(k)d, n, 4) and t.dtype == np.uint64
assert M.to_bytes(32, "little")[:24] == bytes([255]) * 24 and 65536 * 255 * 255 > 1 << 31
proof, ch = zk.ComposedSumcheck(zk.ComposedMultilinear(list(t))).prove()
rp, och = ora.composed_prove(t)
assert np.array_equal(proof.round_polys, rp) and np.array_equal(ch, och)
print("limit ok")
"""


def _limit_child(tables, k, env):
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _LIMIT_CHILD % dict(root=root, tables=tables, k=k)
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "limit ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


ROUND_DOT_LIMIT_TABLES = {
    # Q_t = M on every plane (table 0 = M, tables 1-3 = the stored 1), l = d = M (table 4: M below, 2M mod r above)
    "M": "[const(M), const(ONE), const(ONE), const(ONE), quarters(const(M, n // 2), const(2 * M % R, n // 2))]",
    "zero": "[const(0)] * 5",
}


@pytest.mark.parametrize("grid", ["2", "1"])
@pytest.mark.parametrize("fill", ["M", "zero"])
def test_round_dot_at_the_workgroup_limit(fill, grid):
    """K = 5, 2^18 entries, ZKHIP_ROUND_DOT_MIN_LOG=8.  ZKHIP_ROUND_GRID=2: launch_round() gives the first round (work = 2^17 output pairs)
    two workgroups of per_wg = 65536 staged indices each = CDT_MAX_PER_WG, composed_round_dot_kernel's limit; the later rounds halve it.
    ZKHIP_ROUND_GRID=1: per_wg = 131072 > CDT_MAX_PER_WG, so the first round falls back to the vector form (composed_round_kernel<5>) and
    the second (2^16 pairs, one workgroup of 65536) is the matrix-core one.  Fresh process: the overrides are read once.  The oracle's proof,
    bit for bit."""
    _limit_child(ROUND_DOT_LIMIT_TABLES[fill], 5, dict(ZKHIP_ROUND_DOT_MIN_LOG="8", ZKHIP_ROUND_GRID=grid))


CROSS2_LIMIT_TABLES = {
    "M": "[const(M), const(M)]",
    "zero": "[const(0), const(0)]",
    # the four blocks of each table differ, and so do the sixteen block pairs
    "quarters": "[quarters(const(M, n // 4), const(0, n // 4), rnd(7001), const(M, n // 4)), quarters(rnd(7002), const(M, n // 4), const(0, n // 4), const(M - 1, n // 4))]",
}


@pytest.mark.parametrize("fill", ["M", "zero", "quarters"])
def test_cross2_mfma_at_the_workgroup_limit(fill):
    """Two tables of 2^18 entries, ZKHIP_STAGE=1 (the stage form from 2^15 entries on) and ZKHIP_CROSS_GRID=1: stage_sums() launches
    composed_cross2_mfma_kernel for the first stage with m = 2^16 indices per block and grid = max(min(1, m / 128), ceil(m / 65536)) = 1 --
    ONE workgroup of 65536 indices, the kernel's limit (the default is 512 workgroups of 128).  The oracle's proof, bit for bit."""
    _limit_child(CROSS2_LIMIT_TABLES[fill], 2, dict(ZKHIP_STAGE="1", ZKHIP_CROSS_GRID="1"))
