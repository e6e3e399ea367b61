"""GPU parity: polynomial::Multilinear on the HIP path vs the CPU oracle (bit-exact), through
the C ABI.  Test names follow polynomial/src/multilinear/evaluation_form.rs `mod tests`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def F(zk, vals):
    return zk.Fr.from_ints(vals)


def ints(zk, a):
    return zk.Fr.to_ints(a)


def test_add_mul_distinct(zk):
    p1, p2 = zk.Multilinear(F(zk, [0, 0, 2, 2])), zk.Multilinear(F(zk, [0, 3, 0, 3]))
    assert ints(zk, p1.add_distinct(p2).to_numpy()) == [0, 3, 0, 3, 0, 3, 0, 3, 2, 5, 2, 5, 2, 5, 2, 5]
    assert ints(zk, p1.mul_distinct(p2).to_numpy()) == [0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0, 6, 0, 6, 0, 6]


def test_partial_evaluation_1(zk):
    out = zk.Multilinear(F(zk, [3, 1, 2, 5])).partial_evaluation(F(zk, [5])[0], 0)
    assert ints(zk, out.to_numpy()) == [(-2) % R, 21]


def test_partial_evaluation_2(zk):
    poly = zk.Multilinear(F(zk, [3, 9, 7, 13, 6, 12, 10, 18]))
    pts = F(zk, [3, 2])
    for r, k, want in [(2, 0, 57), (3, 1, 72), (1, 2, 38)]:
        assert ints(zk, poly.partial_evaluation(F(zk, [r])[0], k).evaluation(pts)) == [want]


def test_evaluation_1_and_2(zk):
    assert ints(zk, zk.Multilinear(F(zk, [3, 1, 2, 5])).evaluation(F(zk, [5, 6]))) == [136]
    assert ints(zk, zk.Multilinear(F(zk, [3, 9, 7, 13, 6, 12, 10, 18])).evaluation(F(zk, [2, 3, 1]))) == [39]
    assert ints(zk, zk.Multilinear(F(zk, [0, 0, 0, 3, 0, 0, 2, 5])).evaluation(F(zk, [2, 3, 4]))) == [48]


def test_split_poly_into_two_and_sum_each_part(zk):
    assert ints(zk, zk.Multilinear(F(zk, [0, 0, 0, 2, 2, 2, 2, 4])).split_poly_into_two_and_sum_each_part().to_numpy()) == [2, 10]
    assert ints(zk, zk.Multilinear(F(zk, [0, 0, 2, 7, 3, 3, 6, 11])).split_poly_into_two_and_sum_each_part().to_numpy()) == [9, 23]


def test_sum_over_boolean_hypercube(zk):
    assert ints(zk, zk.Multilinear(F(zk, [1, 2, 3, 4, 5, 6, 7, 8])).sum_over_the_boolean_hypercube()) == [36]


def test_poly_subtraction_add_scale(zk):
    a = zk.Multilinear(F(zk, [0, 0, 0, 5, 4, 4, 7, 12]))
    b = zk.Multilinear(F(zk, [0, 0, 0, 2, 0, 0, 1, 3]))
    assert ints(zk, (a - b).to_numpy()) == [0, 0, 0, 3, 4, 4, 6, 9]
    assert ints(zk, (a + b).to_numpy()) == [0, 0, 0, 7, 4, 4, 8, 15]
    assert ints(zk, (b - a).to_numpy()) == [0, 0, 0, (-3) % R, (-4) % R, (-4) % R, (-6) % R, (-9) % R]
    assert ints(zk, (a * F(zk, [3])[0]).to_numpy()) == [0, 0, 0, 15, 12, 12, 21, 36]


def test_shape_errors_like_the_reference(zk):
    with pytest.raises(AssertionError):
        zk.Multilinear(F(zk, [1, 2, 3]))                                       # evaluation_form.rs:16-20
    with pytest.raises(AssertionError):
        zk.Multilinear(F(zk, [1, 2, 3, 4])).evaluation(F(zk, [5]))             # :163-167
    with pytest.raises(AssertionError):
        zk.Multilinear(F(zk, [1, 2, 3, 4])).partial_evaluation(F(zk, [5])[0], 2)   # utils.rs:31-34
    with pytest.raises(AssertionError):
        zk.Multilinear(F(zk, [1, 2, 3, 4])).partial_evaluations(F(zk, [5, 6]), [0])  # :146-152
    with pytest.raises(AssertionError):
        zk.Multilinear(F(zk, [7])).partial_evaluation(F(zk, [5])[0], 0)        # n must be even


def test_to_bytes(zk, ora):
    a = ora.random_fr(64, 5)
    assert zk.Multilinear(a).to_bytes() == ora.mle_to_bytes(a)
    assert zk.Multilinear(F(zk, [1, 100])).to_bytes() == bytes(31) + b"\x01" + bytes(31) + bytes([100])


# ---- random parity vs the oracle ------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 5, 9, 10, 11, 13, 16])
def test_fold_every_variable_matches_oracle(zk, ora, log_n):
    n = 1 << log_n
    a = ora.random_fr(n, 100 + log_n)
    r = ora.random_fr(1, 7)[0]
    poly = zk.Multilinear(a)
    for k in sorted({0, 1, log_n // 2, log_n - 1} & set(range(log_n))):
        want = ora.mle_partial_evaluation(a, r, k)
        got = poly.partial_evaluation(r, k).to_numpy()
        assert np.array_equal(got, want), "variable %d" % k


def test_fold_edge_field_values(zk, ora):
    # r in {0, 1, r-1}; table entries in {0, r-1, 1}: exercises the conditional subtract / borrow paths
    vals = [0, R - 1, 1, R - 1, R - 1, 0, 2, R - 2] * 8
    a = F(zk, vals)
    for rv in [0, 1, R - 1, 2, (R + 1) // 2]:
        r = F(zk, [rv])[0]
        assert np.array_equal(zk.Multilinear(a).partial_evaluation(r, 0).to_numpy(), ora.mle_partial_evaluation(a, r, 0))


@pytest.mark.parametrize("log_n", [1, 3, 10, 11, 12, 13, 16, 17, 18, 19, 20, 21, 22])
def test_evaluation_matches_oracle(zk, ora, log_n):
    """sizes either side of 2^17, where `evaluation` turns into ONE pass over the table (the k-variable fold whose tiles keep only the
    sum of their outputs weighted by the eq table of the remaining points: zkhip_mle_evaluation)"""
    n = 1 << log_n
    a = ora.random_fr(n, 200 + log_n)
    pts = ora.random_fr(log_n, 9)
    assert np.array_equal(zk.Multilinear(a).evaluation(pts), ora.mle_evaluation(a, pts))


@pytest.mark.parametrize("log_n", [17, 19])
def test_evaluation_one_pass_edge_values(zk, ora, log_n):
    """the one-pass form at boolean points (weights 0 / 1: returns the table entry), at points 0, 1, r - 1 mixed with random ones, on
    tables of extreme entries (0, r - 1), and against the chain of folds that partial_evaluations takes"""
    n = 1 << log_n
    a = ora.random_fr(n, 300 + log_n)
    a[::3] = 0
    a[1::7] = F(zk, [R - 1])[0]
    poly = zk.Multilinear(a)
    for j in (0, n - 1, 0x15A5A % n):
        pt = ora.fr_from_ints([(j >> (log_n - 1 - k)) & 1 for k in range(log_n)])
        assert np.array_equal(poly.evaluation(pt), a[j])
    rnd = ora.random_fr(log_n, 31)
    for special in (0, 1, R - 1):
        pts = rnd.copy()
        pts[0] = pts[7] = pts[8] = pts[log_n - 1] = F(zk, [special])[0]      # leading, either side of the pass's split, last
        want = ora.mle_evaluation(a, pts)
        assert np.array_equal(poly.evaluation(pts), want)
        chain = poly.partial_evaluations(pts, [0] * log_n)                  # the same folds, table by table
        assert np.array_equal(chain.to_numpy().reshape(-1, 4)[0], want)


def test_partial_evaluations_matches_oracle(zk, ora):
    a = ora.random_fr(1 << 12, 77)
    pts = ora.random_fr(5, 78)
    for idx in ([0, 0, 0, 0, 0], [3, 1, 0, 2, 1], [11, 10, 9, 8, 7], [0, 5, 0, 5, 0]):
        want = ora.mle_partial_evaluations(a, pts, idx)
        got = zk.Multilinear(a).partial_evaluations(pts, idx).to_numpy()
        assert np.array_equal(got, want), idx
    assert np.array_equal(zk.Multilinear(a).partial_evaluations(pts[:0], []).to_numpy(), a)


@pytest.mark.parametrize("log_n", [1, 4, 10, 11, 15, 19])
def test_half_sums_match_oracle(zk, ora, log_n):
    a = ora.random_fr(1 << log_n, 300 + log_n)
    m = zk.Multilinear(a)
    assert np.array_equal(m.split_poly_into_two_and_sum_each_part().to_numpy(), ora.mle_half_sums(a))
    assert np.array_equal(m.sum_over_the_boolean_hypercube(), ora.mle_sum(a))


def test_distinct_random(zk, ora):
    a, b = ora.random_fr(32, 1), ora.random_fr(64, 2)
    assert np.array_equal(zk.Multilinear(a).add_distinct(zk.Multilinear(b)).to_numpy(), ora.mle_add_distinct(a, b))
    assert np.array_equal(zk.Multilinear(a).mul_distinct(zk.Multilinear(b)).to_numpy(), ora.mle_mul_distinct(a, b))


# ---- full-size (BASELINE config 2: 2^24 evals) through size-independent properties ------------
def test_fold_2_24_linearity_and_spot_checks(zk, ora):
    import torch
    n = 1 << 24
    g = torch.Generator(device="cuda").manual_seed(1234)
    t = torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)   # limbs < 2^62: valid residues
    poly = zk.Multilinear(t)
    r = ora.random_fr(1, 99)[0]
    folded = poly.partial_evaluation(r, 0)
    # spot-check 4096 scattered outputs against the oracle's scalar formula
    idx = torch.randint(0, n // 2, (4096,), generator=torch.Generator().manual_seed(5))
    lo = t[idx.cuda()].cpu().numpy().view(np.uint64)
    hi = t[(idx + n // 2).cuda()].cpu().numpy().view(np.uint64)
    got = folded.evaluations[idx.cuda()].cpu().numpy().view(np.uint64)
    pair = np.concatenate([lo, hi])          # fold of [lo.., hi..] at variable 0 pairs lo[i] with hi[i]
    assert np.array_equal(got, ora.mle_partial_evaluation(pair, r, 0))
    # sum is preserved by the fold identity: sum(fold(f, r)) = (1-r)*S_lo + r*S_hi
    hs = poly._half_sums()
    one = ora.fr_from_ints([1])[0]
    want = ora.fr_add(ora.fr_mul(ora.fr_sub(one, r), hs[0]), ora.fr_mul(r, hs[1]))
    assert np.array_equal(folded.sum_over_the_boolean_hypercube(), want)
    # evaluation at a boolean point returns the table entry (idempotence of the MLE on the hypercube)
    j = 0xABCDE5
    pt = ora.fr_from_ints([(j >> (23 - k)) & 1 for k in range(24)])
    assert np.array_equal(poly.evaluation(pt), t[j].cpu().numpy().view(np.uint64))


def test_back_to_back_calls_with_different_points_do_not_race(zk, ora):
    """Entry points return before the stream has run; host parameters must be captured at launch.
    Many folds with different points are queued behind a long kernel, then checked."""
    import torch
    big = zk.Multilinear(torch.randint(0, 2 ** 62, (1 << 22, 4), dtype=torch.int64, device="cuda"))
    a = ora.random_fr(1 << 12, 1)
    poly = zk.Multilinear(a)
    rs = ora.random_fr(16, 2)
    _ = big.partial_evaluation(rs[0], 0)            # keeps the stream busy while the host races ahead
    outs = [poly.partial_evaluation(rs[i], 0) for i in range(16)]
    scaled = [poly * rs[i] for i in range(16)]
    for i in range(16):
        assert np.array_equal(outs[i].to_numpy(), ora.mle_partial_evaluation(a, rs[i], 0))
        want = [x * y % zk.Fr.MODULUS for x, y in zip(zk.Fr.to_ints(a[:4]), zk.Fr.to_ints(rs[i:i + 1]) * 4)]
        assert zk.Fr.to_ints(scaled[i].to_numpy()[:4]) == want


def test_add_to_front_and_back(zk):   # evaluation_form.rs:465-507, :548-556
    F = zk.Fr.from_ints
    ints = lambda m: zk.Fr.to_ints(m.to_numpy())   # noqa: E731
    assert ints(zk.Multilinear(F([0, 0, 4, 4])).add_to_front(0)) == [0, 0, 4, 4, 0, 0, 4, 4]
    assert ints(zk.Multilinear(F([0, 4])).add_to_front(1)) == [0, 4, 0, 4, 0, 4, 0, 4]
    assert ints(zk.Multilinear(F([0, 0, 4, 4])).add_to_back(1)) == [0, 0, 0, 0, 4, 4, 4, 4]
    assert ints(zk.Multilinear(F([1, 2])).add_to_back(0)) == [1, 2]
    assert ints(zk.Multilinear.duplicate_evaluation(F([11]))) == [11, 11]
    assert ints(zk.Multilinear.additive_identity(2)) == [0, 0, 0, 0]


def test_add_to_back_front_match_oracle_random(zk, ora):
    v = ora.random_fr(64, 5)
    import numpy as np
    assert np.array_equal(zk.Multilinear(v).add_to_back(3).to_numpy(), ora.mle_add_to_back(v, 3))
    assert np.array_equal(zk.Multilinear(v).add_to_front(2).to_numpy(), ora.mle_add_to_front(v, 2))


# ---- operators, repeats and bytes at size, against the integer model (tests/mle_model.py) -------------------------
import ctypes as C   # noqa: E402
import os            # noqa: E402
import sys           # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mle_model as M   # noqa: E402
import tables as T      # noqa: E402


def same(got, want_ints):
    """the limbs are the canonical ones of the model's integers"""
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 4)
    return bool(T.below_r(got).all()) and np.array_equal(got, M.pack(want_ints))


@pytest.mark.parametrize("kind", T.FILLS_ARITH)
def test_operators_at_2_13_match_the_model(zk, kind):
    """2^13 entries are 32 workgroups; full-range stored values (tests/tables.py), python integers as the reference"""
    n = 1 << 13
    a, b = T.fill(kind, n, 4100), T.fill(T.rotation(T.FILLS_ARITH, kind, 2)[1], n, 4101)
    ta, tb = T.canonical(a), T.canonical(b)
    pa, pb = zk.Multilinear(a), zk.Multilinear(b)
    assert same((pa + pb).to_numpy(), M.elementwise(0, ta, tb))
    assert same((pa - pb).to_numpy(), M.elementwise(1, ta, tb))
    assert same((pb - pa).to_numpy(), M.elementwise(1, tb, ta))
    for s in (tb[5], 0, 1, R - 1):
        assert same((pa * M.pack([s])[0]).to_numpy(), M.elementwise(2, ta, scalar=s))
    x, y = zk.Multilinear(a[:64]), zk.Multilinear(b[:128])
    assert same(x.add_distinct(y).to_numpy(), M.distinct(ta[:64], tb[:128], False))
    assert same(x.mul_distinct(y).to_numpy(), M.distinct(ta[:64], tb[:128], True))
    assert same(y.mul_distinct(x).to_numpy(), M.distinct(tb[:128], ta[:64], True))
    half = zk.Multilinear(a[:n // 4])
    assert np.array_equal(half.add_to_front(1).to_numpy(), a[np.array(M.repeat(list(range(n // 4)), 0, n))])
    assert np.array_equal(half.add_to_back(2).to_numpy(), a[np.array(M.repeat(list(range(n // 4)), 2, n))])
    assert pa.to_bytes() == M.to_bytes(ta)


STREAM_STRIDE = 16384 * 256    # mle_grid_stream's cap times MLE_BLOCK: above 2^22 items the library's own grid takes a second step


def sampled_rows(n, count=4096):
    """the first and last row of each stride step of the capped grid, their neighbours, and scattered rows"""
    import torch
    edges = {0, 1, n - 2, n - 1}
    for s in range(STREAM_STRIDE, n, STREAM_STRIDE):
        edges |= {s - 2, s - 1, s, s + 1}
    rnd = torch.randint(0, n, (count - len(edges),), generator=torch.Generator().manual_seed(n % 1000003))
    return torch.cat([torch.tensor(sorted(edges)), rnd])


def random_device_table(n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)   # limbs < 2^62: valid residues


def rows(t, idx):
    return t[idx.cuda()].cpu().numpy().view(np.uint64)


def test_add_beyond_the_capped_grid(zk):
    """2^22 + 2^21 entries through the raw ABI (any n): lanes of the second stride step write half of a stride only"""
    import torch
    from zk_cryptography_amd import _native as N
    n = (1 << 22) + (1 << 21)
    a, b = random_device_table(n, 4201), random_device_table(n, 4202)
    out = torch.empty_like(a)
    ctx = N.Context.get(a.device.index)
    N.check(N.lib().zkhip_mle_elementwise(ctx.handle, C.c_int(0), N.ptr(a), N.ptr(b), None, C.c_size_t(n), C.c_size_t(n), N.ptr(out)), "elementwise")
    idx = sampled_rows(n)
    assert same(rows(out, idx), M.elementwise(0, T.canonical(rows(a, idx)), T.canonical(rows(b, idx))))


def test_add_distinct_beyond_the_capped_grid(zk):
    na, nb = 1 << 11, 1 << 12
    a, b = random_device_table(na, 4203), random_device_table(nb, 4204)
    out = zk.Multilinear(a).add_distinct(zk.Multilinear(b)).evaluations
    assert out.shape[0] == na * nb
    ta, tb = T.canonical(a.cpu().numpy().view(np.uint64)), T.canonical(b.cpu().numpy().view(np.uint64))
    idx = sampled_rows(na * nb)
    assert same(rows(out, idx), [(ta[q // nb] + tb[q % nb]) % R for q in idx.tolist()])   # out[i * nb + j] = a[i] + b[j]


def test_add_to_back_beyond_the_capped_grid(zk):
    n_in, v = 1 << 13, 10
    a = random_device_table(n_in, 4205)
    out = zk.Multilinear(a).add_to_back(v).evaluations
    assert out.shape[0] == n_in << v
    idx = sampled_rows(n_in << v)
    assert np.array_equal(rows(out, idx), rows(a, idx >> v))


def test_to_bytes_beyond_the_capped_grid(zk):
    import torch
    from zk_cryptography_amd import _native as N
    n = (1 << 22) + (1 << 21)
    a = random_device_table(n, 4206)
    out = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    ctx = N.Context.get(a.device.index)
    N.check(N.lib().zkhip_mle_to_bytes(ctx.handle, N.ptr(a), C.c_size_t(n), N.ptr(out)), "to_bytes")
    idx = sampled_rows(n)
    got = out.view(n, 32)[idx.cuda()].cpu().numpy().tobytes()
    assert got == M.to_bytes(T.canonical(rows(a, idx)))


# ---- DenseUnivariatePolynomial.degree / evaluate where their grids take a second step ---------------------------
def test_degree_above_the_capped_grid(zk):
    """2^19 + 257 coefficients: mle_grid's 2048 workgroups stride 2^19, so 257 lanes take a second step"""
    import torch
    n, stride = (1 << 19) + 257, 1 << 19
    one = torch.from_numpy(T.fill("top", 1, 4300).view(np.int64)).cuda()[0]
    for positions, want in (([], 0), ([0], 0), ([777], 777), ([5, stride - 1], stride - 1), ([stride - 1, stride], stride),
                            ([3, stride + 5], stride + 5), ([stride + 255, n - 1], n - 1), ([n - 1], n - 1), ([stride + 256, 12], stride + 256)):
        c = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        for at in positions:
            c[at] = one
        assert zk.DenseUnivariatePolynomial(c).degree() == want, positions


def test_evaluate_2_21_plus_1_sparse(zk):
    """1025 workgroups of the Horner scan: the top kernel's lanes hold two of them each, the last one"""
    import torch
    n = (1 << 21) + 1
    marks = [0, 7, 8, 2047, 2048, 2 * 2048 - 1, 2 * 2048, 1024 * 2048, n - 1]
    pos = sorted({m + d for m in marks for d in (-1, 0, 1) if 0 <= m + d < n})
    vals = T.fill("uniform_r", len(pos), 4400)
    c = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    c[torch.tensor(pos, device="cuda")] = torch.from_numpy(vals.view(np.int64)).cuda()
    poly = zk.DenseUnivariatePolynomial(c)
    nonzero = dict(zip(pos, T.canonical(vals)))
    for z in (0x1234567890ABCDEF1234567890ABCDEF % R, 0, 1, R - 1):
        assert same(poly.evaluate(M.pack([z])[0]), M.horner_suffix_sparse(nonzero, z, [0])), z
    assert poly.degree() == n - 1


# ---- which kernels fold_chain (csrc/zkhip.hip) launches for which call --------------------------------------------
FOLD_RECORDS = ("multifold", "multifold_valu", "multifold_small", "fold_tail", "fold")
EVAL = "evaluation"
# (log n, number of points, variable_indices or EVAL) -> the records in launch order.  A run of leading zeros is folded k variables at a
# time while more than 2^12 entries and at least 3 points are left, k = min(log2(entries) - 12, 8, points left), never below 3; the
# k-variable fold is the matrix-core one ("multifold") for k >= 4 and >= 2^13 outputs, the streaming VALU one (both records) for k = 3
# there, "multifold_small" below 2^13 outputs.  The rest is one "fold" per point until the indices left are all zero and at most 2^12
# entries remain: those finish in one "fold_tail".
DISPATCH = [
    (16, 3, [0, 0, 0], ["multifold", "multifold_valu"]),                 # k = 3, 2^13 outputs: the VALU streaming shape
    (17, 4, [0] * 4, ["multifold"]),                                     # k = 4, 2^13 outputs: the matrix cores
    (20, 5, [0] * 5, ["multifold"]),                                     # k = 8 clipped to the 5 points left
    (17, 5, [0] * 5, ["multifold_small"]),                               # 2^12 outputs
    (15, 4, [0] * 4, ["multifold_small", "fold_tail"]),                  # k = 3 of the 4 points, the last in the tail
    (16, 5, [0] * 5, ["multifold_small", "fold_tail"]),
    (16, 16, EVAL, ["multifold_small", "fold_tail"]),
    (21, 11, [0] * 11, ["multifold", "fold", "fold_tail"]),              # k = 8, then 2^13 entries: k = 1 < 3 breaks off
    (14, 14, EVAL, ["fold", "fold", "fold_tail"]),                       # k = 2 < 3
    (13, 13, EVAL, ["fold", "fold_tail"]),
    (12, 12, EVAL, ["fold_tail"]),
    (10, 2, [0, 0], ["fold_tail"]),
    (16, 2, [0, 0], ["fold", "fold"]),                                   # fewer than 3 points
    (13, 4, [0, 0, 0, 1], ["fold"] * 4),                                 # a non-zero index after the zeros: no k-variable fold, no tail
    (13, 4, [1, 0, 0, 0], ["fold", "fold_tail"]),                        # zeros after it: the tail once 2^12 entries are left
    (16, 5, [2, 0, 0, 0, 0], ["fold"] * 4 + ["fold_tail"]),              # ... but no k-variable fold, although 2^15 entries remain
    (12, 3, [11, 5, 0], ["fold"] * 2 + ["fold_tail"]),
    (14, 0, [], []),                                                     # no point: a copy
]


def fold_records(work):
    """work() with the library's profile on -> (its result, the names among FOLD_RECORDS in launch order)"""
    from zk_cryptography_amd import _native as N
    ctx = N.Context.get()
    N.check(N.lib().zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        result = work()
        mx = 64
        names = C.create_string_buffer(32 * mx)
        st, sp, cnt = (C.c_double * mx)(), (C.c_double * mx)(), C.c_uint32(0)
        N.check(N.lib().zkhip_profile_timeline(ctx.handle, C.c_uint32(mx), names, st, sp, C.byref(cnt)), "profile_timeline")
    finally:
        N.check(N.lib().zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    got = [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(cnt.value)]
    return result, [g for g in got if g in FOLD_RECORDS]


@pytest.mark.parametrize("log_n,n_pts,indices,records", DISPATCH)
def test_fold_chain_dispatch(zk, ora, log_n, n_pts, indices, records):
    a = T.fill("uniform_r" if log_n % 2 else "top", 1 << log_n, 4500 + log_n)
    pts = T.fill("uniform_r", max(n_pts, 1), 4600 + n_pts)[:n_pts]
    poly = zk.Multilinear(a)
    if indices == EVAL:
        got, names = fold_records(lambda: poly.evaluation(pts))
        want = ora.mle_evaluation(a, pts)
    else:
        got, names = fold_records(lambda: poly.partial_evaluations(pts, indices).to_numpy())
        want = ora.mle_partial_evaluations(a, pts, indices)
    assert names == records
    assert np.array_equal(got, want)
