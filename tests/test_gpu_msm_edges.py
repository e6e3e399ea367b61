"""The MSM end to end against a closed form on adversarial scalars: commit == e G with e = sum s_i k_i mod r in Python integers, k_i the
known discrete logarithm of SRS point i (tau^i, or eq_i(tau) MSB first), and ONE scalar multiplication of the generator -- by the pure-Python
model (tests/golden/model.py) for the SRS spot checks, the populations and the level-2 cases, by the oracle's g1_mul_int where a test
compares dozens of points.  Neither side reads the digits, so a fault shared by the plain, table and level-table paths (DigitStream,
the sort, the heavy passes, the curve arithmetic) does not cancel.  Scalars: the boundary families and threshold populations of
tests/msm_cases.py; paths: the plain bucket pipeline, the short path, the bucket pipeline on the shifted-SRS table, batches, and openings
whose quotients are prescribed level by level.  Every case is paired with a run of the stage driver on the scalars it commits that
shows the stage was reached: n_rec[2] >= 1 for level 2 of the heavy-bucket tree, points in the last bucket of each set of the expected
width for the bucket pipelines, pairs in the top plane for the short path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import model as M  # noqa: E402
import msm_cases as MC  # noqa: E402
import msm_driver as DRV  # noqa: E402

pytestmark = pytest.mark.gpu

R = MC.R
TAU = 0x1F3D5B79A2C4E6F8091A2B3C4D5E6F708192A3B4C5D6E7F8011223344556677 % R
INF_AT = 5


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _point(zk, srs, i):
    return zk.G1Affine(srs.powers_of_tau_in_g1[i].cpu().numpy().view(np.uint64), bool(srs.inf[i].item()))


def _same(got, e, ora=None):
    """got == e G: one scalar multiplication by the pure-Python model, or by the oracle where a test has dozens of them (the model
    takes 0.2 s each)"""
    e %= R
    if ora is None:
        want = M.g1_mul(M.G1, e)
        assert got.infinity if want is None else (not got.infinity and got.coords() == want)
        return
    a = ora.g1_to_affine(ora.g1_mul_int(ora.g1_generator(), e))
    assert got.infinity == bool(a[12]) == (e == 0)
    if e:
        assert np.array_equal(got.xy, a[:12])


def _spot_check(zk, srs, log_of, seed):
    """a wrong SRS is reported as such: a handful of its points against k_i G"""
    for i in MC.spot_indices(len(srs), seed):
        p = _point(zk, srs, i)
        assert not p.infinity and p.coords() == M.g1_mul(M.G1, log_of(i)), "SRS point %d" % i


_UNI = {}


def uni_srs(zk, n, flag=True):
    """(srs with point 5 flagged at infinity when it has one and `flag`, the logarithms, the skipped indices), once per size"""
    if (n, flag) not in _UNI:
        srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(TAU), n - 1)
        assert len(srs) == n
        logs = MC.univariate_logs(TAU, n)
        _spot_check(zk, srs, lambda i: logs[i], n)
        skip = ()
        if flag and n > INF_AT:
            srs.inf[INF_AT] = 1
            srs.invalidate()
            skip = (INF_AT,)
        _UNI[(n, flag)] = (srs, logs, skip)
    return _UNI[(n, flag)]


def _dev(scalars):
    import torch
    return torch.from_numpy(MC.to_mont(scalars).view(np.int64)).cuda()


def _variants(widths, n, seed):
    """every family cycled over the positions, then mixed half-and-half with uniform scalars"""
    for k, (name, pool) in enumerate(MC.families(widths).items()):
        yield name, MC.cycled(pool, n, seed + k)
        yield name + "+uniform", MC.cycled(pool, n, seed + 100 + k, mix=True)


def _half_is_at_the_boundary(g):
    """`half` of every problem's own widths carries magnitude 2^(c - 1) in every window below the top"""
    for j in range(g.n_problems):
        w = g.widths(j)
        assert MC.recode(MC.half(w), w)[0][:-1] == [1 << (c - 1) for c in w[:-1]]


def _last_buckets_hit(scalars, offsets, shared=False, stride=0, inf=None, narrow=None):
    """The stage was reached: a run of the sort driver on these very scalars leaves points in the LAST bucket (magnitude 2^(c - 1)) of
    every bucket set that has a window of the set's own width below its problem's top window.  -> the widths of those sets.
    A window one bit narrower than its set has its boundary digit in the middle of the set: that bucket holds points too, and
    `narrow` (a set) collects those windows' widths."""
    g = DRV.geo(offsets, shared, stride)
    _half_is_at_the_boundary(g)
    d = scalars if hasattr(scalars, "data_ptr") else _dev(scalars)
    counts = DRV.sort(d, offsets, shared, stride, inf=inf, counters_only=True)["counts"]
    hit = set()
    for j in range(g.n_problems):
        if g.offsets[j + 1] == g.offsets[j]:
            continue
        for c, set_idx, _ in g.wins[g.win_first[j]: g.win_first[j + 1] - 1]:
            c_set, base = g.sets[set_idx][0], g.sets[set_idx][1]
            assert counts[base + (1 << (c - 1)) - 1] > 0, (j, set_idx, c_set, c)
            if c == c_set:
                hit.add(c_set)
            elif narrow is not None:
                narrow.add(c)
    assert hit
    return hit


def _top_plane_hit(scalars, widths, inf=None):
    """The short path sums one plane per digit bit: the digits the driver cuts from these very scalars put pairs into the top plane,
    hi - 1, which magnitude 2^(hi - 1) alone reaches.  -> the number of such pairs"""
    hi = widths[0]
    assert MC.recode(MC.half(widths), widths)[0][0] == 1 << (hi - 1)
    d = np.abs(DRV.digits(MC.to_mont(scalars), widths).astype(np.int64))
    if inf is not None:
        d = d[np.asarray(inf) == 0]
    assert d.max() == 1 << (hi - 1)
    pairs = int(((d >> (hi - 1)) & 1).sum())
    assert pairs > 0
    return pairs


def _inf_of(srs, n):
    return srs.inf[:n].cpu().numpy()


def _commit(zk, srs, n_points, scalars, table):
    from zk_cryptography_amd import kzg as K
    return K._commit(srs.powers_of_tau_in_g1, srs.inf, n_points, _dev(scalars), len(scalars), False, table)


# ---- families x paths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c", [(300, 8), (4096, 12), (4097, 16), (1 << 14, 16)])
def test_families_on_the_plain_pipeline(zk, ora, n, c):
    assert n in MC.PLAIN_SIZES
    srs, logs, skip = uni_srs(zk, n)
    widths = DRV.geo([0, n]).widths(0)
    for name, sc in _variants(widths, n, n):
        if name == "half":
            assert _last_buckets_hit(sc, [0, n], inf=_inf_of(srs, n)) == {c}
        _same(_commit(zk, srs, n, sc, None), MC.exponent(sc, logs, skip), ora)


@pytest.mark.parametrize("n,n_points,hi", [(1, 1, 8), (63, 63, 9), (64, 64, 9), (65, 65, 10), (300, 300, 12), (4095, 4095, 15), (4096, 4096, 15),
                                           (100, 256, 11)])
def test_families_on_the_short_path(zk, ora, n, n_points, hi):
    """at most 2^12 scalars against a table: one plain sum per digit bit; magnitude 2^(hi - 1) is alone in the top plane"""
    assert (n, n_points) in MC.TABLES
    srs, logs, skip = uni_srs(zk, n_points)
    table = srs.precompute().table
    widths = DRV.geo([0, n], True, n_points).widths(0)
    assert widths[0] == hi
    for name, sc in _variants(widths, n, 3 * n + n_points):
        if name == "half":
            n_hi = sum(1 for c in widths[:-1] if c == hi)
            assert _top_plane_hit(sc, widths, _inf_of(srs, n)) >= n_hi * (n - (1 if n > INF_AT else 0))
        _same(_commit(zk, srs, n_points, sc, table), MC.exponent(sc, logs, skip), ora)


@pytest.mark.parametrize("n,n_points,c", [(1 << 13, 1 << 13, 16), (1 << 14, 1 << 14, 16), (1 << 15, 1 << 15, 18), (1 << 16, 1 << 16, 19),
                                          (5000, 1 << 16, 19)])
def test_families_on_the_table_pipeline(zk, ora, n, n_points, c):
    """bucket sets of 16, 18 and 19 bits (2^13 ... 2^16 points), and a commit shorter than its table.  No geometry builds a set of 17
    bits (sixteen windows are 16 bits each, fifteen are 18 / 17): 17-bit windows live on the 18-bit set of the 2^15-point table, their
    boundary digit in bucket 2^16 - 1"""
    assert (n, n_points) in MC.TABLES
    srs, logs, skip = uni_srs(zk, n_points)
    table = srs.precompute().table
    widths = DRV.geo([0, n], True, n_points).widths(0)
    for name, sc in _variants(widths, n, 5 * n + n_points):
        if name == "half":
            narrow = set()
            assert _last_buckets_hit(sc, [0, n], True, n_points, inf=_inf_of(srs, n), narrow=narrow) == {c}
            assert narrow == ({c - 1} if len(set(widths)) == 2 else set()) and (n_points != 1 << 15 or narrow == {17})
        _same(_commit(zk, srs, n_points, sc, table), MC.exponent(sc, logs, skip), ora)


@pytest.mark.parametrize("offsets", [[1, 2, 300, 5000, 16384], list(range(3, 3 + 5 * 64 + 1, 5))], ids=["four", "sixty-four"])
def test_families_in_a_batch(zk, ora, offsets):
    """every problem with the families of its OWN widths"""
    from zk_cryptography_amd.kzg import commit_batch
    total = offsets[-1]
    srs, logs, skip = uni_srs(zk, 16384)
    rel = [o - offsets[0] for o in offsets]
    assert rel in MC.BATCHES
    g = DRV.geo(rel)
    names = list(MC.families(g.widths(0)))
    for k, name in enumerate(names):
        for mix in (False, True):
            sc = [0] * total
            for j in range(g.n_problems):
                lo, hi = offsets[j], offsets[j + 1]
                sc[lo:hi] = MC.cycled(MC.families(g.widths(j))[name], hi - lo, 70 + 10 * k + j, mix=mix)
            if name == "half" and not mix:      # every set of every problem below its top window
                hit = _last_buckets_hit(sc[offsets[0]:], rel, inf=srs.inf[offsets[0]: total].cpu().numpy())
                assert hit == {c for j in range(g.n_problems) for c in g.widths(j)[:-1]}
            got = commit_batch(srs.powers_of_tau_in_g1, srs.inf, _dev(sc), offsets)
            for j in range(g.n_problems):
                lo, hi = offsets[j], offsets[j + 1]
                e = sum(sc[i] * logs[i] for i in range(lo, hi) if i not in skip) % R
                _same(got[j], e, ora)


def test_the_last_bucket_of_the_20_bit_set(zk):
    """the widest set there is: 2^19 buckets, the shifted-SRS table of 2^20 points (13 windows of 20 / 19 bits)"""
    import torch
    from zk_cryptography_amd import kzg as K
    n = 1 << 20
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(TAU), n - 1)
    logs = MC.univariate_logs(TAU, n)
    _spot_check(zk, srs, lambda i: logs[i], n)
    widths = DRV.geo([0, n], True, n).widths(0)
    assert widths == [20] * 9 + [19] * 4
    pool = [MC.half(widths), MC.half_plus_one(widths), MC.all_equal(widths, 1 << 18)]
    idx = np.random.default_rng(20).integers(0, len(pool), n)
    d_sc = torch.from_numpy(MC.to_mont(pool)[idx].view(np.int64)).cuda().contiguous()
    assert _last_buckets_hit(d_sc, [0, n], True, n) == {20}
    sums = [0] * len(pool)
    for p, k in zip(idx.tolist(), logs):
        sums[p] += k
    got = K._commit(srs.powers_of_tau_in_g1, srs.inf, n, d_sc, n, False, srs.precompute().table)
    srs.invalidate()                                    # 1.6 GiB of table
    _same(got, sum(s * t for s, t in zip(pool, sums)))


# ---- threshold populations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,table", [(512, False), (4047, False), (14436, False), (1 << 13, True)])
def test_threshold_populations(zk, n, table):
    srs, logs, skip = uni_srs(zk, n)
    g = DRV.geo([0, n], table, n if table else 0)
    sc, placed = MC.population(n, g.widths(0), g.heavy_min, 7 + n, avoid_all_windows=table)
    assert {31, 32, 33} <= set(placed.values())
    _same(_commit(zk, srs, n, sc, srs.precompute().table if table else None), MC.exponent(sc, logs, skip))


# ---- level 2 of the heavy-bucket tree --------------------------------------------------------------------------------------------------------
def _reached_level_2(d_scalars, n, shared=False, stride=0, inf=None):
    ovf = DRV.sort(d_scalars, [0, n], shared, stride, inf=inf, counters_only=True)["ovf"]
    assert ovf[3] >= 1 and ovf[4] == 0, ovf          # n_rec[2] >= 1; level 3 stays unreached
    return ovf


@pytest.fixture(scope="module")
def srs_2_20(zk):
    tau = MC.uniform(20, 2020)
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints(tau))
    _spot_check(zk, srs, lambda i: MC.eq_log(tau, i), 20)
    return srs


@pytest.mark.parametrize("which", ["one", "minus_one", "half"])
def test_heavy_level_2_constant_table(zk, srs_2_20, which):
    """sum_i eq_i(tau) = 1: a constant table c commits to c G; 2^20 points in one bucket of every window with a non-zero digit"""
    import torch
    n = 1 << 20
    c = {"one": 1, "minus_one": R - 1, "half": MC.half(DRV.geo([0, n]).widths(0))}[which]
    d_sc = torch.from_numpy(MC.to_mont([c]).view(np.int64)).cuda().repeat(n, 1).contiguous()
    _reached_level_2(d_sc, n)
    _same(zk.MultilinearKZG.commitment(zk.Multilinear(d_sc), srs_2_20), c)


def test_heavy_level_2_at_the_tree_thresholds(zk):
    """buckets of 524288 (level 1) and 524289 points (one tree level more), 2049 and 33"""
    import torch
    n = 1050659
    srs, logs, skip = uni_srs(zk, n, flag=False)          # every point counts: the populations are exact
    vals = np.repeat(np.array([1, 2, 3, 4]), [524288, 524289, 2049, 33])
    assert len(vals) == n and not skip
    vals = vals[np.random.default_rng(n).permutation(n)]
    d_sc = torch.from_numpy(MC.to_mont([0, 1, 2, 3, 4])[vals].view(np.int64)).cuda().contiguous()
    ovf = _reached_level_2(d_sc, n)
    assert [MC.filing(c)[1] for c in (524288, 524289, 2049)] == [1, 2, 1]
    assert DRV.geo([0, n]).heavy_min == 132                    # 33 points stay a light bucket at this size
    assert ovf == [256 + 259 + 2, 256 + 257 + 2, 1 + 2 + 1, 1, 0]
    e = sum(v * k for v, k in zip(vals.tolist(), logs)) % R
    from zk_cryptography_amd import kzg as K
    _same(K._commit(srs.powers_of_tau_in_g1, srs.inf, n, d_sc, n, False, None), e)


@pytest.mark.parametrize("family", ["all_equal_1", "all_equal_half"])
def test_heavy_level_2_on_the_table(zk, family):
    """2^16 scalars with one digit value in every window: the 14 windows share one bucket set, 917504 entries in one bucket (less the 14
    of the point at infinity)"""
    n = 1 << 16
    srs, logs, skip = uni_srs(zk, n)
    widths = DRV.geo([0, n], True, n).widths(0)
    assert widths == [19] * 4 + [18] * 10
    s = MC.families(widths)[family][0]
    assert MC.recode(s, widths)[0][:-1] == [1 if family == "all_equal_1" else 1 << 17] * 13
    d_sc = _dev([s] * n)
    ovf = _reached_level_2(d_sc, n, True, n, inf=srs.inf.cpu().numpy())
    assert ovf == [450, 448, 2 if family == "all_equal_1" else 3, 1, 0]
    from zk_cryptography_amd import kzg as K
    got = K._commit(srs.powers_of_tau_in_g1, srs.inf, n, d_sc, n, False, srs.precompute().table)
    _same(got, s * sum(k for i, k in enumerate(logs) if i not in skip))


# ---- openings with crafted quotients ---------------------------------------------------------------------------------------------------------
levels_of = MC.levels_of


def crafted_table(quotients, last):
    """With z = (1, ..., 1) the remainder of a round is the upper half of the table: built from the last round backwards (upper half A,
    lower half A - q) the table has the prescribed quotient vectors, and p(z) = last"""
    f = [last % R]
    for q in reversed(quotients):
        assert len(q) == len(f)
        f = [(a - b) % R for a, b in zip(f, q)] + f
    return f


def open_reference(table, z, tau):
    """MultilinearKZG::open in Python integers -> (p(z), the quotient vectors, Q_k(tau_{k+1}, ...) for every round k)"""
    f, qs, logs = list(table), [], []
    for k in range(len(z)):
        h = len(f) // 2
        q = [(f[h + i] - f[i]) % R for i in range(h)]
        qs.append(q)
        logs.append(MC.mle_eval(q, tau[k + 1:]))
        f = [(f[i] + z[k] * q[i]) % R for i in range(h)]
    return f[0], qs, logs


def _check_proof(zk, ora, proof, ev, logs):
    assert zk.Fr.to_ints(proof.evaluation) == [ev]
    assert len(proof.proofs) == len(logs)
    for got, e in zip(proof.proofs, logs):
        _same(got, e, ora)


@pytest.mark.parametrize("n_vars,tables", [(8, True), (12, True), (13, True), (13, False)])
def test_openings_with_crafted_quotients(zk, ora, n_vars, tables):
    """n_vars 8, 12: the short path against level tables built on first use; 13 with precompute_open(): the bucket pipeline on the level
    tables; 13 without: the plain batch.  Every level's quotient vector is the families of that level's own widths."""
    n = 1 << n_vars
    tau = MC.uniform(n_vars, 900 + n_vars)
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints(tau))
    _spot_check(zk, srs, lambda i: MC.eq_log(tau, i), n_vars)
    if tables and n > zk.TrustedSetup.SMALL_SRS:
        srs.precompute_open()
    g = DRV.geo(levels_of(n_vars), tables, 0)
    quotients = [MC.cycled(MC.family_scalars(g.widths(k)), n >> (k + 1), 31 * n_vars + k) for k in range(n_vars)]
    last = MC.uniform(1, 5)[0]
    table = crafted_table(quotients, last)
    z = [1] * n_vars
    ev, qs, logs = open_reference(table, z, tau)
    assert ev == last and qs == quotients
    assert n_vars in MC.LEVEL_VARS
    flat = [s for q in quotients for s in q]
    if n > zk.TrustedSetup.SMALL_SRS:      # the bucket pipeline: the last bucket of every level's set(s): 15 ... 8 bits wide with tables, 11 ... 8 without
        hit = _last_buckets_hit(flat, levels_of(n_vars), tables, 0)
        assert hit == ({8, 9, 10, 11, 12, 13, 14, 15} if tables else {8, 9, 10, 11})
    else:                                   # the short path: every level's top plane
        for k in range(n_vars):
            _top_plane_hit(quotients[k], g.widths(k))
    poly = zk.Multilinear(MC.to_mont(table))
    proof = zk.MultilinearKZG.open(poly, zk.Fr.from_ints(z), srs)
    assert (srs.level_tables is not None) == tables
    _check_proof(zk, ora, proof, ev, logs)
    if n_vars == 8:      # and in a batch: the crafted table twice, a uniform one between
        uni, zu = MC.uniform(n, 77), MC.uniform(n_vars, 78)
        evu, _, logsu = open_reference(uni, zu, tau)
        got = zk.MultilinearKZG.open_batch([poly, zk.Multilinear(MC.to_mont(uni)), poly], [zk.Fr.from_ints(z), zk.Fr.from_ints(zu), zk.Fr.from_ints(z)], srs)
        _check_proof(zk, ora, got[0], ev, logs)
        _check_proof(zk, ora, got[1], evu, logsu)
        _check_proof(zk, ora, got[2], ev, logs)
