"""GPU parity of Multilinear.evaluation_batch / evaluation(points3d) (zkhip_mle_evaluation_batch): every value of a batch equals the
CPU oracle's and, limb for limb, the single call's -- on the resident sizes, on tables of 2 .. 16 blocks, across the chunk bound, on
the fall-through to the single call, with pointers and points that repeat, at binary points (the bit order) and beside a commit in
flight."""
import ctypes as C

import numpy as np
import pytest

import tables as T

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def batch_min(n):
    from zk_cryptography_amd import _native as N
    return int(N.lib().zkhip_mle_evaluation_batch_min(n))


_CASES = {}


def case(ora, zk, log_n, count, kind="random"):
    """(host tables, device tables, points, the oracle's values) of `count` jobs at 2^log_n entries: made once, shared and left unchanged"""
    key = (log_n, kind)
    if key not in _CASES or len(_CASES[key][0]) < count:
        n = 1 << log_n
        if kind == "random":
            host = [ora.random_fr(n, 21000 + 64 * log_n + b) for b in range(count)]
        else:
            host = [T.fill(T.FILLS_ARITH[b % len(T.FILLS_ARITH)], n, 22000 + 64 * log_n + b) for b in range(count)]
        pts = T.fill("uniform_r", count * max(log_n, 1), 23000 + log_n).reshape(count, max(log_n, 1), 4)[:, :log_n]
        want = np.stack([ora.mle_evaluation(host[b], pts[b]) for b in range(count)])
        _CASES[key] = (host, [zk.Multilinear(t) for t in host], np.ascontiguousarray(pts), want)
    host, dev, pts, want = _CASES[key]
    return host[:count], dev[:count], pts[:count], want[:count]


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------
# 12: the last resident size, 13: the first with two blocks, 16: the last size of the kernels, 17: the fall-through
@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 6, 11, 12, 13, 14, 16, 17])
@pytest.mark.parametrize("which", ["three", "min"])
def test_every_value_is_the_oracles(zk, ora, log_n, which):
    B = 3 if which == "three" else batch_min(1 << log_n)      # (0 at 2^17: no batch is taken there, and the empty batch is empty)
    _host, dev, pts, want = case(ora, zk, log_n, max(B, 3))
    got = zk.Multilinear.evaluation_batch(dev[:B], pts[:B])
    assert got.shape == (B, 4) and got.dtype == np.uint64
    assert np.array_equal(got, want[:B])


# ---- 2. the batch is the single calls, limb for limb ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 8, 12, 13, 16])
def test_batch_equals_single_calls(zk, ora, log_n):
    kmin = batch_min(1 << log_n)
    sizes = sorted({1, 2, 7, kmin, kmin + 1})
    _host, dev, pts, want = case(ora, zk, log_n, max(sizes), kind="arith")
    single = np.stack([p.evaluation(pts[b]) for b, p in enumerate(dev)])
    assert np.array_equal(single, want)
    for B in sizes:
        assert np.array_equal(zk.Multilinear.evaluation_batch(dev[:B], pts[:B]), single[:B]), B


# ---- 3. bit order -----------------------------------------------------------------------------------------------------------------
def binary_point(index, log_n):
    """the point that selects table[index]: coordinate i is bit log_n - 1 - i of the index (point 0 = the top bit), as 0 or stored 1"""
    return np.stack([T.stored((index >> (log_n - 1 - i)) & 1) for i in range(log_n)])


@pytest.mark.parametrize("log_n", [5, 13, 16])
def test_binary_points_select_the_entry_with_point_0_as_the_top_bit(zk, ora, log_n):
    n, h = 1 << log_n, max(log_n - 12, 0)
    host, dev, _pts, _want = case(ora, zk, log_n, 1)
    index = {0, n - 1} | {1 << k for k in range(log_n)}                         # every bit position, those of the h block bits among them
    for q in range(1, 1 << h):                                                 # both sides of every block boundary
        index |= {q << 12, (q << 12) - 1}
    index = sorted(index)
    pts = np.stack([binary_point(i, log_n) for i in index])
    got = dev[0].evaluation(pts)
    assert np.array_equal(got, host[0][index])
    got = zk.Multilinear.evaluation_batch([dev[0]] * len(index), pts)
    assert np.array_equal(got, host[0][index])
    # every coordinate r - 1
    minus_one = np.tile(T.stored(T.R - 1), (log_n, 1))
    want = ora.mle_evaluation(host[0], minus_one)
    assert np.array_equal(dev[0].evaluation(np.stack([minus_one, minus_one])), np.stack([want, want]))
    assert np.array_equal(dev[0].evaluation(minus_one), want)


# ---- 4. pointers and points that repeat ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [5, 13])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_one_table_at_several_points(zk, ora, log_n, P):
    host, dev, pts, _want = case(ora, zk, log_n, 5)
    got = dev[0].evaluation(pts[:P])
    assert got.shape == (P, 4)
    assert np.array_equal(got, np.stack([ora.mle_evaluation(host[0], pts[b]) for b in range(P)]))
    two_d = dev[0].evaluation(pts[0])                                          # a 2-D argument is the single call, as ever
    assert two_d.shape == (4,) and np.array_equal(two_d, got[0])


@pytest.mark.parametrize("log_n", [5, 13])
def test_one_point_for_all_tables(zk, ora, log_n):
    host, dev, pts, _want = case(ora, zk, log_n, 5)
    got = zk.Multilinear.evaluation_batch(dev, pts[2])
    assert np.array_equal(got, np.stack([ora.mle_evaluation(t, pts[2]) for t in host]))


def test_the_mirror_checks_its_arguments(zk, ora):
    assert zk.Multilinear.evaluation_batch([], np.empty((0, 3, 4), dtype=np.uint64)).shape == (0, 4)
    _h5, dev5, pts5, _w5 = case(ora, zk, 5, 3)
    _h6, dev6, _p6, _w6 = case(ora, zk, 6, 3)
    with pytest.raises(AssertionError):
        zk.Multilinear.evaluation_batch([dev5[0], dev6[0]], pts5[:2])           # one length
    with pytest.raises(AssertionError):
        zk.Multilinear.evaluation_batch(dev5, pts5[:2])                         # one point per table
    with pytest.raises(AssertionError):
        zk.Multilinear.evaluation_batch(dev6, pts5)                             # as many coordinates as variables
    with pytest.raises(AssertionError):
        dev6[0].evaluation(pts5)


# ---- 5. across the chunk bound ----------------------------------------------------------------------------------------------------
def test_a_batch_of_one_chunk_and_one_job(zk, ora):
    import torch
    B = zk.Multilinear.BATCH_CHUNK + 1
    flat = ora.random_fr(4 * B, 24000)
    devflat = torch.from_numpy(flat.view(np.int64)).cuda()
    polys = [zk.Multilinear(devflat[4 * b:4 * b + 4]) for b in range(B)]
    pts = T.fill("uniform_r", 2 * B, 24001).reshape(B, 2, 4)
    got = zk.Multilinear.evaluation_batch(polys, pts)
    want = np.stack([ora.mle_evaluation(flat[4 * b:4 * b + 4], pts[b]) for b in range(B)])
    assert np.array_equal(got, want)


# ---- 6. refusals through the raw ABI ------------------------------------------------------------------------------------------------
class Raw:
    def __init__(self, zk, ora, log_n=5, B=3):
        from zk_cryptography_amd import _native as N
        self.N, self.B, self.n, self.log_n = N, B, 1 << log_n, log_n
        self.host, self.dev, self.pts, self.want = case(ora, zk, log_n, B)
        self.handle = self.dev[0]._ctx.handle
        self.ptr_list = [p.evaluations.data_ptr() for p in self.dev]
        self.ptrs = (C.c_void_p * B)(*self.ptr_list)
        self.out = np.full((B, 4), FILL)

    def call(self, **kw):
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        a = dict(h=self.handle, batch=self.B, ptrs=self.ptrs, n=self.n, pts=self.pts, n_pts=self.log_n, out=self.out)
        a.update(kw)
        return self.N.lib().zkhip_mle_evaluation_batch(a["h"], a["batch"], a["ptrs"], a["n"], vp(a["pts"]), a["n_pts"], vp(a["out"]))

    def untouched(self):
        return bool((self.out == FILL).all())


def test_raw_refusals_leave_the_outputs_alone(zk, ora):
    r = Raw(zk, ora)
    N = r.N
    holed = (C.c_void_p * r.B)(*(r.ptr_list[:-1] + [None]))
    assert r.call(h=None) == N.ERR_ARG
    assert r.call(ptrs=None) == N.ERR_ARG
    assert r.call(out=None) == N.ERR_ARG
    assert r.call(ptrs=holed) == N.ERR_ARG
    assert r.call(pts=None) == N.ERR_ARG
    for n in (0, 3, r.n - 2, r.n + 1):
        assert r.call(n=n) == N.ERR_SHAPE, n
    for n_pts in (0, r.log_n - 1, r.log_n + 1):
        assert r.call(n_pts=n_pts) == N.ERR_SHAPE, n_pts
    assert r.call(n=2 * r.n) == N.ERR_SHAPE                                      # the points of another length
    assert r.call(batch=0) == N.ZKHIP_OK
    assert r.call(batch=0, ptrs=None, pts=None, out=None) == N.ZKHIP_OK
    assert r.untouched()
    assert r.call() == N.ZKHIP_OK
    assert np.array_equal(r.out, r.want)


@pytest.mark.parametrize("log_n", [5, 13])
def test_beside_a_commit_in_flight_it_is_busy(zk, ora, log_n):
    r = Raw(zk, ora, log_n=log_n)
    N = r.N
    srs = zk.TrustedSetup.setup(ora.random_fr(10, 25000))
    poly = zk.Multilinear(ora.random_fr(1 << 10, 25001))
    want_commit = zk.MultilinearKZG.commitment(poly, srs)
    pending = zk.MultilinearKZG.commitment_begin(poly, srs)
    try:
        assert r.call() == N.ERR_BUSY and r.untouched()
        assert r.call(batch=1) == N.ERR_BUSY and r.untouched()                   # the single call's path is a user of the workspace too
        with pytest.raises(N.ZkhipError) as ei:
            zk.Multilinear.evaluation_batch(r.dev, r.pts)
        assert ei.value.status == N.ERR_BUSY
        with pytest.raises(N.ZkhipError) as ei:
            r.dev[0].evaluation(r.pts)
        assert ei.value.status == N.ERR_BUSY
    finally:
        got_commit = pending.wait()
    assert got_commit == want_commit
    assert r.call() == N.ZKHIP_OK
    assert np.array_equal(r.out, r.want)


# ---- 7. ComposedMultilinear.evaluation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 13])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_composed_evaluation_is_the_product_of_single_evaluations(zk, ora, log_n, K):
    host, dev, pts, _want = case(ora, zk, log_n, 5)
    got = zk.ComposedMultilinear(dev[:K]).evaluation(pts[1])
    want = 1
    for p, t in zip(dev[:K], host[:K]):
        v = zk.Fr.to_ints(p.evaluation(pts[1]))[0]
        assert v == ora.fr_to_ints(ora.mle_evaluation(t, pts[1]))[0]
        want = want * v % zk.Fr.MODULUS
    assert got == want
