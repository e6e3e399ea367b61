"""GPU parity of Sumcheck.prove_batch / ComposedSumcheck.prove_batch (zkhip_sumcheck_prove_batch, zkhip_composed_prove_batch): every
proof of a batch equals the CPU oracle's and, bit for bit, the single call's -- on the fully resident sizes, across the rounds that run
from global memory, across the chunk bound and on the fall-through to the single provers."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import tables as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _basic_single(zk, evals, claimed="true"):
    sc = zk.Sumcheck(evals if isinstance(evals, zk.Multilinear) else zk.Multilinear(evals))
    if isinstance(claimed, str):
        sc.poly_sum()
    elif claimed is not None:
        sc.sum = claimed
    return sc.prove()


def _same_basic(got, want):
    (gp, gch), (wp, wch) = got, want
    assert np.array_equal(gp.sum, wp.sum)
    assert gp.univariate_poly.shape == wp.univariate_poly.shape and np.array_equal(gp.univariate_poly, wp.univariate_poly)
    assert gch.shape == wch.shape and np.array_equal(gch, wch)


def _same_composed(got, want):
    (gp, gch), (wp, wch) = got, want
    assert gp.round_polys.shape == wp.round_polys.shape and np.array_equal(gp.round_polys, wp.round_polys)
    assert gch.shape == wch.shape and np.array_equal(gch, wch)


def _composed(zk, tabs):
    return zk.ComposedMultilinear([zk.Multilinear(t) for t in tabs])


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------
# 12: the last fully resident size; 13: one round from global memory; 14: two, the slab folded in place; 16: the last batched size;
# 17: above it, the single provers one after another.  Three proofs of 2^8 entries and more are fewer than the batch kernel is
# faster for (csrc/sumcheck_batch_kernels.hpp scb_min_batch: they run as proofs in flight), so the kernel's seams come a second time
# with the fewest proofs that reach it.
@pytest.mark.parametrize("log_n,B", [(0, 3), (1, 3), (2, 3), (5, 3), (12, 3), (13, 3), (14, 3), (16, 3), (17, 2),
                                     (8, 4), (12, 4), (13, 6), (14, 6), (16, 16)])
def test_basic_batch_matches_oracle(zk, ora, log_n, B):
    evs = [ora.random_fr(1 << log_n, 7000 + 16 * log_n + b) for b in range(B)]
    got = zk.Sumcheck.prove_batch([zk.Multilinear(e) for e in evs])
    assert len(got) == B
    for b in range(B):
        s, rp, ch = ora.sumcheck_prove(evs[b])
        proof, gch = got[b]
        assert np.array_equal(proof.sum, s)
        assert proof.univariate_poly.shape == (log_n, 2, 4) and np.array_equal(proof.univariate_poly, rp)
        assert gch.shape == (log_n, 4) and np.array_equal(gch, ch)
        if log_n:
            assert ora.sumcheck_verify(evs[b], proof.sum, proof.univariate_poly)


# (2, 11): exactly 2^12 entries; (3, 11): one global round, into LDS; (5, 9) resident, (5, 10) not; (4, 14): 2^16 entries;
# (2, 16): above, the single provers one after another; (4, 14) a second time with the six proofs from which on the kernel takes it
@pytest.mark.parametrize("K,log_n,B", [(1, 3, 3), (2, 11, 3), (3, 11, 3), (5, 4, 3), (5, 9, 3), (5, 10, 3), (4, 14, 3), (2, 16, 2), (4, 14, 6)])
def test_composed_batch_matches_oracle(zk, ora, K, log_n, B):
    tabs = [np.stack([ora.random_fr(1 << log_n, 7500 + 64 * log_n + 8 * b + q) for q in range(K)]) for b in range(B)]
    got = zk.ComposedSumcheck.prove_batch([_composed(zk, t) for t in tabs])
    assert len(got) == B
    for b in range(B):
        rp, ch = ora.composed_prove(tabs[b])
        proof, gch = got[b]
        assert proof.round_polys.shape == (log_n, K + 1, 4) and np.array_equal(proof.round_polys, rp)
        assert gch.shape == (log_n, 4) and np.array_equal(gch, ch)
        assert ora.composed_verify(tabs[b], ora.composed_sum(tabs[b]), proof.round_polys)


def test_composed_batch_of_one_entry_tables_delivers_nothing(zk, ora):
    got = zk.ComposedSumcheck.prove_batch([_composed(zk, [ora.random_fr(1, 7900 + b), ora.random_fr(1, 7910 + b)]) for b in range(3)])
    assert [(p.round_polys.shape, ch.shape) for p, ch in got] == [((0, 3, 4), (0, 4))] * 3


# ---- 2. batch == single calls, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 7])
def test_batch_equals_single_calls(zk, ora, B):
    for log_n in (3, 8, 13):
        polys = [zk.Multilinear(ora.random_fr(1 << log_n, 8000 + 16 * log_n + b)) for b in range(B)]
        for g, p in zip(zk.Sumcheck.prove_batch(polys), polys):
            _same_basic(g, _basic_single(zk, p))
    for K, log_n in ((2, 6), (3, 11)):
        cps = [_composed(zk, [ora.random_fr(1 << log_n, 8200 + 64 * log_n + 8 * b + q) for q in range(K)]) for b in range(B)]
        for g, cp in zip(zk.ComposedSumcheck.prove_batch(cps), cps):
            _same_composed(g, zk.ComposedSumcheck(cp).prove())


def test_one_more_than_a_chunk(zk, ora):
    """tables of four entries, Sumcheck.BATCH_CHUNK + 1 of them: the second chunk is one proof.  Every proof against the oracle (a
    two-round proof costs it microseconds), the chunk's neighbours against the single calls as well."""
    B = zk.Sumcheck.BATCH_CHUNK + 1
    import torch
    flat = ora.random_fr(4 * B, 8400)
    dev = torch.from_numpy(flat.view(np.int64)).cuda()
    polys = [zk.Multilinear(dev[4 * b: 4 * b + 4]) for b in range(B)]
    got = zk.Sumcheck.prove_batch(polys)
    assert len(got) == B
    for b in range(B):
        s, rp, ch = ora.sumcheck_prove(flat[4 * b: 4 * b + 4])
        assert np.array_equal(got[b][0].sum, s) and np.array_equal(got[b][0].univariate_poly, rp) and np.array_equal(got[b][1], ch)
    for b in (0, B - 3, B - 2, B - 1):
        _same_basic(got[b], _basic_single(zk, polys[b]))
    cps = [zk.ComposedMultilinear([polys[b], polys[(b + 1) % B]]) for b in range(B)]
    cgot = zk.ComposedSumcheck.prove_batch(cps)
    assert len(cgot) == B
    for b in range(B):
        rp, ch = ora.composed_prove(np.stack([flat[4 * b: 4 * b + 4], flat[4 * ((b + 1) % B): 4 * ((b + 1) % B) + 4]]))
        assert np.array_equal(cgot[b][0].round_polys, rp) and np.array_equal(cgot[b][1], ch)


# ---- 3. claimed sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,B", [(6, 3), (13, 3), (13, 6)])       # (13, 3): proofs in flight; (13, 6): the kernel's global rounds
def test_claimed_sums(zk, ora, log_n, B):
    evs = [ora.random_fr(1 << log_n, 8600 + 16 * log_n + b) for b in range(B)]
    polys = [zk.Multilinear(e) for e in evs]
    for g, p in zip(zk.Sumcheck.prove_batch(polys), polys):                                   # None: poly_sum() + prove()
        _same_basic(g, _basic_single(zk, p, "true"))
    for g, p in zip(zk.Sumcheck.prove_batch(polys, np.zeros((B, 4), dtype=np.uint64)), polys):  # zeros: prove() alone
        _same_basic(g, _basic_single(zk, p, None))
        assert zk.Fr.to_ints(g[0].sum) == [0]
    claimed = ora.random_fr(B, 8700 + log_n)                                                  # arbitrary: absorbed as given
    R = zk.Fr.MODULUS
    for b, g in enumerate(zk.Sumcheck.prove_batch(polys, claimed)):
        proof, ch = g
        assert np.array_equal(proof.sum, claimed[b])
        hs = ora.mle_half_sums(evs[b])
        assert np.array_equal(proof.univariate_poly[0], hs)
        d = hashlib.sha256(ora.fr_to_bytes_be(claimed[b]) + ora.fr_to_bytes_be(hs[0]) + ora.fr_to_bytes_be(hs[1])).digest()
        assert zk.Fr.to_ints(ch[0]) == [int.from_bytes(d, "big") % R]
        rp, och = T.sumcheck_with_claimed_sum(ora, evs[b], claimed[b])
        assert np.array_equal(proof.univariate_poly, rp) and np.array_equal(ch, och)
        _same_basic(g, _basic_single(zk, polys[b], claimed[b]))


# ---- 4. K = 1 composed against basic ------------------------------------------------------------------------------------------
def test_composed_k1_has_the_basic_provers_first_round_and_other_challenges(zk, ora):
    polys = [zk.Multilinear(ora.random_fr(1 << 7, 8800 + b)) for b in range(3)]
    basic = zk.Sumcheck.prove_batch(polys)
    comp = zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([p]) for p in polys])
    for (bp, bch), (cp, cch) in zip(basic, comp):
        assert np.array_equal(bp.univariate_poly[0], cp.round_polys[0])          # (lo, hi) = the values at t = 0, 1
        assert not np.array_equal(bch[0], cch[0])                                # only the basic transcript absorbed a sum first
        assert not np.array_equal(bp.univariate_poly[1], cp.round_polys[1])


# ---- 5. repeated pointers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [5, 13])
def test_repeated_tables_are_only_read(zk, ora, log_n):
    ev = ora.random_fr(1 << log_n, 8900 + log_n)
    poly = zk.Multilinear(ev)
    want = _basic_single(zk, poly)
    for g in zk.Sumcheck.prove_batch([poly] * 6):                                # one table in every proof
        _same_basic(g, want)
    other = zk.Multilinear(ora.random_fr(1 << log_n, 8950 + log_n))
    cps = [zk.ComposedMultilinear([poly] * 3), zk.ComposedMultilinear([poly, other, poly]), zk.ComposedMultilinear([poly] * 3)]
    got = zk.ComposedSumcheck.prove_batch(cps)                                   # one table K times within a proof, and across proofs
    for g, cp in zip(got, cps):
        _same_composed(g, zk.ComposedSumcheck(cp).prove())
    rp, ch = ora.composed_prove(np.stack([ev] * 3))
    assert np.array_equal(got[0][0].round_polys, rp) and np.array_equal(got[0][1], ch)
    assert np.array_equal(poly.to_numpy(), ev)                                   # the tables are unchanged


# ---- 6. structured tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [6, 13])
def test_structured_tables_basic(zk, ora, log_n):
    kinds = ["zero", "minus_one", "stored_max", "one_hot", "halves_cancel", "top"]
    evs =[T.fill(k, 1 << log_n, 9000 + log_n) for k in kinds]
    got = zk.Sumcheck.prove_batch([zk.Multilinear(e) for e in evs])
    for e, (proof, ch), kind in zip(evs, got, kinds):
        s, rp, och = ora.sumcheck_prove(e)
        assert np.array_equal(proof.sum, s) and np.array_equal(proof.univariate_poly, rp) and np.array_equal(ch, och), kind


@pytest.mark.parametrize("K,log_n", [(3, 5), (3, 11)])
def test_structured_tables_composed(zk, ora, K, log_n):
    kinds = ["zero", "minus_one", "stored_max", "one_hot", "top"]
    tabs = [np.stack([T.fill(f, 1 << log_n, 9100 + log_n + q) for q, f in enumerate(T.rotation(kinds, lead, K))]) for lead in kinds]
    tabs.append(np.stack([T.fill("minus_one", 1 << log_n, 0)] * K))             # every factor r - 1
    got = zk.ComposedSumcheck.prove_batch([_composed(zk, t) for t in tabs])
    for t, (proof, ch) in zip(tabs, got):
        rp, och = ora.composed_prove(t)
        assert np.array_equal(proof.round_polys, rp) and np.array_equal(ch, och)


# ---- 7. the golden vectors, grouped by shape and proven as batches ---------------------------------------------------------------
def test_golden_vectors_as_batches(zk, ora):
    G = json.load(open(os.path.join(HERE, "golden", "hot_path_vectors.json")))
    F = lambda hexes: zk.Fr.from_ints([int(h, 16) for h in hexes])   # noqa: E731
    hx = lambda arr: ["%064x" % v for v in ora.fr_to_ints(np.asarray(arr).reshape(-1, 4))]   # noqa: E731
    groups = {}
    for e in G["sumcheck"]:
        groups.setdefault(len(e["evals"]), []).append(e)
    assert groups
    for n, es in groups.items():
        got = zk.Sumcheck.prove_batch([zk.Multilinear(F(e["evals"])) for e in es])
        for e, (proof, ch) in zip(es, got):
            assert hx(proof.sum)[0] == e["sum"] and [hx(r) for r in proof.univariate_poly] == e["round_polys"] and hx(ch) == e["challenges"]
    groups = {}
    for e in G["composed"]:
        groups.setdefault((len(e["tables"]), len(e["tables"][0])), []).append(e)
    assert groups
    for shape, es in groups.items():
        got = zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([F(v) for v in e["tables"]]) for e in es])
        for e, (proof, ch) in zip(es, got):
            assert [hx(r) for r in proof.round_polys] == e["round_polys"] and hx(ch) == e["challenges"]
    # a golden group of ONE entry goes to the single prover: the same entries four times each are a batch for the kernel
    for e in G["sumcheck"]:
        if len(e["evals"]) > 1:
            for proof, ch in zk.Sumcheck.prove_batch([zk.Multilinear(F(e["evals"]))] * 4):
                assert hx(proof.sum)[0] == e["sum"] and [hx(r) for r in proof.univariate_poly] == e["round_polys"] and hx(ch) == e["challenges"]
    for e in G["composed"]:
        for proof, ch in zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([F(v) for v in e["tables"]])] * 4):
            assert [hx(r) for r in proof.round_polys] == e["round_polys"] and hx(ch) == e["challenges"]


# ---- 8. it really is one launch -------------------------------------------------------------------------------------------------
SINGLE_SCOPES = ("sumcheck_small", "composed_tail", "composed_round")


def _profiled(work, names):
    from zk_cryptography_amd import _native as N
    ctx = N.Context.get()
    N.check(N.lib().zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        result = work()
        counts = {}
        for name in names:
            cnt = C.c_uint64()
            N.check(N.lib().zkhip_profile_read(ctx.handle, name.encode(), None, C.byref(cnt), None), "profile_read")
            counts[name] = cnt.value
    finally:
        N.check(N.lib().zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    return result, counts


def test_launch_count_does_not_depend_on_the_batch(zk, ora):
    names = ("sumcheck_batch",) + SINGLE_SCOPES
    polys = [zk.Multilinear(ora.random_fr(1 << 8, 9300 + b)) for b in range(16)]
    # the basic prover's smallest batch on the kernel at this size is four (fewer measured faster as proofs in flight: scb_min_batch);
    # B = 2 is counted on the composed prover below, whose batches of two the kernel serves
    got16, c16 = _profiled(lambda: zk.Sumcheck.prove_batch(polys), names)
    got2, c2 = _profiled(lambda: zk.Sumcheck.prove_batch(polys[:4]), names)
    loop, cl = _profiled(lambda: [_basic_single(zk, p) for p in polys], names)
    assert c16["sumcheck_batch"] == c2["sumcheck_batch"] == 1 and cl["sumcheck_batch"] == 0, (c16, c2, cl)
    assert c16["sumcheck_small"] == c2["sumcheck_small"] == 0 and cl["sumcheck_small"] >= 16, (c16, c2, cl)
    for g, w in zip(got16, loop):
        _same_basic(g, w)
    for g, w in zip(got2, loop):
        _same_basic(g, w)
    cps = [zk.ComposedMultilinear([polys[b], polys[(b + 5) % 16]]) for b in range(16)]
    cgot16, c16 = _profiled(lambda: zk.ComposedSumcheck.prove_batch(cps), names)
    cgot2, c2 = _profiled(lambda: zk.ComposedSumcheck.prove_batch(cps[:2]), names)
    cloop, cl = _profiled(lambda: [zk.ComposedSumcheck(cp).prove() for cp in cps], names)
    assert c16["sumcheck_batch"] == c2["sumcheck_batch"] == 1 and cl["sumcheck_batch"] == 0, (c16, c2, cl)
    assert c16["composed_tail"] + c16["composed_round"] == c2["composed_tail"] + c2["composed_round"] == 0, (c16, c2)
    assert cl["composed_tail"] + cl["composed_round"] >= 16, cl
    for g, w in zip(cgot16, cloop):
        _same_composed(g, w)
    for g, w in zip(cgot2, cloop):
        _same_composed(g, w)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_shape_panics(zk, ora):
    a, b = zk.Multilinear(ora.random_fr(8, 9400)), zk.Multilinear(ora.random_fr(4, 9401))
    assert zk.Sumcheck.prove_batch([]) == [] and zk.ComposedSumcheck.prove_batch([]) == []
    with pytest.raises(AssertionError):        # mixed lengths
        zk.Sumcheck.prove_batch([a, b])
    with pytest.raises(AssertionError):        # not a power of two: Multilinear::new
        zk.Sumcheck.prove_batch([a, ora.random_fr(6, 9402)])
    with pytest.raises(AssertionError):        # one claimed sum per table
        zk.Sumcheck.prove_batch([a, a], np.zeros((3, 4), dtype=np.uint64))
    with pytest.raises(AssertionError):        # mixed K
        zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([a, a]), zk.ComposedMultilinear([a])])
    with pytest.raises(AssertionError):        # mixed lengths across proofs
        zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([a, a]), zk.ComposedMultilinear([b, b])])
    with pytest.raises(IndexError):            # no tables: `self.polys[0]`, as prove()
        zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([])])
    with pytest.raises(IndexError):
        zk.ComposedSumcheck(zk.ComposedMultilinear([])).prove()
    from zk_cryptography_amd._native import ZkhipError
    with pytest.raises(ZkhipError):            # six tables: what prove() refuses
        zk.ComposedSumcheck.prove_batch([zk.ComposedMultilinear([a] * 6)] * 2)


def test_raw_refusals_leave_the_outputs_alone(zk, ora):
    from zk_cryptography_amd import _native as N
    lib = N.lib()
    B, log_n = 3, 4
    n = 1 << log_n
    polys = [zk.Multilinear(ora.random_fr(n, 9500 + b)) for b in range(B)]
    ctx = polys[0]._ctx
    ptrs = (C.c_void_p * (2 * B))(*[p.evaluations.data_ptr() for p in polys] * 2)
    holed = (C.c_void_p * (2 * B))(*([p.evaluations.data_ptr() for p in polys] * 2)[:-1] + [None])
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    s = np.full((B, 4), FILL)
    rp = np.full((B, log_n, 3, 4), FILL)
    ch = np.full((B, log_n, 4), FILL)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    sz, u32 = C.c_size_t, C.c_uint32

    def basic(h, batch, ptrs, n, s_, rp_, ch_):
        return lib.zkhip_sumcheck_prove_batch(h, u32(batch), ptrs, sz(n), None, s_, rp_, ch_)

    def composed(h, batch, ptrs, k, n, rp_, ch_):
        return lib.zkhip_composed_prove_batch(h, u32(batch), ptrs, u32(k), sz(n), rp_, ch_)

    assert basic(None, B, ptrs, n, vp(s), vp(rp), vp(ch)) == N.ERR_ARG
    assert basic(ctx.handle, B, None, n, vp(s), vp(rp), vp(ch)) == N.ERR_ARG
    assert basic(ctx.handle, 2 * B, holed, n, vp(s), vp(rp), vp(ch)) == N.ERR_ARG
    assert basic(ctx.handle, B, ptrs, n, None, vp(rp), vp(ch)) == N.ERR_ARG
    assert basic(ctx.handle, B, ptrs, n, vp(s), None, vp(ch)) == N.ERR_ARG
    assert basic(ctx.handle, B, ptrs, n, vp(s), vp(rp), None) == N.ERR_ARG
    assert basic(ctx.handle, B, ptrs, n - 1, vp(s), vp(rp), vp(ch)) == N.ERR_SHAPE
    assert basic(ctx.handle, 0, ptrs, n, vp(s), vp(rp), vp(ch)) == N.ZKHIP_OK
    assert composed(None, B, ptrs, 2, n, vp(rp), vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, B, None, 2, n, vp(rp), vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, B, holed, 2, n, vp(rp), vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, B, ptrs, 0, n, vp(rp), vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, 1, ptrs, 6, n, vp(rp), vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, B, ptrs, 2, n, None, vp(ch)) == N.ERR_ARG
    assert composed(ctx.handle, B, ptrs, 2, n, vp(rp), None) == N.ERR_ARG
    assert composed(ctx.handle, B, ptrs, 2, n + 2, vp(rp), vp(ch)) == N.ERR_SHAPE
    assert composed(ctx.handle, 0, ptrs, 2, n, vp(rp), vp(ch)) == N.ZKHIP_OK
    # while a proof is in flight the result slots are taken: the basic batch is refused as the basic single call is
    sc = zk.Sumcheck(polys[0])
    pending = sc.prove_begin()
    try:
        assert basic(ctx.handle, B, ptrs, n, vp(s), vp(rp), vp(ch)) == N.ERR_BUSY
        with pytest.raises(N.ZkhipError) as ei:
            zk.Sumcheck.prove_batch(polys)
        assert ei.value.status == N.ERR_BUSY
    finally:
        want = pending.wait()
    for a in (s, rp, ch):
        assert (a == FILL).all()
    # the proof that was in flight absorbed the default sum: the batch with zeros gives it again, now that the slots are free
    _same_basic(zk.Sumcheck.prove_batch(polys, np.zeros((B, 4), dtype=np.uint64))[0], want)
