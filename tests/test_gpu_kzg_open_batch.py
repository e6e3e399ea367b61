"""GPU parity of MultilinearKZG.open_batch (zkhip_kzg_open_batch): a batch of openings against one SRS equals the CPU oracle's naive
opening and, bit for bit, the single calls -- on the batched short path (level tables, at most 2^12 entries), across its chunk bound,
and on the sequential fallback of every other size and configuration."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 64          # csrc/msm.hip OPEN_BATCH_CHUNK: openings per chunk of the batched short path
BATCH_SCOPES = ("open_batch_steps", "open_batch_planes", "open_batch_reduce", "open_batch_fold")


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _assert_bit_identical(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g.evaluation, w.evaluation)
        assert len(g.proofs) == len(w.proofs)
        assert [p.infinity for p in g.proofs] == [p.infinity for p in w.proofs]
        assert np.array_equal(np.stack([p.xy for p in g.proofs]), np.stack([p.xy for p in w.proofs]))


def _singles(zk, polys, points, srs, **kw):
    return [zk.MultilinearKZG.open(p, z, srs, **kw) for p, z in zip(polys, points)]


def _random_batch(zk, ora, n_vars, batch, seed):
    polys = [zk.Multilinear(ora.random_fr(1 << n_vars, seed + 10 * b)) for b in range(batch)]
    points = [ora.random_fr(n_vars, seed + 10 * b + 1) for b in range(batch)]
    return polys, points


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vars", [2, 3, 5, 8])       # 2: the smallest legal shape, its last round a commit of one point
def test_open_batch_matches_naive_oracle(zk, ora, n_vars):
    B = 3
    tau = ora.random_fr(n_vars, 5100 + n_vars)
    vals = [ora.random_fr(1 << n_vars, 5200 + 16 * n_vars + b) for b in range(B)]
    points = [ora.random_fr(n_vars, 5300 + 16 * n_vars + b) for b in range(B)]
    srs = zk.TrustedSetup.setup(tau).precompute_open()
    got = zk.MultilinearKZG.open_batch([zk.Multilinear(v) for v in vals], points, srs)
    assert len(got) == B
    srs_g1 = ora.kzg_multilinear_srs_g1(tau)
    for b in range(B):
        want_ev, want_proofs = ora.kzg_open(vals[b], points[b], srs_g1)
        assert np.array_equal(got[b].evaluation, want_ev)
        assert len(got[b].proofs) == n_vars
        for g, w in zip(got[b].proofs, want_proofs):
            a = ora.g1_to_affine(w)
            assert g.infinity == bool(a[12])
            if not g.infinity:
                assert np.array_equal(g.xy, a[:12])


# ---- 2. against the single call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vars,batch", [(8, 1), (8, 2), (8, 17),     # 17 x 8 = 136 problems: well past MSM_SMALL_PROBS, B a multiple of nothing
                                          (12, 5),                      # MSM_SMALL_MAX itself, twelve rounds
                                          (13, 3)])                     # the first size off the short path (tables present, too large)
def test_open_batch_equals_single_calls(zk, ora, n_vars, batch):
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 5400 + n_vars)).precompute_open()
    assert srs.level_tables is not None
    polys, points = _random_batch(zk, ora, n_vars, batch, 5500 + 100 * n_vars)
    _assert_bit_identical(zk.MultilinearKZG.open_batch(polys, points, srs), _singles(zk, polys, points, srs))


def test_open_batch_plain_path_equals_single_calls(zk, ora):
    """No level tables and the SRS folded per call: the bucket pipeline, one opening after another."""
    n_vars, batch = 10, 4
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 5600))
    polys, points = _random_batch(zk, ora, n_vars, batch, 5610)
    got = zk.MultilinearKZG.open_batch(polys, points, srs, cache_folded_srs=False)
    assert srs.level_tables is None
    _assert_bit_identical(got, _singles(zk, polys, points, srs, cache_folded_srs=False))


# ---- 3. one polynomial at many points -----------------------------------------------------------------------------------------
def test_open_batch_one_polynomial_at_many_points(zk, ora):
    n_vars, batch = 6, 9
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 5700))
    vals = ora.random_fr(1 << n_vars, 5701)
    poly = zk.Multilinear(vals)
    points = [ora.random_fr(n_vars, 5710 + b) for b in range(batch)]
    got = zk.MultilinearKZG.open_batch([poly] * batch, points, srs)
    assert np.array_equal(poly.to_numpy(), vals)                # the table is only read
    _assert_bit_identical(got, _singles(zk, [poly] * batch, points, srs))
    assert len({g.evaluation.tobytes() for g in got}) == batch  # nine different openings, not one nine times


# ---- 4. degenerate data inside a batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_tau", [False, True])
def test_open_batch_degenerate_data(zk, ora, zero_tau):
    """Beside a random table: the zero polynomial (every proof at infinity), tiny values (sparse top digits), one repeated quotient
    value, all -1 (negative digits throughout), a point with a zero coordinate; once more on an SRS half of which is at infinity."""
    n_vars, n = 10, 1 << 10
    tau = np.ascontiguousarray(ora.random_fr(n_vars, 5800))
    if zero_tau:
        tau[0] = zk.Fr.from_int(0)
    rng = np.random.default_rng(5801)
    half = zk.Fr.to_ints(ora.random_fr(n // 2, 5802))
    tables = [
        ora.random_fr(n, 5803),
        zk.Fr.from_ints([0] * n),
        zk.Fr.from_ints([int(v) for v in rng.integers(0, 4, n)]),                                            # small
        zk.Fr.from_ints(half + [v + 0x1234567890abcdef1234567890abcdef1234567890abcdef for v in half]),      # equal
        zk.Fr.from_ints([0] * (n // 2) + [-1] * (n // 2)),                                                   # minus_one
        ora.random_fr(n, 5804),
    ]
    points = [np.ascontiguousarray(ora.random_fr(n_vars, 5810 + b)) for b in range(len(tables))]
    points[5][3] = zk.Fr.from_int(0)
    srs = zk.TrustedSetup.setup(tau)
    polys = [zk.Multilinear(t) for t in tables]
    got = zk.MultilinearKZG.open_batch(polys, points, srs)
    assert srs.level_tables is not None                         # a small SRS builds them on first use, as `open` does
    _assert_bit_identical(got, _singles(zk, polys, points, srs))
    for g, t, z in zip(got, tables, points):
        assert np.array_equal(g.evaluation, ora.mle_evaluation(np.ascontiguousarray(t), z))
    assert all(p.infinity for p in got[1].proofs) and not all(p.infinity for p in got[0].proofs)


# ---- 5. chunking --------------------------------------------------------------------------------------------------------------
def test_open_batch_across_the_chunk_bound(zk, ora):
    """More openings than one chunk of the short path holds (a full chunk and a short one): the boundary does not show."""
    n_vars, batch = 3, CHUNK + 6
    tau = ora.random_fr(n_vars, 5900)
    srs = zk.TrustedSetup.setup(tau)
    tabs =[zk.Multilinear(ora.random_fr(1 << n_vars, 5901 + k)) for k in range(5)]
    polys = [tabs[b % 5] for b in range(batch)]
    points = [ora.random_fr(n_vars, 5910 + b) for b in range(batch)]
    got = zk.MultilinearKZG.open_batch(polys, points, srs)
    _assert_bit_identical(got, _singles(zk, polys, points, srs))
    # (and against the oracle on both sides of the boundary)
    srs_g1 = ora.kzg_multilinear_srs_g1(tau)
    for b in (CHUNK - 1, CHUNK, batch - 1):
        want_ev, want_proofs = ora.kzg_open(polys[b].to_numpy(), points[b], srs_g1)
        assert np.array_equal(got[b].evaluation, want_ev)
        for g, w in zip(got[b].proofs, want_proofs):
            a = ora.g1_to_affine(w)
            assert g.infinity == bool(a[12]) and (g.infinity or np.array_equal(g.xy, a[:12]))


# ---- 6. the verifier accepts --------------------------------------------------------------------------------------------------
def test_open_batch_proofs_verify(zk, ora):
    n_vars, batch = 4, 8
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 6000), g2=True)
    polys, points = _random_batch(zk, ora, n_vars, batch, 6010)
    commits = [zk.MultilinearKZG.commitment(p, srs) for p in polys]
    proofs = zk.MultilinearKZG.open_batch(polys, points, srs)
    assert zk.MultilinearKZG.verify_batch(commits, points, proofs, srs).all()
    bad = 5
    proofs[bad] = zk.MultilinearKZGProof(zk.Fr.from_int(zk.Fr.to_ints(proofs[bad].evaluation)[0] + 1), proofs[bad].proofs)
    ok = zk.MultilinearKZG.verify_batch(commits, points, proofs, srs)
    assert [bool(v) for v in ok] == [b != bad for b in range(batch)]


# ---- 7. it really is one batch ------------------------------------------------------------------------------------------------
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


def test_open_batch_launch_count_does_not_depend_on_the_batch(zk, ora):
    n_vars = 8
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 6100)).precompute_open()
    polys, points = _random_batch(zk, ora, n_vars, 16, 6110)
    names = BATCH_SCOPES + ("msm_small", "msm_accumulate")
    got16, c16 = _profiled(lambda: zk.MultilinearKZG.open_batch(polys, points, srs), names)
    got2, c2 = _profiled(lambda: zk.MultilinearKZG.open_batch(polys[:2], points[:2], srs), names)
    loop, cl = _profiled(lambda: _singles(zk, polys, points, srs), names)
    for name in BATCH_SCOPES:
        assert c16[name] == c2[name] == 1 and cl[name] == 0, (name, c16, c2, cl)
    assert c16["msm_small"] == c2["msm_small"] == 0 and cl["msm_small"] == 16      # the loop pays the short path once per opening
    assert c16["msm_accumulate"] == c2["msm_accumulate"] == cl["msm_accumulate"] == 0
    _assert_bit_identical(got16, loop)
    _assert_bit_identical(got2, loop[:2])


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_open_batch_shape_panics(zk, ora):
    srs = zk.TrustedSetup.setup(zk.Fr.from_ints([2, 3, 4]))
    poly = zk.Multilinear(zk.Fr.from_ints([0, 7, 0, 5, 0, 7, 4, 9]))
    z = zk.Fr.from_ints([5, 9, 6])
    assert len(zk.MultilinearKZG.open_batch([poly, poly], [z, z], srs)) == 2
    with pytest.raises(AssertionError):    # lists of unequal length
        zk.MultilinearKZG.open_batch([poly, poly], [z], srs)
    with pytest.raises(AssertionError):    # polynomials of unequal size
        zk.MultilinearKZG.open_batch([poly, zk.Multilinear(zk.Fr.from_ints([0, 7, 0, 5]))], [z, z], srs)
    with pytest.raises(AssertionError):    # a point vector of the wrong length: one of them, and all of them (evaluation_form.rs:163-167)
        zk.MultilinearKZG.open_batch([poly, poly], [z, zk.Fr.from_ints([5, 9])], srs)
    with pytest.raises(AssertionError):
        zk.MultilinearKZG.open_batch([poly, poly], [zk.Fr.from_ints([5, 9])] * 2, srs)
    with pytest.raises(AssertionError):    # one variable: `variable_index - 1` underflows in the reference (multilinear_kzg.rs:73)
        one = zk.Multilinear(zk.Fr.from_ints([3, 4]))
        zk.MultilinearKZG.open_batch([one, one], [zk.Fr.from_ints([5])] * 2, zk.TrustedSetup.setup(zk.Fr.from_ints([2])))


def test_open_batch_raw_refusals_leave_the_outputs_alone(zk, ora):
    import torch
    from zk_cryptography_amd import _native as N
    lib = N.lib()
    n_vars, batch = 6, 3
    n = 1 << n_vars
    srs = zk.TrustedSetup.setup(ora.random_fr(n_vars, 6200)).precompute_open()
    other = zk.TrustedSetup.setup(ora.random_fr(n_vars + 1, 6201)).precompute_open()      # level tables of another size
    fxy, finf = srs.folded()
    evs = [torch.from_numpy(ora.random_fr(n, 6210 + b).view(np.int64)).cuda() for b in range(batch)]
    z = np.ascontiguousarray(np.stack([ora.random_fr(n_vars, 6220 + b) for b in range(batch)]))
    ptrs = (C.c_void_p * batch)(*[e.data_ptr() for e in evs])
    ctx = N.Context.get(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def buffers():
        return np.full((batch, 4), 0xA5A5A5A5A5A5A5A5, np.uint64), np.full((batch * n_vars, 12), 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(batch * n_vars, 0xC3, np.uint8)

    def open_batch(count, tables, ev, pxy, pinf):
        return lib.zkhip_kzg_open_batch(ctx.handle, C.c_uint32(count), ptrs, C.c_size_t(n), p(z), C.c_size_t(n_vars), N.ptr(srs.powers_of_tau_in_g1),
                                        N.ptr(srs.inf), C.c_size_t(n), N.ptr(fxy), N.ptr(finf), N.ptr(tables), p(ev), p(pxy), p(pinf))
    pattern = buffers()
    # batch = 0: OK, nothing touched
    out = buffers()
    assert open_batch(0, srs._level_tables, *out) == N.ZKHIP_OK
    assert all(np.array_equal(a, b) for a, b in zip(out, pattern))
    # level tables built for another size: the single call's status, nothing touched
    h_ev, pxy, pinf = np.zeros(4, np.uint64), np.zeros((n_vars, 12), np.uint64), np.zeros(n_vars, np.uint8)
    single = lib.zkhip_kzg_open_tables(ctx.handle, N.ptr(evs[0]), C.c_size_t(n), p(z), C.c_size_t(n_vars), N.ptr(srs.powers_of_tau_in_g1), N.ptr(srs.inf),
                                       C.c_size_t(n), N.ptr(fxy), N.ptr(finf), N.ptr(other._level_tables), p(h_ev), p(pxy), p(pinf))
    assert single == N.ERR_ARG
    out = buffers()
    assert open_batch(batch, other._level_tables, *out) == single
    assert all(np.array_equal(a, b) for a, b in zip(out, pattern))
    # the same call with the right tables goes through and equals the mirror
    out = buffers()
    assert open_batch(batch, srs._level_tables, *out) == N.ZKHIP_OK
    want = [zk.MultilinearKZG.open(zk.Multilinear(e), z[b], srs) for b, e in enumerate(evs)]
    for b in range(batch):
        assert np.array_equal(out[0][b], want[b].evaluation)
        assert np.array_equal(out[1][b * n_vars:(b + 1) * n_vars], np.stack([q.xy for q in want[b].proofs]))
        assert np.array_equal(out[2][b * n_vars:(b + 1) * n_vars], np.array([q.infinity for q in want[b].proofs], np.uint8))
