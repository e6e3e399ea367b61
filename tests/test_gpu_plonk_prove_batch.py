"""GPU: PlonkProver.prove_batch / zkhip_plonk_prove_batch against the single call zkhip_plonk_prove on the same key, bit for bit -- the
nine points with their flags, the six evaluations and the six challenges of every proof -- and, at one shape, against the independent
model of tests/plonk_model.py and the batched verifier.  A batch holds witnesses of ONE structure with a value stream per witness
(random_circuit's second generator) and a blinding of its own per proof.  Shapes: n = 4 is the one order whose coset has D / n = 8;
B = 64 / 65 / 67 are a full chunk and a full chunk followed by a chunk of one and of three; the memory-bound case is the smallest order whose chunk is
cut by the work-area budget; n = 1024 / 2048 give the grand product one and two workgroups per proof, n = 2048 / 4096 are the last
order on the short commit path and the first off it; n = 64 under ZKHIP_PLONK_CACHE_BUDGET=0 is the key without a coset cache."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402
from test_gpu_plonk import blinding, package_inputs, proof_dict, srs_for  # noqa: E402

pytestmark = pytest.mark.gpu
R = PL.R
VP = C.c_void_p
OK, ERR_SHAPE, ERR_ARG, ERR_BUSY = 0, -2, -4, -6


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


class Batch:
    """one structure of n rows with `count` witnesses on the device, the key, and the single proofs (computed once, on demand)"""

    def __init__(self, zk, n, count, seed=None, srs=None, uncached=False):
        from zk_cryptography_amd import plonk
        seed = n if seed is None else seed
        self.n, self.tau, self.seed = n, 17 + seed, seed
        self.srs = srs if srs is not None else zk.UnivariateKZG.generate_srs(zk.Fr.from_int(self.tau), n + 5, g2=True)
        self.wits = []
        for b in range(count):
            cpi, wit = PL.random_circuit(n, random.Random(seed), random.Random(900 + 7 * seed + b))
            assert b == 0 or cpi == self.cpi
            self.cpi = cpi
            self.wits.append(wit)
        self.c, _ = package_inputs(zk, self.cpi, self.wits[0])
        before = os.environ.get("ZKHIP_PLONK_CACHE_BUDGET")
        if uncached:
            os.environ["ZKHIP_PLONK_CACHE_BUDGET"] = "0"
        try:
            self.key = plonk._key_for(self.c, self.srs)
        finally:
            if uncached:
                if before is None:
                    del os.environ["ZKHIP_PLONK_CACHE_BUDGET"]
                else:
                    os.environ["ZKHIP_PLONK_CACHE_BUDGET"] = before
        self.cols = [[plonk._column(w[f]) for f in ("a", "b", "c", "public_poly")] for w in self.wits]
        self.bl = [blinding(1000 * seed + b) for b in range(count)]
        self._single = {}

    def blinding_limbs(self, scalars):
        from zk_cryptography_amd import Fr
        return Fr.from_ints([int(v) for v in scalars])

    def single(self, b, cols=None, bl=None):
        """zkhip_plonk_prove of witness b -> (status, xy, inf, ev, ch)"""
        from zk_cryptography_amd import _native as N
        cached = cols is None and bl is None
        if cached and b in self._single:
            return self._single[b]
        cols = self.cols[b] if cols is None else cols
        limbs = self.blinding_limbs(self.bl[b]) if bl is None else bl
        xy, inf = np.zeros((9, 12), dtype=np.uint64), np.zeros(9, dtype=np.uint8)
        ev, ch = np.zeros((6, 4), dtype=np.uint64), np.zeros((6, 4), dtype=np.uint64)
        self.key.ctx.sync_stream()
        st = N.lib().zkhip_plonk_prove(self.key.handle, N.ptr(cols[0]), N.ptr(cols[1]), N.ptr(cols[2]), N.ptr(cols[3]), limbs.ctypes.data_as(VP),
                                       xy.ctypes.data_as(VP), inf.ctypes.data_as(VP), ev.ctypes.data_as(VP), ch.ctypes.data_as(VP))
        out = (st, xy, inf, ev, ch)
        if cached:
            self._single[b] = out
        return out

    def batch(self, which, cols=None, bl=None, fill=0, null_entry=None, count=None):
        """zkhip_plonk_prove_batch of the witnesses `which` -> (status, xy, inf, ev, ch, per-proof status); outputs start as `fill` bytes"""
        from zk_cryptography_amd import _native as N
        B = len(which)
        cols = [self.cols[b] for b in which] if cols is None else cols
        limbs = np.stack([self.blinding_limbs(self.bl[b]) for b in which]) if bl is None else bl
        ptrs = []
        for j in range(4):
            col = [row[j].data_ptr() for row in cols]
            if null_entry is not None and null_entry[0] == j:
                col[null_entry[1]] = None
            ptrs.append((C.c_void_p * max(B, 1))(*col))
        xy, inf = np.full((max(B, 1), 9, 12), fill * 0x0101010101010101, dtype=np.uint64), np.full((max(B, 1), 9), fill, dtype=np.uint8)
        ev, ch = np.full((max(B, 1), 6, 4), fill * 0x0101010101010101, dtype=np.uint64), np.full((max(B, 1), 6, 4), fill * 0x0101010101010101, dtype=np.uint64)
        status = np.full(4 * max(B, 1), fill, dtype=np.uint8).view(np.int32)
        self.key.ctx.sync_stream()
        st = N.lib().zkhip_plonk_prove_batch(self.key.handle, C.c_uint32(B if count is None else count), ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                             limbs.ctypes.data_as(VP), xy.ctypes.data_as(VP), inf.ctypes.data_as(VP), ev.ctypes.data_as(VP),
                                             ch.ctypes.data_as(VP), status.ctypes.data_as(VP))
        return st, xy, inf, ev, ch, status

    def chunk(self):
        from zk_cryptography_amd import _native as N
        return int(N.lib().zkhip_plonk_batch_chunk(self.key.handle))

    def objects(self, zk, which):
        return [zk.Witness(*(self.wits[b][f] for f in ("a", "b", "c", "public_poly"))) for b in which]


_batches = {}


def batch_of(zk, n, count, **kw):
    tag = (n, tuple(sorted(kw.items())))
    if tag not in _batches or len(_batches[tag].wits) < count:
        _batches[tag] = Batch(zk, n, count, **kw)
    return _batches[tag]


def assert_equals_singles(bt, which, got):
    st, xy, inf, ev, ch, status = got
    assert st == OK and not status[:len(which)].any()
    for i, b in enumerate(which):
        s_st, s_xy, s_inf, s_ev, s_ch = bt.single(b)
        assert s_st == OK
        assert np.array_equal(xy[i], s_xy) and np.array_equal(inf[i], s_inf), (i, b)
        assert np.array_equal(ev[i], s_ev) and np.array_equal(ch[i], s_ch), (i, b)


@pytest.mark.parametrize("n", [4, 8, 64])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_every_proof_equals_the_single_call(zk, n, B):
    bt = batch_of(zk, n, 5)
    which = list(range(B))
    assert_equals_singles(bt, which, bt.batch(which))
    if (n, B) == (8, 2):                                                        # and the model's proofs, which the batched verifier accepts
        prover = zk.PlonkProver(bt.c, bt.srs)
        mark = dict(prover.random_number)
        proofs = prover.prove_batch(bt.objects(zk, which), blindings=[bt.bl[b] for b in which])
        assert prover.random_number == mark                                     # prove_batch leaves the prover's own state alone
        srs4 = srs_for(zk, bt.tau, n)                                           # the model's SRS: the same tau, more points than the prover needs
        for b, proof in zip(which, proofs):
            assert proof_dict(proof) == PL.prove(bt.cpi, bt.wits[b], bt.tau, bt.bl[b], n_srs=4 * n + 1), b
        v = zk.VerifierPreprocessedInput.vpi(srs4, bt.c)
        assert zk.PlonkVerifier.verify_batch(n, proofs, srs4, v, [bt.wits[b]["public_poly"] for b in which]) == [True] * B


@pytest.mark.parametrize("B", [64, 65, 67])
def test_a_full_chunk_and_what_comes_behind_it(zk, B):
    """one full chunk; a chunk of one behind it, which is the single prover; a chunk of three behind it, which is the batched rounds again"""
    bt = batch_of(zk, 4, 67)
    assert bt.chunk() == 64
    which = list(range(B))
    assert_equals_singles(bt, which, bt.batch(which))


def test_a_chunk_cut_by_the_work_area_budget(zk):
    """the smallest order whose chunk the budget cuts below 64, with one proof more than a chunk: a full chunk, then a chunk of one"""
    sizes = (1 << 12, 1 << 13, 1 << 14)
    for n in sizes:
        bt = batch_of(zk, n, 1)
        if bt.chunk() < 64:
            break
    else:
        pytest.fail("no order of %s has a chunk below 64: lower PLONK_BATCH_BUDGET or add sizes" % (sizes,))
    chunk = bt.chunk()
    assert 1 <= chunk < 64
    bt = batch_of(zk, n, 2)                                                     # two witnesses, taken in turns, each with a blinding of its own
    which = [b % 2 for b in range(chunk + 1)]
    bls = [blinding(5000 + i) for i in range(chunk + 1)]
    limbs = np.stack([bt.blinding_limbs(s) for s in bls])
    st, xy, inf, ev, ch, status = bt.batch(which, bl=limbs)
    assert st == OK and not status.any()
    for i in (0, 1, chunk - 1, chunk):                                          # both ends of the full chunk and the chunk of one
        s_st, s_xy, s_inf, s_ev, s_ch = bt.single(which[i], bl=limbs[i])
        assert s_st == OK and np.array_equal(xy[i], s_xy) and np.array_equal(inf[i], s_inf) and np.array_equal(ev[i], s_ev) and np.array_equal(ch[i], s_ch), i
    assert len({xy[i].tobytes() for i in range(chunk + 1)}) == chunk + 1        # every blinding made a proof of its own


@pytest.mark.parametrize("n,uncached", [(1024, False), (2048, False), (4096, False), (64, True)])
def test_kernel_and_path_edges(zk, n, uncached):
    bt = batch_of(zk, n, 3, uncached=True, seed=n + 1) if uncached else batch_of(zk, n, 3)
    assert (bt.srs.table is not None) == (n + 6 <= bt.srs.SMALL_SRS)            # the short commit path is taken up to n = 2048
    assert_equals_singles(bt, [0, 1, 2], bt.batch([0, 1, 2]))
    if uncached:                                                                # the same proofs as a key with its coset cache
        cached = batch_of(zk, n, 3, seed=n + 1, srs=bt.srs)
        assert cached.key is not bt.key
        for b in range(3):
            for got, want in zip(bt.single(b), cached.single(b)):
                assert np.array_equal(got, want)


def test_refused_proofs_leave_the_others_alone(zk):
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    n, B = 8, 6
    bt = batch_of(zk, n, B)
    wits = [dict(w) for w in bt.wits[:B]]
    row = next(i for i in range(n) if bt.cpi["q_o"][i] % R)                     # a row whose gate depends on c
    wits[0]["c"] = [(v + 1) % R if i == row else v for i, v in enumerate(wits[0]["c"])]
    assert not PL.gate_identity_holds(bt.cpi, wits[0])
    # a padding row has no selector, so any value keeps its gate; but its cells are wired to every other unused cell, which hold zero:
    # the copy constraint breaks alone and the accumulator does not close
    mixed = dict(wits[3], a=list(wits[3]["a"][:n - 1]) + [1])
    assert wits[3]["a"][n - 1] == 0 and PL.gate_identity_holds(bt.cpi, mixed)
    wits[3] = mixed
    cols = [[plonk._column(w[f]) for f in ("a", "b", "c", "public_poly")] for w in wits]
    limbs = np.stack([bt.blinding_limbs(bt.bl[b]) for b in range(B)])
    limbs[5, 7] = [(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]      # the limbs of r itself
    for b in (0, 3):                                                            # what the single call says of the two witnesses
        assert bt.single(b, cols=cols[b], bl=limbs[b])[0] == ERR_ARG
    assert bt.single(5, bl=limbs[5])[0] == ERR_ARG
    st, xy, inf, ev, ch, status = bt.batch(list(range(B)), cols=cols, bl=limbs, fill=0xA5)
    assert st == ERR_ARG
    assert list(status) == [ERR_ARG, OK, OK, ERR_ARG, OK, ERR_ARG]
    for b in (0, 3, 5):
        assert not xy[b].any() and not inf[b].any() and not ev[b].any() and not ch[b].any()
    for b in (1, 2, 4):
        s_st, s_xy, s_inf, s_ev, s_ch = bt.single(b)
        assert s_st == OK and np.array_equal(xy[b], s_xy) and np.array_equal(inf[b], s_inf) and np.array_equal(ev[b], s_ev) and np.array_equal(ch[b], s_ch)
    objects = [zk.Witness(w["a"], w["b"], w["c"], w["public_poly"]) for w in wits]
    bls = [list(s) for s in bt.bl[:B]]
    bls[5][7] = R
    prover = zk.PlonkProver(bt.c, bt.srs)
    with pytest.raises(N.ZkhipError) as e:
        prover.prove_batch(objects, blindings=bls)
    assert e.value.status == N.ERR_ARG and "[0, 3, 5]" in str(e.value)
    proofs = prover.prove_batch(objects, blindings=bls, allow_failures=True)
    assert [p is None for p in proofs] == [True, False, False, True, False, True]
    for b in (1, 2, 4):
        assert proof_dict(proofs[b]) == proof_dict(prover.prove(objects[b], blinding=bls[b]))


def test_one_witness_twice(zk):
    n = 8
    bt = batch_of(zk, n, 2)
    same = np.stack([bt.blinding_limbs(bt.bl[0])] * 2)
    st, xy, inf, ev, ch, status = bt.batch([0, 0], bl=same)
    assert st == OK and np.array_equal(xy[0], xy[1]) and np.array_equal(ev[0], ev[1]) and np.array_equal(ch[0], ch[1])
    assert np.array_equal(xy[0], bt.single(0)[1])
    prover = zk.PlonkProver(bt.c, bt.srs)
    w = bt.objects(zk, [0])[0]
    p1, p2 = prover.prove_batch([w, w], blindings=[bt.bl[0], bt.bl[1]])
    assert proof_dict(p1) != proof_dict(p2) and p1.as_commitment != p2.as_commitment
    srs4 = srs_for(zk, bt.tau, n)
    v = zk.VerifierPreprocessedInput.vpi(srs4, bt.c)
    assert zk.PlonkVerifier.verify_batch(n, [p1, p2], srs4, v, [w.public_poly, w.public_poly]) == [True, True]
    fresh = prover.prove_batch([w, w])                                          # default blinding: fresh scalars per proof
    assert proof_dict(fresh[0]) != proof_dict(fresh[1])


def _records(bt, which):
    """the names the library's profile recorded during one batch call, in host enqueue order"""
    from zk_cryptography_amd import _native as N
    ctx, lib, mx = bt.key.ctx, N.lib(), 1024
    N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        got = bt.batch(which)
        names, st, sp, cnt = C.create_string_buffer(32 * mx), (C.c_double * mx)(), (C.c_double * mx)(), C.c_uint32(0)
        N.check(lib.zkhip_profile_timeline(ctx.handle, mx, names, st, sp, C.byref(cnt)), "profile_timeline")
    finally:
        N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    assert got[0] == OK and 0 < cnt.value < mx
    return [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(cnt.value)]


def test_the_launches_of_a_chunk_do_not_depend_on_its_proofs(zk):
    bt = batch_of(zk, 8, 7)
    assert bt.srs.table is not None                                             # the short commit path
    two, seven = _records(bt, [0, 1]), _records(bt, list(range(7)))
    assert two == seven
    assert two.count("plonk_batch_commit_planes") == 4 and two.count("plonk_batch_commit_reduce") == 4     # one chain per round that commits
    one = _records(bt, [0])                                                     # a chunk of one is the single prover: none of the batch's launches
    assert not [name for name in one if name.startswith("plonk_batch")]


def test_refusals_of_the_whole_call_touch_nothing(zk):
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import kzg
    bt = batch_of(zk, 8, 3)

    def untouched(got, fill=0x5A):
        _, xy, inf, ev, ch, status = got
        word = np.uint64(fill * 0x0101010101010101)
        return (xy == word).all() and (inf == fill).all() and (ev == word).all() and (ch == word).all() and (status.view(np.uint8) == fill).all()

    for column in range(4):
        got = bt.batch([0, 1, 2], fill=0x5A, null_entry=(column, 1))
        assert got[0] == ERR_ARG and untouched(got)
    got = bt.batch([0, 1, 2], fill=0x5A, count=65536)
    assert got[0] == ERR_SHAPE and untouched(got)
    got = bt.batch([0, 1, 2], fill=0x5A, count=0)
    assert got[0] == OK and untouched(got)
    assert N.lib().zkhip_plonk_prove_batch(None, C.c_uint32(0), None, None, None, None, None, None, None, None, None, None) == ERR_ARG
    scalars = bt.cols[0][0]
    pending = kzg._commit_begin(bt.srs.powers_of_tau_in_g1, bt.srs.inf, len(bt.srs), scalars, bt.n, False)    # holds the context's workspace
    try:
        got = bt.batch([0, 1, 2], fill=0x5A)
        assert got[0] == ERR_BUSY and untouched(got)
    finally:
        pending.wait()
    assert_equals_singles(bt, [0, 1, 2], bt.batch([0, 1, 2]))                   # and proves again once the commit has ended
