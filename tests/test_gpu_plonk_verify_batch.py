"""GPU: PlonkVerifier.verify_batch / zkhip_plonk_verify_batch against the independent model of tests/plonk_model.py and against the
single call.  Every comparison is bit for bit: the G1 arguments of the two pairings equal the model's `verifier_points`, every verdict
equals the model's `verify_tau` and `PlonkVerifier.verify` on the same proof.  A batch holds proofs of ONE structure with a value
stream per proof (random_circuit's second generator), so the public columns differ.  Sizes: n = 4 is the smallest order the verifier
takes; B = 64 / 65 / 130 are the lane and workgroup edges of the per-proof kernels (64 lanes per workgroup); n = 2048 and 4096 give the
PI pass two and four workgroups per proof."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402
from test_gpu_plonk import (blinding, from_affine, package_inputs, point_outside_the_subgroup, proof_dict, proof_object,  # noqa: E402
                            srs_for, to_affine)

pytestmark = pytest.mark.gpu
M, R = PL.M, PL.R
P = M.P
VP = C.c_void_p


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


class Circuit:
    """one structure of n rows with `count` witnesses: model proofs (dicts), their public columns, both forms of vpi, the SRS"""

    def __init__(self, zk, n, count, seed=None):
        from zk_cryptography_amd import plonk
        seed = n if seed is None else seed
        self.n, self.tau = n, 11 + seed
        self.srs = srs_for(zk, self.tau, n)
        self.proofs, self.publics = [], []
        for b in range(count):
            cpi, wit = PL.random_circuit(n, random.Random(seed), random.Random(500 + 13 * seed + b))
            assert b == 0 or cpi == self.cpi
            self.cpi = cpi
            self.proofs.append(PL.prove(cpi, wit, self.tau, blinding(seed + b), n_srs=4 * n + 1))
            self.publics.append(wit["public_poly"])
        assert len({tuple(p) for p in self.publics}) == count
        c, _ = package_inputs(zk, self.cpi, wit)
        self.v = zk.VerifierPreprocessedInput.vpi(self.srs, c)
        self.model_v = PL.vpi(self.cpi, self.tau)
        self.columns = [plonk._column(p) for p in self.publics]
        self._single, self._points = {}, {}

    def single(self, zk, b, fields=None, public=None):
        """PlonkVerifier.verify of proof b (or of `fields` in its place, against `public` in place of its column)"""
        if fields is None and public is None:
            if b not in self._single:
                self._single[b] = zk.PlonkVerifier(self.n, proof_object(zk, self.proofs[b]), self.srs, self.v).verify(self.publics[b])
            return self._single[b]
        return zk.PlonkVerifier(self.n, proof_object(zk, fields or self.proofs[b]), self.srs, self.v).verify(public or self.publics[b])

    def points(self, b):
        if b not in self._points:
            self._points[b] = PL.verifier_points(self.n, self.proofs[b], self.model_v, self.publics[b])
        return self._points[b]


_circuits = {}


def circuit(zk, n, count, seed=None):
    key = (n, seed)
    if key not in _circuits or len(_circuits[key].proofs) < count:
        _circuits[key] = Circuit(zk, n, count, seed)
    return _circuits[key]


def make_key(zk, n, v, srs, n_g2=None, raw=False):
    """zkhip_plonk_vkey_create -> (status, handle)"""
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    vxy, vinf = plonk._points_arrays(v if isinstance(v, list) else v._commitments())
    ctx = N.Context.get()
    h = C.c_void_p()
    g2 = srs.powers_of_tau_in_g2
    st = N.lib().zkhip_plonk_vkey_create(ctx.handle, C.c_size_t(n), vxy.ctypes.data_as(VP), vinf.ctypes.data_as(VP), N.ptr(g2), N.ptr(srs.g2_inf),
                                         C.c_size_t(len(g2) if n_g2 is None else n_g2), C.byref(h))
    return st, h


def destroy_key(h):
    from zk_cryptography_amd import _native as N
    assert N.lib().zkhip_plonk_vkey_destroy(h) == N.ZKHIP_OK


def call(zk, handle, proofs, columns, pairs=False, evals=None):
    """zkhip_plonk_verify_batch on PlonkProof objects and device columns -> (status, ok[B], pair points as model tuples or None)"""
    from zk_cryptography_amd import _native as N
    B = len(proofs)
    xy, inf = np.zeros((B, 9, 12), dtype=np.uint64), np.zeros((B, 9), dtype=np.uint8)
    ev = np.zeros((B, 6, 4), dtype=np.uint64)
    for b, p in enumerate(proofs):
        xy[b], inf[b], ev[b] = p._arrays()
    if evals is not None:
        ev = evals
    ptrs = (C.c_void_p * max(B, 1))(*[t.data_ptr() if t is not None else None for t in columns])
    ok = np.full(max(B, 1), 7, dtype=np.uint8)
    pxy, pinf = np.zeros((max(B, 1), 2, 12), dtype=np.uint64), np.zeros((max(B, 1), 2), dtype=np.uint8)
    st = N.lib().zkhip_plonk_verify_batch(handle, C.c_size_t(B), xy.ctypes.data_as(VP), inf.ctypes.data_as(VP), ev.ctypes.data_as(VP), ptrs,
                                          ok.ctypes.data_as(VP), pxy.ctypes.data_as(VP) if pairs else None,
                                          pinf.ctypes.data_as(VP) if pairs else None)
    points = None
    if pairs:
        for b in range(B):
            for k in range(2):
                assert not pinf[b, k] or not pxy[b, k].any()             # an identity has zero coordinates
        points = [tuple(from_affine(zk.G1Affine(pxy[b, k], pinf[b, k])) for k in range(2)) for b in range(B)]
    return st, ok[:B], points


@pytest.mark.parametrize("n", [8, 4])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_valid_batches_equal_the_model_and_the_single_call(zk, n, B):
    from zk_cryptography_amd import _native as N
    cir = circuit(zk, n, 5)
    proofs = [proof_object(zk, p) for p in cir.proofs[:B]]
    assert zk.PlonkVerifier.verify_batch(n, proofs, cir.srs, cir.v, cir.publics[:B]) == [True] * B
    st, h = make_key(zk, n, cir.v, cir.srs)
    assert st == N.ZKHIP_OK
    try:
        st, ok, points = call(zk, h, proofs, cir.columns[:B], pairs=True)
    finally:
        destroy_key(h)
    assert st == N.ZKHIP_OK
    for b in range(B):
        left, right = cir.points(b)
        assert points[b] == (right, left), b                                    # `right` first, then `left` itself
        assert PL.g1_mul(left, cir.tau) == right                                # verify_tau: the model's verdict is True
        assert bool(ok[b]) is True and cir.single(zk, b) is True


def test_mixed_batch_of_tampered_proofs(zk):
    n = 16
    cir = circuit(zk, n, 1)
    good, public = cir.proofs[0], cir.publics[0]
    wrong_public = [(public[0] + 1) % R] + list(public[1:])
    fields = [good] + [PL.tamper(good, f) for f in PL.PROOF_FIELDS] + [good, good]
    publics = [public] * 16 + [wrong_public, public]
    assert len(fields) == 18
    mask = zk.PlonkVerifier.verify_batch(n, [proof_object(zk, f) for f in fields], cir.srs, cir.v, publics)
    model = [PL.verify_tau(n, f, cir.model_v, p, cir.tau) for f, p in zip(fields, publics)]
    single = [cir.single(zk, 0, f, p) for f, p in zip(fields, publics)]
    assert mask == model and mask == single
    assert mask == [True] + [False] * 16 + [True]                               # a bad neighbour changes nothing


@pytest.mark.parametrize("B", [64, 65, 130])
def test_lane_and_workgroup_edges(zk, B):
    n = 8
    cir = circuit(zk, n, 5)
    tampered = sorted({p for p in (0, 63, 64, B - 1) if p < B})
    fields = [cir.proofs[b % 5] for b in range(B)]
    for k, p in enumerate(tampered):
        fields[p] = PL.tamper(fields[p], PL.PROOF_FIELDS[(4 * k + 1) % len(PL.PROOF_FIELDS)])
    publics = [cir.publics[b % 5] for b in range(B)]
    # one column for each of the five witnesses, shared by the proofs that use it
    from zk_cryptography_amd import plonk
    cols = [plonk._column(p) for p in cir.publics]
    mask = zk.PlonkVerifier.verify_batch(n, [proof_object(zk, f) for f in fields], cir.srs, cir.v, [cols[b % 5] for b in range(B)])
    assert mask == [b not in tampered for b in range(B)]
    for p in tampered + [1, B - 2]:
        assert mask[p] == cir.single(zk, p % 5, fields[p], publics[p]), p


@pytest.mark.parametrize("n", [2048, 4096])
def test_pi_pass_over_more_than_one_workgroup(zk, n):
    tau = 0xFACE + n
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(tau), n + 5, g2=True)
    proofs, publics = [], []
    for b in range(3):
        cpi, wit = PL.random_circuit(n, random.Random(n), random.Random(900 + b))
        c, w = package_inputs(zk, cpi, wit)
        if b == 0:
            shared = c
        proofs.append(zk.PlonkProver(shared, srs).prove(w, blinding=blinding(n + b)))
        publics.append(wit["public_poly"])
    v = zk.VerifierPreprocessedInput.vpi(srs, shared)
    assert zk.PlonkVerifier.verify_batch(n, proofs, srs, v, publics) == [True, True, True]
    changed = list(publics[1])
    changed[n - 1] = (changed[n - 1] + 1) % R                                   # the last row: the PI pass's last lane of its last workgroup
    assert zk.PlonkVerifier.verify_batch(n, proofs, srs, v, [publics[0], changed, publics[2]]) == [True, False, True]


class RawProof:
    """a proof as the arrays of the ABI, for what PlonkProof cannot hold (an evaluation that is not reduced)"""

    def __init__(self, xy, inf, ev):
        self.a = (xy, inf, ev)

    def _arrays(self):
        return self.a


def test_malformed_proofs_get_status_two_and_leave_the_others_alone(zk):
    from zk_cryptography_amd import _native as N
    n = 8
    cir = circuit(zk, n, 5)
    good = cir.proofs[1]
    x, y = good["t_mid"]
    off_curve = (x, (y + 1) % P)
    stray = point_outside_the_subgroup()
    assert not M.on_curve(off_curve) and M.on_curve(stray)
    xy, inf, ev = proof_object(zk, good)._arrays()
    ev = ev.copy()
    ev[3] = [(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]             # the limbs of r itself
    middles = [proof_object(zk, dict(good, w_zeta_commitment=stray)), proof_object(zk, dict(good, t_mid=off_curve)), RawProof(xy, inf, ev)]
    st, h = make_key(zk, n, cir.v, cir.srs)
    assert st == N.ZKHIP_OK
    try:
        for mid in middles:
            batch = [proof_object(zk, cir.proofs[0]), mid, proof_object(zk, cir.proofs[2])]
            with pytest.raises(ValueError, match=r"\[1\]"):
                zk.PlonkVerifier.verify_batch(n, batch, cir.srs, cir.v, cir.publics[:3])
            st, ok, points = call(zk, h, batch, cir.columns[:3], pairs=True)
            assert st == N.ERR_ARG and list(ok) == [1, 2, 1]
            for b in (0, 2):
                left, right = cir.points(b)
                assert points[b] == (right, left)
        # a proof point at infinity is the identity: a verdict, not an error, and the single call's
        at_inf = dict(cir.proofs[0], t_high=None)
        st, ok, points = call(zk, h, [proof_object(zk, at_inf), proof_object(zk, cir.proofs[1])], cir.columns[:2], pairs=True)
        assert st == N.ZKHIP_OK
        left, right = PL.verifier_points(n, at_inf, cir.model_v, cir.publics[0])
        assert points[0] == (right, left)
        assert bool(ok[0]) == cir.single(zk, 0, at_inf) == PL.verify_tau(n, at_inf, cir.model_v, cir.publics[0], cir.tau)
        assert ok[1] == 1
    finally:
        destroy_key(h)


def test_keys_and_arguments(zk):
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    n = 8
    cir, other = circuit(zk, n, 5), circuit(zk, n, 2, seed=77)
    assert cir.cpi != other.cpi
    st, h1 = make_key(zk, n, cir.v, cir.srs)
    st2, h2 = make_key(zk, n, other.v, other.srs)
    assert st == N.ZKHIP_OK and st2 == N.ZKHIP_OK
    try:
        mine = [proof_object(zk, p) for p in cir.proofs[:2]]
        theirs = [proof_object(zk, p) for p in other.proofs[:2]]
        for _ in range(3):                                                      # one key, three calls, beside a second key
            st, ok, _p = call(zk, h1, mine, cir.columns[:2])
            assert st == N.ZKHIP_OK and list(ok) == [1, 1]
            st, ok, _p = call(zk, h2, theirs, other.columns[:2])
            assert st == N.ZKHIP_OK and list(ok) == [1, 1]
        st, ok, _p = call(zk, h2, mine, cir.columns[:2])                        # the other circuit's key: no verdict carries over
        assert st == N.ZKHIP_OK and list(ok) == [0, 0]
        st, ok, _p = call(zk, h1, [], [])                                       # batch == 0: nothing touched
        assert st == N.ZKHIP_OK
        st, ok, _p = call(zk, h1, mine, [cir.columns[0], None])                 # a null column pointer
        assert st == N.ERR_ARG and list(ok) == [7, 7]
    finally:
        destroy_key(h1)
        destroy_key(h2)
    st, h = make_key(zk, n, cir.v, cir.srs, n_g2=1)
    assert st == N.ERR_INDEX and not h
    st, h = make_key(zk, 12, cir.v, cir.srs)
    assert st == N.ERR_SHAPE and not h
    vk = cir.v._commitments()
    vx, vy = from_affine(vk[5])
    st, h = make_key(zk, n, vk[:5] + [to_affine(zk, (vx, (vy + 1) % P))] + vk[6:], cir.srs)
    assert st == N.ERR_ARG and not h                                            # a bad vpi commitment is refused with the key
    st, h = make_key(zk, n, vk[:2] + [to_affine(zk, point_outside_the_subgroup())] + vk[3:], cir.srs)
    assert st == N.ERR_ARG and not h
    # the mirror class: its cache hands the same key to a second call, the empty batch is the empty list, no G2 half is verify's error
    assert zk.PlonkVerifier.verify_batch(n, mine, cir.srs, cir.v, cir.publics[:2]) == [True, True]
    keys = dict(plonk._vkeys)
    assert zk.PlonkVerifier.verify_batch(n, mine, cir.srs, cir.v, cir.publics[0]) == [True, False]      # one column for all proofs
    assert dict(plonk._vkeys) == keys
    assert zk.PlonkVerifier.verify_batch(n, [], cir.srs, cir.v, []) == []
    no_g2 = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(5), 4 * n)
    with pytest.raises(ValueError, match="no G2 half"):
        zk.PlonkVerifier.verify_batch(n, mine, no_g2, cir.v, cir.publics[:2])
