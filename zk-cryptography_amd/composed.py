"""polynomial::ComposedMultilinear and the composed / multi-composed sumcheck provers on the GPU.

Mirrors polynomial/src/composed/composed_multilinear.rs:8-120,
sumcheck/src/composed/composed_sumcheck.rs:20-67 and
sumcheck/src/composed/multi_composed_sumcheck.rs:13-121 (provers only; verifiers are host-side, out of scope).
"""
import ctypes as C

import numpy as np

from zk_cryptography_amd import _native as N
from zk_cryptography_amd.field import Fr
from zk_cryptography_amd.polynomial import Multilinear

MAX_MONO = 7


class ComposedMultilinear:
    def __init__(self, polys):
        """ComposedMultilinear::new (composed_multilinear.rs:12-18): all tables share n_vars."""
        polys = [p if isinstance(p, Multilinear) else Multilinear(p) for p in polys]
        assert all(p.n_vars == polys[0].n_vars for p in polys)
        self.polys = polys

    def n_vars(self):
        return self.polys[0].n_vars

    def max_degree(self):
        """composed_multilinear.rs:101-103"""
        return len(self.polys)

    def partial_evaluation(self, evaluation_point, variable_index):
        """composed_multilinear.rs:63-75"""
        return ComposedMultilinear([p.partial_evaluation(evaluation_point, variable_index) for p in self.polys])

    def evaluation(self, points):
        """composed_multilinear.rs:51-61: product of the tables' evaluations -> python int (canonical)"""
        acc = 1
        for v in Fr.to_ints(Multilinear.evaluation_batch(self.polys, points)):     # the K factors in one call
            acc = acc * v % Fr.MODULUS
        return acc

    def to_bytes(self):
        """composed_multilinear.rs:40-48"""
        return b"".join(p.to_bytes() for p in self.polys)

    def _element_wise(self, op):
        if not self.polys:
            raise IndexError("element_wise on an empty ComposedMultilinear")      # self.polys[0] panics
        first = self.polys[0]
        if any(len(p) < len(first) for p in self.polys):
            raise IndexError("a table is shorter than the first one")             # v.evaluations[i] panics
        out = first._new_like(len(first))
        N.check(N.lib().zkhip_composed_element_wise(first._ctx.handle, C.c_int(op), _ptr_array(self._ptrs()),
                                                    C.c_uint32(len(self.polys)), C.c_size_t(len(first)), N.ptr(out)),
                "composed_element_wise")
        return out

    def element_wise_product(self):
        """ComposedMultilinearTrait::element_wise_product (composed_multilinear.rs:105-111) -> device tensor int64 [n, 4]
        (the reference's Vec<F>)"""
        return self._element_wise(0)

    def element_wise_add(self):
        """ComposedMultilinearTrait::element_wise_add (composed_multilinear.rs:113-119)"""
        return self._element_wise(1)

    def _ptrs(self):
        return [p.evaluations.data_ptr() for p in self.polys]


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class ComposedSumcheckProof:
    """composed_sumcheck.rs:15-18: {poly, round_polys}; round_polys is uint64 [n_vars, K+1, 4]"""

    def __init__(self, poly, round_polys):
        self.poly = poly
        self.round_polys = round_polys


class ComposedSumcheck:
    def __init__(self, poly):
        """ComposedSumcheck::new (composed_sumcheck.rs:21-26)"""
        self.poly = poly
        self.sum = np.zeros(4, dtype=np.uint64)

    @staticmethod
    def calculate_poly_sum(poly):
        """composed_sumcheck.rs:28-30"""
        out = np.empty(4, dtype=np.uint64)
        ctx = N.Context.get(poly.polys[0].evaluations.device.index)
        N.check(N.lib().zkhip_composed_sum(ctx.handle, _ptr_array(poly._ptrs()), C.c_uint32(len(poly.polys)),
                                           C.c_size_t(len(poly.polys[0])), out.ctypes.data_as(C.c_void_p)), "composed_sum")
        return out

    def prove(self):
        """composed_sumcheck.rs:32-67 -> (ComposedSumcheckProof, challenges [n_vars, 4])"""
        k, nv = len(self.poly.polys), self.poly.n_vars()
        rp = np.empty((max(nv, 1), k + 1, 4), dtype=np.uint64)
        ch = np.empty((max(nv, 1), 4), dtype=np.uint64)
        ctx = N.Context.get(self.poly.polys[0].evaluations.device.index)
        N.check(N.lib().zkhip_composed_prove(ctx.handle, _ptr_array(self.poly._ptrs()), C.c_uint32(k),
                                             C.c_size_t(len(self.poly.polys[0])), rp.ctypes.data_as(C.c_void_p),
                                             ch.ctypes.data_as(C.c_void_p)), "composed_prove")
        return ComposedSumcheckProof(self.poly, rp[:nv]), ch[:nv]

    @staticmethod
    def prove_batch(polys):
        """The proofs of a list of ComposedMultilinear of one K and one length in one call (zkhip_composed_prove_batch)
        -> [(ComposedSumcheckProof, challenges)], each as from prove()."""
        polys = list(polys)
        if not polys:
            return []
        first = polys[0].polys[0]               # (an empty table list: IndexError, as prove() raises)
        k, nv, n, dev = len(polys[0].polys), first.n_vars, len(first), first.evaluations.device
        for p in polys:
            assert len(p.polys) == k, "the products of a batch share their number of tables"
            assert all(len(t) == n for t in p.polys), "the tables of a batch share their length"
            assert all(t.evaluations.device == dev for t in p.polys), "the tables of a batch live on one device"
        B, m = len(polys), max(nv, 1)
        if B == 1:
            return [ComposedSumcheck(polys[0]).prove()]
        rp = np.empty((B, m, k + 1, 4), dtype=np.uint64)
        ch = np.empty((B, m, 4), dtype=np.uint64)
        ctx = N.Context.get(dev.index)
        N.check(N.lib().zkhip_composed_prove_batch(ctx.handle, C.c_uint32(B), _ptr_array([a for p in polys for a in p._ptrs()]), C.c_uint32(k),
                                                   C.c_size_t(n), rp.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p)), "composed_prove_batch")
        return [(ComposedSumcheckProof(polys[b], rp[b, :nv]), ch[b, :nv]) for b in range(B)]


class SparseUnivariatePolynomial:
    """polynomial/src/univariate/sparse_univariate.rs:12-20: monomials (coeff, pow), both Montgomery uint64[4]."""

    def __init__(self, coeffs, pows):
        self.coeffs = coeffs
        self.pows = pows

    def monomials(self):
        return list(zip(Fr.to_ints(self.coeffs), Fr.to_ints(self.pows))) if len(self.coeffs) else []

    def to_bytes(self):
        """sparse_univariate.rs:27-34"""
        out = b""
        for c, p in self.monomials():
            out += c.to_bytes(32, "big") + p.to_bytes(32, "big")
        return out


class MultiComposedSumcheckProof:
    """multi_composed_sumcheck.rs:12-16 (named ComposedSumcheckProof there): {round_polys, sum}"""

    def __init__(self, round_polys, sum_):
        self._round_polys = round_polys
        self._packed = None
        self.sum = sum_

    @classmethod
    def from_packed(cls, monomials, lens, sum_):
        """The prover's output as it comes off the device -- monomials uint64 [n_rounds, MAX_MONO, 2, 4] (coeff, pow), lens
        [n_rounds] -- wrapped without building a SparseUnivariatePolynomial per round; `round_polys` builds them on first
        use (a depth-20 GKR proof has ~420 rounds, and host time between proofs is GPU idle time)."""
        self = cls(None, sum_)
        self._packed = (monomials, lens)
        return self

    @property
    def round_polys(self):
        if self._round_polys is None:
            mono, lens = self._packed
            self._round_polys = [SparseUnivariatePolynomial(mono[r, : lens[r], 0].copy(), mono[r, : lens[r], 1].copy()) for r in range(len(lens))]
        return self._round_polys

    @round_polys.setter
    def round_polys(self, v):
        self._round_polys = v

    def to_bytes(self):
        """multi_composed_sumcheck.rs:24-31"""
        return b"".join(rp.to_bytes() for rp in self.round_polys)


class MultiComposedSumcheckProver:
    @staticmethod
    def _flat(poly):
        ptrs, sizes = [], []
        for term in poly:
            ptrs += term._ptrs()
            sizes.append(len(term.polys))
        return ptrs, sizes

    @staticmethod
    def calculate_poly_sum(poly):
        """multi_composed_sumcheck.rs:36-45"""
        ptrs, sizes = MultiComposedSumcheckProver._flat(poly)
        out = np.empty(4, dtype=np.uint64)
        ctx = N.Context.get(poly[0].polys[0].evaluations.device.index)
        N.check(N.lib().zkhip_multi_composed_sum(ctx.handle, _ptr_array(ptrs), (C.c_uint32 * len(sizes))(*sizes),
                                                 C.c_uint32(len(sizes)), C.c_size_t(len(poly[0].polys[0])),
                                                 out.ctypes.data_as(C.c_void_p)), "multi_composed_sum")
        return out

    @staticmethod
    def _prove(polys, sums, partial):
        """The proofs of a list of claims of one term shape, one length and one device -> (lens [B, n_vars], monomials
        [B, n_vars, MAX_MONO, 2, 4], challenges [B, n_vars, 4], sums [B, 4]).  One claim goes to zkhip_multi_composed_prove, more to
        zkhip_multi_composed_prove_batch."""
        flat = [MultiComposedSumcheckProver._flat(p) for p in polys]
        sizes, first = flat[0][1], polys[0][0].polys[0]
        nv, n, dev = first.n_vars, len(first), first.evaluations.device
        for p, (_, sz) in zip(polys, flat):
            assert sz == sizes, "the claims of a batch share their term sizes"
            assert all(len(t) == n for term in p for t in term.polys), "the tables of a batch share their length"
            assert all(t.evaluations.device == dev for term in p for t in term.polys), "the tables of a batch live on one device"
        B, m = len(polys), max(nv, 1)
        s = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 4)
        assert len(s) == B, "one claimed sum per claim"
        lens = np.zeros((B, m), dtype=np.uint32)
        rp = np.zeros((B, m, MAX_MONO, 2, 4), dtype=np.uint64)
        ch = np.empty((B, m, 4), dtype=np.uint64)
        ctx = N.Context.get(dev.index)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        shape = ((C.c_uint32 * len(sizes))(*sizes), C.c_uint32(len(sizes)), C.c_size_t(n))
        if B == 1:
            st = N.lib().zkhip_multi_composed_prove(ctx.handle, _ptr_array(flat[0][0]), *shape, vp(s), C.c_int(1 if partial else 0),
                                                    vp(lens), vp(rp), vp(ch))
            N.check(st, "multi_composed_prove")
        else:
            st = N.lib().zkhip_multi_composed_prove_batch(ctx.handle, C.c_uint32(B), _ptr_array([a for ptrs, _ in flat for a in ptrs]), *shape,
                                                          vp(s), C.c_int(1 if partial else 0), vp(lens), vp(rp), vp(ch))
            N.check(st, "multi_composed_prove_batch")
        return lens[:, :nv], rp[:, :nv], ch[:, :nv], s

    @staticmethod
    def _prove_one(poly, sum_, partial):
        lens, rp, ch, s = MultiComposedSumcheckProver._prove([poly], sum_, partial)
        polys = [SparseUnivariatePolynomial(rp[0, r, : lens[0, r], 0].copy(), rp[0, r, : lens[0, r], 1].copy()) for r in range(lens.shape[1])]
        return MultiComposedSumcheckProof(polys, s[0].copy()), ch[0]

    @staticmethod
    def _prove_many(polys, sums, partial):
        polys = list(polys)
        if not polys:
            return []
        if len(polys) == 1:
            return [MultiComposedSumcheckProver._prove_one(polys[0], np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 4)[0], partial)]
        lens, rp, ch, s = MultiComposedSumcheckProver._prove(polys, sums, partial)
        return [(MultiComposedSumcheckProof.from_packed(rp[b], lens[b], s[b].copy()), ch[b]) for b in range(len(polys))]

    @staticmethod
    def prove(poly, sum_):
        """multi_composed_sumcheck.rs:47-54 -> Ok((proof, challenges))"""
        return MultiComposedSumcheckProver._prove_one(poly, sum_, False)

    @staticmethod
    def prove_partial(poly, sum_):
        """multi_composed_sumcheck.rs:56-62"""
        return MultiComposedSumcheckProver._prove_one(poly, sum_, True)

    @staticmethod
    def prove_batch(polys, sums):
        """prove() of a list of claims of one term shape and one length in one call (zkhip_multi_composed_prove_batch)
        -> [(MultiComposedSumcheckProof, challenges)], each as from prove(); sums: one claimed sum per claim, [B, 4]."""
        return MultiComposedSumcheckProver._prove_many(polys, sums, False)

    @staticmethod
    def prove_partial_batch(polys, sums):
        """prove_partial() of a list of claims in one call -> [(MultiComposedSumcheckProof, challenges)]"""
        return MultiComposedSumcheckProver._prove_many(polys, sums, True)
