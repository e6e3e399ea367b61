"""sumcheck::Sumcheck prover on the GPU (sumcheck/src/sumcheck.rs:17-61).

`prove` runs the whole round loop on the device -- fused half-sums + fold kernels, and a
device-resident SHA-256 Fiat-Shamir transcript -- and returns the same observable values as
the reference: the claimed sum, one 2-evaluation round polynomial per variable, and the
challenges.  Verifiers are host-side and out of scope.
"""
import ctypes as C

import numpy as np

from zk_cryptography_amd import _native as N
from zk_cryptography_amd.polynomial import Multilinear


class SumcheckProof:
    """sumcheck.rs:11-15: {poly, sum, univariate_poly}.  `poly` is a reference to the prover's table
    (the Rust struct clones it); univariate_poly is uint64 [n_vars, 2, 4]."""

    def __init__(self, poly, sum_, univariate_poly):
        self.poly = poly
        self.sum = sum_
        self.univariate_poly = univariate_poly


def _proof_buffers(nv):
    """(sum [4], round polynomials [nv, 2, 4], challenges [nv, 4]) as views of ONE fresh allocation, and its address"""
    m = max(nv, 1)
    buf = np.empty(4 + 12 * m, dtype=np.uint64)
    return buf[:4], buf[4:4 + 8 * m].reshape(m, 2, 4)[:nv], buf[4 + 8 * m:].reshape(m, 4)[:nv], buf.ctypes.data


class PendingProof:
    """A Sumcheck::prove in flight (zkhip_sumcheck_prove_begin / _end)."""

    def __init__(self, poly, ticket):
        self._poly, self._ticket = poly, ticket

    def wait(self):
        if self._ticket is None:
            raise RuntimeError("proof already collected")
        nv = self._poly.n_vars
        s, rp, ch, base = _proof_buffers(nv)
        t, self._ticket = self._ticket, None
        N.check(N.lib().zkhip_sumcheck_prove_end(self._poly._ctx.handle, t, base, base + 32, base + 32 + 64 * max(nv, 1)), "sumcheck_prove_end")
        return SumcheckProof(self._poly, s, rp), ch

    def __del__(self):
        if getattr(self, "_ticket", None) is not None:
            try:
                N.lib().zkhip_sumcheck_prove_end(self._poly._ctx.handle, C.c_uint32(self._ticket), None, None, None)
            except Exception:
                pass


class Sumcheck:
    def __init__(self, poly):
        """Sumcheck::new (sumcheck.rs:18-23)"""
        self.poly = poly if isinstance(poly, Multilinear) else Multilinear(poly)
        self._sum_host = np.zeros(4, dtype=np.uint64)   # Default::default()
        self._sum_dev = None                       # poly_sum() leaves the sum on the device until someone reads it
        self._sum_ptr = None                       # its device address (no tensor view per call: host time is GPU idle time)
        self._block_sums = None                    # device tensor kept by poly_sum() for prove()
        self._log_blocks = 0
        self._sum_deferred = False                 # poly_sum() ran but left the total to prove()'s own sum tree (zkhip_mle_block_sums_deferred)

    @property
    def sum(self):
        """`self.sum` (private in the reference, sumcheck.rs:7-10): fetched from the device on first read."""
        if self._sum_deferred:
            out = np.empty(4, dtype=np.uint64)
            N.check(N.lib().zkhip_mle_block_sums_total(self.poly._ctx.handle, C.c_void_p(self._block_sums.data_ptr()), C.c_uint32(self._log_blocks),
                                                       out.ctypes.data_as(C.c_void_p)), "block_sums_total")
            self._sum_host, self._sum_deferred = out, False
        elif self._sum_dev is not None:
            self._sum_host = self._sum_dev[-1].cpu().numpy().view(np.uint64).reshape(4).copy()
            self._sum_dev = None
        return self._sum_host

    @sum.setter
    def sum(self, v):
        self._sum_host = np.ascontiguousarray(v, dtype=np.uint64).reshape(4)
        self._sum_dev = None
        self._sum_deferred = False

    def poly_sum(self):
        """sumcheck.rs:25-27.  One streaming pass, asynchronous: the sum and the block sums it produces on the way
        stay on the device, so that prove() neither re-reads the table for its first rounds nor waits for a
        device->host copy of the sum."""
        import torch
        n = len(self.poly)
        if n == 1:
            self.sum = self.poly.to_numpy()[0].copy()
            return
        cached = getattr(self.poly, "_block_sum_buf", None)     # (lb, buffer): reused by every Sumcheck over this table
        if cached is None:
            lb = N.lib().zkhip_sumcheck_plan_log_blocks(C.c_size_t(n))
            cached = (lb, torch.empty(((1 << lb) + 1, 4), dtype=torch.int64, device=self.poly.evaluations.device))
            self.poly._block_sum_buf = cached
        lb, buf = cached
        if lb > 9:
            # the fine granularity of the overlapped plan: the total would be a launch of its own, and prove() has it as the root of
            # its sum tree -- deferred until someone reads `self.sum`
            N.check(N.lib().zkhip_mle_block_sums_deferred(self.poly._ctx.handle, self.poly.evaluations.data_ptr(), n, lb, buf.data_ptr()), "block_sums")
            self._block_sums, self._log_blocks = buf, lb
            self._sum_dev, self._sum_ptr, self._sum_deferred = None, None, True
            return
        N.check(N.lib().zkhip_mle_block_sums(self.poly._ctx.handle, self.poly.evaluations.data_ptr(), n, lb, buf.data_ptr(), None), "block_sums")
        self._block_sums, self._log_blocks = (buf, lb) if lb else (None, 0)
        self._sum_dev = buf
        self._sum_deferred = False
        self._sum_ptr = buf.data_ptr() + 32 * (1 << lb)

    def prove_begin(self):
        """The same proof, in flight (zkhip_sumcheck_prove_begin): -> PendingProof; .wait() yields what prove() returns.  At most
        eight per context, each on buffers of its own: a prover with several tables begins the next proofs before it
        collects the previous ones, and their streaming passes overlap the others' transcript rounds (from the third proof in flight
        on, part of a proof is enqueued by a later prove_begin() / wait(): every PendingProof must be waited for or dropped).  The table and its block
        sums (poly_sum() of the SAME Multilinear) must stay untouched until wait()."""
        if len(self.poly) < 2:
            raise AssertionError("prove_begin needs a table of at least two entries")
        ticket = C.c_uint32(0)
        st = N.lib().zkhip_sumcheck_prove_begin(self.poly._ctx.handle, self.poly.evaluations.data_ptr(), len(self.poly),
                                                None if (self._sum_dev is not None or self._sum_deferred) else self._sum_host.ctypes.data,
                                                self._sum_ptr if self._sum_dev is not None else None,
                                                self._block_sums.data_ptr() if self._block_sums is not None else None,
                                                self._log_blocks, C.addressof(ticket))
        N.check(st, "sumcheck_prove_begin")
        return PendingProof(self.poly, ticket.value)

    def prove(self):
        """sumcheck.rs:29-61 -> (SumcheckProof, challenges uint64 [n_vars, 4]).

        The transcript absorbs `self.sum` exactly as the reference does (zero if poly_sum() was never
        called)."""
        nv = self.poly.n_vars
        s, rp, ch, base = _proof_buffers(nv)
        st = N.lib().zkhip_sumcheck_prove(self.poly._ctx.handle, self.poly.evaluations.data_ptr(), len(self.poly),
                                          None if (self._sum_dev is not None or self._sum_deferred) else self._sum_host.ctypes.data,
                                          self._sum_ptr if self._sum_dev is not None else None,
                                          self._block_sums.data_ptr() if self._block_sums is not None else None,
                                          self._log_blocks, base, base + 32, base + 32 + 64 * max(nv, 1))
        N.check(st, "sumcheck_prove")
        return SumcheckProof(self.poly, s, rp), ch

    BATCH_CHUNK = 1024          # csrc/sumcheck_batch_kernels.hpp SCB_CHUNK: proofs per launch of the batch kernel

    @staticmethod
    def prove_batch(polys, sums=None):
        """The proofs of a list of tables of one length in one call (zkhip_sumcheck_prove_batch) -> [(SumcheckProof, challenges)],
        each as from prove().  sums=None: every proof absorbs its table's true sum, as poly_sum() + prove() does; otherwise one
        claimed sum per table, uint64 [B, 4], absorbed as given (zeros: prove() without poly_sum())."""
        polys = [p if isinstance(p, Multilinear) else Multilinear(p) for p in polys]
        if not polys:
            return []
        evs = [p.evaluations for p in polys]
        n, nv, dev = evs[0].shape[0], polys[0].n_vars, evs[0].device
        assert all(e.shape[0] == n for e in evs), "the tables of a batch share their length"
        assert all(e.device == dev for e in evs), "the tables of a batch live on one device"
        B, m = len(polys), max(nv, 1)
        claimed = None
        if sums is not None:
            claimed = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 4)
            assert claimed.shape[0] == B, "one claimed sum per table"
        if B == 1:      # the single prover, by the single call's own path (both claimed-sum arguments NULL: the true sum)
            s, rp, ch, base = _proof_buffers(nv)
            N.check(N.lib().zkhip_sumcheck_prove(polys[0]._ctx.handle, evs[0].data_ptr(), n, claimed.ctypes.data if claimed is not None else None,
                                                 None, None, 0, base, base + 32, base + 32 + 64 * m), "sumcheck_prove")
            return [(SumcheckProof(polys[0], s, rp), ch)]
        s = np.empty((B, 4), dtype=np.uint64)
        rp = np.empty((B, m, 2, 4), dtype=np.uint64)
        ch = np.empty((B, m, 4), dtype=np.uint64)
        ptrs = (C.c_void_p * B)(*[e.data_ptr() for e in evs])
        st = N.lib().zkhip_sumcheck_prove_batch(polys[0]._ctx.handle, C.c_uint32(B), ptrs, C.c_size_t(n),
                                                claimed.ctypes.data_as(C.c_void_p) if claimed is not None else None,
                                                s.ctypes.data_as(C.c_void_p), rp.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p))
        N.check(st, "sumcheck_prove_batch")
        if nv:      # (the C layout is [B][n_vars][...]: m == n_vars)
            return [(SumcheckProof(polys[b], s[b], rp[b]), ch[b]) for b in range(B)]
        return [(SumcheckProof(polys[b], s[b], rp[b, :0]), ch[b, :0]) for b in range(B)]
