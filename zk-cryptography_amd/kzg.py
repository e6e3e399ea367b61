"""kzg::{TrustedSetup, MultilinearKZG, UnivariateKZG} on the GPU: commit, open and verify.

Mirrors kzg/src/interface.rs:10-55: `commitment` (a Pippenger multi-scalar multiplication over BLS12-381 G1), `open` (one
commitment per variable against the folded SRS), `verify` (the BLS12-381 optimal ate pairing: one Miller loop per pairing and
lane over prepared G2 lines, a product tree and one final exponentiation per opening; `verify_batch` checks many openings in one
pass) and both halves of the trusted setup (the G2 half on request: `setup(..., g2=True)`).  Points are returned as affine
coordinates (Montgomery limbs + infinity flag): the reference's projective representation is algorithm dependent, equality is
defined on the affine point.
"""
import ctypes as C

import numpy as np

from zk_cryptography_amd import _native as N
from zk_cryptography_amd.polynomial import Multilinear, _fr_host, _to_device


class G1Affine:
    def __init__(self, xy, inf):
        self.xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(12)
        self.infinity = bool(inf)

    def __eq__(self, o):
        return isinstance(o, G1Affine) and self.infinity == o.infinity and (self.infinity or np.array_equal(self.xy, o.xy))

    def coords(self):
        """(x, y) as canonical python ints"""
        q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
        rinv = pow(pow(2, 384, q), -1, q)
        x = sum(int(self.xy[k]) << (64 * k) for k in range(6)) * rinv % q
        y = sum(int(self.xy[6 + k]) << (64 * k) for k in range(6)) * rinv % q
        return x, y


class G2Affine:
    """A point of the twist y^2 = x^3 + 4 (u + 1): x.c0, x.c1, y.c0, y.c1 as Montgomery limbs (uint64 [24]) + infinity flag."""

    def __init__(self, xy, inf):
        self.xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(24)
        self.infinity = bool(inf)

    def __eq__(self, o):
        return isinstance(o, G2Affine) and self.infinity == o.infinity and (self.infinity or np.array_equal(self.xy, o.xy))

    def coords(self):
        """((x.c0, x.c1), (y.c0, y.c1)) as canonical python ints"""
        v = [_fq_int(self.xy[6 * k: 6 * k + 6]) for k in range(4)]
        return (v[0], v[1]), (v[2], v[3])


_Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def _fq_int(limbs):
    """6 Montgomery limbs -> canonical int"""
    return sum(int(limbs[k]) << (64 * k) for k in range(6)) * pow(pow(2, 384, _Q), -1, _Q) % _Q


def gt_ints(gt):
    """one GT value (uint64 [72], as pairing() returns) -> its 12 Fq coefficients as canonical ints, arkworks order"""
    gt = np.asarray(gt, dtype=np.uint64).reshape(72)
    return [_fq_int(gt[6 * k: 6 * k + 6]) for k in range(12)]


def _g1_arrays(points):
    xy = np.zeros((max(len(points), 1), 12), dtype=np.uint64)
    inf = np.zeros(max(len(points), 1), dtype=np.uint8)
    for i, p in enumerate(points):
        xy[i], inf[i] = p.xy, 1 if p.infinity else 0
    return xy, inf


def _g2_device(points):
    import torch
    xy = np.zeros((max(len(points), 1), 24), dtype=np.uint64)
    inf = np.zeros(max(len(points), 1), dtype=np.uint8)
    for i, q in enumerate(points):
        xy[i], inf[i] = q.xy, 1 if q.infinity else 0
    return torch.from_numpy(xy.view(np.int64)).cuda(), torch.from_numpy(inf).cuda()


def g2_prepare(g2_points):
    """zkhip_g2_prepare: the Miller-loop lines of each G2 point (a uint8 CUDA tensor) for pairing(..., prepared=...)"""
    import torch
    n = len(g2_points)
    qxy, qinf = _g2_device(g2_points)
    prep = torch.empty(max(N.lib().zkhip_g2_prepared_bytes(C.c_size_t(n)), 1), dtype=torch.uint8, device=qxy.device)
    ctx = N.Context.get(qxy.device.index)
    st = N.lib().zkhip_g2_prepare(ctx.handle, N.ptr(qxy), N.ptr(qinf), C.c_size_t(n), N.ptr(prep))
    _check_points(st, "g2_prepare")
    return prep


def _check_points(st, what):
    if st == N.ERR_ARG:
        raise ValueError("%s: a point is off its curve, outside the prime-order subgroup or has an unreduced coordinate, or a scalar is "
                         "not a reduced field element" % what)
    N.check(st, what)


def pairing(g1_points, g2_points=None, prepared=None):
    """zkhip_pairing: e(g1_points[k], g2_points[k]) for every k -> uint64 [n, 72] GT values (gt_ints() for canonical ints).
    With `prepared` (g2_prepare's lines) instead of g2_points: zkhip_pairing_prepared."""
    import torch
    n = len(g1_points)
    pxy, pinf = _g1_arrays(g1_points)
    pxy_d = torch.from_numpy(pxy.view(np.int64)).cuda()
    pinf_d = torch.from_numpy(pinf).cuda()
    out = torch.empty((max(n, 1), 72), dtype=torch.int64, device=pxy_d.device)
    ctx = N.Context.get(pxy_d.device.index)
    if prepared is not None:
        st = N.lib().zkhip_pairing_prepared(ctx.handle, N.ptr(pxy_d), N.ptr(pinf_d), N.ptr(prepared), C.c_size_t(n), N.ptr(out))
    else:
        if len(g2_points) != n:
            raise AssertionError("pairing: as many G2 as G1 points")
        qxy, qinf = _g2_device(g2_points)
        st = N.lib().zkhip_pairing(ctx.handle, N.ptr(pxy_d), N.ptr(pinf_d), N.ptr(qxy), N.ptr(qinf), C.c_size_t(n), N.ptr(out))
    _check_points(st, "pairing")
    return out.cpu().numpy().view(np.uint64)[:n]


def _is_points(x):
    """a 2-D [m, 4] argument (numpy or torch), as opposed to one field element"""
    return x.dim() == 2 if hasattr(x, "is_cuda") else np.ndim(x) == 2


def _empty_fr(n, device):
    import torch
    return torch.empty((n, 4), dtype=torch.int64, device=device)


def _rows_device(a, device):
    """[..., 4] limbs (numpy uint64 or an int64 tensor) -> a contiguous int64 device tensor of the same shape"""
    import torch
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int64 or a.shape[-1] != 4:
            raise AssertionError("field elements are int64 [..., 4]")
        return (a if a.is_cuda else a.cuda(device)).contiguous()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim < 2 or a.shape[-1] != 4:
        raise AssertionError("field elements are uint64 [..., 4] Montgomery limbs")
    return torch.from_numpy(a.view(np.int64)).cuda(device)


def _points_device(points, device):
    """[m, 4] points -> (device tensor, whether the caller gave host memory and gets host memory back)"""
    t = _rows_device(points, device)
    if t.dim() != 2:
        raise AssertionError("points are [m, 4]")
    return t, not hasattr(points, "is_cuda") or not points.is_cuda


def _rows_or_shared_device(a, batch, device, what):
    """[m, 4] shared by the batch or [batch, m, 4] -> (device tensor, whether the caller gave host memory)"""
    t = _rows_device(a, device)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != batch):
        raise AssertionError(what)
    return t, not hasattr(a, "is_cuda") or not a.is_cuda


class DenseUnivariatePolynomial:
    """polynomial::DenseUnivariatePolynomial (dense_univariate.rs:15-17): coefficients, low degree first, in HBM."""

    def __init__(self, coefficients, device=None):
        self.coefficients = _to_device(coefficients, device)

    def __len__(self):
        return self.coefficients.shape[0]

    def is_zero(self):
        """dense_univariate.rs:41-43: an EMPTY coefficient vector"""
        return len(self) == 0

    def degree(self):
        """dense_univariate.rs:199-207: zero leading coefficients do not count; 0 for the zero polynomial"""
        d = C.c_size_t(0)
        if len(self):
            ctx = N.Context.get(self.coefficients.device.index)
            N.check(N.lib().zkhip_dense_degree(ctx.handle, N.ptr(self.coefficients), C.c_size_t(len(self)), C.byref(d)), "degree")
        return d.value

    def evaluate(self, point):
        """dense_univariate.rs:184-196 -> uint64[4] (Montgomery).  A 2-D [m, 4] argument is m points in one call
        (zkhip_dense_points): a numpy array gives a numpy [m, 4], a device tensor gives a device tensor without a synchronisation."""
        if _is_points(point):
            if len(point) == 1 and not hasattr(point, "is_cuda"):
                # one host point: the single call's scan cuts the coefficients finer than a lane's Horner can (measured 115 against
                # 212 us at 2^8 coefficients, 117 against 735 at 2^16: profiles/dense_points/NOTES.md, "One point")
                return self.evaluate(np.asarray(point, dtype=np.uint64)[0]).reshape(1, 4)
            pts, to_host = _points_device(point, self.coefficients.device)
            out = _empty_fr(pts.shape[0], pts.device)
            ctx = N.Context.get(pts.device.index)
            N.check(N.lib().zkhip_dense_points(ctx.handle, N.DENSE_EVALUATE, 1, self.coefficients.data_ptr(), 0, len(self),
                                               pts.data_ptr(), 0, pts.shape[0], out.data_ptr(), pts.shape[0]), "evaluate")
            return out.cpu().numpy().view(np.uint64) if to_host else out
        out = np.zeros(4, dtype=np.uint64)
        if len(self):
            z = _fr_host(point).reshape(4)
            ctx = N.Context.get(self.coefficients.device.index)
            N.check(N.lib().zkhip_dense_evaluate(ctx.handle, N.ptr(self.coefficients), C.c_size_t(len(self)),
                                                 z.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), "evaluate")
        return out

    @staticmethod
    def evaluate_batch(polys, points):
        """B polynomials of one length at many points in one call (zkhip_dense_points).  polys: a list of polynomials, or their
        coefficients as [B, n, 4]; points: [m, 4] shared by all polynomials or [B, m, 4], one row per polynomial -> [B, m, 4]
        (numpy when the points are numpy, a device tensor otherwise)."""
        import torch
        if isinstance(polys, (list, tuple)):
            if not polys:
                return np.empty((0, 0, 4), dtype=np.uint64)
            if any(len(p) != len(polys[0]) for p in polys):
                raise AssertionError("evaluate_batch: polynomials of one length")
            coeffs = torch.stack([p.coefficients for p in polys])
        else:
            coeffs = _rows_device(polys, None)
        B, n = coeffs.shape[0], coeffs.shape[1]
        pts, to_host = _rows_or_shared_device(points, B, coeffs.device, "evaluate_batch: points are [m, 4] or [B, m, 4]")
        m = pts.shape[-2]
        out = torch.empty((B, m, 4), dtype=torch.int64, device=coeffs.device)
        ctx = N.Context.get(coeffs.device.index)
        N.check(N.lib().zkhip_dense_points(ctx.handle, N.DENSE_EVALUATE, B, coeffs.data_ptr(), n, n, pts.data_ptr(),
                                           m if pts.dim() == 3 else 0, m, out.data_ptr(), m), "evaluate_batch")
        return out.cpu().numpy().view(np.uint64) if to_host else out

    @staticmethod
    def interpolate(point_ys, point_xs):
        """DenseUnivariatePolynomial::interpolate (dense_univariate.rs:76-85; the reference's argument order): the polynomial of
        degree < n through (point_xs[i], point_ys[i]), n <= 2^14, as n device coefficients.  Repeated nodes raise ValueError (the
        reference unwraps the inverse of zero), different lengths AssertionError (dense_langrange_basis, utils.rs:108-114).
        One deviation: when all ys are zero the result holds n zero coefficients where the reference's Add fold returns the empty
        vector; degree() and evaluate agree on both."""
        ys = _to_device(point_ys)
        xs = _to_device(point_xs, ys.device)
        if ys.shape[0] != xs.shape[0]:
            raise AssertionError("interpolate: as many ys as xs")
        return DenseUnivariatePolynomial(DenseUnivariatePolynomial.interpolate_batch(ys[None], xs)[0])

    @staticmethod
    def interpolate_batch(ys, xs):
        """B interpolations in one call (zkhip_dense_points): ys [B, n, 4]; xs [n, 4] for shared nodes -- their weights are computed
        once -- or [B, n, 4] for nodes per job -> the coefficients as a device tensor [B, n, 4]"""
        import torch
        ys = _rows_device(ys, None)
        B, n = ys.shape[0], ys.shape[1]
        xs, _ = _rows_or_shared_device(xs, B, ys.device, "interpolate_batch: xs are [n, 4] or [B, n, 4]")
        if xs.shape[-2] != n:
            raise AssertionError("interpolate_batch: as many ys as xs")
        out = torch.empty((B, n, 4), dtype=torch.int64, device=ys.device)
        ctx = N.Context.get(ys.device.index)
        st = N.lib().zkhip_dense_points(ctx.handle, N.DENSE_INTERPOLATE, B, ys.data_ptr(), n, n, xs.data_ptr(), n if xs.dim() == 3 else 0,
                                        n, out.data_ptr(), n)
        if st == N.ERR_ARG:
            raise ValueError("interpolate: a node is repeated")
        N.check(st, "interpolate")
        return out

    def __mul__(self, other):
        """Mul (dense_univariate.rs:210-233): schoolbook product of the first degree()+1 coefficients in the reference,
        the same coefficients through three NTTs here; Mul<F> (:235-251) for a field element."""
        import torch
        if isinstance(other, DenseUnivariatePolynomial):
            if self.is_zero() or other.is_zero():
                return DenseUnivariatePolynomial(torch.empty((0, 4), dtype=torch.int64, device="cuda"))
            from zk_cryptography_amd.univariate import UnivariateEval
            a = DenseUnivariatePolynomial(self.coefficients[: self.degree() + 1])
            b = DenseUnivariatePolynomial(other.coefficients[: other.degree() + 1])
            return UnivariateEval.multiply(a, b)
        scalar = _fr_host(other).reshape(4)
        if self.is_zero() or not scalar.any():
            return DenseUnivariatePolynomial(torch.empty((0, 4), dtype=torch.int64, device="cuda"))
        return DenseUnivariatePolynomial((Multilinear._wrap(self.coefficients) * scalar).evaluations)


class TrustedSetup:
    """kzg/src/trusted_setup.rs:9-13, stored affine in HBM: G1 points int64 [n, 12], inf uint8 [n]; the G2 half (what `verify`
    needs) when asked for: powers_of_tau_in_g2 int64 [m, 24], g2_inf uint8 [m], else None."""

    def __init__(self, points_xy, inf, g2_xy=None, g2_inf=None):
        import torch
        if not isinstance(points_xy, torch.Tensor):
            points_xy = torch.from_numpy(np.ascontiguousarray(points_xy, dtype=np.uint64).view(np.int64)).cuda()
            inf = torch.from_numpy(np.ascontiguousarray(inf, dtype=np.uint8)).cuda()
        self.powers_of_tau_in_g1 = points_xy.contiguous()
        self.inf = inf.contiguous()
        if g2_xy is not None and not isinstance(g2_xy, torch.Tensor):
            g2_xy = torch.from_numpy(np.ascontiguousarray(g2_xy, dtype=np.uint64).reshape(-1, 24).view(np.int64)).cuda()
            g2_inf = torch.from_numpy(np.ascontiguousarray(g2_inf, dtype=np.uint8)).cuda()
        self.powers_of_tau_in_g2 = None if g2_xy is None else g2_xy.contiguous()
        self.g2_inf = None if g2_inf is None else g2_inf.contiguous()

    def g2_points(self):
        """the G2 half as a list of G2Affine"""
        if self.powers_of_tau_in_g2 is None:
            return []
        xy = self.powers_of_tau_in_g2.cpu().numpy().view(np.uint64)
        inf = self.g2_inf.cpu().numpy()
        return [G2Affine(xy[i], inf[i]) for i in range(xy.shape[0])]

    def __len__(self):
        return self.powers_of_tau_in_g1.shape[0]

    def _stamp(self):
        """Identity of the SRS the derived caches were built from: the tensors' storage and torch's in-place version counters (an
        in-place edit of `powers_of_tau_in_g1` / `inf`, or assigning new tensors, invalidates the shifted table and the folded levels)."""
        p, i = self.powers_of_tau_in_g1, self.inf
        g2 = getattr(self, "powers_of_tau_in_g2", None)
        g2s = () if g2 is None else (g2.data_ptr(), g2.shape[0], g2._version, self.g2_inf.data_ptr(), self.g2_inf._version)
        return (p.data_ptr(), p.shape[0], p._version, i.data_ptr(), i._version) + g2s

    def _fingerprint(self):
        """Content check for what the stamp cannot see -- writes through raw pointers (a kernel filling the tensors via data_ptr())
        and a new tensor that landed on the same address with the same shape and version: the first and last two points and their
        infinity flags (zkhip_srs_fingerprint: one small launch and one copy, ~20 us against a >= 1 ms commitment)."""
        p, i = self.powers_of_tau_in_g1, self.inf
        n = p.shape[0]
        if n == 0:
            return b""
        out = np.empty(52, dtype=np.uint64)
        ctx = N.Context.get(p.device.index)
        N.check(N.lib().zkhip_srs_fingerprint(ctx.handle, N.ptr(p), N.ptr(i), C.c_size_t(n), out.ctypes.data_as(C.c_void_p)), "srs_fingerprint")
        return out.tobytes()

    def _drop_tables(self):
        """The derived tables go: their addresses are released first (zkhip_table_release) -- the allocator may hand them to a buffer that
        is no table, and the library does not read the header of an address it remembers."""
        for t in (getattr(self, "_table", None), getattr(self, "_level_tables", None)):
            if t is not None:
                try:
                    N.lib().zkhip_table_release(N.Context.get(t.device.index).handle, N.ptr(t))
                except Exception:       # noqa: BLE001 -- interpreter shutdown
                    pass
        self._table = self._folded = self._level_tables = None
        self._prepared = {}

    def prepared_lines(self, univariate):
        """The Miller-loop lines of [G2, the G2 half] (multilinear) or [G2, tau G2] (univariate) that every `verify` against this SRS
        uses (zkhip_kzg_prepare, ~19 KiB per point): built once, kept with the other derived tables."""
        if self.powers_of_tau_in_g2 is None:
            raise ValueError("this TrustedSetup has no G2 half: build it with setup(..., g2=True) / generate_srs(..., g2=True)")
        self._check_caches()
        prepared = getattr(self, "_prepared", None)
        if prepared is None:
            prepared = self._prepared = {}
        if univariate not in prepared:
            import torch
            g2, inf = self.powers_of_tau_in_g2, self.g2_inf
            if univariate:
                if g2.shape[0] < 2:
                    raise IndexError("powers_of_tau_in_g2[1]: the G2 half has %d points" % g2.shape[0])
                g2, inf = g2[1:2], inf[1:2]
            n = g2.shape[0]
            buf = torch.empty(N.lib().zkhip_g2_prepared_bytes(C.c_size_t(n + 1)), dtype=torch.uint8, device=g2.device)
            ctx = N.Context.get(g2.device.index)
            _check_points(N.lib().zkhip_kzg_prepare(ctx.handle, N.ptr(g2), N.ptr(inf), C.c_size_t(n), N.ptr(buf)), "kzg_prepare")
            prepared[univariate] = buf
        return prepared[univariate]

    def __del__(self):
        self._drop_tables()

    def invalidate(self):
        """Drops the shifted table and the folded levels (call after writing the SRS through raw pointers; commitments in flight
        keep the table they were started with alive through their PendingCommitment)."""
        self._drop_tables()
        self._cache_stamp = self._cache_print = None

    def _check_caches(self):
        have = getattr(self, "_table", None) is not None or getattr(self, "_folded", None) is not None
        if getattr(self, "_cache_stamp", None) != self._stamp() or (have and getattr(self, "_cache_print", None) != self._fingerprint()):
            self._drop_tables()
            self._cache_stamp = self._stamp()
            self._cache_print = None

    def _caches_built(self):
        if getattr(self, "_cache_print", None) is None:
            self._cache_print = self._fingerprint()

    @property
    def table(self):
        """the shifted-SRS table, or None (never a stale one: see _stamp)"""
        self._check_caches()
        return getattr(self, "_table", None)

    SMALL_SRS = 4096      # zkhip_kzg_commit_table's short path (no sort, no buckets) serves commits of at most this many scalars

    def table_for(self, n_scalars):
        """the table a commitment of n_scalars coefficients should use: a SMALL SRS builds its table on first use (a few ms, a few
        MiB, once per SRS) -- the short commits of plonk-style callers then take two launches instead of the bucket pipeline"""
        t = self.table
        if t is None and 0 < n_scalars <= TrustedSetup.SMALL_SRS and 0 < len(self) <= TrustedSetup.SMALL_SRS:
            t = self.precompute().table
        return t

    def precompute(self):
        """Build (once) the shifted-SRS table 2^(first bit of window w) * point for the digit windows of a scalar (13 at 2^20): commitments then need
        13 instead of 16 bucket additions per point and one bucket reduction (zkhip_srs_precompute); 1.6 GiB at 2^20."""
        self._check_caches()
        if getattr(self, "_table", None) is None:
            import torch
            n = len(self)
            N.lib().zkhip_srs_table_bytes.restype = C.c_size_t
            nbytes = N.lib().zkhip_srs_table_bytes(C.c_size_t(n))
            table = torch.empty(nbytes, dtype=torch.uint8, device=self.powers_of_tau_in_g1.device)
            ctx = N.Context.get(table.device.index)
            N.check(N.lib().zkhip_srs_precompute(ctx.handle, N.ptr(self.powers_of_tau_in_g1), N.ptr(self.inf), C.c_size_t(n),
                                                 N.ptr(table)), "srs_precompute")
            self._table = table
            self._caches_built()
        return self

    def folded(self):
        """The SRS summed over its leading variables, level after level (n - 1 points): what commitments to the
        blown-up quotients of `open` reduce to.  Depends on the SRS only; derived once and kept."""
        self._check_caches()
        if getattr(self, "_folded", None) is None:
            n = len(self)
            xy, inf = TrustedSetup._alloc(n - 1)
            ctx = N.Context.get(self.powers_of_tau_in_g1.device.index)
            N.check(N.lib().zkhip_srs_fold_levels(ctx.handle, N.ptr(self.powers_of_tau_in_g1), N.ptr(self.inf), C.c_size_t(n),
                                                  N.ptr(xy), N.ptr(inf)), "srs_fold_levels")
            self._folded = (xy, inf)
            self._caches_built()
        return self._folded

    @property
    def level_tables(self):
        """the shifted tables of the folded levels, or None (never stale ones: see _stamp)"""
        self._check_caches()
        return getattr(self, "_level_tables", None)

    def precompute_open(self):
        """Build (once) the folded levels and their shifted tables 2^(c w) * S_i[j], c ~ log2 |S_i| (zkhip_srs_level_tables; 1.9 GiB at
        2^20): every `open` against this SRS then spends ~14 instead of ~18 bucket additions per quotient entry, reduces one bucket
        set per round and ends in a host epilogue of ~20 instead of 255 doublings per round."""
        n = len(self)
        if n < 4 or n & (n - 1):
            return self
        fxy, finf = self.folded()
        if getattr(self, "_level_tables", None) is None:
            import torch
            N.lib().zkhip_srs_level_tables_bytes.restype = C.c_size_t
            nbytes = N.lib().zkhip_srs_level_tables_bytes(C.c_size_t(n))
            tables = torch.empty(nbytes, dtype=torch.uint8, device=self.powers_of_tau_in_g1.device)
            ctx = N.Context.get(tables.device.index)
            N.check(N.lib().zkhip_srs_level_tables(ctx.handle, N.ptr(fxy), N.ptr(finf), C.c_size_t(n), N.ptr(tables)), "srs_level_tables")
            self._level_tables = tables
            self._caches_built()
        return self

    @staticmethod
    def _alloc(n):
        import torch
        return (torch.empty((n, 12), dtype=torch.int64, device="cuda"), torch.empty((n,), dtype=torch.uint8, device="cuda"))

    @staticmethod
    def setup(eval_points, g2=False):
        """TrustedSetup::setup (trusted_setup.rs:15-35): G * eq_i(tau) over the boolean hypercube, MSB first; with g2=True also
        generate_powers_of_tau_in_g2 (:37-45): tau_i * G2, what `verify` needs."""
        tau = _fr_host(eval_points)
        nv = tau.shape[0]
        pts, inf = TrustedSetup._alloc(1 << nv)
        ctx = N.Context.get()
        N.check(N.lib().zkhip_srs_multilinear_g1(ctx.handle, tau.ctypes.data_as(C.c_void_p), C.c_uint32(nv),
                                                 N.ptr(pts), N.ptr(inf)), "srs_multilinear")
        if not g2:
            return TrustedSetup(pts, inf)
        qxy, qinf = TrustedSetup._alloc_g2(nv)
        N.check(N.lib().zkhip_srs_multilinear_g2(ctx.handle, tau.ctypes.data_as(C.c_void_p), C.c_uint32(nv),
                                                 N.ptr(qxy), N.ptr(qinf)), "srs_multilinear_g2")
        return TrustedSetup(pts, inf, qxy, qinf)

    @staticmethod
    def _alloc_g2(n):
        import torch
        return (torch.zeros((n, 24), dtype=torch.int64, device="cuda"), torch.zeros((n,), dtype=torch.uint8, device="cuda"))


def _commit(points, inf, n_points, scalars, n_scalars, require_equal_len, table=None):
    """The commitment of `scalars` (a tensor, n_scalars of them) against the SRS -> G1Affine; a LIST of tensors with a list of lengths
    is a batch against the one SRS in one call (zkhip_kzg_commit_polys) -> a list of G1Affine, each what the single call returns."""
    if isinstance(scalars, (list, tuple)):
        b = len(scalars)
        if b == 0:
            return []
        for s in scalars:
            assert s.is_contiguous()
            if s.device != points.device:
                raise ValueError("commitment_batch: the polynomials must live on the device of the SRS")
        xy = np.zeros((b, 12), dtype=np.uint64)
        oinf = np.zeros(b, dtype=np.uint8)
        ptrs = (C.c_void_p * b)(*[s.data_ptr() if n else None for s, n in zip(scalars, n_scalars)])
        lens = (C.c_size_t * b)(*[int(n) for n in n_scalars])
        ctx = N.Context.get(points.device.index)
        vp = C.c_void_p
        st = N.lib().zkhip_kzg_commit_polys(ctx.handle, None if table is not None else N.ptr(points), N.ptr(table) if table is not None else None,
                                            N.ptr(inf), C.c_size_t(n_points), C.c_uint32(b), ptrs, lens, C.c_int(1 if require_equal_len else 0),
                                            xy.ctypes.data_as(vp), oinf.ctypes.data_as(vp))
        N.check(st, "The length of powers_of_tau_in_g1 and the length of the evaluations of the polynomial should tally!")
        return [G1Affine(xy[j], oinf[j]) for j in range(b)]
    out = np.empty(12, dtype=np.uint64)
    oinf = C.c_uint8(0)
    ctx = N.Context.get(points.device.index)
    if table is not None:
        st = N.lib().zkhip_kzg_commit_table(ctx.handle, N.ptr(table), N.ptr(inf), C.c_size_t(n_points), N.ptr(scalars),
                                            C.c_size_t(n_scalars), C.c_int(1 if require_equal_len else 0),
                                            out.ctypes.data_as(C.c_void_p), C.byref(oinf))
    else:
        st = N.lib().zkhip_kzg_commit(ctx.handle, N.ptr(points), N.ptr(inf), C.c_size_t(n_points), N.ptr(scalars),
                                      C.c_size_t(n_scalars), C.c_int(1 if require_equal_len else 0),
                                      out.ctypes.data_as(C.c_void_p), C.byref(oinf))
    N.check(st, "The length of powers_of_tau_in_g1 and the length of the evaluations of the polynomial should tally!")
    return G1Affine(out, oinf.value)


class PendingCommitment:
    """A commitment in flight (zkhip_kzg_commit_begin / _end): wait() delivers the G1Affine the synchronous call returns."""

    def __init__(self, ctx, ticket, keep):
        self._ctx, self._ticket, self._keep = ctx, ticket, keep     # `keep`: the tensors the kernels still read

    def wait(self):
        if self._ticket is None:
            raise RuntimeError("commitment already collected")
        out = np.empty(12, dtype=np.uint64)
        oinf = C.c_uint8(0)
        t, self._ticket = self._ticket, None
        N.check(N.lib().zkhip_kzg_commit_end(self._ctx.handle, C.c_uint32(t), out.ctypes.data_as(C.c_void_p), C.byref(oinf)), "commit_end")
        self._keep = None
        return G1Affine(out, oinf.value)

    def __del__(self):
        if getattr(self, "_ticket", None) is not None:
            try:
                N.lib().zkhip_kzg_commit_end(self._ctx.handle, C.c_uint32(self._ticket), None, None)
            except Exception:
                pass


def _commit_begin(points, inf, n_points, scalars, n_scalars, require_equal_len, table=None):
    ctx = N.Context.get(points.device.index)
    ticket = C.c_uint32(0)
    st = N.lib().zkhip_kzg_commit_begin(ctx.handle, None if table is not None else N.ptr(points), N.ptr(table) if table is not None else None,
                                        N.ptr(inf), C.c_size_t(n_points), N.ptr(scalars), C.c_size_t(n_scalars),
                                        C.c_int(1 if require_equal_len else 0), C.byref(ticket))
    N.check(st, "The length of powers_of_tau_in_g1 and the length of the evaluations of the polynomial should tally!")
    return PendingCommitment(ctx, ticket.value, (points, inf, scalars, table))


def commit_batch(points, inf, scalars, offsets):
    """zkhip_kzg_commit_batch: commitments of the slices [offsets[j], offsets[j+1]) of (points, scalars), one pass"""
    nprob = len(offsets) - 1
    xy = np.zeros((max(nprob, 1), 12), dtype=np.uint64)
    oinf = np.zeros(max(nprob, 1), dtype=np.uint8)
    offs = (C.c_size_t * len(offsets))(*[int(o) for o in offsets])
    ctx = N.Context.get(points.device.index)
    N.check(N.lib().zkhip_kzg_commit_batch(ctx.handle, N.ptr(points), N.ptr(inf), N.ptr(scalars), offs, C.c_uint32(nprob),
                                           xy.ctypes.data_as(C.c_void_p), oinf.ctypes.data_as(C.c_void_p)), "commit_batch")
    return [G1Affine(xy[j], oinf[j]) for j in range(nprob)]


class MultilinearKZGProof:
    """kzg/src/multilinear_kzg.rs:17-21: evaluation (Montgomery limbs, uint64 [4]) + one G1 proof per variable"""

    def __init__(self, evaluation, proofs):
        self.evaluation = evaluation
        self.proofs = proofs


class MultilinearKZG:
    @staticmethod
    def commitment(poly, srs):
        """MultilinearKZGInterface::commitment (multilinear_kzg.rs:33-48)"""
        assert isinstance(poly, Multilinear)
        return _commit(srs.powers_of_tau_in_g1, srs.inf, len(srs), poly.evaluations, len(poly), True, srs.table_for(len(poly)))

    @staticmethod
    def commitment_batch(polys, srs):
        """`commitment` of every polynomial of `polys` against the one SRS in one call (zkhip_kzg_commit_polys) -> a list of G1Affine,
        each limb for limb what `commitment` returns; the same object may appear several times.  A polynomial whose length is not the
        SRS's raises `commitment`'s AssertionError before anything is committed; [] returns []."""
        for p in polys:
            assert isinstance(p, Multilinear)
        if not polys:
            return []
        lens = [len(p) for p in polys]
        return _commit(srs.powers_of_tau_in_g1, srs.inf, len(srs), [p.evaluations for p in polys], lens, True, srs.table_for(max(lens)))

    @staticmethod
    def commitment_begin(poly, srs):
        """The same commitment, in flight: -> PendingCommitment (at most three at a time); .wait() yields the G1Affine."""
        assert isinstance(poly, Multilinear)
        return _commit_begin(srs.powers_of_tau_in_g1, srs.inf, len(srs), poly.evaluations, len(poly), True, srs.table)

    @staticmethod
    def _open_srs(srs, n, cache_folded_srs):
        """what an opening of n entries commits against -> (folded xy, folded inf, level tables): pointers to the SRS's folded levels and
        the tensor of their tables, or None where the call folds the SRS itself / runs without tables"""
        if not (cache_folded_srs and len(srs) == n and n >= 4 and n & (n - 1) == 0):
            return None, None, None
        fxy, finf = srs.folded()
        tables = getattr(srs, "_level_tables", None)       # present after srs.precompute_open(); folded() has just run the cache guard
        if tables is None and n <= TrustedSetup.SMALL_SRS:  # a small SRS builds them on first use (a few ms): its openings take the
            tables = srs.precompute_open()._level_tables    # short path, two launches for all rounds (zkhip_kzg_open_tables)
        return N.ptr(fxy), N.ptr(finf), tables

    @staticmethod
    def open(poly, evaluation_points, srs, cache_folded_srs=True):
        """MultilinearKZGInterface::open (multilinear_kzg.rs:50-88)"""
        assert isinstance(poly, Multilinear)
        pts = _fr_host(evaluation_points)
        nv = pts.shape[0]
        ev = np.empty(4, dtype=np.uint64)
        pxy = np.zeros((max(nv, 1), 12), dtype=np.uint64)
        pinf = np.zeros(max(nv, 1), dtype=np.uint8)
        ctx = N.Context.get(poly.evaluations.device.index)
        n = len(poly)
        fxy_p, finf_p, tables = MultilinearKZG._open_srs(srs, n, cache_folded_srs)
        st = N.lib().zkhip_kzg_open_tables(ctx.handle, N.ptr(poly.evaluations), C.c_size_t(n), pts.ctypes.data_as(C.c_void_p),
                                           C.c_size_t(nv), N.ptr(srs.powers_of_tau_in_g1), N.ptr(srs.inf), C.c_size_t(len(srs)),
                                           fxy_p, finf_p, N.ptr(tables) if tables is not None else None,
                                           ev.ctypes.data_as(C.c_void_p), pxy.ctypes.data_as(C.c_void_p),
                                           pinf.ctypes.data_as(C.c_void_p))
        N.check(st, "open: points / SRS length must match the polynomial (and n_vars >= 2)")
        return MultilinearKZGProof(ev, [G1Affine(pxy[i], pinf[i]) for i in range(nv)])

    @staticmethod
    def open_batch(polys, evaluation_points, srs, cache_folded_srs=True):
        """`open` of polys[b] at evaluation_points[b] for every b against one SRS in one call (zkhip_kzg_open_batch) -> a list of
        MultilinearKZGProof, each bit for bit what `open` returns.  The polynomials have one length; the same object may appear several
        times (one polynomial at several points).  With at most 2^12 entries the whole batch shares three launches."""
        b = len(polys)
        if len(evaluation_points) != b:
            raise AssertionError("open_batch: one point vector per polynomial")
        if b == 0:
            return []
        for p in polys:
            assert isinstance(p, Multilinear)
        n = len(polys[0])
        pts = [_fr_host(v) for v in evaluation_points]
        nv = pts[0].shape[0]
        for i in range(b):
            if len(polys[i]) != n:
                raise AssertionError("open_batch: the polynomials must have one length")
            if pts[i].shape[0] != nv:
                raise AssertionError("open_batch: the point vectors must have one length")
        device = polys[0].evaluations.device
        for p in polys:
            if p.evaluations.device != device:
                raise ValueError("open_batch: the polynomials must live on one device")
        z = np.ascontiguousarray(np.stack(pts).reshape(b * nv, 4)) if nv else np.zeros((1, 4), dtype=np.uint64)
        ev = np.empty((b, 4), dtype=np.uint64)
        pxy = np.zeros((b * max(nv, 1), 12), dtype=np.uint64)
        pinf = np.zeros(b * max(nv, 1), dtype=np.uint8)
        ctx = N.Context.get(device.index)
        fxy_p, finf_p, tables = MultilinearKZG._open_srs(srs, n, cache_folded_srs)
        for p in polys:
            assert p.evaluations.is_contiguous()
        ptrs = (C.c_void_p * b)(*[p.evaluations.data_ptr() for p in polys])
        vp = C.c_void_p
        st = N.lib().zkhip_kzg_open_batch(ctx.handle, C.c_uint32(b), ptrs, C.c_size_t(n), z.ctypes.data_as(vp), C.c_size_t(nv),
                                          N.ptr(srs.powers_of_tau_in_g1), N.ptr(srs.inf), C.c_size_t(len(srs)), fxy_p, finf_p,
                                          N.ptr(tables) if tables is not None else None, ev.ctypes.data_as(vp), pxy.ctypes.data_as(vp),
                                          pinf.ctypes.data_as(vp))
        N.check(st, "open_batch: points / SRS length must match the polynomials (and n_vars >= 2)")
        return [MultilinearKZGProof(ev[i].copy(), [G1Affine(pxy[i * nv + k], pinf[i * nv + k]) for k in range(nv)]) for i in range(b)]

    @staticmethod
    def verify(commit, verifier_points, proof, srs):
        """MultilinearKZGInterface::verify (multilinear_kzg.rs:90-112) -> bool"""
        return bool(MultilinearKZG.verify_batch([commit], [verifier_points], [proof], srs)[0])

    @staticmethod
    def verify_batch(commits, verifier_points, proofs, srs):
        """`verify` of many openings of the same number of variables against one SRS in one pass -> np.ndarray[bool]"""
        b = len(commits)
        if not (len(verifier_points) == len(proofs) == b):
            raise AssertionError("verify_batch: one point vector and one proof per commitment")
        if srs.powers_of_tau_in_g2 is None:
            srs.prepared_lines(False)                       # raises the missing-G2 error
        n_g2 = len(srs.powers_of_tau_in_g2)
        pts = [_fr_host(v) for v in verifier_points]
        nv = pts[0].shape[0] if b else n_g2
        for i in range(b):
            if pts[i].shape[0] != nv or len(proofs[i].proofs) != nv:
                raise AssertionError("Length mismatch")
        if nv != n_g2:
            raise AssertionError("Length mismatch")         # sum_pairing_results (utils.rs:49-50)
        prep = srs.prepared_lines(False)
        cxy, cinf = _g1_arrays(commits)
        pxy, pinf = _g1_arrays([q for p in proofs for q in p.proofs])
        ev = np.zeros((max(b, 1), 4), dtype=np.uint64)
        z = np.zeros((max(b * nv, 1), 4), dtype=np.uint64)
        for i in range(b):
            ev[i] = np.asarray(proofs[i].evaluation, dtype=np.uint64).reshape(4)
            z[i * nv: (i + 1) * nv] = pts[i]
        ok = np.zeros(max(b, 1), dtype=np.uint8)
        ctx = N.Context.get(prep.device.index)
        vp = C.c_void_p
        st = N.lib().zkhip_kzg_verify_batch(ctx.handle, C.c_size_t(b), C.c_uint32(nv), cxy.ctypes.data_as(vp), cinf.ctypes.data_as(vp),
                                            ev.ctypes.data_as(vp), z.ctypes.data_as(vp), pxy.ctypes.data_as(vp), pinf.ctypes.data_as(vp),
                                            N.ptr(srs.powers_of_tau_in_g2), N.ptr(srs.g2_inf), C.c_size_t(n_g2), N.ptr(prep),
                                            ok.ctypes.data_as(vp))
        _check_points(st, "multilinear verify")
        return ok[:b].astype(bool)


class UnivariateKZGProof:
    """kzg/src/univariate_kzg.rs:11-15: evaluation (Montgomery limbs uint64 [4]) + the quotient's commitment"""

    def __init__(self, evaluation, proof):
        self.evaluation = evaluation
        self.proof = proof


class UnivariateKZG:
    @staticmethod
    def open(poly, evaluation_point, srs):
        """UnivariateKZGInterface::open (univariate_kzg.rs:60-81); a LIST of polynomials with a list of points is a batch against the
        one SRS in one call (zkhip_univariate_kzg_open_batch) -> a list of UnivariateKZGProof, each what the single call returns."""
        if isinstance(poly, (list, tuple)):
            b = len(poly)
            if b == 0:
                return []
            for p in poly:
                if len(p) and p.coefficients.device != srs.powers_of_tau_in_g1.device:
                    raise ValueError("open_batch: the polynomials must live on the device of the SRS")
            z = np.ascontiguousarray(np.stack([_fr_host(e).reshape(4) for e in evaluation_point]), dtype=np.uint64)
            ev, xy, oinf = np.zeros((b, 4), dtype=np.uint64), np.zeros((b, 12), dtype=np.uint64), np.zeros(b, dtype=np.uint8)
            ptrs = (C.c_void_p * b)(*[p.coefficients.data_ptr() if len(p) else None for p in poly])
            lens = (C.c_size_t * b)(*[len(p) for p in poly])
            table = srs.table_for(max(lens) - 1) if max(lens) > 1 else None      # the quotients are what is committed
            ctx = N.Context.get(srs.powers_of_tau_in_g1.device.index)
            vp = C.c_void_p
            st = N.lib().zkhip_univariate_kzg_open_batch(ctx.handle, C.c_uint32(b), ptrs, lens, z.ctypes.data_as(vp),
                                                         None if table is not None else N.ptr(srs.powers_of_tau_in_g1),
                                                         N.ptr(table) if table is not None else None, N.ptr(srs.inf), C.c_size_t(len(srs)),
                                                         ev.ctypes.data_as(vp), xy.ctypes.data_as(vp), oinf.ctypes.data_as(vp))
            N.check(st, "univariate open")
            return [UnivariateKZGProof(ev[j].copy(), G1Affine(xy[j], oinf[j])) for j in range(b)]
        assert isinstance(poly, DenseUnivariatePolynomial)
        z = _fr_host(evaluation_point).reshape(4)
        ev, xy, inf = np.empty(4, dtype=np.uint64), np.empty(12, dtype=np.uint64), C.c_uint8(0)
        ctx = N.Context.get(srs.powers_of_tau_in_g1.device.index)
        st = N.lib().zkhip_univariate_kzg_open(ctx.handle, N.ptr(poly.coefficients) if len(poly) else None, C.c_size_t(len(poly)),
                                               z.ctypes.data_as(C.c_void_p), N.ptr(srs.powers_of_tau_in_g1), N.ptr(srs.inf),
                                               C.c_size_t(len(srs)), ev.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p),
                                               C.byref(inf))
        N.check(st, "univariate open")
        return UnivariateKZGProof(ev, G1Affine(xy, inf.value))

    @staticmethod
    def open_batch(polys, evaluation_points, srs):
        """`open` of polys[b] at evaluation_points[b], for every b, against the one SRS in one call (zkhip_univariate_kzg_open_batch)
        -> a list of UnivariateKZGProof, each limb for limb what `open` returns.  The polynomials may differ in length and may repeat
        (one polynomial at several points); one too long for the SRS raises `open`'s IndexError before anything is opened."""
        polys = list(polys)
        evaluation_points = list(evaluation_points)
        for p in polys:
            assert isinstance(p, DenseUnivariatePolynomial)
        assert len(polys) == len(evaluation_points), "open_batch: one evaluation point per polynomial"
        if not polys:
            return []
        return UnivariateKZG.open(polys, evaluation_points, srs)

    @staticmethod
    def generate_srs(tau, max_degree, g2=False):
        """UnivariateKZGInterface::generate_srs (univariate_kzg.rs:18-35): G1 powers; with g2=True also the G2 powers tau^i G2"""
        t = _fr_host(tau)
        pts, inf = TrustedSetup._alloc(max_degree + 1)
        ctx = N.Context.get()
        N.check(N.lib().zkhip_srs_univariate_g1(ctx.handle, t.ctypes.data_as(C.c_void_p), C.c_size_t(max_degree),
                                                N.ptr(pts), N.ptr(inf)), "srs_univariate")
        if not g2:
            return TrustedSetup(pts, inf)
        qxy, qinf = TrustedSetup._alloc_g2(max_degree + 1)
        N.check(N.lib().zkhip_srs_univariate_g2(ctx.handle, t.ctypes.data_as(C.c_void_p), C.c_size_t(max_degree),
                                                N.ptr(qxy), N.ptr(qinf)), "srs_univariate_g2")
        return TrustedSetup(pts, inf, qxy, qinf)

    @staticmethod
    def verify(commit, verifier_point, proof, srs):
        """UnivariateKZGInterface::verify (univariate_kzg.rs:83-104) -> bool"""
        return bool(UnivariateKZG.verify_batch([commit], [verifier_point], [proof], srs)[0])

    @staticmethod
    def verify_batch(commits, verifier_points, proofs, srs):
        """`verify` of many openings against one SRS in one pass -> np.ndarray[bool], one verdict per opening"""
        b = len(commits)
        if not (len(verifier_points) == len(proofs) == b):
            raise AssertionError("verify_batch: one point and one proof per commitment")
        prep = srs.prepared_lines(True)
        cxy, cinf = _g1_arrays(commits)
        pxy, pinf = _g1_arrays([p.proof for p in proofs])
        ev = np.zeros((max(b, 1), 4), dtype=np.uint64)
        z = np.zeros((max(b, 1), 4), dtype=np.uint64)
        for i in range(b):
            ev[i] = np.asarray(proofs[i].evaluation, dtype=np.uint64).reshape(4)
            z[i] = _fr_host(verifier_points[i]).reshape(4)
        ok = np.zeros(max(b, 1), dtype=np.uint8)
        ctx = N.Context.get(prep.device.index)
        vp = C.c_void_p
        st = N.lib().zkhip_univariate_kzg_verify_batch(ctx.handle, C.c_size_t(b), cxy.ctypes.data_as(vp), cinf.ctypes.data_as(vp),
                                                       ev.ctypes.data_as(vp), z.ctypes.data_as(vp), pxy.ctypes.data_as(vp),
                                                       pinf.ctypes.data_as(vp), N.ptr(srs.powers_of_tau_in_g2), N.ptr(srs.g2_inf),
                                                       C.c_size_t(len(srs.powers_of_tau_in_g2)), N.ptr(prep), ok.ctypes.data_as(vp))
        _check_points(st, "univariate verify")
        return ok[:b].astype(bool)

    @staticmethod
    def commitment(poly, srs):
        """UnivariateKZGInterface::commitment (univariate_kzg.rs:37-58): no length assert; a polynomial longer
        than the SRS indexes out of bounds (IndexError), exactly what the unregistered bench would hit."""
        assert isinstance(poly, DenseUnivariatePolynomial)
        return _commit(srs.powers_of_tau_in_g1, srs.inf, len(srs), poly.coefficients, len(poly), False, srs.table_for(len(poly)))

    @staticmethod
    def commitment_batch(polys, srs):
        """`commitment` of every polynomial of `polys` against the one SRS in one call (zkhip_kzg_commit_polys) -> a list of G1Affine,
        each limb for limb what `commitment` returns.  The polynomials may differ in length (the zero polynomial commits to the
        identity); one with more coefficients than the SRS has points raises `commitment`'s IndexError before anything is committed."""
        for p in polys:
            assert isinstance(p, DenseUnivariatePolynomial)
        if not polys:
            return []
        lens = [len(p) for p in polys]
        return _commit(srs.powers_of_tau_in_g1, srs.inf, len(srs), [p.coefficients for p in polys], lens, False, srs.table_for(max(lens)))
