"""GPU: every kernel of csrc/plonk_batch_kernels.hpp through tests/cpp/plonk_batch_driver.hip, against python integers
(tests/plonk_model.py and the references of tests/test_gpu_plonk_kernels.py).  A launch serves B = 1 and 3 proofs whose areas lie `ws`
elements apart in ONE buffer that starts as a byte pattern; every per-proof parameter (the row of `par`) is drawn per proof, so a kernel
that reads another proof's row, or writes another proof's area, gives a wrong element somewhere.  After each launch the test compares
the WHOLE buffer with what it should hold: the outputs, the inputs unchanged, the pattern everywhere else -- between the rows, between
the areas and behind the last one.  Shapes: 1023 / 1024 / 1025 rows are the edges of one grand-product workgroup; (32, 8) and (4096, 4)
the two coset ratios of the quotient; 1, 10 and 1030 coefficients are one lane, one partial lane and more than one lane's loop of the
linearisation, and for the Horner scan (2048 coefficients per workgroup) 1030 and 2049 together are jobs of one and two workgroups in
one launch."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_batch_driver as DRV  # noqa: E402
import plonk_model as PL  # noqa: E402
from test_gpu_plonk_kernels import GP_COLUMNS, PATTERN, column, dev, gp_reference, hp, launched, pack, stream  # noqa: E402

pytestmark = pytest.mark.gpu
R = PL.R
SLOTS = 40
BETA, GAMMA, ALPHA, ALPHA2, BLIND, ZETA, ZETA_W, LIN, C0 = 0, 1, 2, 3, 4, 15, 16, 17, 32
BATCHES = [1, 3]


class Arena:
    """B areas of ws elements and a guard of 8, all pattern; `want` mirrors what the device buffer should hold (None = pattern)"""

    def __init__(self, B, ws, flags_at=None):
        import torch
        self.B, self.ws = B, ws
        self.buf = torch.full((B * ws + 8, 4), PATTERN, dtype=torch.int64, device="cuda")
        self.want = np.full((B * ws + 8, 4), PATTERN, dtype=np.uint64)
        self.flags_at = flags_at
        if flags_at is not None:                                # four ints at element flags_at of every area, zero as the prover clears them
            for b in range(B):
                self.want[b * ws + flags_at] = 0
                self.buf[b * ws + flags_at] = 0

    def ptr(self, off):
        """the address of element `off` of proof 0's area"""
        return self.buf.data_ptr() + 32 * off

    def put(self, off, rows):
        """rows[b]: the ints proof b holds from `off` on, as inputs"""
        import torch
        for b, vals in enumerate(rows):
            limbs = pack(vals)
            at = b * self.ws + off
            assert off + len(vals) <= self.ws
            self.want[at:at + len(vals)] = limbs
            self.buf[at:at + len(vals)] = torch.from_numpy(limbs.view(np.int64)).cuda()

    def expect(self, off, rows):
        for b, vals in enumerate(rows):
            at = b * self.ws + off
            assert off + len(vals) <= self.ws
            self.want[at:at + len(vals)] = pack(vals)

    def expect_flags(self, rows):
        for b, f in enumerate(rows):
            self.want[b * self.ws + self.flags_at] = np.array(f, dtype=np.int32).view(np.uint64).tolist() + [0, 0]

    def flags_ptr(self):
        return self.ptr(self.flags_at)

    def check(self, what, ignore=()):
        got = self.buf.cpu().numpy().view(np.uint64)
        want = self.want
        if ignore:                                              # (offset, length) per proof: scratch whose content is checked elsewhere or not defined
            got, want = got.copy(), want.copy()
            for off, length in ignore:
                for b in range(self.B):
                    got[b * self.ws + off:b * self.ws + off + length] = 0
                    want[b * self.ws + off:b * self.ws + off + length] = 0
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).any(axis=1))[0]
            raise AssertionError("%s: %d elements differ, the first at proof %d offset %d" % (what, len(bad), bad[0] // self.ws, bad[0] % self.ws))


def params(B, seed):
    """-> (ints [B][SLOTS], device table): every slot of every proof a value of its own"""
    rng = random.Random(seed)
    rows = [[rng.randrange(R) for _ in range(SLOTS)] for _ in range(B)]
    return rows, dev([v for row in rows for v in row])


def vec(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def host_ptrs(addresses):
    return np.array(addresses, dtype=np.uint64)


@pytest.mark.parametrize("B", BATCHES)
def test_gather(B):
    import torch
    n, ws, rng = 300, 1300, random.Random(B)
    cols = [[vec(rng, n) for _ in range(4)] for _ in range(B)]
    tensors = [[dev(c) for c in row] for row in cols]
    table = torch.tensor([t.data_ptr() for row in tensors for t in row], dtype=torch.int64, device="cuda")
    for grid in (1, 2):
        ar = Arena(B, ws)
        launched(DRV.lib().plonk_batch_driver_gather(table.data_ptr(), n, ar.ptr(40), ws, B, grid, stream()))
        ar.expect(40, [[v for c in row for v in c] for row in cols])
        ar.check("gather")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("m,k", [(3, 2), (1, 3)])
def test_blind(B, m, k):
    n, ws, rng = 8, 64, random.Random(10 * B + m)
    par, d_par = params(B, 50 + B)
    offs = [0, 16, 32][:m]
    slots = [[1, 0, 0], [3, 2, 0], [5, 4, 0]] if m == 3 else [[6, 7, 8]]
    polys = [[vec(rng, n) + [0] * k for _ in range(B)] for _ in range(m)]
    ar = Arena(B, ws)
    for q in range(m):
        ar.put(offs[q], polys[q])
    ptrs, sl = host_ptrs([ar.ptr(o) for o in offs]), np.array(slots, dtype=np.uint8)
    launched(DRV.lib().plonk_batch_driver_blind(hp(ptrs), m, hp(sl), n, k, d_par.data_ptr(), ws, B, stream()))
    for q in range(m):
        rows = []
        for b in range(B):
            p = list(polys[q][b])
            for j in range(k):
                bj = par[b][BLIND + slots[q][j]]
                p[j], p[n + j] = (p[j] - bj) % R, bj
            rows.append(p)
        ar.expect(offs[q], rows)
    ar.check("blind")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_grand_product(B, n):
    L = DRV.lib()
    rows_per_block = L.plonk_batch_driver_gp_rows()
    nb = (n + rows_per_block - 1) // rows_per_block
    rng = random.Random(n + B)
    shared = {name: column(rng, n) for name in ["w"] + GP_COLUMNS}
    d_shared = {k: dev(v) for k, v in shared.items()}
    cols = host_ptrs([d_shared[k].data_ptr() for k in GP_COLUMNS])
    par, d_par = params(B, n)
    o_a, o_b, o_c, o_pub, o_f, o_acc, o_bp, o_bx, o_flags = 0, 1032, 2064, 3096, 4128, 5160, 6192, 6200, 6208
    ws = 6216
    wires = {name: [column(rng, n) for _ in range(B)] for name in ("a", "b", "c", "pub")}
    ar = Arena(B, ws, flags_at=o_flags)
    for name, off in (("a", o_a), ("b", o_b), ("c", o_c), ("pub", o_pub)):
        ar.put(off, wires[name])
    launched(L.plonk_batch_driver_gp_ratio(ar.ptr(o_a), ar.ptr(o_b), ar.ptr(o_c), ar.ptr(o_pub), hp(cols), d_shared["w"].data_ptr(), n, d_par.data_ptr(),
                                           ar.ptr(o_f), ar.ptr(o_bp), ar.flags_ptr(), ws, 8 * ws, B, stream()))
    launched(L.plonk_batch_driver_gp_top(ar.ptr(o_bp), nb, ar.ptr(o_bx), ws, B, stream()))
    launched(L.plonk_batch_driver_gp_apply(ar.ptr(o_f), ar.ptr(o_bx), n, ar.ptr(o_acc), ar.flags_ptr(), ws, 8 * ws, B, stream()))
    refs = [gp_reference(dict(shared, **{k: wires[k][b] for k in wires}), n, par[b][BETA], par[b][GAMMA], rows_per_block) for b in range(B)]
    assert all(r["flags"][1] == 0 for r in refs)
    for key, off in (("f", o_f), ("acc", o_acc), ("block_prod", o_bp), ("block_excl", o_bx)):
        ar.expect(off, [r[key] for r in refs])
    ar.expect_flags([r["flags"] for r in refs])
    assert all(r["flags"][0] == 1 for r in refs)                # arbitrary columns break the gate: the flag is every proof's own
    ar.check("grand product")


@pytest.mark.parametrize("B", BATCHES)
def test_grand_product_flags_are_per_proof(B):
    """a satisfied circuit in every proof but the last, whose gate is broken in one row: only its flags are raised"""
    L = DRV.lib()
    n, ws, o_flags = 64, 8 * 64, 8 * 64 - 8
    cpi, _ = PL.random_circuit(n, random.Random(3), random.Random(4))
    wits = [PL.random_circuit(n, random.Random(3), random.Random(40 + b))[1] for b in range(B)]
    wits[B - 1] = dict(wits[B - 1], c=[(v + 1) % R if i == 5 else v for i, v in enumerate(wits[B - 1]["c"])])
    shared = dict(w=PL.roots_of_unity(n), q_m=cpi["q_m"], q_l=cpi["q_l"], q_r=cpi["q_r"], q_o=cpi["q_o"], q_c=cpi["q_c"], s1=cpi["sigma_1"],
                  s2=cpi["sigma_2"], s3=cpi["sigma_3"])
    d_shared = {k: dev(v) for k, v in shared.items()}
    cols = host_ptrs([d_shared[k].data_ptr() for k in GP_COLUMNS])
    par, d_par = params(B, 77)
    ar = Arena(B, ws, flags_at=o_flags)
    for j, name in enumerate(("a", "b", "c", "public_poly")):
        ar.put(64 * j, [w[name] for w in wits])
    launched(L.plonk_batch_driver_gp_ratio(ar.ptr(0), ar.ptr(64), ar.ptr(128), ar.ptr(192), hp(cols), d_shared["w"].data_ptr(), n, d_par.data_ptr(),
                                           ar.ptr(256), ar.ptr(384), ar.flags_ptr(), ws, 8 * ws, B, stream()))
    launched(L.plonk_batch_driver_gp_top(ar.ptr(384), 1, ar.ptr(392), ws, B, stream()))
    launched(L.plonk_batch_driver_gp_apply(ar.ptr(256), ar.ptr(392), n, ar.ptr(320), ar.flags_ptr(), ws, 8 * ws, B, stream()))
    refs = [gp_reference(dict(shared, a=w["a"], b=w["b"], c=w["c"], pub=w["public_poly"]), n, par[b][BETA], par[b][GAMMA], 1024) for b, w in enumerate(wits)]
    assert [r["flags"] for r in refs] == [[0, 0, 0, 0]] * (B - 1) + [[1, 0, 1, 0]]
    for key, off in (("f", 256), ("acc", 320), ("block_prod", 384), ("block_excl", 392)):
        ar.expect(off, [r[key] for r in refs])
    ar.expect_flags([r["flags"] for r in refs])
    ar.check("grand product flags")


@pytest.mark.parametrize("B", BATCHES)
def test_scale_pad(B):
    D, rng = 512, random.Random(B + 5)
    lens = [10, 300, 512, 1, 259]                               # the five sources are the proof's own: they lie in its area behind the five rows
    mul = vec(rng, D)
    d_mul = dev(mul)
    offs, srcs, at = [], [], 5 * D
    for length in lens:
        offs.append(at)
        srcs.append([vec(rng, length) for _ in range(B)])
        at += length + (8 - length % 8) % 8
    ws = at + 8
    ar = Arena(B, ws)
    for off, rows in zip(offs, srcs):
        ar.put(off, rows)
    ptrs, hl = host_ptrs([ar.ptr(o) for o in offs]), np.array(lens, dtype=np.uint32)
    ar.expect(0, [[(srcs[j][b][i] * mul[i] % R if i < lens[j] else 0) for j in range(5) for i in range(D)] for b in range(B)])
    for grid in (1, 2):
        launched(DRV.lib().plonk_batch_driver_scale_pad(hp(ptrs), hp(hl), d_mul.data_ptr(), D, ar.ptr(0), ws, B, grid, stream()))
        ar.check("scale_pad grid %d" % grid)


def quotient_reference(ev, pre, D, rot, beta, gamma, alpha, alpha2, zh_inv):
    out = []
    for j in range(D):
        a, b, c, z, pi = (ev[k][j] for k in range(5))
        zw = ev[3][(j + rot) % D]
        qm, ql, qr, qo, qc, s1, s2, s3, l1, x = (pre[k][j] for k in range(10))
        gate = a * b * qm + a * ql + b * qr + c * qo + pi + qc
        p1 = (a + beta * x + gamma) * (b + 2 * beta * x + gamma) * (c + 3 * beta * x + gamma) * z
        p2 = (a + beta * s1 + gamma) * (b + beta * s2 + gamma) * (c + beta * s3 + gamma) * zw
        out.append((gate + alpha * (p1 - p2) + alpha2 * (z - 1) * l1) * zh_inv[j % rot] % R)
    return out


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D,rot", [(32, 8), (4096, 4)])
def test_quotient(B, D, rot):
    rng = random.Random(D + B)
    ws = 6 * D + 8
    pre = [vec(rng, D) for _ in range(10)]
    d_pre = dev([v for c in pre for v in c])
    zh_inv = vec(rng, rot) + [0] * (8 - rot)
    zi = pack(zh_inv)
    par, d_par = params(B, D)
    evs = [[vec(rng, D) for _ in range(5)] for _ in range(B)]
    want = [quotient_reference(evs[b], pre, D, rot, par[b][BETA], par[b][GAMMA], par[b][ALPHA], par[b][ALPHA2], zh_inv) for b in range(B)]
    flat = [[v for c in ev for v in c] for ev in evs]
    for grid in sorted({1, (D + 255) // 256}):                  # one workgroup per proof (every lane loops), and the prover's grid
        ar = Arena(B, ws)
        ar.put(0, flat)
        launched(DRV.lib().plonk_batch_driver_quotient(ar.ptr(0), d_pre.data_ptr(), D, rot, hp(zi), d_par.data_ptr(), ar.ptr(5 * D), ws, B, grid, stream()))
        ar.expect(5 * D, want)
        ar.check("quotient grid %d" % grid)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n,D,dirty", [(4, 32, False), (8, 32, True), (300, 1024, False)])
def test_split(B, n, D, dirty):
    rng = random.Random(n + B)
    o_t, o_tl, o_tm, o_th = 0, D, D + n + 8, D + 2 * n + 16
    o_flags = o_th + n + 8
    ws = o_flags + 8
    ginv = vec(rng, 3 * n + 6)
    d_ginv = dev(ginv)
    par, d_par = params(B, n)
    ts = [vec(rng, 3 * n + 6) + [0] * (D - 3 * n - 6) for _ in range(B)]
    if dirty:
        ts[B - 1][D - 1] = 1                                    # Z_H does not divide the LAST proof's numerator: its flag alone
    for grid in sorted({1, (D + 255) // 256}):
        ar = Arena(B, ws, flags_at=o_flags)
        ar.put(o_t, ts)
        launched(DRV.lib().plonk_batch_driver_split(ar.ptr(o_t), d_ginv.data_ptr(), n, D, d_par.data_ptr(), ar.ptr(o_tl), ar.ptr(o_tm), ar.ptr(o_th),
                                                    ar.flags_ptr(), ws, 8 * ws, B, grid, stream()))
        tl, tm, th = [], [], []
        for b in range(B):
            u = [ts[b][i] * ginv[i] % R for i in range(3 * n + 6)]
            b10, b11 = par[b][BLIND + 9], par[b][BLIND + 10]
            tl.append(u[:n] + [b10])
            tm.append([(u[n] - b10) % R] + u[n + 1:2 * n] + [b11])
            th.append([(u[2 * n] - b11) % R] + u[2 * n + 1:])
        ar.expect(o_tl, tl); ar.expect(o_tm, tm); ar.expect(o_th, th)
        ar.expect_flags([[0, 0, 0, int(dirty and b == B - 1)] for b in range(B)])
        ar.check("split grid %d" % grid)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("length", [1, 10, 1030])
def test_linearise(B, length):
    rng = random.Random(length + B)
    own_terms = [5, 7, 8, 9, 10, 11, 12]                         # the prover's split: z, the parts of t, the wires are the proof's own
    own = sum(1 << q for q in own_terms)
    stride = length + (8 - length % 8) % 8
    ws = stride * (len(own_terms) + 1) + 8
    shared = {q: vec(rng, length) for q in range(15) if q not in own_terms}
    d_shared = {q: dev(v) for q, v in shared.items()}
    mine = {q: [vec(rng, length) for _ in range(B)] for q in own_terms}
    par, d_par = params(B, length)
    o_out = stride * len(own_terms)
    for grid in sorted({1, (length + 255) // 256}):
        ar = Arena(B, ws)
        for k, q in enumerate(own_terms):
            ar.put(stride * k, mine[q])
        ptrs = host_ptrs([ar.ptr(stride * own_terms.index(q)) if q in own_terms else d_shared[q].data_ptr() for q in range(15)])
        launched(DRV.lib().plonk_batch_driver_linearise(hp(ptrs), own, length, d_par.data_ptr(), ar.ptr(o_out), ws, B, grid, stream()))
        rows = []
        for b in range(B):
            term = lambda q, i: (mine[q][b] if q in own_terms else shared[q])[i]
            rows.append([(sum(par[b][LIN + q] * term(q, i) for q in range(15)) + (par[b][C0] if i == 0 else 0)) % R for i in range(length)])
        ar.expect(o_out, rows)
        ar.check("linearise grid %d" % grid)


def horner(coeffs, z):
    """-> (p(z), the coefficients of (p(X) - p(z)) / (X - z))"""
    v, out = 0, []
    for c in reversed(coeffs):
        v = (c + z * v) % R
        out.append(v)
    out.reverse()
    return out[0], out[1:]


HORNER_JOBS = {                                                 # lengths of the jobs of one launch
    "one": [1], "ten": [10], "1030": [1030],
    "unequal": [1030, 1, 2049, 10, 2048, 7, 300],               # one and two workgroups, and jobs of a single lane, in one launch
}


def horner_setup(B, lens, seed):
    rng = random.Random(seed)
    L = DRV.lib()
    rows = L.plonk_batch_driver_horner_rows()
    vstride = max((n + rows - 1) // rows for n in lens) + 1
    njobs = len(lens)
    own_jobs = [j for j in range(njobs) if j % 3 != 1]           # every third job reads a polynomial all proofs share
    own = sum(1 << j for j in own_jobs)
    zslot = [ZETA_W if j % 2 else ZETA for j in range(njobs)]
    offs, at = {}, 0
    for j in own_jobs:
        offs[j] = at
        at += lens[j] + (8 - lens[j] % 8) % 8
    shared = {j: vec(rng, lens[j]) for j in range(njobs) if j not in own_jobs}
    mine = {j: [vec(rng, lens[j]) for _ in range(B)] for j in own_jobs}
    return dict(rng=rng, vstride=vstride, njobs=njobs, own_jobs=own_jobs, own=own, zslot=zslot, offs=offs, end=at, shared=shared, mine=mine,
                d_shared={j: dev(v) for j, v in shared.items()})


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("jobs", list(HORNER_JOBS))
def test_horner_evaluations(B, jobs):
    lens = HORNER_JOBS[jobs]
    s = horner_setup(B, lens, 7 * B + len(lens))
    par, d_par = params(B, 900 + len(lens))
    scratch = s["njobs"] * s["vstride"]
    o_hv, o_hc, o_ev = s["end"], s["end"] + scratch, s["end"] + 2 * scratch
    ws = o_ev + 8
    ar = Arena(B, ws)
    for j in s["own_jobs"]:
        ar.put(s["offs"][j], s["mine"][j])
    ptrs = host_ptrs([ar.ptr(s["offs"][j]) if j in s["own_jobs"] else s["d_shared"][j].data_ptr() for j in range(s["njobs"])])
    hl, hz = np.array(lens, dtype=np.uint32), np.array(s["zslot"], dtype=np.uint8)
    launched(DRV.lib().plonk_batch_driver_horner_eval(hp(ptrs), hp(hl), hp(hz), s["own"], s["njobs"], s["vstride"], d_par.data_ptr(), ar.ptr(o_hv),
                                                      ar.ptr(o_hc), ar.ptr(o_ev), ws, B, stream()))
    poly = lambda j, b: s["mine"][j][b] if j in s["own_jobs"] else s["shared"][j]
    ar.expect(o_ev, [[horner(poly(j, b), par[b][s["zslot"][j]])[0] for j in range(s["njobs"])] for b in range(B)])
    ar.check("evaluations", ignore=[(o_hv, 2 * scratch)])     # the workgroup values and carries: scratch, inside the area


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("jobs", list(HORNER_JOBS))
def test_horner_divisions(B, jobs):
    lens = HORNER_JOBS[jobs]
    s = horner_setup(B, lens, 11 * B + len(lens))
    par, d_par = params(B, 1900 + len(lens))
    q_off, at = [], s["end"]
    for n in lens:
        q_off.append(at)
        at += max(n - 1, 1) + (8 - max(n - 1, 1) % 8) % 8
    scratch = s["njobs"] * s["vstride"]
    o_hv, o_hc, o_ev = at, at + scratch, at + 2 * scratch
    ws = o_ev + 8
    ar = Arena(B, ws)
    for j in s["own_jobs"]:
        ar.put(s["offs"][j], s["mine"][j])
    ptrs = host_ptrs([ar.ptr(s["offs"][j]) if j in s["own_jobs"] else s["d_shared"][j].data_ptr() for j in range(s["njobs"])])
    quots = host_ptrs([ar.ptr(o) for o in q_off])
    hl, hz = np.array(lens, dtype=np.uint32), np.array(s["zslot"], dtype=np.uint8)
    launched(DRV.lib().plonk_batch_driver_horner_divide(hp(ptrs), hp(quots), hp(hl), hp(hz), s["own"], s["njobs"], s["vstride"], d_par.data_ptr(),
                                                        ar.ptr(o_hv), ar.ptr(o_hc), ar.ptr(o_ev), ws, B, stream()))
    poly = lambda j, b: s["mine"][j][b] if j in s["own_jobs"] else s["shared"][j]
    res = [[horner(poly(j, b), par[b][s["zslot"][j]]) for j in range(s["njobs"])] for b in range(B)]
    ar.expect(o_ev, [[r[0] for r in row] for row in res])
    for j in range(s["njobs"]):
        ar.expect(q_off[j], [res[b][j][1] for b in range(B)])
    ar.check("divisions", ignore=[(o_hv, 2 * scratch)])


def test_launchers_refuse_what_would_index_out_of_bounds():
    L = DRV.lib()
    bad = 1                                                     # hipErrorInvalidValue
    ar = Arena(2, 64)
    _, d_par = params(2, 1)
    p = ar.ptr(0)
    assert L.plonk_batch_driver_gather(p, 20, p, 64, 2, 1, stream()) == bad                    # 4 n > ws
    assert L.plonk_batch_driver_gp_top(p, 65, p, 64, 2, stream()) == bad                       # more workgroup products than an area holds
    assert L.plonk_batch_driver_quotient(p, p, 16, 4, p, d_par.data_ptr(), p, 64, 2, 1, stream()) == bad    # 5 D > ws
    assert L.plonk_batch_driver_split(p, p, 4, 16, d_par.data_ptr(), p, p, p, p, 64, 512, 2, 1, stream()) == bad   # D < 3 n + 6
    one = host_ptrs([p])
    assert L.plonk_batch_driver_horner_eval(hp(one), hp(np.array([5000], dtype=np.uint32)), hp(np.array([ZETA], dtype=np.uint8)), 1, 1, 2,
                                            d_par.data_ptr(), p, p, p, 64, 2, stream()) == bad   # three workgroups, room for two values
    assert L.plonk_batch_driver_horner_eval(hp(one), hp(np.array([5], dtype=np.uint32)), hp(np.array([SLOTS], dtype=np.uint8)), 1, 1, 2,
                                            d_par.data_ptr(), p, p, p, 64, 2, stream()) == bad   # a slot outside a proof's row
    ar.check("refused launches")
