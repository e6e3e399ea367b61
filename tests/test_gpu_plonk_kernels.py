"""GPU: every kernel of csrc/plonk_kernels.hpp on its own, against python integers.

tests/test_gpu_plonk.py compares whole proofs, which pins only the branches its sizes take.  Here each kernel is launched through
tests/cpp/plonk_kernels_driver.hip with inputs no satisfied circuit would give it: ragged row counts, more than 1024 block products,
D / n = 8, grids so small that every lane loops, denominators and numerators that vanish, a quotient that does not divide.  The
reference is python `int` and `% R` in this file (plus roots_of_unity, random_circuit, fast_accumulator of tests/plonk_model.py); no
field operation of the library is used, Montgomery packing included.  Every comparison is == on every output element, as packed limbs:
an unreduced result fails too.  Every output buffer is pre-filled with a pattern and carries one guard element that must keep it.
"""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_kernels_driver as DRV  # noqa: E402
import plonk_model as PL  # noqa: E402

pytestmark = pytest.mark.gpu
R = PL.R
MONT = (1 << 256) % R
SPECIAL = (0, 1, R - 1)
PATTERN = 0x5A5A5A5A5A5A5A5A
FLAG_GATE, FLAG_DENOM, FLAG_CLOSE, FLAG_QUOTIENT = 0, 1, 2, 3
GP_COLUMNS = ["q_m", "q_l", "q_r", "q_o", "q_c", "s1", "s2", "s3"]             # the order of PlonkCols


# ---- plumbing: python ints <-> device tensors of Montgomery limbs --------------------------------------------------------------
def pack(vals):
    """canonical ints -> uint64 [n, 4] Montgomery limbs, with integers only"""
    raw = b"".join((v % R * MONT % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def dev(vals):
    import torch
    return torch.from_numpy(pack(vals).view(np.int64)).cuda()


def scalars(*vals):
    """host scalars for a launcher: a contiguous uint64 array the caller keeps alive across the call"""
    return pack(vals)


def hp(a):
    return a.ctypes.data


def outbuf(n):
    """n elements and one guard, all pattern"""
    import torch
    return torch.full((n + 1, 4), PATTERN, dtype=torch.int64, device="cuda")


def flagbuf():
    import torch
    return torch.zeros(4, dtype=torch.int32, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def launched(status):
    assert status == 0, "launcher returned hipError %d" % status


def check(buf, want, what):
    """all of `want`, bit for bit, and the guard behind it untouched"""
    got = buf.cpu().numpy().view(np.uint64)
    assert got.shape[0] == len(want) + 1, what
    exp = pack(want)
    if not np.array_equal(got[:-1], exp):
        bad = np.nonzero((got[:-1] != exp).any(axis=1))[0]
        raise AssertionError("%s: %d of %d elements differ, the first at index %d" % (what, len(bad), len(want), bad[0]))
    assert (got[-1] == np.uint64(PATTERN)).all(), what + ": the element behind the output was written"


def flags_of(buf):
    return [int(v) for v in buf.cpu().numpy()]


def column(rng, n):
    """n random elements, with 0, 1 and R - 1 in six rows (in at most half of the rows when there are fewer than twelve)"""
    v = [rng.randrange(R) for _ in range(n)]
    first = rng.randrange(3)
    for k, row in enumerate(rng.sample(range(n), min(n // 2, 6))):
        v[row] = SPECIAL[(first + k) % 3]
    return v


def grids(n_items):
    """one workgroup (every lane loops once n_items > 256), and the prover's grid"""
    return sorted({1, DRV.lib().plonk_driver_stream_grid(n_items)})


# ---- the grand product: ratio -> top -> apply ---------------------------------------------------------------------------------
def gp_inputs_arbitrary(n, seed):
    rng = random.Random(seed)
    inp = {name: column(rng, n) for name in ["a", "b", "c", "pub", "w"] + GP_COLUMNS}
    return inp, rng.randrange(R), rng.randrange(R)


def gp_inputs_circuit(n, seed):
    cpi, wit = PL.random_circuit(n, random.Random(seed), random.Random(seed + 1000))
    assert PL.gate_identity_holds(cpi, wit)
    inp = dict(a=list(wit["a"]), b=list(wit["b"]), c=list(wit["c"]), pub=list(wit["public_poly"]), w=PL.roots_of_unity(n),
               q_m=cpi["q_m"], q_l=cpi["q_l"], q_r=cpi["q_r"], q_o=cpi["q_o"], q_c=cpi["q_c"],
               s1=cpi["sigma_1"], s2=cpi["sigma_2"], s3=cpi["sigma_3"])
    rng = random.Random(seed + 2000)
    return inp, rng.randrange(R), rng.randrange(R), cpi, wit


def gp_reference(inp, n, beta, gamma, rows_per_block):
    """-> dict(flags, f, block_prod, block_excl, acc); with a vanishing denominator only the flags are defined"""
    gate_bad, den_zero, f = False, False, []
    for i in range(n):
        a, b, c, w = inp["a"][i], inp["b"][i], inp["c"][i], inp["w"][i]
        gate = (a * b * inp["q_m"][i] + a * inp["q_l"][i] + b * inp["q_r"][i] + c * inp["q_o"][i] + inp["pub"][i] + inp["q_c"][i]) % R
        gate_bad = gate_bad or gate != 0
        num = (a + beta * w + gamma) * (b + 2 * beta * w + gamma) * (c + 3 * beta * w + gamma) % R
        den = (a + beta * inp["s1"][i] + gamma) * (b + beta * inp["s2"][i] + gamma) * (c + beta * inp["s3"][i] + gamma) % R
        den_zero = den_zero or den == 0
        f.append(num * pow(den, R - 2, R) % R)
    if den_zero:
        return dict(flags=[int(gate_bad), 1, None, 0])
    acc, run = [], 1
    for v in f:
        acc.append(run)
        run = run * v % R
    n_blocks = (n + rows_per_block - 1) // rows_per_block
    block_prod = []
    for b in range(n_blocks):
        p = 1
        for v in f[b * rows_per_block:(b + 1) * rows_per_block]:
            p = p * v % R
        block_prod.append(p)
    block_excl, p = [], 1
    for v in block_prod:
        block_excl.append(p)
        p = p * v % R
    return dict(flags=[int(gate_bad), 0, int(acc[n - 1] * f[n - 1] % R != 1), 0], f=f, block_prod=block_prod, block_excl=block_excl, acc=acc)


def gp_run(inp, n, beta, gamma):
    """the three passes as zkhip_plonk_prove enqueues them -> (f, block_prod, block_excl, acc, flags) still on the device"""
    L = DRV.lib()
    rows = L.plonk_driver_gp_rows()
    n_blocks = (n + rows - 1) // rows
    d = {k: dev(v) for k, v in inp.items()}
    cols = np.array([d[k].data_ptr() for k in GP_COLUMNS], dtype=np.uint64)
    sc = scalars(beta, gamma)
    f, bp, bx, acc, flags = outbuf(n), outbuf(n_blocks), outbuf(n_blocks), outbuf(n), flagbuf()
    launched(L.plonk_driver_gp_ratio(d["a"].data_ptr(), d["b"].data_ptr(), d["c"].data_ptr(), d["pub"].data_ptr(), hp(cols), d["w"].data_ptr(),
                                     n, hp(sc), hp(sc) + 32, f.data_ptr(), bp.data_ptr(), flags.data_ptr(), stream()))
    launched(L.plonk_driver_gp_top(bp.data_ptr(), n_blocks, bx.data_ptr(), stream()))
    launched(L.plonk_driver_gp_apply(f.data_ptr(), bx.data_ptr(), n, acc.data_ptr(), flags.data_ptr(), stream()))
    return f, bp, bx, acc, flags, rows


def gp_check(inp, n, beta, gamma):
    f, bp, bx, acc, flags, rows = gp_run(inp, n, beta, gamma)
    want = gp_reference(inp, n, beta, gamma, rows)
    assert want["flags"][FLAG_DENOM] == 0
    check(f, want["f"], "f")
    check(bp, want["block_prod"], "block_prod")
    check(bx, want["block_excl"], "block_excl")
    check(acc, want["acc"], "acc")
    assert flags_of(flags) == want["flags"]
    return want


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 2048, 4100])
def test_grand_product_of_arbitrary_columns(n):
    inp, beta, gamma = gp_inputs_arbitrary(n, 100 + n)
    want = gp_check(inp, n, beta, gamma)
    assert want["flags"] == [1, 0, 1, 0]            # no circuit: some gate does not hold and the product does not close


@pytest.mark.parametrize("n", [4, 1024, 2048])
def test_grand_product_of_a_satisfied_circuit_raises_no_flag(n):
    inp, beta, gamma, cpi, wit = gp_inputs_circuit(n, 200 + n)
    want = gp_check(inp, n, beta, gamma)
    assert want["flags"] == [0, 0, 0, 0]
    assert want["acc"] == PL.fast_accumulator(cpi, wit, beta, gamma)


def test_grand_product_flags_one_broken_gate_in_the_last_lane():
    n = 2048
    inp, beta, gamma, _, _ = gp_inputs_circuit(n, 300)
    inp["pub"][n - 1] = (inp["pub"][n - 1] + 1) % R  # row 3 of lane 255 of the second workgroup; no wire changes, so the product still closes
    want = gp_check(inp, n, beta, gamma)
    assert want["flags"] == [1, 0, 0, 0]


@pytest.mark.parametrize("row", [7, 4099])
def test_grand_product_flags_a_vanishing_denominator(row):
    n = 4100                                        # five workgroups; row 7 in the first, row 4099 the last row of the partly filled fifth
    inp, beta, gamma = gp_inputs_arbitrary(n, 400)
    inp["a"][row] = -(beta * inp["s1"][row] + gamma) % R
    flags = gp_run(inp, n, beta, gamma)[4]
    want = gp_reference(inp, n, beta, gamma, 1024)
    assert want["flags"][FLAG_DENOM] == 1
    assert flags_of(flags)[FLAG_DENOM] == 1         # the substituted denominator makes every other output meaningless


def test_grand_product_with_a_vanishing_numerator():
    n, row = 4100, 1500
    inp, beta, gamma = gp_inputs_arbitrary(n, 500)
    inp["a"][row] = -(beta * inp["w"][row] + gamma) % R
    want = gp_check(inp, n, beta, gamma)
    assert want["f"][row] == 0 and all(v != 0 for v in want["acc"][:row + 1]) and all(v == 0 for v in want["acc"][row + 1:])
    assert want["block_prod"][1] == 0 and want["block_excl"][1] != 0 and want["block_excl"][2:] == [0, 0, 0]


@pytest.mark.parametrize("n_blocks", [1, 2, 1023, 1024, 1025, 2048, 2049, 5000])
def test_top_pass_alone(n_blocks):
    """above 1024 block products a lane takes per = 2 .. 5 of them and the last lanes none (lo == hi == n_blocks)"""
    rng = random.Random(600 + n_blocks)
    prod = [rng.randrange(R) for _ in range(n_blocks)]
    if n_blocks >= 8:                               # 1 and R - 1 anywhere; 0 near the end only: everything behind a 0 is 0
        for v in (1, R - 1, 1, R - 1):
            prod[rng.randrange(n_blocks)] = v
        prod[n_blocks - 3] = 0
    want, p = [], 1
    for v in prod:
        want.append(p)
        p = p * v % R
    out = outbuf(n_blocks)
    src = dev(prod)
    launched(DRV.lib().plonk_driver_gp_top(src.data_ptr(), n_blocks, out.data_ptr(), stream()))
    check(out, want, "block_excl")


# ---- quotient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rot", [(32, 8), (32, 4), (4096, 4), (8192, 4)])
def test_quotient(D, rot):
    rng = random.Random(700 + D + rot)
    a, b, c, z, pi = (column(rng, D) for _ in range(5))
    qm, ql, qr, qo, qc, s1, s2, s3, l1, x = (column(rng, D) for _ in range(10))
    beta, gamma, alpha, alpha2 = (rng.randrange(R) for _ in range(4))
    zh_inv = []
    while len(zh_inv) < 8:
        v = rng.randrange(1, R)
        if v not in zh_inv:
            zh_inv.append(v)
    want = []
    for j in range(D):
        zw = z[(j + rot) % D]
        gate = a[j] * b[j] * qm[j] + a[j] * ql[j] + b[j] * qr[j] + c[j] * qo[j] + pi[j] + qc[j]
        p1 = (a[j] + beta * x[j] + gamma) * (b[j] + 2 * beta * x[j] + gamma) * (c[j] + 3 * beta * x[j] + gamma) * z[j]
        p2 = (a[j] + beta * s1[j] + gamma) * (b[j] + beta * s2[j] + gamma) * (c[j] + beta * s3[j] + gamma) * zw
        want.append((gate + alpha * (p1 - p2) + alpha2 * (z[j] - 1) * l1[j]) % R * zh_inv[j % rot] % R)
    ev, pre = dev(a + b + c + z + pi), dev(qm + ql + qr + qo + qc + s1 + s2 + s3 + l1 + x)
    sc, zi = scalars(beta, gamma, alpha, alpha2), scalars(*zh_inv)
    for grid in sorted({1, 3, DRV.lib().plonk_driver_stream_grid(D)}):
        out = outbuf(D)
        launched(DRV.lib().plonk_driver_quotient(ev.data_ptr(), pre.data_ptr(), D, rot, hp(sc), hp(zi), out.data_ptr(), grid, stream()))
        check(out, want, "t at grid %d" % grid)
        tail = out.cpu().numpy().view(np.uint64)[D - rot:D]                     # the points whose z(w x) wraps to the front
        assert np.array_equal(tail, pack(want[D - rot:])), "wrapped reads at grid %d" % grid


# ---- split --------------------------------------------------------------------------------------------------------------------
def split_reference(t, ginv, n, b10, b11):
    v = [t[i] * ginv[i] % R for i in range(3 * n + 6)]
    tl, tm, th = v[:n] + [b10], v[n:2 * n] + [b11], v[2 * n:3 * n + 6]
    tm[0] = (tm[0] - b10) % R
    th[0] = (th[0] - b11) % R
    return tl, tm, th, int(any(x % R for x in t[3 * n + 6:]))


def split_run(t, ginv, n, D, b10, b11, grid):
    tl, tm, th, flags = outbuf(n + 1), outbuf(n + 1), outbuf(n + 6), flagbuf()
    src, g, sc = dev(t), dev(ginv), scalars(b10, b11)
    launched(DRV.lib().plonk_driver_split(src.data_ptr(), g.data_ptr(), n, D, hp(sc), hp(sc) + 32, tl.data_ptr(), tm.data_ptr(), th.data_ptr(),
                                          flags.data_ptr(), grid, stream()))
    return tl, tm, th, flags_of(flags)


@pytest.mark.parametrize("n,D", [(4, 32), (8, 32), (16, 64), (1024, 4096)])
def test_split(n, D):
    rng = random.Random(800 + n)
    top = 3 * n + 6
    t = column(rng, top) + [0] * (D - top)
    ginv = column(rng, top)
    b10, b11 = rng.randrange(R), rng.randrange(R)
    past, last, inside = list(t), list(t), list(t)
    past[top] = 1                                   # the first coefficient a quotient of this degree cannot have
    last[D - 1] = R - 1
    inside[top - 1] = (t[top - 1] + 1) % R          # the last one it can
    for grid in grids(D):
        for name, vec, flag in (("t", t, 0), ("t with [3n + 6] set", past, 1), ("t with [D - 1] set", last, 1), ("t with [3n + 5] changed", inside, 0)):
            tl, tm, th, flags = split_run(vec, ginv, n, D, b10, b11, grid)
            wl, wm, wh, wflag = split_reference(vec, ginv, n, b10, b11)
            assert wflag == flag
            assert flags == [0, 0, 0, flag], "%s at grid %d" % (name, grid)
            check(tl, wl, "t_low of %s at grid %d" % (name, grid))
            check(tm, wm, "t_mid of %s at grid %d" % (name, grid))
            check(th, wh, "t_high of %s at grid %d" % (name, grid))
    assert split_reference(inside, ginv, n, b10, b11)[2][n + 5] != split_reference(t, ginv, n, b10, b11)[2][n + 5]


# ---- linearisation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 10, 1030, 5000])
def test_linearise(length):
    rng = random.Random(900 + length)
    vecs = [column(rng, length) for _ in range(15)]
    weights = column(rng, 15)
    c0 = rng.randrange(R)
    tensors = [dev(v) for v in vecs]
    sc, c = scalars(*weights), scalars(c0)
    for which in (list(range(15)), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 5, 12, 5, 14]):      # distinct; one vector behind three pointers
        want = [(sum(weights[k] * vecs[which[k]][i] for k in range(15)) + (c0 if i == 0 else 0)) % R for i in range(length)]
        ptrs = np.array([tensors[k].data_ptr() for k in which], dtype=np.uint64)
        for grid in grids(length):
            out = outbuf(length)
            launched(DRV.lib().plonk_driver_linearise(hp(ptrs), hp(sc), hp(c), length, out.data_ptr(), grid, stream()))
            check(out, want, "linearisation at grid %d" % grid)


# ---- blinding -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(4, 2), (4, 3), (1024, 2), (1024, 3)])
def test_blind(n, k):
    import torch
    rng = random.Random(1000 + n + k)
    p, b = column(rng, n), [rng.randrange(R) for _ in range(k)]
    want = p + [0] * k                              # p + (b_0 + b_1 X + b_2 X^2) (X^n - 1)
    for j in range(k):
        want[j] = (want[j] - b[j]) % R
        want[n + j] = (want[n + j] + b[j]) % R
    buf = torch.cat([dev(p + [0] * k), outbuf(0)])
    sc = scalars(*b)
    launched(DRV.lib().plonk_driver_blind(buf.data_ptr(), n, k, hp(sc), stream()))
    check(buf, want, "blinded polynomial")          # the guard is element n + k


# ---- powers, scale and pad ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 257, 3080])
def test_powers(count):
    rng = random.Random(1100 + count)
    scale = rng.randrange(R)
    for base in (1, 7, rng.randrange(R)):
        want, p = [], scale
        for _ in range(count):
            want.append(p)
            p = p * base % R
        sc = scalars(base, scale)
        for grid in grids(count):
            out = outbuf(count)
            launched(DRV.lib().plonk_driver_powers(hp(sc), hp(sc) + 32, count, out.data_ptr(), grid, stream()))
            check(out, want, "powers of %d at grid %d" % (base, grid))


@pytest.mark.parametrize("n_src,n", [(2, 32), (7, 32), (32, 32), (1027, 2048)])
def test_scale_pad(n_src, n):
    rng = random.Random(1200 + n_src)
    a, b = column(rng, n_src), column(rng, n_src)
    want = [x * y % R for x, y in zip(a, b)] + [0] * (n - n_src)
    da, db = dev(a), dev(b)
    for grid in grids(n):
        out = outbuf(n)
        launched(DRV.lib().plonk_driver_scale_pad(da.data_ptr(), db.data_ptr(), n_src, n, out.data_ptr(), grid, stream()))
        check(out, want, "scaled and padded at grid %d" % grid)


# ---- the launchers' own argument checks ------------------------------------------------------------------------------------------
def test_launchers_refuse_what_would_index_out_of_bounds():
    """a refused call launches nothing: its outputs keep their pattern"""
    L, s = DRV.lib(), stream()
    rng = random.Random(1300)
    vec, out, flags, sc = dev(column(rng, 512)), outbuf(64), flagbuf(), scalars(*[rng.randrange(R) for _ in range(12)])
    v, o, fl = vec.data_ptr(), out.data_ptr(), flags.data_ptr()
    ptrs = np.array([v] * 15, dtype=np.uint64)
    refused = [
        L.plonk_driver_powers(hp(sc), hp(sc), 0, o, 1, s), L.plonk_driver_powers(hp(sc), hp(sc), 8, o, 0, s),
        L.plonk_driver_scale_pad(v, v, 0, 0, o, 1, s), L.plonk_driver_scale_pad(v, v, 8, 8, o, 0, s), L.plonk_driver_scale_pad(v, v, 9, 8, o, 1, s),
        L.plonk_driver_blind(o, 0, 2, hp(sc), s), L.plonk_driver_blind(o, 8, 4, hp(sc), s), L.plonk_driver_blind(o, 8, 0, hp(sc), s),
        L.plonk_driver_gp_ratio(v, v, v, v, hp(ptrs), v, 0, hp(sc), hp(sc), o, o, fl, s),
        L.plonk_driver_gp_top(v, 0, o, s), L.plonk_driver_gp_apply(v, v, 0, o, fl, s),
        L.plonk_driver_quotient(v, v, 32, 2, hp(sc), hp(sc), o, 1, s), L.plonk_driver_quotient(v, v, 32, 16, hp(sc), hp(sc), o, 1, s),
        L.plonk_driver_quotient(v, v, 24, 4, hp(sc), hp(sc), o, 1, s), L.plonk_driver_quotient(v, v, 0, 4, hp(sc), hp(sc), o, 1, s),
        L.plonk_driver_quotient(v, v, 32, 4, hp(sc), hp(sc), o, 0, s),
        L.plonk_driver_split(v, v, 0, 32, hp(sc), hp(sc), o, o, o, fl, 1, s), L.plonk_driver_split(v, v, 4, 24, hp(sc), hp(sc), o, o, o, fl, 1, s),
        L.plonk_driver_split(v, v, 16, 32, hp(sc), hp(sc), o, o, o, fl, 1, s), L.plonk_driver_split(v, v, 4, 32, hp(sc), hp(sc), o, o, o, fl, 0, s),
        L.plonk_driver_linearise(hp(ptrs), hp(sc), hp(sc), 0, o, 1, s), L.plonk_driver_linearise(hp(ptrs), hp(sc), hp(sc), 8, o, 0, s),
    ]
    assert all(st != 0 for st in refused), refused
    assert (out.cpu().numpy().view(np.uint64) == np.uint64(PATTERN)).all() and flags_of(flags) == [0, 0, 0, 0]
