"""GPU: every kernel of csrc/mle_kernels.hpp, and eq_weights / eval_weights / sum_records of csrc/multifold_kernels.hpp, ALONE and at a
grid the test chooses, against python integers (tests/mle_model.py).

Through the public API these kernels run at the grid mle_grid() / mle_grid_stream() pick, which covers every table the suite uses in one
step.  Here tests/cpp/mle_kernels_driver.hip launches them at grids of 1, 2 and 3 workgroups (strides of 256, 512 and 768 items), so the
grid-stride loops take a second, third and fifth step at a few thousand entries: lengths either side of one workgroup and of one and
two strides, and 4 stride + 3 for the 4-way unrolled sums.  The Horner scan is taken above 1024 workgroups, where one lane of its top
kernel holds several of them.

Every comparison is == on limbs, every output must be canonical (below r), and every output buffer is pre-filled with a pattern and
longer than the kernel may write: what lies behind must keep the pattern.  Inputs are the full-range fills of tests/tables.py."""
import os
import random
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mle_kernels_driver as DRV  # noqa: E402
import mle_model as M  # noqa: E402
import tables as T  # noqa: E402

pytestmark = pytest.mark.gpu
R = T.R
PATTERN = 0x5A5A5A5A5A5A5A5A
GUARD = 8
POOL = 16384
BLOCK = DRV.BLOCK
GRIDS = [1, 2, 3, "lib"]
SPECIAL = [0, 1, R - 1]


def lengths(grid):
    """the lengths of a kernel that takes any: either side of a workgroup and of one, two and four strides"""
    if grid == "lib":
        return [1, 5, 255, 256, 257, 1000, 3075]
    s = BLOCK * grid
    return sorted({1, 5, 255, 256, 257, s, s + 1, 2 * s - 1, 2 * s + 1, 4 * s + 3})


def grid_for(grid, n_items, stream=True):
    return DRV.library_grid(n_items, stream) if grid == "lib" else grid


@pytest.fixture(scope="module")
def L():
    return DRV.lib()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def pool():
    """one table per arithmetic fill, its canonical integers and its device copy, made once; a case takes a slice"""
    import torch as t
    out = {}
    for q, kind in enumerate(T.FILLS_ARITH):
        a = T.fill(kind, POOL, 9000 + q)
        out[kind] = {"limbs": a, "ints": T.canonical(a), "dev": t.from_numpy(a.view(np.int64)).cuda()}
    return out


def take(pool, kind, n, off=0):
    """(device tensor [n, 4], canonical ints) of entries off .. off + n of a fill"""
    p = pool[kind]
    assert off + n <= POOL
    return p["dev"][off:off + n].contiguous(), p["ints"][off:off + n]


def other(kind, step=1):
    return T.rotation(T.FILLS_ARITH, kind, step + 1)[step]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def dev_ints(torch, vals):
    return dev(torch, M.pack(vals))


def host(t):
    return t.cpu().numpy().view(np.uint64)


def blank(torch, rows):
    """an output buffer of rows + GUARD elements holding the pattern"""
    return torch.full((rows + GUARD, 4), PATTERN, dtype=torch.int64, device="cuda")


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def fr(v):
    """a host field element for a by-value argument: (array kept alive, its address)"""
    a = np.ascontiguousarray(M.pack([v]).reshape(-1))
    return a, a.ctypes.data


def pts_arg(vals):
    a = np.ascontiguousarray(M.pack(vals).reshape(-1)) if len(vals) else np.zeros(4, dtype=np.uint64)
    return a, a.ctypes.data


def expect(buf, want, what=""):
    """the first len(want) elements of buf are the canonical limbs of `want` (ints), the rest kept the pattern"""
    got = host(buf)
    n = len(want)
    assert (got[n:] == np.uint64(PATTERN)).all(), "%s: written behind the %d outputs" % (what, n)
    assert T.below_r(got[:n]).all(), "%s: an output is not below r" % what
    exp = M.pack(want)
    bad = np.nonzero((got[:n] != exp).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d outputs differ, the first at %d" % (what, len(bad), n, bad[0])


def ok(status):
    assert status == 0, "launcher returned hipError %d" % status


# ---- elementwise, to_bytes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.FILLS_ARITH)
@pytest.mark.parametrize("grid", GRIDS)
def test_elementwise(L, torch, pool, grid, kind):
    for q, n in enumerate(lengths(grid)):
        g = grid_for(grid, n)
        a, ta = take(pool, kind, n, q)
        b, tb = take(pool, other(kind), n, 2 * q + 1)
        s = pool[other(kind, 2)]["ints"][q]
        keep, sp = fr(s)
        for op in (0, 1, 2):
            out = blank(torch, n)
            ok(L.mle_driver_elementwise(op, a.data_ptr(), b.data_ptr() if op < 2 else None, sp if op == 2 else None, n, out.data_ptr(), g, stream(torch)))
            expect(out, M.elementwise(op, ta, tb, s), "op %d n %d grid %d" % (op, n, g))


@pytest.mark.parametrize("grid", [1, 3])
def test_elementwise_edges(L, torch, pool, grid):
    """a - a, a + (r - a), and scaling by 0, 1, r - 1; 0 +- 0; 1 - (r - 1)"""
    n = 2 * BLOCK * grid + 1
    for kind in T.FILLS_ARITH:
        a, ta = take(pool, kind, n, 3)
        neg = dev(torch, T.negate(pool[kind]["limbs"][3:3 + n]))
        for op, b, want in ((1, a, [0] * n), (0, neg, [0] * n)):
            out = blank(torch, n)
            ok(L.mle_driver_elementwise(op, a.data_ptr(), b.data_ptr(), None, n, out.data_ptr(), grid, stream(torch)))
            expect(out, want, "%s op %d" % (kind, op))
        for s in SPECIAL:
            keep, sp = fr(s)
            out = blank(torch, n)
            ok(L.mle_driver_elementwise(2, a.data_ptr(), None, sp, n, out.data_ptr(), grid, stream(torch)))
            expect(out, M.elementwise(2, ta, scalar=s), "%s scaled by %d" % (kind, s))
    shapes = {k: dev(torch, T.fill(k, n, 1)) for k in ("zero", "one", "minus_one")}
    vals = {"zero": 0, "one": 1, "minus_one": R - 1}
    for ka in shapes:
        for kb in shapes:
            for op in (0, 1):
                out = blank(torch, n)
                ok(L.mle_driver_elementwise(op, shapes[ka].data_ptr(), shapes[kb].data_ptr(), None, n, out.data_ptr(), grid, stream(torch)))
                expect(out, M.elementwise(op, [vals[ka]] * n, [vals[kb]] * n), "%s %s %s" % (ka, "+-"[op], kb))


@pytest.mark.parametrize("kind", T.FILLS_ARITH + ["zero", "minus_one"])
@pytest.mark.parametrize("grid", GRIDS)
def test_to_bytes(L, torch, pool, grid, kind):
    for q, n in enumerate(lengths(grid)):
        g = grid_for(grid, n)
        if kind in T.FILLS_ARITH:
            a, ta = take(pool, kind, n, q)
        else:
            a, ta = dev(torch, T.fill(kind, n, 0)), [0 if kind == "zero" else R - 1] * n
        out = torch.full((32 * (n + GUARD),), 0x5A, dtype=torch.uint8, device="cuda")
        ok(L.mle_driver_to_bytes(a.data_ptr(), n, out.data_ptr(), g, stream(torch)))
        got = out.cpu().numpy().tobytes()
        assert got[32 * n:] == b"\x5a" * (32 * GUARD), "n %d: written behind the output" % n
        assert got[:32 * n] == M.to_bytes(ta), "n %d grid %d" % (n, g)


# ---- half_sums, finish_sums, sum_records ---------------------------------------------------------------------
def records_sum(part, grid):
    """(sum of the lower-half records, sum of the upper-half records) of `grid` workgroups, as integers; the records are canonical"""
    assert T.below_r(part[:2 * grid]).all(), "a record is not below r"
    v = T.canonical(part[:2 * grid])
    return sum(v[0::2]) % R, sum(v[1::2]) % R


@pytest.mark.parametrize("kind", T.FILLS_ARITH)
@pytest.mark.parametrize("grid", GRIDS)
def test_half_sums_and_finish(L, torch, pool, grid, kind):
    for q, n in enumerate(lengths(grid)):
        g = grid_for(grid, (n + 1) // 2, stream=False)                  # the library's: zkhip_mle_half_sums
        a, ta = take(pool, kind, n, q)
        part = blank(torch, 2 * g)
        ok(L.mle_driver_half_sums(a.data_ptr(), n, part.data_ptr(), g, stream(torch)))
        got = host(part)
        assert (got[2 * g:] == np.uint64(PATTERN)).all(), "n %d: a record beyond the grid was written" % n
        want = M.half_sums(ta)
        assert records_sum(got, g) == want, "n %d grid %d" % (n, g)
        out = blank(torch, 3)
        ok(L.mle_driver_finish_sums(part.data_ptr(), g, out.data_ptr(), stream(torch)))
        expect(out, [want[0], want[1], sum(want) % R], "finish n %d grid %d" % (n, g))


@pytest.mark.parametrize("n_partials", [1, 255, 256, 257, 1023, 1024, 1025, 2048])
def test_finish_sums(L, torch, pool, n_partials):
    for kind in T.FILLS_ARITH:
        a, ta = take(pool, kind, 2 * n_partials, 5)
        out = blank(torch, 3)
        ok(L.mle_driver_finish_sums(a.data_ptr(), n_partials, out.data_ptr(), stream(torch)))
        lo, hi = sum(ta[0::2]) % R, sum(ta[1::2]) % R
        expect(out, [lo, hi, (lo + hi) % R], kind)


@pytest.mark.parametrize("n", [1, 255, 256, 1024, 1025, 4 * 256 * 2 + 1])
def test_sum_records(L, torch, pool, n):
    for kind in T.FILLS_ARITH:
        a, ta = take(pool, kind, n, 7)
        out = blank(torch, 1)
        ok(L.mle_driver_sum_records(a.data_ptr(), n, out.data_ptr(), stream(torch)))
        expect(out, [M.sum_records(ta)], kind)


# ---- fold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("n_out", [1, 2, 256, 512, 1024, 4096])
def test_fold_every_pair_distance(L, torch, pool, n_out, grid):
    """every log_half at grids whose stride (256, 512, 768) does and does not divide n_out.  Each case runs without sums and with them,
    the point once by value and once from device memory.  The input is followed by n_out + GUARD spare elements."""
    rng = random.Random(n_out * 16 + grid)
    for log_half in range(n_out.bit_length()):
        kind = T.FILLS_ARITH[log_half % 4]
        p = pool[kind]
        a = p["dev"][:3 * n_out + GUARD]                                 # 2 n_out entries and what lies behind
        r = rng.randrange(R)
        keep, rp = fr(r)
        d_r = dev_ints(torch, [r])
        want = M.fold(p["ints"][:2 * n_out], r, log_half)
        by_value = log_half % 2 == 0
        out = blank(torch, n_out)
        ok(L.mle_driver_fold(a.data_ptr(), out.data_ptr(), n_out, log_half, rp if by_value else None, None if by_value else d_r.data_ptr(), None,
                             grid, stream(torch)))
        expect(out, want, "n_out %d log_half %d grid %d" % (n_out, log_half, grid))
        out, part = blank(torch, n_out), blank(torch, 2 * grid)
        ok(L.mle_driver_fold(a.data_ptr(), out.data_ptr(), n_out, log_half, None if by_value else rp, d_r.data_ptr() if by_value else None,
                             part.data_ptr(), grid, stream(torch)))
        expect(out, want, "with sums: n_out %d log_half %d grid %d" % (n_out, log_half, grid))
        got = host(part)
        assert (got[2 * grid:] == np.uint64(PATTERN)).all(), "a record beyond the grid was written"
        assert records_sum(got, grid) == M.half_sums(want), "sums: n_out %d log_half %d grid %d" % (n_out, log_half, grid)


def test_fold_special_points_and_library_grid(L, torch, pool):
    n_out = 1024
    for kind in T.FILLS_ARITH:
        a, ta = take(pool, kind, 2 * n_out)
        for r in SPECIAL + [(R + 1) // 2]:
            keep, rp = fr(r)
            for grid, log_half in ((3, 10), (DRV.library_grid((n_out + 1) // 2, True), 0)):
                out = blank(torch, n_out)
                ok(L.mle_driver_fold(a.data_ptr(), out.data_ptr(), n_out, log_half, rp, None, None, grid, stream(torch)))
                expect(out, M.fold(ta, r, log_half), "%s r %d grid %d" % (kind, r, grid))


@pytest.mark.parametrize("n", [2, 256, 4096])
def test_fold_tail(L, torch, pool, n):
    log_n = n.bit_length() - 1
    rng = random.Random(n)
    for q, kind in enumerate(T.FILLS_ARITH):
        a, ta = take(pool, kind, n, q)
        for n_pts in sorted({0, 1, log_n // 2, log_n}):
            for first, special in ((0, None), (5, SPECIAL[q % 3])):
                pts = [rng.randrange(R) for _ in range(first + n_pts)]
                if special is not None and n_pts:
                    pts[first] = pts[first + n_pts // 2] = pts[-1] = special
                keep, pp = pts_arg(pts)
                out = blank(torch, n >> n_pts)
                ok(L.mle_driver_fold_tail(a.data_ptr(), n, pp, first, n_pts, out.data_ptr(), stream(torch)))
                expect(out, M.fold_tail(ta, pts[first:]), "%s n %d points %d from %d" % (kind, n, n_pts, first))


# ---- distinct, repeat ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3, "lib"])
@pytest.mark.parametrize("na,nb", [(1, 1), (1, 64), (64, 1), (2, 1024), (1024, 2), (32, 64)])
def test_distinct(L, torch, pool, na, nb, grid):
    g = grid_for(grid, na * nb)
    room = max(na, nb)                                                   # both inputs hold max(na, nb) entries
    for kind in T.FILLS_ARITH:
        a, ta = take(pool, kind, room, 1)
        b, tb = take(pool, other(kind), room, 2)
        for mul in (0, 1):
            out = blank(torch, na * nb)
            ok(L.mle_driver_distinct(mul, a.data_ptr(), na, b.data_ptr(), nb, out.data_ptr(), g, stream(torch)))
            expect(out, M.distinct(ta[:na], tb[:nb], mul), "%s %dx%d %s grid %d" % (kind, na, nb, "+*"[mul], g))


@pytest.mark.parametrize("grid", [1, 3, "lib"])
@pytest.mark.parametrize("n_in", [1, 2, 64, 512])
def test_repeat(L, torch, pool, n_in, grid):
    """both forms; nothing is computed, so the rows must be the input's rows (full-range stored values included)"""
    for q, kind in enumerate(T.FILLS_ARITH):
        limbs = pool[kind]["limbs"][q:q + n_in]
        a = dev(torch, limbs)
        cases = [(0, n_in * 2 << v) for v in (0, 3)] + [(0, 4 * 768 + 5), (0, 4096)] + [(s, n_in << s) for s in (1, 3, 7)] + [(3, (n_in << 3) - 1)]
        for shift, n_out in cases:
            g = grid_for(grid, n_out)
            out = blank(torch, n_out)
            ok(L.mle_driver_repeat(a.data_ptr(), n_in, shift, n_out, out.data_ptr(), g, stream(torch)))
            got = host(out)
            assert (got[n_out:] == np.uint64(PATTERN)).all(), "written behind the output"
            idx = np.array(M.repeat(list(range(n_in)), shift, n_out))
            assert np.array_equal(got[:n_out], limbs[idx]), "%s n_in %d shift %d n_out %d grid %d" % (kind, n_in, shift, n_out, g)


# ---- MultilinearKZG::open ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3, "lib"])
@pytest.mark.parametrize("n", [2, 4, 512, 1024, 4096, 8192])
def test_open_step(L, torch, pool, n, grid):
    g = grid_for(grid, n // 2)
    rng = random.Random(n)
    for q, kind in enumerate(T.FILLS_ARITH):
        a, ta = take(pool, kind, n)
        z = rng.randrange(R) if q != 1 else SPECIAL[(n.bit_length() + (0 if grid == "lib" else grid)) % 3]
        keep, zp = fr(z)
        quo, rem = blank(torch, n // 2), blank(torch, n // 2)
        ok(L.mle_driver_open_step(a.data_ptr(), n, zp, quo.data_ptr(), rem.data_ptr(), g, stream(torch)))
        want_q, want_r = M.open_step(ta, z)
        expect(quo, want_q, "quotient %s n %d grid %d" % (kind, n, g))
        expect(rem, want_r, "remainder %s n %d grid %d" % (kind, n, g))


def ping_pong(rems, n):
    """what the two scratch tables hold after the rounds: round i leaves its remainder at the front of ping (i even) or pong (i odd)"""
    ping, pong = [None] * (n // 2), [None] * max(n // 4, 1)
    for i, t in enumerate(rems):
        (pong if i & 1 else ping)[:len(t)] = t
    return ping, pong


def expect_scratch(buf, want, what):
    """like expect(), with None for an element that no round wrote"""
    got = host(buf)
    keep = np.array([w is None for w in want] + [True] * (len(got) - len(want)))
    assert (got[keep] == np.uint64(PATTERN)).all(), "%s: written where no round writes" % what
    assert T.below_r(got[~keep]).all()
    assert np.array_equal(got[~keep], M.pack([w for w in want if w is not None])), what


@pytest.mark.parametrize("n", [2, 4, 256, 512, 4096])
def test_open_steps_small(L, torch, pool, n):
    log_n = n.bit_length() - 1
    rng = random.Random(n)
    for q, kind in enumerate(T.FILLS_ARITH):
        a, ta = take(pool, kind, n, q)
        for n_rounds in sorted({log_n, log_n - 1, 1} - {0}):
            pts = [rng.randrange(R) for _ in range(n_rounds)]
            if q == 1:
                pts[0] = pts[n_rounds // 2] = pts[-1] = SPECIAL[n_rounds % 3]
            keep, pp = pts_arg(pts)
            n_q = n - (n >> n_rounds)
            quo, ping, pong = blank(torch, n_q), blank(torch, n // 2), blank(torch, max(n // 4, 1))
            ok(L.mle_driver_open_steps_small(a.data_ptr(), n, pp, n_rounds, quo.data_ptr(), ping.data_ptr(), pong.data_ptr(), stream(torch)))
            want_q, rems = M.open_steps(ta, pts)
            what = "%s n %d rounds %d" % (kind, n, n_rounds)
            expect(quo, want_q, what)                                    # level order: n/2 of round 0, n/4 of round 1, ..
            w_ping, w_pong = ping_pong(rems, n)
            expect_scratch(ping, w_ping, what + " ping")                 # the final remainder is in the table its round's parity names:
            expect_scratch(pong, w_pong, what + " pong")                 # the other one still holds the round before at its front


@pytest.mark.parametrize("n", [4, 512, 4096])
def test_open_steps_small_batch(L, torch, pool, n):
    """three openings, the first two of one table at different points; every opening has its own quotients, scratch and evaluation"""
    log_n = n.bit_length() - 1
    rng = random.Random(n + 1)
    for kind in T.FILLS_ARITH:
        t0, i0 = take(pool, kind, n, 1)
        t1, i1 = take(pool, other(kind), n, 2)
        tabs, ints = [t0, t0, t1], [i0, i0, i1]
        d_tabs = torch.tensor([t.data_ptr() for t in tabs], dtype=torch.int64, device="cuda")
        pts = [[rng.randrange(R) for _ in range(log_n)] for _ in range(3)]
        pts[2][0] = pts[2][-1] = SPECIAL[log_n % 3]
        d_pts = dev_ints(torch, [p for row in pts for p in row])
        qs, s1, s2 = n + 3, n // 2 + 1, n // 4 + 2                       # strides wider than the data: the gaps must keep the pattern
        quo, ping, pong, evals = blank(torch, 3 * qs), blank(torch, 3 * s1), blank(torch, 3 * s2), blank(torch, 3)
        ok(L.mle_driver_open_steps_small_batch(d_tabs.data_ptr(), 3, n, d_pts.data_ptr(), log_n, quo.data_ptr(), qs, ping.data_ptr(), s1,
                                               pong.data_ptr(), s2, evals.data_ptr(), stream(torch)))
        w_quo, w_ping, w_pong, w_ev = [], [], [], []
        for b in range(3):
            q, rems = M.open_steps(ints[b], pts[b])
            a, o = ping_pong(rems, n)
            w_quo += q + [None] * (qs - len(q))
            w_ping += a + [None] * (s1 - len(a))
            w_pong += (o if n >= 4 else [None]) + [None] * (s2 - len(o))
            w_ev.append(rems[-1][0])
        expect_scratch(quo, w_quo, kind + " quotients")
        expect_scratch(ping, w_ping, kind + " ping")
        expect_scratch(pong, w_pong, kind + " pong")
        expect(evals, w_ev, kind + " evaluations")
        assert w_ev[0] != w_ev[1] or kind == "stored_max"


# ---- dense_degree ----------------------------------------------------------------------------------------------
def degree_cases(n, stride):
    """(positions of the non-zero coefficients, expected degree)"""
    last_wg = (n - 1) // BLOCK * BLOCK                                   # first index of the last workgroup's share of the last step
    last_step = (n - 1) // stride * stride
    cases = [([], 0), ([0], 0)]
    for at in (63, 64, 255, 256, stride - 1, stride, n - 1, 1, 65, 2 * stride + 1):
        if 0 < at < n:
            cases += [([at], at), ([0, at // 2, at], at)]
    for at in {last_wg - 1, last_step - 1, min(last_wg, last_step) // 2}:
        if 0 < at < n:
            cases.append(([3 % (at + 1), at], at))                       # zeros for the whole last workgroup / the whole last stride step
    return cases


@pytest.mark.parametrize("grid", GRIDS)
def test_dense_degree(L, torch, pool, grid):
    vals = pool["limb_edges"]["dev"]
    assert bool(vals[17:20].ne(0).any(dim=1).all())
    for n in lengths(grid):
        g = grid_for(grid, n, stream=False)                              # the library's: zkhip_dense_degree
        for positions, want in degree_cases(n, BLOCK * g):
            c = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            for q, at in enumerate(positions):
                c[at] = vals[17 + q]
            assert M.dense_degree([1 if i in positions else 0 for i in range(n)]) == want
            out = torch.full((2,), PATTERN, dtype=torch.int64, device="cuda")   # the launcher zeroes the word, as the library does
            ok(L.mle_driver_dense_degree(c.data_ptr(), n, out.data_ptr(), g, stream(torch)))
            got = out.cpu().tolist()
            assert got == [want, PATTERN], "n %d grid %d non-zero at %s" % (n, g, positions)
    n = 2 * BLOCK + 7                                                    # every coefficient non-zero; full-range values
    for kind in ("top", "stored_max"):
        a, _ = take(pool, kind, n)
        out = torch.full((2,), PATTERN, dtype=torch.int64, device="cuda")
        ok(L.mle_driver_dense_degree(a.data_ptr(), n, out.data_ptr(), 1, stream(torch)))
        assert out.cpu().tolist() == [n - 1, PATTERN]


# ---- circuit tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_circuit_layer(L, torch, pool, grid):
    rng = random.Random(77)
    for q, n in enumerate(lengths(grid)):
        kind = T.FILLS_ARITH[q % 4]
        n_in = (1, 2, 64, 1000)[q % 4]
        a, ta = take(pool, kind, n_in, q)
        gates = [(rng.randrange(2), rng.randrange(n_in), rng.randrange(n_in)) for _ in range(n)]
        d_g = torch.tensor(gates, dtype=torch.int32, device="cuda").contiguous()
        g = grid_for(grid, n, stream=False)
        out = blank(torch, n)
        ok(L.mle_driver_circuit_layer(a.data_ptr(), d_g.data_ptr(), n, out.data_ptr(), g, stream(torch)))
        expect(out, M.circuit_layer(ta, gates), "%s gates %d grid %d" % (kind, n, g))


@pytest.mark.parametrize("grid", GRIDS)
def test_wiring_ones(L, torch, grid):
    rng = random.Random(78)
    one = T.stored(1)
    for q, n in enumerate(lengths(grid)):
        shift = 1 + q % 2
        size = n << (2 * shift)
        gates = [(rng.randrange(2), rng.randrange(1 << shift), rng.randrange(1 << shift)) for _ in range(n)]
        d_g = torch.tensor(gates, dtype=torch.int32, device="cuda").contiguous()
        g = grid_for(grid, n, stream=False)
        add, mul = blank(torch, size), blank(torch, size)
        add[:size] = 0
        mul[:size] = 0
        ok(L.mle_driver_wiring_ones(d_g.data_ptr(), n, shift, add.data_ptr(), mul.data_ptr(), g, stream(torch)))
        for buf, want in zip((add, mul), M.wiring_ones(gates, shift, size)):
            exp = np.full((size + GUARD, 4), PATTERN, dtype=np.uint64)
            exp[:size] = 0
            exp[np.nonzero(want)[0]] = one
            assert np.array_equal(host(buf), exp), "gates %d shift %d grid %d" % (n, shift, g)
        assert sum(map(sum, M.wiring_ones(gates, shift, size))) == n     # one entry per gate


# ---- the Horner scan -------------------------------------------------------------------------------------------
def horner_buffers(torch, n):
    nb = (n + DRV.HORNER_BLOCK - 1) // DRV.HORNER_BLOCK
    return blank(torch, nb), blank(torch, nb)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 2 * 2048 + 1])
def test_horner_divide_quotient_coefficients(L, torch, pool, n):
    """the quotient's coefficients themselves, not only p(z): lengths either side of a lane's 8 coefficients and of a workgroup's 2048"""
    rng = random.Random(n)
    for q, kind in enumerate(T.FILLS_ARITH):
        c, tc = take(pool, kind, n, q)
        for z in [rng.randrange(R), SPECIAL[(q + n) % 3]]:
            keep, zp = fr(z)
            v = M.horner_suffix(tc, z)
            vals, carries = horner_buffers(torch, n)
            quo, ev = blank(torch, n - 1), blank(torch, 1)
            ok(L.mle_driver_horner_divide(c.data_ptr(), n, zp, vals.data_ptr(), carries.data_ptr(), quo.data_ptr(), ev.data_ptr(), stream(torch)))
            expect(quo, v[1:], "quotient %s n %d z %d" % (kind, n, z))
            expect(ev, v[:1], "evaluation %s n %d z %d" % (kind, n, z))
            vals, carries = horner_buffers(torch, n)
            v0 = blank(torch, 1)
            ok(L.mle_driver_horner_eval(c.data_ptr(), n, zp, vals.data_ptr(), carries.data_ptr(), v0.data_ptr(), stream(torch)))
            expect(v0, v[:1], "p(z) %s n %d z %d" % (kind, n, z))


def horner_top_layout(n):
    """(blocks, per, first block of the last lane that holds any) of horner_top_kernel's 1024 lanes"""
    nb = (n + DRV.HORNER_BLOCK - 1) // DRV.HORNER_BLOCK
    per = (nb + 1023) // 1024
    return nb, per, (nb - 1) // per * per


def sparse_positions(n):
    """the boundaries that matter above 1024 blocks, each with its neighbours"""
    nb, per, last_lo = horner_top_layout(n)
    marks = [0, 7, 8, 2047, 2048, per * 2048 - 1, per * 2048, last_lo * 2048, n - 1]
    return sorted({m + d for m in marks for d in (-1, 0, 1) if 0 <= m + d < n})


LARGE = [(1 << 21) + 1, (1 << 21) + 3 * 2048 + 5, (1 << 22) + 1]


def sparse_coefficients(torch, pool, n):
    """(device coefficients, {index: canonical value}): zero but for full-range values at sparse_positions(n)"""
    pos = sparse_positions(n)
    c = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    rows = torch.cat([pool["uniform_r"]["dev"][40:40 + len(pos) // 2], pool["top"]["dev"][40:40 + len(pos) - len(pos) // 2]])
    ints = pool["uniform_r"]["ints"][40:40 + len(pos) // 2] + pool["top"]["ints"][40:40 + len(pos) - len(pos) // 2]
    c[torch.tensor(pos, device="cuda")] = rows
    return c, dict(zip(pos, ints))


@pytest.mark.parametrize("n", LARGE)
def test_horner_above_1024_workgroups(L, torch, pool, n):
    """per = 2 (the last lane holding one block, then two) and per = 3: the in-lane Horner over several blocks, R^per and the carries of
    every block, seen through p(z) and through the quotient either side of every boundary and at scattered indices"""
    nb, per, last_lo = horner_top_layout(n)
    assert nb > 1024 and per == (3 if n > 1 << 22 else 2) and (nb - last_lo == 1) == (n in (LARGE[0],))
    t0 = time.perf_counter()
    c, nonzero = sparse_coefficients(torch, pool, n)
    rng = random.Random(n)
    at = sorted(set(sparse_positions(n)) | {rng.randrange(1, n) for _ in range(40)} | {2048 * b for b in (1, 2, 3, 1023, 1024, 1025, nb - 1)})
    at = [i for i in at if 1 <= i < n]
    d_at = torch.tensor([i - 1 for i in at], device="cuda")              # V_i is quotient[i - 1]
    assert 0 <= min(at) - 1 and max(at) - 1 < n - 1                      # inside the quotient: the gather below is not to leave it
    for z in [rng.randrange(R)] + SPECIAL:
        keep, zp = fr(z)
        want = M.horner_suffix_sparse(nonzero, z, [0] + at)
        vals, carries = horner_buffers(torch, n)
        quo, ev = blank(torch, n - 1), blank(torch, 1)
        ok(L.mle_driver_horner_divide(c.data_ptr(), n, zp, vals.data_ptr(), carries.data_ptr(), quo.data_ptr(), ev.data_ptr(), stream(torch)))
        expect(ev, want[:1], "p(z), z = %d" % z)
        expect(quo[d_at], want[1:], "quotient, z = %d" % z)
        assert (host(quo[n - 1:]) == np.uint64(PATTERN)).all() and (host(vals[nb:]) == np.uint64(PATTERN)).all()
        assert (host(carries[nb:]) == np.uint64(PATTERN)).all()
        vals, carries = horner_buffers(torch, n)
        v0 = blank(torch, 1)
        ok(L.mle_driver_horner_eval(c.data_ptr(), n, zp, vals.data_ptr(), carries.data_ptr(), v0.data_ptr(), stream(torch)))
        expect(v0, want[:1], "horner_eval, z = %d" % z)
    print("horner n = %d (%d blocks, per %d): %.2f s" % (n, nb, per, time.perf_counter() - t0))


def test_horner_dense_random_2_21_plus_1(L, torch):
    """every coefficient random (limbs below 2^62: valid residues), p(z) by an integer Horner over the downloaded coefficients.  The
    Montgomery map is linear, so the recurrence runs on the STORED integers with the canonical z and ends on the stored p(z)."""
    n = LARGE[0]
    t0 = time.perf_counter()
    g = torch.Generator(device="cuda").manual_seed(2101)
    c = torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    z = random.Random(2102).randrange(R)
    keep, zp = fr(z)
    vals, carries = horner_buffers(torch, n)
    v0 = blank(torch, 1)
    ok(L.mle_driver_horner_eval(c.data_ptr(), n, zp, vals.data_ptr(), carries.data_ptr(), v0.data_ptr(), stream(torch)))
    raw = c.cpu().numpy().tobytes()
    acc = 0
    for i in range(n - 1, -1, -1):                                       # chunked by nothing but the interpreter: one multiply-add per coefficient
        acc = (acc * z + int.from_bytes(raw[32 * i:32 * i + 32], "little")) % R
    got = host(v0)
    assert (got[1:] == np.uint64(PATTERN)).all()
    assert T.to_int(got[0]) == acc
    print("dense horner 2^21 + 1: %.2f s" % (time.perf_counter() - t0))


# ---- the weights of `evaluation` ---------------------------------------------------------------------------------
def weight_points(rng, count, special=None, at=()):
    pts = [rng.randrange(R) for _ in range(count)]
    for i in at:
        pts[i] = special
    return pts


@pytest.mark.parametrize("k", range(1, 9))
def test_eq_weights(L, torch, k):
    rng = random.Random(k)
    for first in (0, 1, 5, 48 - k):
        cases = [weight_points(rng, first + k)]
        cases += [weight_points(rng, first + k, s, {first, first + k // 2, first + k - 1}) for s in SPECIAL]
        for pts in cases:
            keep, pp = pts_arg(pts)
            out = blank(torch, 1 << k)
            ok(L.mle_driver_eq_weights(pp, first, k, out.data_ptr(), stream(torch)))
            expect(out, M.eq_weights(pts, first, k), "k %d first %d" % (k, first))


@pytest.mark.parametrize("log_n", [17, 18, 22])
def test_eval_weights(L, torch, log_n):
    k1, k2, s = M.evaluation_split(log_n)
    rng = random.Random(log_n)
    edges = {0, k1 // 2, k1 - 1, k1, k1 + (k2 - s) // 2, k1 + k2 - s - 1, k1 + k2 - s, log_n - 1}   # leading, middle and last place of each table
    for pts in [weight_points(rng, log_n)] + [weight_points(rng, log_n, v, edges) for v in SPECIAL]:
        keep, pp = pts_arg(pts)
        w1, wa, wb = blank(torch, 1 << k1), blank(torch, 1 << (k2 - s)), blank(torch, 1 << s)
        ok(L.mle_driver_eval_weights(pp, k1, k2, s, w1.data_ptr(), wa.data_ptr(), wb.data_ptr(), stream(torch)))
        for buf, want, what in zip((w1, wa, wb), M.eval_weights(pts, k1, k2, s), ("w1", "wa", "wb")):
            expect(buf, want, "%s of 2^%d" % (what, log_n))
