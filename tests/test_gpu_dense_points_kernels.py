"""GPU: every kernel of csrc/dense_points_kernels.hpp ALONE, at a grid, a segment length and a number of segments the test chooses,
against python integers (tests/dense_points_model.py, held to the oracle by tests/test_dense_points_model_cpu.py).

Through zkhip_dense_points these kernels run at the one plan dp_plan picks for a shape.  Here tests/cpp/dense_points_driver.hip launches
them at grids of 1, 2 and 3 point blocks, so that the point-block stride loops of the evaluation take a second, third and fifth step at a
few hundred points (in the library: above 2^24 points); with a batch and a cut together; with segments of several staged chunks and a
partial last chunk; with an empty segment; with nodes on the transform domain in every segment; and every stage's OWN output -- the
evaluation records, the partial products, 1 / D_i, the (Num, Den) records -- is compared, not only what the stages add up to.

Every comparison is == on limbs, every output must be canonical (below r), and every output buffer is pre-filled with a pattern and GUARD
elements longer than the kernel may write: what lies behind, the padding of a wider stride and the slots of lanes beyond the range must
keep the pattern.  Inputs are the full-range fills of tests/tables.py; points and nodes include 0, 1 and r - 1.

The records of a cut into segments of several chunks are derived from the model's records of the one-chunk cut, combined in order with the
model's own combine (a product for the weights, domain_fold for (Num, Den)): the CPU test proves the two equal, and the model then walks
every (node, point) pair once per node set instead of once per cut.

What each case catches was TRIED: the kernels header was changed in a scratch copy, the driver (or the library) built from it and the
named tests run on an MI355X; the changes were not kept.
- dropping the leading __syncthreads() of dp_eval_kernel: test_eval_stride_loop_on_a_full_chip fails (a few hundred to a few thousand
  of 2.1 M values, whole waves of 64 points).  test_eval at grids 1 to 3 does NOT: with three workgroups on the chip the four waves of a
  workgroup run in step and none overtakes another by the two loads that lie before its next store to LDS; it takes eight waves per
  SIMD to pull them apart, which is what that test is for.
- `seg` for `job * gridDim.y + seg` in the three record indices: test_eval_records_and_sum, every test_weights and every test_domain
  case fail (jobs = rows = 3 with the records buffer compared slot by slot: jobs 1 and 2 overwrite job 0's records and leave their own
  slots holding the pattern).
- dropping 4 * ch.first * in_stride in the chunk loop of zkhip_dense_points: test_interpolation_in_two_chunks of
  tests/test_gpu_dense_points.py fails from the first job of the second chunk on (the ys of job b are row b % 7 and the chunk is no
  multiple of 7); the batches of 64 of that file do not notice.
- truncating dp_pow's exponent to 32 bits: test_pow fails at e = 2^32, 2^32 + 1 and 2^40 - 1 for 2 and the uniform x, and at 2^32 for
  x = 0 (0^0 = 1): 28 of 130 pairs.  The x of order 2^32 cannot tell e from e mod 2^32.
- the fold skipping `den` one segment EARLY (s + 2 < segs): test_domain_fold_alone at 3 and 64 segments, test_domain at 2 chunk + 88 and
  4 chunk + 1 and test_domain_node_placements at 2 chunk + 1 fail in nearly every lane.  The fold multiplying `den` on the LAST segment
  too changes no Num and no test fails, as it should be: that product is only work saved.  test_domain_fold_alone zeroes the last
  segment's Den in half the lanes so that a fold which USED it would show."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_points_driver as DRV  # noqa: E402
import dense_points_model as M  # noqa: E402
import tables as T  # noqa: E402

pytestmark = pytest.mark.gpu
R = T.R
PATTERN = 0x5A5A5A5A5A5A5A5A
PATTERN32 = 0x5A5A5A5A
GUARD = 8
POOL = 16384
GRIDS = [1, 2, 3, "lib"]
SPECIAL = [0, 1, R - 1]
STRIDES = [(a, b) for a in (1, 0) for b in (1, 0)]                       # (coefficients, points): own rows or the one shared row


@pytest.fixture(scope="module")
def L():
    return DRV.lib()


@pytest.fixture(scope="module")
def K():
    """DP_LANES, DP_CHUNK, DP_MAX_SEGS, DP_MAX_GRID_X from the header the kernels were built with"""
    return DRV.constants()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def pool():
    """one table per arithmetic fill and its canonical integers, made once; a case takes a slice"""
    out = {}
    for q, kind in enumerate(T.FILLS_ARITH):
        a = T.fill(kind, POOL, 61000 + q)
        out[kind] = {"limbs": a, "ints": T.canonical(a)}
    return out


def take(pool, kind, n, off=0):
    assert off + n <= POOL
    return pool[kind]["ints"][off:off + n]


def spread(pool, kind, n, off=0):
    """n values of a fill, more than the pool holds: taken round the pool at a stride coprime to its length"""
    ints = pool[kind]["ints"]
    return [ints[(off + 7919 * k) % POOL] for k in range(n)]


def pack(vals):
    return np.stack([T.stored(v) for v in vals]) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def dev(torch, vals):
    """canonical ints -> device tensor [max(n, 1), 4] of stored limbs (one spare row for an empty input)"""
    a = pack(vals) if len(vals) else np.zeros((1, 4), dtype=np.uint64)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def blank(torch, rows):
    return torch.full((rows + GUARD, 4), PATTERN, dtype=torch.int64, device="cuda")


def flag_word(torch, value):
    """[the flag, the word behind it]"""
    return torch.tensor([value, PATTERN32], dtype=torch.int32, device="cuda")


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def ok(status):
    assert status == 0, "launcher returned hipError %d" % status


def expect(buf, want, what=""):
    """buf holds the stored limbs of `want` (canonical ints; None: an element no lane may write) and the pattern behind them"""
    got = host(buf)
    assert len(want) + GUARD == len(got), what
    keep = np.array([w is None for w in want] + [True] * GUARD)
    assert (got[keep] == np.uint64(PATTERN)).all(), "%s: written where no lane may write" % what
    assert T.below_r(got[~keep]).all(), "%s: an output is not below r" % what
    exp = pack([w for w in want if w is not None])
    bad = np.nonzero((got[~keep] != exp).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d outputs differ, the first at %d" % (what, len(bad), len(exp), bad[0])


def rows_with_padding(rows, stride):
    """rows of canonical ints -> one list, each row padded with None to `stride`"""
    out = []
    for r in rows:
        out += list(r) + [None] * (stride - len(r))
    return out


def with_specials(vals, lead=0):
    """0, 1 and r - 1 among the values (as far as they fit), spread out; `lead` rotates which comes first"""
    vals = list(vals)
    n = len(vals)
    for k in range(min(3, n)):
        vals[(k * 7 + lead) % n if n > 21 else k] = SPECIAL[(k + lead) % 3]
    return vals


def point_counts(K, grid):
    """the numbers of points of a kernel that strides over point blocks: either side of a block and of one, two and four strides"""
    ln = K["lanes"]
    if grid == "lib":
        return [1, ln - 1, ln, ln + 1, 1000, 3075]
    s = ln * grid
    return sorted({1, ln - 1, ln, ln + 1, s, s + 1, 2 * s - 1, 2 * s + 1, 4 * s + 3})


def grid_for(grid, n_points):
    return DRV.library_grid(n_points) if grid == "lib" else grid


def group_len(K, n, segs):
    """the segment length of a cut of n inner elements into `segs` segments of whole chunks"""
    ch = K["chunk"]
    chunks = max(-(-n // ch), 1)
    return -(-chunks // segs) * ch


def cuts(K, n):
    """(seg_len, segs): the whole range as one segment, two and three segments (the later ones EMPTY where the range is one chunk),
    and one chunk per segment"""
    ch = K["chunk"]
    chunks = max(-(-n // ch), 1)
    return sorted({(chunks * ch, 1), (group_len(K, n, 2), 2), (group_len(K, n, 3), 3), (ch, chunks)})


# ---- dp_eval_kernel<false> ---------------------------------------------------------------------------------------------------------------
_HORNER = {}


def horner_row(ckey, coeffs, xkey, xs):
    if (ckey, xkey) not in _HORNER:
        _HORNER[ckey, xkey] = [M.horner(coeffs, x) for x in xs]
    return _HORNER[ckey, xkey]


def eval_inputs(torch, pool, kind, n_in, n_x, jobs, own_c, own_x, seed):
    """(device coefficients, in_stride, device points, x_stride, per job (key, ints) of both): rows 5 and 3 elements wider than they hold"""
    in_stride, x_stride = (n_in + 5 if own_c else 0), (n_x + 3 if own_x else 0)
    crow = [take(pool, kind, n_in, 11 + j * (n_in + 5)) for j in range(jobs)]
    flat = take(pool, kind, (jobs - 1) * (n_in + 5) + n_in, 11)
    other = T.rotation(T.FILLS_ARITH, kind, 2)[1]
    xrow = [with_specials(take(pool, other, n_x, seed + j * (n_x + 3)), j) for j in range(jobs)]
    xflat = []
    for j in range(jobs):
        xflat += xrow[j] + take(pool, other, 3, 40 + j)
    cs = [(("c", kind, n_in, j if own_c else 0), crow[j if own_c else 0]) for j in range(jobs)]
    xs = [(("x", other, n_x, seed, j if own_x else 0), xrow[j if own_x else 0]) for j in range(jobs)]
    return dev(torch, flat), in_stride, dev(torch, xflat), x_stride, cs, xs


@pytest.mark.parametrize("grid", GRIDS)
def test_eval(L, K, torch, pool, grid):
    """dp_eval_kernel<false> against horner(): every number of points with one job and the numbers of coefficients in rotation, 2 chunk + 1
    of them (three staged chunks per stride step) wherever the stride loop steps; three jobs at every combination of a zero and a non-zero
    in_stride and x_stride where the cost of the reference allows (up to two stride steps).  The rows of `out` are 3 wider than n_x."""
    ln, ch = K["lanes"], K["chunk"]
    n_ins = [0, 1, ch - 1, ch, ch + 1, 2 * ch + 1]
    s = ln * (3 if grid == "lib" else grid)
    cases = []
    for q, n_x in enumerate(point_counts(K, grid)):
        cases.append((n_x, n_ins[q % 6], 1, (1, 1), T.FILLS_ARITH[q % 4]))
        if n_x > ln * grid_for(grid, n_x) and n_ins[q % 6] != 2 * ch + 1:
            cases.append((n_x, 2 * ch + 1, 1, (1, 1), T.FILLS_ARITH[(q + 1) % 4]))
    for q, (n_x, n_in) in enumerate(((1, ch + 1), (ln + 1, 0), (s + 1, 2 * ch + 1), (2 * s + 1, 1), (ln - 1, ch))):
        cases += [(n_x, n_in, 3, st, T.FILLS_ARITH[q % 4]) for st in STRIDES]   # one fill per shape: the four combinations share their references
    for n_x, n_in, jobs, (own_c, own_x), kind in cases:
        g = grid_for(grid, n_x)
        d_c, in_stride, d_x, x_stride, cs, xs = eval_inputs(torch, pool, kind, n_in, n_x, jobs, own_c, own_x, 100 + n_x % 50)
        out_stride = n_x + 3
        out = blank(torch, jobs * out_stride)
        ok(L.dp_driver_eval(0, d_c.data_ptr() if n_in else None, in_stride, n_in, d_x.data_ptr(), x_stride, n_x, out.data_ptr(), out_stride,
                            group_len(K, n_in, 1), g, 1, jobs, stream(torch)))
        want = [horner_row(cs[j][0], cs[j][1], xs[j][0], xs[j][1]) for j in range(jobs)]
        expect(out, rows_with_padding(want, out_stride), "n_x %d n_in %d jobs %d strides %d %d grid %d %s" % (n_x, n_in, jobs, in_stride, x_stride, g, kind))


@pytest.mark.parametrize("n_in_of", ["2ch", "2ch+1"])
def test_eval_stride_loop_on_a_full_chip(L, K, torch, pool, n_in_of):
    """the stride loop with the chip full: 4096 jobs of one polynomial at one set of 2 lanes + 1 points, grid_x = 1, so every workgroup
    re-stages its two or three chunks for three point blocks while eight waves share each SIMD.  The four waves of a workgroup then run at
    different rates, which is when a wave that re-stages the top chunk for the next point block could overtake one that still reads the
    bottom chunk of the block before.  Every job must give the one row of horner(); compared on the device."""
    ln, ch = K["lanes"], K["chunk"]
    n_in = 2 * ch + (n_in_of == "2ch+1")
    n_x, jobs = 2 * ln + 1, 4096
    coeffs, xs = take(pool, "uniform_r", n_in, 21), with_specials(take(pool, "top", n_x, 22))
    d_c, d_x = dev(torch, coeffs), dev(torch, xs)
    want = dev(torch, [M.horner(coeffs, x) for x in xs])
    stride = n_x + 3
    out = torch.full((jobs, stride, 4), PATTERN, dtype=torch.int64, device="cuda")
    ok(L.dp_driver_eval(0, d_c.data_ptr(), 0, n_in, d_x.data_ptr(), 0, n_x, out.data_ptr(), stride, group_len(K, n_in, 1), 1, 1, jobs, stream(torch)))
    assert bool((out[:, n_x:] == PATTERN).all()), "the padding of a wider out_stride was written"
    bad = (out[:, :n_x] != want).any(dim=2).nonzero()
    assert not len(bad), "%d of %d values differ, the first is (job, point) %s" % (len(bad), jobs * n_x, bad[0].tolist())


# ---- dp_eval_kernel<true>, dp_eval_sum_kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_eval_records_and_sum(L, K, torch, pool, grid):
    """three jobs and a cut together; segments of two staged chunks with a partial last chunk; one segment; two EMPTY segments.  The records
    themselves against eval_records -- slot (job * segs + seg) * n_x + p, so a record stored for the wrong job or segment shows even where
    the sum kernel would read it back the same wrong way -- then the sums.  0, 1 and r - 1 are points of every job, so they meet every
    segment with lo > 0: x = 0 must give 0 there (dp_pow(0, lo)) and x = r - 1 the sign of lo's parity."""
    ln, ch = K["lanes"], K["chunk"]
    s = ln * (3 if grid == "lib" else grid)
    shapes = [(2 * ch + 88, ch, 3, s + 1), (5 * ch + 20, 2 * ch, 3, ln + 1), (3 * ch + 1, ch, 4, s), (ch, ch, 1, 2 * s + 1), (ch + 44, ch, 4, ln - 1)]
    for q, (n_in, seg_len, segs, n_x) in enumerate(shapes):
        kind = T.FILLS_ARITH[(q + (0 if grid == "lib" else grid)) % 4]
        own_c, own_x = STRIDES[q % 4] if q else (1, 1)
        g = grid_for(grid, n_x)
        jobs = 3
        d_c, in_stride, d_x, x_stride, cs, xs = eval_inputs(torch, pool, kind, n_in, n_x, jobs, own_c, own_x, 200 + q)
        rec = blank(torch, jobs * segs * n_x)
        ok(L.dp_driver_eval(1, d_c.data_ptr(), in_stride, n_in, d_x.data_ptr(), x_stride, n_x, rec.data_ptr(), 0, seg_len, g, segs, jobs, stream(torch)))
        memo = {}
        for (ck, c), (xk, x) in zip(cs, xs):
            if (ck, xk) not in memo:
                memo[ck, xk] = M.eval_records(c, x, seg_len, segs)
        model = [memo[cs[j][0], xs[j][0]] for j in range(jobs)]
        what = "n_in %d seg_len %d segs %d n_x %d strides %d %d grid %d %s" % (n_in, seg_len, segs, n_x, in_stride, x_stride, g, kind)
        expect(rec, [v for j in range(jobs) for seg in range(segs) for v in model[j][seg]], "records: " + what)
        for j in range(jobs):
            for seg in range(1, segs):
                lo, hi = M.segment(n_in, seg_len, seg)
                for p, x in enumerate(xs[j][1]):
                    if x == 0:
                        assert model[j][seg][p] == 0
                    if lo == hi:
                        assert model[j][seg][p] == 0
        out_stride = n_x + 3
        out = blank(torch, jobs * out_stride)
        ok(L.dp_driver_eval_sum(rec.data_ptr(), segs, n_x, out.data_ptr(), out_stride, g, jobs, stream(torch)))
        sums = [[sum(model[j][seg][p] for seg in range(segs)) % R for p in range(n_x)] for j in range(jobs)]
        for j in range(jobs):                                              # the model's own cross-check on the points that matter most
            at = [p for p, x in enumerate(xs[j][1]) if x in SPECIAL] + [n_x - 1]
            assert [sums[j][p] for p in at] == [M.horner(cs[j][1], xs[j][1][p]) for p in at]
        expect(out, rows_with_padding(sums, out_stride), "sums: " + what)


@pytest.mark.parametrize("segs", [1, 2, 64])
@pytest.mark.parametrize("grid", [1, 3, "lib"])
def test_eval_sum_alone(L, K, torch, pool, grid, segs):
    """the sum kernel over records of every fill (sums that wrap r, r - 1 added 64 times), three jobs, its own stride loop stepping"""
    ln = K["lanes"]
    jobs = 3
    for q, kind in enumerate(T.FILLS_ARITH):
        steps = 2 * ln * (1 if grid == "lib" else grid) + 1                  # two strides and one point
        n_x = [steps if segs <= 2 else 2 * ln + 1, ln - 1, ln + 1, 1][(q + segs) % 4]
        g = grid_for(grid, n_x)
        recs = spread(pool, kind, jobs * segs * n_x, q)
        d_rec = dev(torch, recs)
        out_stride = n_x + 2
        out = blank(torch, jobs * out_stride)
        ok(L.dp_driver_eval_sum(d_rec.data_ptr(), segs, n_x, out.data_ptr(), out_stride, g, jobs, stream(torch)))
        want = [[sum(recs[(j * segs + sg) * n_x + p] for sg in range(segs)) % R for p in range(n_x)] for j in range(jobs)]
        expect(out, rows_with_padding(want, out_stride), "%s segs %d n_x %d grid %d" % (kind, segs, n_x, g))


# ---- the weights -----------------------------------------------------------------------------------------------------------------------------
def distinct(vals, n):
    out = list(dict.fromkeys(vals))[:n]
    assert len(out) == n
    return out


def node_rows(pool, n, rows, seed, specials=True):
    """`rows` sets of n distinct nodes; with 0, 1 and r - 1 (as far as they fit) at the front, in the middle and at the end"""
    out = []
    for j in range(rows):
        xs = distinct([v for v in take(pool, "uniform_r", n + 8, seed + j * (n + 8)) if v not in SPECIAL], n)
        if specials:
            for at, v in zip(sorted({0, n // 2, n - 1}), SPECIAL[j % 3:] + SPECIAL[:j % 3]):
                xs[at] = v
        else:
            xs[0] = 0
        assert len(set(xs)) == n
        out.append(xs)
    return out


def grouped(fine, group, segs, combine, empty):
    """the records of `segs` segments of `group` chunks each from the one-chunk records `fine` ([chunk][lane]): combined in order"""
    out = []
    for sg in range(segs):
        part = fine[sg * group:(sg + 1) * group]
        out.append(combine(part) if part else [empty] * len(fine[0]))
    return out


def product(part):
    out = list(part[0])
    for nxt in part[1:]:
        out = [a * b % R for a, b in zip(out, nxt)]
    return out


def run_weights(L, K, torch, xs_rows, x_stride_own, n, flags=(0, PATTERN32)):
    """every cut of n nodes through the record kernel and the fold, and the whole range through dp_weights_kernel<false>; the records,
    1 / D_i and the flag against the model.  Returns nothing: asserts."""
    ch = K["chunk"]
    rows = 3
    chunks = max(-(-n // ch), 1)
    x_stride = n + 4 if x_stride_own else 0
    flat = []
    for xs in xs_rows:
        flat += xs + [5, 6, 7, 8]
    d_x = dev(torch, flat)
    use = [xs_rows[j if x_stride_own else 0] for j in range(rows)]
    fine = [M.weight_records(xs, ch, chunks) for xs in (use if x_stride_own else use[:1])]
    fine = fine if x_stride_own else fine * rows
    D = [product(f) for f in fine]
    winv = [[M.invert(d) for d in row] for row in D]
    raised = any(d == 0 for row in D for d in row)
    for seg_len, segs in cuts(K, n):
        what = "n %d seg_len %d segs %d x_stride %d" % (n, seg_len, segs, x_stride)
        rec = blank(torch, rows * segs * n)
        fl = flag_word(torch, PATTERN32)
        ok(L.dp_driver_weights(1, d_x.data_ptr(), x_stride, n, seg_len, rec.data_ptr(), fl.data_ptr(), segs, rows, stream(torch)))
        model = [grouped(f, seg_len // ch, segs, product, 1) for f in fine]
        expect(rec, [v for j in range(rows) for sg in range(segs) for v in model[j][sg]], "records: " + what)
        assert fl.cpu().tolist() == [PATTERN32, PATTERN32], "the record kernel wrote the flag"
        for given in flags:
            out, fl = blank(torch, rows * n), flag_word(torch, given)
            ok(L.dp_driver_weights_fold(rec.data_ptr(), segs, n, out.data_ptr(), fl.data_ptr(), rows, stream(torch)))
            expect(out, [v for row in winv for v in row], "fold: " + what)
            assert fl.cpu().tolist() == [1 if raised else given, PATTERN32], "fold, the flag given %#x: %s" % (given, what)
    for given in flags:
        out, fl = blank(torch, rows * n), flag_word(torch, given)
        ok(L.dp_driver_weights(0, d_x.data_ptr(), x_stride, n, chunks * ch, out.data_ptr(), fl.data_ptr(), 1, rows, stream(torch)))
        expect(out, [v for row in winv for v in row], "dp_weights_kernel<false> n %d x_stride %d" % (n, x_stride))
        assert fl.cpu().tolist() == [1 if raised else given, PATTERN32], "dp_weights_kernel<false>, the flag given %#x, n %d" % (given, n)
    return D


@pytest.mark.parametrize("n_of", ["1", "2", "ch-1", "ch", "ch+1", "2ch+1", "4ch+1"])
def test_weights(L, K, torch, pool, n_of):
    """partial products per segment (slot (row * segs + seg) * n + i), their fold, 1 / D_i and the flag, at three node sets of their own
    and at one shared set; with distinct nodes the flag word keeps what it was given -- 0, and a pattern: the kernels may only ever store
    1 -- and the word behind it keeps the pattern.  At one chunk the cuts into 2 and 3 segments leave EMPTY segments (records of 1)."""
    ch = K["chunk"]
    n = {"1": 1, "2": 2, "ch-1": ch - 1, "ch": ch, "ch+1": ch + 1, "2ch+1": 2 * ch + 1, "4ch+1": 4 * ch + 1}[n_of]
    xs_rows = node_rows(pool, n, 3, 300 + n)
    D = run_weights(L, K, torch, xs_rows, True, n)
    assert all(d != 0 for row in D for d in row)
    run_weights(L, K, torch, xs_rows, False, n)


@pytest.mark.parametrize("where", ["one_segment", "two_segments"])
def test_weights_repeated_nodes(L, K, torch, pool, where):
    """a node repeated in ONE row of three, inside one segment and across two: both lanes' D_i and 1 / D_i are zero, the flag becomes 1
    whatever it held, the other rows are exact"""
    ch = K["chunk"]
    n = 2 * ch + 1
    xs_rows = node_rows(pool, n, 3, 400)
    row, a, b = (1, 5, ch - 56) if where == "one_segment" else (2, 7, ch + 9)
    xs_rows[row][b] = xs_rows[row][a]
    D = run_weights(L, K, torch, xs_rows, True, n)
    assert [(j, i) for j, r in enumerate(D) for i, d in enumerate(r) if d == 0] == [(row, a), (row, b)]


# ---- the domain values -------------------------------------------------------------------------------------------------------------------------
def omega_arg(N):
    a = np.ascontiguousarray(T.stored(M.root_of_unity(N)))
    return a, a.ctypes.data


_FINE = {}


def fine_domain(key, xs, ys, winv, N, ch):
    """the model's (Num, Den) records at one chunk per segment, once per (node set, values, weights)"""
    if key not in _FINE:
        _FINE[key] = M.domain_records(xs, ys, winv, N, ch, max(-(-len(xs) // ch), 1))
    return _FINE[key]


def run_domain(L, K, torch, tag, xs_rows, ys_rows, winv_rows, n, strides, lagrange_rows, first=0):
    """three jobs; job j reads row j of a table whose stride is non-zero, row 0 else.  Every cut through the record kernel and the fold,
    the whole range through dp_domain_kernel<false>: the records against the model, the values against the model's fold and, for the
    jobs of `lagrange_rows` (whose three rows belong together), against the Lagrange model's polynomial at w^t.  `first`: the tables
    hold more than three rows and job 0 is row `first`."""
    ch = K["chunk"]
    jobs = 3
    log_N = (n - 1).bit_length()
    N = 1 << log_N
    chunks = max(-(-n // ch), 1)
    own_y, own_x, own_w = strides
    flat = lambda rows: [v for r in rows for v in list(r) + [9, 10]]     # noqa: E731  -- rows two elements wider than they hold
    d_y, d_x, d_w = dev(torch, flat(ys_rows)), dev(torch, flat(xs_rows)), dev(torch, flat(winv_rows))
    pick = [(first + (j if own_y else 0), first + (j if own_x else 0), first + (j if own_w else 0)) for j in range(jobs)]
    fine = [fine_domain((tag, n) + p, xs_rows[p[1]], ys_rows[p[0]], winv_rows[p[2]], N, ch) for p in pick]
    vals = [[num for num, _den in M.domain_fold(f)] for f in fine]
    for j in lagrange_rows:
        if pick[j] == (first + j,) * 3:
            coeffs = M.lagrange_coefficients(xs_rows[first + j], ys_rows[first + j])
            w = M.root_of_unity(N)
            assert vals[j] == [M.horner(coeffs, pow(w, t, R)) for t in range(N)], "the models disagree"
    keep, om = omega_arg(N)
    at = 32 * first * (n + 2)
    args = (d_y.data_ptr() + at, (n + 2) * own_y, d_x.data_ptr() + at, (n + 2) * own_x, d_w.data_ptr() + at, (n + 2) * own_w, n, log_N)
    for seg_len, segs in cuts(K, n):
        what = "%s n %d N %d seg_len %d segs %d strides %s" % (tag, n, N, seg_len, segs, strides)
        rec = blank(torch, 2 * jobs * segs * N)
        ok(L.dp_driver_domain(1, *args, seg_len, om, rec.data_ptr(), segs, jobs, stream(torch)))
        model = [grouped(f, seg_len // ch, segs, lambda part: M.domain_fold(part), (0, 1)) for f in fine]
        expect(rec, [v for j in range(jobs) for sg in range(segs) for pair in model[j][sg] for v in pair], "records: " + what)
        out = blank(torch, jobs * N)
        ok(L.dp_driver_domain_fold(rec.data_ptr(), segs, N, out.data_ptr(), jobs, stream(torch)))
        expect(out, [v for row in vals for v in row], "fold: " + what)
    out = blank(torch, jobs * N)
    ok(L.dp_driver_domain(0, *args, chunks * ch, om, out.data_ptr(), 1, jobs, stream(torch)))
    expect(out, [v for row in vals for v in row], "dp_domain_kernel<false> %s n %d strides %s" % (tag, n, strides))
    return fine


def domain_tables(pool, n, xs_rows, seed):
    ys_rows = [take(pool, T.FILLS_ARITH[j % 4], n, seed + j * (n + 2)) for j in range(len(xs_rows))]
    return ys_rows, [M.weights_inv(xs) for xs in xs_rows]                 # 1 / D_i from the model, not from the kernel under test


@pytest.mark.parametrize("n_of", ["1", "2", "3", "ch-1", "ch", "ch+1", "2ch+88", "4ch+1"])
def test_domain(L, K, torch, pool, n_of):
    """(Num, Den) per segment (slot 2 ((job * segs + seg) * N + t)), their fold and dp_domain_kernel<false>.  The nodes hold 0, 1 = w^0 and
    r - 1 = w^(N/2) at the front, in the middle and at the end: the lanes t = 0 and t = N / 2 meet z - x_i == 0 in the first, a middle or
    the LAST segment.  Up to chunk + 1 nodes the three jobs have node sets of their own (the specials in a different order per job) and
    every combination of zero and non-zero y, x and w strides runs (the recurrence takes 1 / D_i as given, so rows that do not belong
    together still have a model).  Above, the model's N n steps per job weigh seconds, so jobs 1 and 2 are job 0's problem moved by a
    power of the domain's generator and scaled (model.rotate_problem: other nodes, other values, other weights, other lanes on a node;
    their records follow from job 0's, which the CPU test proves), with all strides own and all zero; at 4 chunk + 1 the comparison with
    the Lagrange model's polynomial is left to the sizes below (1025^2 steps more), the records and the fold are compared as everywhere."""
    ch = K["chunk"]
    n = {"1": 1, "2": 2, "3": 3, "ch-1": ch - 1, "ch": ch, "ch+1": ch + 1, "2ch+88": 2 * ch + 88, "4ch+1": 4 * ch + 1}[n_of]
    N = 1 << (n - 1).bit_length()
    xs_rows = node_rows(pool, n, 3, 500 + n)
    if n <= ch + 1:
        ys_rows, winv_rows = domain_tables(pool, n, xs_rows, 600)
        combos, lagrange = list(itertools.product((1, 0), repeat=3)), [0, 1, 2]
    else:
        ys0, winv0 = take(pool, "top", n, 600), M.weights_inv(xs_rows[0])
        moved = [(xs_rows[0], ys0, winv0)] + [M.rotate_problem(xs_rows[0], ys0, winv0, N, k, c) for k, c in ((N // 2 + 3, R - 2), (N - 1, ys0[1]))]
        xs_rows, ys_rows, winv_rows = ([m[q] for m in moved] for q in range(3))
        assert all(len(set(xs)) == n for xs in xs_rows)
        first = fine_domain(("sweep", n, 0, 0, 0), xs_rows[0], ys_rows[0], winv_rows[0], N, ch)
        for j, (k, c) in ((1, (N // 2 + 3, R - 2)), (2, (N - 1, ys0[1]))):
            _FINE["sweep", n, j, j, j] = M.rotate_domain_records(first, N, n, k, c, ch)
        combos, lagrange = [(1, 1, 1), (0, 0, 0)], ([0] if n <= 2 * ch + 88 else [])
    for strides in combos:
        fine = run_domain(L, K, torch, "sweep", xs_rows, ys_rows, winv_rows, n, strides, lagrange)
    if n >= 3:                                                             # all shared: job 0's rows; its lanes 0 and N / 2 sit on nodes
        zero_dens = [(c, t) for c, chunk in enumerate(fine[0]) for t, (_num, den) in enumerate(chunk) if den == 0]
        assert sorted(t for _c, t in zero_dens) == [0, N // 2]


@pytest.mark.parametrize("n_of", ["ch+1", "2ch+1"])
def test_domain_node_placements(L, K, torch, pool, n_of):
    """where the nodes meet the domain, in four node sets A to D: nowhere (the nodes hold 0 but neither 1 nor r - 1, which are domain
    points); one node in the last segment only; two nodes in two different segments; two nodes in the same segment.  Jobs A, B, C, then
    B, C, D of the one table.  Lanes with z == x_i (Den stays 0 to the end of that segment, and Num must still end on y_i) and lanes
    without are compared alike, in the records and in the values.  At chunk + 1 nodes the values are also the Lagrange model's
    polynomial; at 2 chunk + 1 that comparison is left out for its cost (the value on a node is still held to the node's y)."""
    ch = K["chunk"]
    n = ch + 1 if n_of == "ch+1" else 2 * ch + 1
    N = 1 << (n - 1).bit_length()
    w = M.root_of_unity(N)
    chunks = -(-n // ch)
    base = (chunks - 2) * ch
    rows = node_rows(pool, n, 4, 700 + n, specials=False)
    A, B, C, D = rows
    B[n - 1] = pow(w, 5, R)
    C[3], C[n - 1] = w, pow(w, N - 1, R)
    D[base + 44], D[base + 144] = pow(w, 2, R), pow(w, N // 2 + 44, R)
    where = [[], [(chunks - 1, 5)], [(0, 1), (chunks - 1, N - 1)], [(chunks - 2, 2), (chunks - 2, N // 2 + 44)]]
    assert all(len(set(r)) == n for r in rows)
    ys_rows, winv_rows = domain_tables(pool, n, rows, 800)
    for first in (0, 1):
        fine = run_domain(L, K, torch, "placed", rows, ys_rows, winv_rows, n, (1, 1, 1), [0, 1, 2] if n <= ch + 1 else [], first)
        for j in range(3):
            zero_dens = [(c, t) for c, chunk in enumerate(fine[j]) for t, (_num, den) in enumerate(chunk) if den == 0]
            assert zero_dens == sorted(where[first + j]), first + j
            for _c, t in zero_dens:                                      # the value on a node is the node's y
                i = rows[first + j].index(pow(w, t, R))
                assert M.domain_fold(fine[j])[t][0] == ys_rows[first + j][i]


@pytest.mark.parametrize("n_of", ["1", "2", "ch", "2ch"])
def test_domain_all_nodes_on_the_domain(L, K, torch, pool, n_of):
    """n == N and x_i = w^(a i + b): EVERY lane meets z - x_i == 0, in whichever segment its node lies"""
    ch = K["chunk"]
    n = {"1": 1, "2": 2, "ch": ch, "2ch": 2 * ch}[n_of]
    w = M.root_of_unity(n)
    rows = [[pow(w, (a * i + b) % n, R) for i in range(n)] for a, b in ((1, 0), (5, 3), (n - 1, 7))]
    ys_rows, winv_rows = domain_tables(pool, n, rows, 900)
    fine = run_domain(L, K, torch, "all", rows, ys_rows, winv_rows, n, (1, 1, 1), [0, 1, 2])
    for j in range(3):
        assert [num for num, _den in M.domain_fold(fine[j])] == [ys_rows[j][rows[j].index(pow(w, t, R))] for t in range(n)]


@pytest.mark.parametrize("segs", [1, 2, 3, 64])
def test_domain_fold_alone(L, K, torch, pool, segs):
    """the fold over (Num, Den) records of every fill, three jobs, N = lanes + 44 (no power of two; two point blocks, the second partial),
    with zero denominators: in the first segment, in the last, in the one before the last, and in two segments of one lane
    (den_A == 0 and db == 0 together).  With 3 and 64 segments a fold that drops the product of denominators one segment early, or
    never takes it, differs in every lane; the last segment's Den must not matter: it is set to 0 in half the lanes."""
    N, jobs = K["lanes"] + 44, 3
    for q, kind in enumerate(T.FILLS_ARITH):
        flat = spread(pool, kind, 2 * jobs * segs * N, 3 * q)
        recs = [[[(flat[2 * ((j * segs + sg) * N + t)], flat[2 * ((j * segs + sg) * N + t) + 1]) for t in range(N)] for sg in range(segs)] for j in range(jobs)]
        zero = [(0, 0, 5), (1, segs - 1, 6), (2, max(segs - 2, 0), 7), (1, 0, 300 % N), (1, segs - 1, 300 % N), (2, segs // 2, N - 1)]
        zero += [(0, segs - 1, t) for t in range(0, N, 2)]
        for j, sg, t in zero:
            recs[j][sg][t] = (recs[j][sg][t][0], 0)
        d_rec = dev(torch, [v for j in range(jobs) for sg in range(segs) for pair in recs[j][sg] for v in pair])
        out = blank(torch, jobs * N)
        ok(L.dp_driver_domain_fold(d_rec.data_ptr(), segs, N, out.data_ptr(), jobs, stream(torch)))
        want = [[num for num, _den in M.domain_fold(recs[j])] for j in range(jobs)]
        expect(out, [v for row in want for v in row], "%s segs %d" % (kind, segs))


# ---- dp_pow, dp_invert ---------------------------------------------------------------------------------------------------------------------------
def test_pow(L, torch, pool):
    """x^e with exponents that need 33 and 40 bits: the exponent is a size_t (DP_MAX_N = 2^40 coefficients).  x of order 2^32 tells
    e from e mod 2^32 apart as little as x = 0, 1 and r - 1 do -- x^(2^32) = 1 = x^0 -- so the uniform values and 2 carry that case."""
    xs = [0, 1, 2, R - 1, M.root_of_unity(1 << 32)] + take(pool, "uniform_r", 8, 77)
    es = [0, 1, 2, 3, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1]
    pairs = [(x, e) for x in xs for e in es]
    exps = np.array([e for _x, e in pairs], dtype=np.uint64)
    d_x, out = dev(torch, [x for x, _e in pairs]), blank(torch, len(pairs))
    ok(L.dp_driver_pow(d_x.data_ptr(), exps.ctypes.data, len(pairs), out.data_ptr(), stream(torch)))
    expect(out, [pow(x, e, R) for x, e in pairs], "dp_pow")
    assert pow(2, 1 << 32, R) != 1 and pow(xs[4], 1 << 32, R) == 1 and pow(xs[4], 1 << 31, R) == R - 1


def test_invert(L, K, torch, pool):
    """d * out == 1, or out == 0 for d == 0; the flag becomes 1 if and only if a zero was among the inputs, and is not written otherwise"""
    ds = [0, 1, R - 1] + [v for kind in T.FILLS_ARITH for v in take(pool, kind, 100, 9)] + [0, 2]
    for with_zero in (True, False):
        vals = ds if with_zero else [d for d in ds if d]
        assert len(vals) > K["lanes"]
        for given in (0, PATTERN32):
            d_in, out, fl = dev(torch, vals), blank(torch, len(vals)), flag_word(torch, given)
            ok(L.dp_driver_invert(d_in.data_ptr(), len(vals), out.data_ptr(), fl.data_ptr(), stream(torch)))
            got = T.canonical(host(out)[:len(vals)])
            assert all((d * v) % R == (1 if d else 0) and (d or v == 0) for d, v in zip(vals, got))
            expect(out, [M.invert(d) for d in vals], "dp_invert")
            assert fl.cpu().tolist() == [1 if with_zero else given, PATTERN32]
