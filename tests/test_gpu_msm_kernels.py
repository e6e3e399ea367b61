"""Stage pins of the bucket-method MSM (csrc/msm_kernels.hpp) through tests/cpp/msm_driver.hip, integer-exact and without any curve
arithmetic: the signed digits of DigitStream against the recoding rule restated in tests/msm_cases.py, and the state the sort, the heavy
filing and the order pass leave behind -- bucket counts, every bucket's run of entries, the record lists -- against the expectation
computed from those digits, on scalars aimed at the digit boundaries and bucket populations aimed at the filing thresholds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402
import msm_driver as DRV  # noqa: E402

pytestmark = pytest.mark.gpu

levels_of = MC.levels_of


def width_lists(kind):
    if kind == "uniform":
        return [MC.uniform_widths(c) for c in range(8, 21)]
    if kind == "plain":
        geos = [DRV.geo([0, n]) for n in MC.DIGIT_SIZES] + [DRV.geo(b) for b in MC.BATCHES]
    elif kind == "table":
        geos = [DRV.geo([0, n], True, n) for n in MC.DIGIT_SIZES]
    else:
        geos = [DRV.geo(levels_of(nv), True, 0) for nv in MC.LEVEL_VARS]
    return sorted({tuple(g.widths(j)) for g in geos for j in range(g.n_problems)})


@pytest.mark.parametrize("kind", ["uniform", "plain", "table", "level"])
def test_digits_equal_the_recoding_rule(kind):
    lists = width_lists(kind)
    assert len(lists) >= 3
    if kind != "uniform":
        assert any(len(set(w)) == 2 for w in lists)          # mixed hi / hi - 1 lists among them
    for widths in lists:
        widths = list(widths)
        sc = MC.family_scalars(widths) + MC.uniform(256, 100 + sum(widths[:3]))
        got = DRV.digits(MC.to_mont(sc), widths)
        want = MC.digits_np(sc, widths)
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want), widths
        # the boundary digit itself was among them
        assert all((want[:, w] == (1 << (c - 1))).any() for w, c in enumerate(widths[:-1]))
        assert all((want[:, w] == -((1 << (c - 1)) - 1)).any() for w, c in enumerate(widths[:-1]))


def check_sort(scalars, offsets, shared=False, stride=0, inf=None):
    """runs the sort / filing / order sequence and compares everything it leaves behind with the expectation; -> (driver output, geometry)"""
    g = DRV.geo(offsets, shared, stride)
    out = DRV.sort(MC.to_mont(scalars), offsets, shared, stride, inf)
    want_counts, want_keys = MC.expected_sort(scalars, g, inf)
    counts, offs, order, srt = out["counts"], out["offsets"], out["order"], out["sorted"]
    assert np.array_equal(counts, want_counts)
    total = int(want_counts.sum(dtype=np.int64))
    # the runs are disjoint and tile [0, total)
    nz = np.nonzero(counts)[0]
    by_start = nz[np.argsort(offs[nz], kind="stable")]
    starts, lens = offs[by_start].astype(np.int64), counts[by_start].astype(np.int64)
    if total:
        assert starts[0] == 0 and np.array_equal(starts[1:], (starts + lens)[:-1]) and starts[-1] + lens[-1] == total
    # per bucket, the multiset of its run
    bucket_of_pos = np.repeat(by_start.astype(np.int64), lens)
    got_keys = np.sort((bucket_of_pos << 32) | srt[:total].astype(np.int64))
    assert np.array_equal(got_keys, want_keys)
    # order: a permutation, counts non-increasing up to the clamp
    assert np.array_equal(np.sort(order), np.arange(g.n_buckets, dtype=np.uint32))
    clamped = np.minimum(counts[order].astype(np.int64), MC.COUNT_CLAMP)
    assert (np.diff(clamped) <= 0).all()
    # the heavy filing
    L = out["L"]
    assert L["heavy_min"] == g.heavy_min
    want_slots, want_rec, want_final = MC.expected_overflow(want_counts, g.heavy_min)
    assert out["ovf"] == [want_slots] + want_rec
    rec = out["rec"]
    finals, slots_seen = {}, []
    for level in range(4):
        for first, count, dst, final in rec[level].tolist():
            if final:
                assert dst not in finals
                finals[dst] = level
            else:
                slots_seen.append(dst)
    assert finals == want_final                                     # one final record per heavy bucket, at its level, dst = the bucket
    assert len(set(slots_seen)) == len(slots_seen) == want_slots and all(s < L["slots_cap"] for s in slots_seen)
    # level 0: the records of a heavy bucket tile its run, all but the last of 2048 points
    r0 = rec[0][np.argsort(rec[0][:, 0], kind="stable")] if len(rec[0]) else rec[0]
    heavy = sorted(want_final, key=lambda b: int(offs[b]))
    k = 0
    for b in heavy:
        pos, left = int(offs[b]), int(counts[b])
        n_groups = (left + MC.HEAVY_REC - 1) // MC.HEAVY_REC
        for q in range(n_groups):
            first, count, dst, final = (int(v) for v in r0[k])
            assert first == pos and count == min(MC.HEAVY_REC, left) and final == (1 if n_groups == 1 else 0)
            pos, left, k = pos + count, left - count, k + 1
        assert left == 0
    assert k == len(r0)
    # levels above: the records of level l cover exactly the slots the non-final records of level l - 1 wrote
    for level in (1, 2, 3):
        below = sorted(int(r[2]) for r in rec[level - 1] if not r[3])
        covered = sorted(s for r in rec[level] for s in range(int(r[0]), int(r[0]) + int(r[1])))
        assert covered == below and all(1 <= int(r[1]) <= MC.HEAVY_FAN for r in rec[level])
    return out, g


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_sort_at_the_tile_edges(n, with_inf):
    inf = None
    if with_inf:
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = inf[-1] = 1
    check_sort(MC.uniform(n, 40 + n), [0, n], inf=inf)


@pytest.mark.parametrize("n,c", [(512, 8), (4047, 12), (14436, 16)])
def test_sort_and_filing_at_the_threshold_populations(n, c):
    g = DRV.geo([0, n])
    widths = g.widths(0)
    assert set(widths) == {c} and g.heavy_min == 32
    sc, placed = MC.population(n, widths, g.heavy_min, 7 + n)
    out, _ = check_sort(sc, [0, n])
    level_of = {}
    for level in range(4):
        for first, count, dst, final in out["rec"][level].tolist():
            if final:
                level_of[dst] = level
    got = {cnt: level_of.get(v - 1) for v, cnt in placed.items()}          # window 0's set starts at bucket 0
    assert got == {cnt: (MC.filing(cnt)[1] if cnt > 32 else None) for cnt in placed.values()}
    if n == 14436:     # 1, 2, 31 and 32 points stay light; 33, 2047 and 2048 file one record; 2049, 4096 and 4097 reach level 1
        assert got == {1: None, 2: None, 31: None, 32: None, 33: 0, 2047: 0, 2048: 0, 2049: 1, 4096: 1, 4097: 1}


@pytest.mark.parametrize("offsets", MC.BATCHES, ids=["four", "sixty-four"])
def test_sort_of_a_batch_with_every_problems_own_boundary_scalars(offsets):
    g = DRV.geo(offsets)
    sc = []
    for j in range(g.n_problems):
        w = g.widths(j)
        pool = [MC.half(w), MC.half_plus_one(w), MC.ones_run(w)]
        sc += MC.cycled(pool, offsets[j + 1] - offsets[j], 50 + j)
    assert len({tuple(g.widths(j)) for j in range(g.n_problems)}) >= (3 if len(offsets) == 5 else 1)
    check_sort(sc, offsets)


@pytest.mark.parametrize("family", ["all_equal_1", "half"])
@pytest.mark.parametrize("n,stride", [(1 << 13, 1 << 13), (1 << 16, 1 << 16), (5000, 1 << 16)])
def test_sort_on_the_table_geometry(n, stride, family):
    g = DRV.geo([0, n], True, stride)
    widths = g.widths(0)
    s = MC.families(widths)[family][0]
    out, _ = check_sort([s] * n, [0, n], True, stride)
    if stride == 1 << 16:
        assert widths == [19] * 4 + [18] * 10
    if family == "all_equal_1":
        assert int(out["counts"][0]) == n * len(widths)                  # every digit of every scalar in bucket 0
        if n == 1 << 16:
            assert int(out["counts"][0]) == 917504 and out["ovf"] == [450, 448, 2, 1, 0]
    else:
        assert int(out["counts"][(1 << (widths[0] - 1)) - 1]) >= n       # the last bucket of the set


def test_sort_on_the_level_geometry_of_an_opening():
    offsets = levels_of(13)
    g = DRV.geo(offsets, True, 0)
    sc = []
    for j in range(g.n_problems):
        sc += MC.cycled(MC.family_scalars(g.widths(j)), offsets[j + 1] - offsets[j], 60 + j)
    check_sort(sc, offsets, True, 0)
