"""No GPU: the inputs of tests/msm_cases.py are what they claim to be.  For every window-width list the MSM geometry produces over the
sizes of tests/test_gpu_msm_kernels.py and tests/test_gpu_msm_edges.py every scalar family is canonical, recodes without a final carry,
reconstructs, and hits the digit boundary it is named after; the population builder and the filing helper give the stated counts and
tree levels; every geometry kind keeps its invariants; tests/cpp/msm_driver.hip compiles for gfx950, loads, and refuses null and
out-of-range arguments before it touches a device (on a machine without one a launch would come back with another error)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402
import msm_driver as DRV  # noqa: E402


def all_geometries():
    """every geometry tests/test_gpu_msm_kernels.py and tests/test_gpu_msm_edges.py run: the lists of tests/msm_cases.py"""
    out = [("plain-%d" % n, DRV.geo([0, n])) for n in MC.PLAIN_SIZES]
    out += [("batch-%d" % (len(b) - 1), DRV.geo(b)) for b in MC.BATCHES]
    out += [("table-%dof%d" % (n, s), DRV.geo([0, n], True, s)) for n, s in MC.TABLES]
    out += [("levels-%d" % nv, DRV.geo(MC.levels_of(nv), True, 0)) for nv in MC.LEVEL_VARS]
    out += [("levels-plain-%d" % nv, DRV.geo(MC.levels_of(nv))) for nv in MC.LEVEL_VARS]
    return out


@pytest.fixture(scope="module")
def geos():
    return all_geometries()


@pytest.fixture(scope="module")
def width_lists(geos):
    lists = {tuple(MC.uniform_widths(c)) for c in range(8, 21)}
    for _, g in geos:
        for j in range(g.n_problems):
            lists.add(tuple(g.widths(j)))
    return sorted(lists)


def test_every_width_from_8_to_20_occurs(width_lists):
    assert {c for w in width_lists for c in w} >= set(range(8, 21))
    assert any(len(set(w)) == 2 and w[0] == w[-1] + 1 for w in width_lists)        # the mixed hi / hi - 1 lists


def test_families_are_canonical_and_recode_as_claimed(width_lists):
    for widths in width_lists:
        widths = list(widths)
        nw, fam = len(widths), MC.families(widths)
        for name, scalars in fam.items():
            for s in scalars:
                d, carries, final = MC.recode(s, widths)
                assert 0 <= s < MC.R and final == 0, (widths, name)
                assert MC.reconstruct(d, widths) == s, (widths, name)
                assert all(-((1 << (c - 1)) - 1) <= x <= (1 << (c - 1)) for x, c in zip(d, widths))
        below = widths[:-1]
        d, carries, _ = MC.recode(fam["half"][0], widths)
        assert d[:-1] == [1 << (c - 1) for c in below] and not any(carries)                    # nw - 1 boundary digits, no carry
        d, carries, _ = MC.recode(fam["half_plus_one"][0], widths)
        assert d[:-1] == [-((1 << (c - 1)) - 1) for c in below] and carries[:-1] == [1] * (nw - 1) and d[-1] > 0
        d, carries, _ = MC.recode(fam["ones_run"][0], widths)
        assert d == [-1] + [0] * (nw - 2) + [1] and carries == [1] * (nw - 1) + [0]
        for name, v in (("all_equal_1", 1), ("all_equal_2", min(2, 1 << (min(widths) - 1))), ("all_equal_half", 1 << (min(widths) - 1))):
            d, carries, _ = MC.recode(fam[name][0], widths)
            assert d[:-1] == [v] * (nw - 1) and 0 <= d[-1] <= v and not any(carries)
        assert sum(1 for x in MC.recode(MC.R - 1, widths)[0] if x < 0) >= 1
        # the carry into the top window at its largest value
        T = (MC.R - 1) >> MC.bit_offsets(widths)[-1]
        th = fam["top_heavy"]
        assert th[:3] == [MC.R - 2, MC.R - 3, MC.R - 4]
        assert MC.recode(th[3], widths)[0][-1] == T
        if len(th) > 4:
            assert th[4] == th[3] + 1 and MC.recode(th[4], widths)[0][-1] == T + 1


def test_the_vector_recoder_is_the_rule(width_lists):
    for widths in width_lists:
        sc = MC.family_scalars(list(widths)) + MC.uniform(32, len(widths))
        want = [MC.recode(s, widths)[0] for s in sc]
        assert all(MC.recode(s, widths)[2] == 0 for s in sc)
        assert MC.digits_np(sc, list(widths)).tolist() == want


def test_filing_levels_at_the_thresholds():
    want = {1: 0, 2047: 0, 2048: 0, 2049: 1, 4096: 1, 4097: 1, 524288: 1, 524289: 2, 917504: 2, 1 << 20: 2}
    assert {c: MC.filing(c)[1] for c in want} == want
    assert MC.filing(2048) == ([1, 0, 0, 0], 0, 0)
    assert MC.filing(2049) == ([2, 1, 0, 0], 1, 2)
    assert MC.filing(524288) == ([256, 1, 0, 0], 1, 256)
    assert MC.filing(524289) == ([257, 2, 1, 0], 2, 259)
    assert MC.filing(917504) == ([448, 2, 1, 0], 2, 450)           # 448 records, then 2, then 1
    assert MC.filing(1 << 20) == ([512, 2, 1, 0], 2, 514)
    assert MC.filing((1 << 27) + 1)[1] == 3                         # level 3: out of any test's reach


@pytest.mark.parametrize("n,shared", [(512, False), (4047, False), (14436, False), (1 << 13, True)])
def test_populations_hold_the_stated_counts(n, shared):
    g = DRV.geo([0, n], shared, n if shared else 0)
    widths = g.widths(0)
    sc, placed = MC.population(n, widths, g.heavy_min, 7 + n, avoid_all_windows=shared)
    assert len(sc) == n and all(0 <= s < MC.R for s in sc)
    dig = MC.digits_np(sc, widths)
    cols = dig if shared else dig[:, :1]
    for v, c in placed.items():
        assert int((np.abs(cols) == v).sum()) == c and sc.count(v) == c
    assert g.heavy_min == 32
    h = 1 << (widths[0] - 1)
    assert placed[h] == 1 and placed[h - 1] == 2                                    # the last two buckets are populated
    assert set(placed.values()) >= {1, 2, 31, 32, 33}
    if n == 14436:
        assert sorted(placed.values()) == [1, 2, 31, 32, 33, 2047, 2048, 2049, 4096, 4097] and sum(placed.values()) == n
    if n == 4047:
        assert 2047 in placed.values()
    if shared:
        assert {2047, 2048, 2049} <= set(placed.values())
    counts, keys = MC.expected_sort(sc, g)
    for v, c in placed.items():
        assert counts[g.sets[0][1] + v - 1] == c
    slots, n_rec, final = MC.expected_overflow(counts, g.heavy_min)
    # (other buckets may be heavy too: the 12-bit geometry's top window holds three significant bits, eight buckets for every point)
    base = g.sets[0][1]
    assert {v: final.get(base + v - 1) for v in placed} == {v: (MC.filing(c)[1] if c > 32 else None) for v, c in placed.items()}


def test_geometry_invariants_for_every_kind(geos):
    L = DRV.lib()
    for name, g in geos:
        assert g.n_wins == len(g.wins) and g.n_sets == len(g.sets) and g.n_parts <= 4096, name
        n_rc = n_buckets = n_parts = 0
        for c, bucket_base, part_base, part_bits in g.sets:
            rc, sh, fits = DRV.set_shape(c)
            assert rc == 0 and fits and max(sh["R"], sh["C"]) <= 256, name
            assert bucket_base % 8 == 0 and bucket_base == n_buckets and part_base == n_parts, name
            assert part_bits == max(c - 1 - 8, 0)
            n_rc += 2 * sh["R"] + sh["C"]
            n_buckets += 1 << (c - 1)
            n_parts += 1 << part_bits
        assert (n_rc, n_buckets, n_parts) == (g.n_rc, g.n_buckets, g.n_parts), name
        items = 0
        for j in range(g.n_problems):
            widths = g.widths(j)
            nj = g.offsets[j + 1] - g.offsets[j]
            items += nj * len(widths)
            assert sum(widths) >= 256 and all(8 <= c <= 20 for c in widths), (name, j)
            if len(set(widths)) > 1:
                assert sum(widths) == 256 and set(widths) == {widths[0], widths[0] - 1} and widths == sorted(widths, reverse=True), (name, j)
            for w, (c, set_idx, entry_off) in enumerate(g.wins[g.win_first[j]: g.win_first[j + 1]]):
                assert c <= g.sets[set_idx][0] <= c + 1                 # a window's digits fit its set
                if not g.shared:
                    assert entry_off == 0 and set_idx == g.win_first[j] + w
        assert items == g.items, name
        if g.shared:
            assert g.n_sets == g.n_problems
    assert L.msm_driver_heavy_rec() == MC.HEAVY_REC and L.msm_driver_sort_tile() == 2048
    # every set width the GPU files can reach: 8 ... 20 without 17 (sixteen windows are 16 bits each, fifteen are 18 / 17, so a 17-bit
    # window only ever sits on an 18-bit set)
    assert {s[0] for _, g in geos for s in g.sets} == set(range(8, 21)) - {17}
    assert any(w[0] == 17 and g.sets[w[1]][0] == 18 for _, g in geos for w in g.wins)


def test_table_entry_offsets(geos):
    by = dict(geos)
    g = by["table-5000of65536"]
    assert [w[2] for w in g.wins] == [k << 16 for k in range(g.n_wins)] and g.widths(0) == [19] * 4 + [18] * 10
    g = by["levels-13"]
    entry = 0
    for j in range(g.n_problems):
        nj = g.offsets[j + 1] - g.offsets[j]
        for w, (_, _, entry_off) in enumerate(g.wins[g.win_first[j]: g.win_first[j + 1]]):
            assert (entry_off + g.offsets[j]) & 0xFFFFFFFF == entry + w * nj          # the tables lie end to end; + the index in the batch
        entry += nj * len(g.widths(j))


def test_sets_a_wave_cannot_sum_are_refused():
    """a set of 2^20 buckets or more has lines of more than 256 values: the widths stop at 20 bits, and a list whose table entries leave
    31 bits is refused as a whole"""
    for c in range(8, 21):
        assert DRV.set_shape(c)[2]
    for c in (21, 22, 24):
        rc, sh, fits = DRV.set_shape(c)
        assert rc == 0 and max(sh["R"], sh["C"]) > 256 and not fits
    rc, status, g = DRV.geometry([0, 1 << 27, 2 << 27, 3 << 27], True, 0)
    assert rc == 0 and status != 0 and g is None


def test_driver_builds_for_gfx950_and_loads():
    L = DRV.lib()
    assert os.path.exists(DRV.LIB_PATH)
    mk = open(os.path.join(DRV.CPP, "Makefile")).read()
    assert "libmsm_driver.so: msm_driver.hip" in mk and "gfx950" in mk
    assert L.msm_driver_max_wins() == 2048


def test_driver_refuses_before_touching_a_device():
    L = DRV.lib()
    fake = 4096                                          # never dereferenced: the refusal comes first
    offs = np.array([0, 300], dtype=np.uint32)
    o = offs.ctypes.data
    buf = np.zeros(8192 * 4, dtype=np.uint32).ctypes.data
    inv = DRV.INVALID
    # geometry
    assert L.msm_driver_geometry(None, 1, 0, 0, buf, buf, buf, buf) == inv
    for k in range(4):
        args = [buf] * 4
        args[k] = None
        assert L.msm_driver_geometry(o, 1, 0, 0, *args) == inv
    assert L.msm_driver_geometry(o, 0, 0, 0, buf, buf, buf, buf) == inv
    assert L.msm_driver_geometry(o, 65, 0, 0, buf, buf, buf, buf) == inv
    assert L.msm_driver_geometry(o, 1, 0, 300, buf, buf, buf, buf) == inv                 # a stride without a table
    assert L.msm_driver_geometry(o, 1, 1, 299, buf, buf, buf, buf) == inv                 # a table shorter than the scalars
    assert L.msm_driver_geometry(o, 1, 1, 1 << 27, buf, buf, buf, buf) == inv             # entry index + sign bit
    for bad in ([1, 300], [0, 0], [0, 300, 200], [0, 1 << 31]):
        b = np.array(bad, dtype=np.uint32)
        assert L.msm_driver_geometry(b.ctypes.data, len(bad) - 1, 0, 0, buf, buf, buf, buf) == inv
    assert DRV.set_shape(3)[0] == inv and DRV.set_shape(32)[0] == inv
    # digits
    w = np.array([16] * 16, dtype=np.uint32)
    assert L.msm_driver_digits(None, 4, w.ctypes.data, 16, fake, None) == inv
    assert L.msm_driver_digits(fake, 4, None, 16, fake, None) == inv
    assert L.msm_driver_digits(fake, 4, w.ctypes.data, 16, None, None) == inv
    assert L.msm_driver_digits(fake, 0, w.ctypes.data, 16, fake, None) == inv
    assert L.msm_driver_digits(fake, 4, w.ctypes.data, 0, fake, None) == inv
    for bad in ([0] + [16] * 15, [32] + [16] * 14, [16] * 17, [1] * 265):
        b = np.array(bad, dtype=np.uint32)
        assert L.msm_driver_digits(fake, 4, b.ctypes.data, len(bad), fake, None) == inv
    # sort
    rc, lay = DRV.sort_layout([0, 300])
    assert rc == 0 and lay["n_buckets"] == 32 * 128 and lay["n_items"] == 32 * 300 and lay["heavy_min"] == 32
    assert lay["rec_cap"] == 9600 // 32 + 9600 // 2048 + 2 and lay["slots_cap"] == 3 * (9600 // 2048) + 8
    assert L.msm_driver_sort_layout(o, 1, 0, 0, None) == inv and L.msm_driver_sort_layout(None, 1, 0, 0, buf) == inv
    ok = (fake, None, 300, o, 1, 0, 0, fake, lay["total"], None)
    for k, v in ((0, None), (2, 299), (2, 301), (3, None), (4, 0), (4, 65), (4, 2), (6, 300), (7, None), (7, fake + 8), (8, lay["total"] - 1)):
        args = list(ok)
        args[k] = v
        if k == 4 and v:        # an offsets array as long as the claimed number of problems: the refusal reads it
            many = np.array([0, 200] + [301] * (v - 1), dtype=np.uint32)       # 65 problems; two whose sizes disagree with n
            args[3] = many.ctypes.data
        assert L.msm_driver_sort(*args) == inv, (k, v)
