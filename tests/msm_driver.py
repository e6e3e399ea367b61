"""Builds and loads tests/cpp/libmsm_driver.so: the geometry, the digit recoding and the sort / filing / order passes of
csrc/msm_kernels.hpp, for tests/test_gpu_msm_kernels.py, tests/test_gpu_msm_edges.py and tests/test_msm_cases_cpu.py.
Test infrastructure only: nothing of libzkhip is linked into it."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LIB_PATH = os.path.join(CPP, "libmsm_driver.so")
INVALID = 1   # hipErrorInvalidValue
LAYOUT = ["total", "counts", "offsets", "order", "bins", "ovf", "sorted", "items", "wg_counts", "part_count", "part_off", "rec", "tab_wins",
          "tab_sets", "tab_part", "n_buckets", "n_items", "n_wgs", "n_parts", "rec_cap", "slots_cap", "heavy_min"]

_lib = None


def build():
    """`make` is a no-op when the library is newer than the driver and the csrc headers"""
    subprocess.check_call(["make", "-C", CPP, "-s", "libmsm_driver.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  -- first, as _native.lib() does: the driver must bind to the HIP runtime torch loaded
        _lib = C.CDLL(LIB_PATH)
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        _lib.msm_driver_set_shape.argtypes = [u, vp, vp]
        _lib.msm_driver_geometry.argtypes = [vp, u, i, sz, vp, vp, vp, vp]
        _lib.msm_driver_digits.argtypes = [vp, sz, vp, u, vp, vp]
        _lib.msm_driver_sort_layout.argtypes = [vp, u, i, sz, vp]
        _lib.msm_driver_sort.argtypes = [vp, vp, sz, vp, u, i, sz, vp, sz, vp]
        assert _lib.msm_driver_layout_words() == len(LAYOUT)
    return _lib


def _offs(offsets):
    return np.ascontiguousarray(offsets, dtype=np.uint32)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Geometry:
    """What msm_build_geometry decided for a list of problems.  wins: (width, set, entry_off) per digit window; sets: (c, bucket_base,
    part_base, part_bits) per bucket set; win_first[j]: problem j's first window."""

    def __init__(self, offsets, shared, stride, wins, sets, win_first, totals):
        self.offsets, self.shared, self.stride = [int(o) for o in offsets], bool(shared), int(stride)
        self.wins, self.sets, self.win_first = wins, sets, win_first
        (self.n_wins, self.n_sets, self.n_buckets, self.n_parts, self.n_terms, self.n_rc, self.n_rcwg, self.n_termwg, lo, hi,
         self.heavy_min) = [int(v) for v in totals[:11]]
        self.items = lo | (hi << 32)

    @property
    def n_problems(self):
        return len(self.offsets) - 1

    def widths(self, j=0):
        """the window widths of problem j, low window first"""
        return [w[0] for w in self.wins[self.win_first[j]: self.win_first[j + 1]]]


def geometry(offsets, shared=False, stride=0):
    """(hip status, geometry status, Geometry or None).  Plain: shared=False; the shifted-SRS table: shared=True, one problem, stride = the
    SRS size; level tables: shared=True, several problems, stride 0."""
    offs = _offs(offsets)
    cap = lib().msm_driver_max_wins()
    wins, sets = np.zeros((cap, 3), dtype=np.uint32), np.zeros((cap, 4), dtype=np.uint32)
    first, totals = np.zeros(len(offs), dtype=np.uint32), np.zeros(12, dtype=np.uint32)
    rc = lib().msm_driver_geometry(_vp(offs), len(offs) - 1, 1 if shared else 0, stride, _vp(wins), _vp(sets), _vp(first), _vp(totals))
    if rc != 0:
        return rc, None, None
    if totals[11] != 0:
        return rc, int(totals[11]), None
    nw, ns = int(totals[0]), int(totals[1])
    g = Geometry(offs, shared, stride, [tuple(int(v) for v in w) for w in wins[:nw]], [tuple(int(v) for v in s) for s in sets[:ns]],
                 [int(v) for v in first], totals)
    return 0, 0, g


def geo(offsets, shared=False, stride=0):
    rc, st, g = geometry(offsets, shared, stride)
    assert rc == 0 and st == 0, (rc, st)
    return g


def set_shape(c):
    sh, fits = (C.c_uint * 9)(), C.c_uint(0)
    rc = lib().msm_driver_set_shape(c, sh, C.byref(fits))
    return rc, dict(zip(("n_bits", "lo_bits", "C", "R", "row_lines", "col_lines", "row_wgs", "col_wgs", "term_wgs"), sh)), bool(fits.value)


def sort_layout(offsets, shared=False, stride=0):
    offs = _offs(offsets)
    out = np.zeros(len(LAYOUT), dtype=np.uint64)
    rc = lib().msm_driver_sort_layout(_vp(offs), len(offs) - 1, 1 if shared else 0, stride, _vp(out))
    return rc, dict(zip(LAYOUT, (int(v) for v in out)))


def digits(scalars, widths):
    """scalars: uint64 [n, 4] Montgomery limbs (host) -> int32 [n, len(widths)] (host)"""
    import torch
    sc = torch.from_numpy(np.ascontiguousarray(scalars, dtype=np.uint64).view(np.int64)).cuda()
    w = np.ascontiguousarray(widths, dtype=np.uint32)
    out = torch.empty((sc.shape[0], len(w)), dtype=torch.int32, device="cuda")
    rc = lib().msm_driver_digits(sc.data_ptr(), sc.shape[0], _vp(w), len(w), out.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def sort(scalars, offsets, shared=False, stride=0, inf=None, counters_only=False):
    """counters_only: just {"counts", "ovf", "L"} (a 2^20-point pass leaves 64 MiB of sorted entries behind).
    scalars: a CUDA int64 [n, 4] tensor or host limbs; inf: None or n uint8 flags -> dict of host arrays: counts, offsets, order (per
    bucket), sorted (per item), ovf = (n_slots, n_rec[0..3]), rec[level] = uint32 [n_rec[level], 4] (first, count, dst, final), and the
    layout's sizes"""
    import torch
    if not isinstance(scalars, torch.Tensor):
        scalars = torch.from_numpy(np.ascontiguousarray(scalars, dtype=np.uint64).view(np.int64)).cuda()
    scalars = scalars.contiguous()
    d_inf = None if inf is None else torch.from_numpy(np.ascontiguousarray(inf, dtype=np.uint8)).cuda()
    offs = _offs(offsets)
    rc, L = sort_layout(offsets, shared, stride)
    assert rc == 0, rc
    ws = torch.zeros(L["total"], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib().msm_driver_sort(scalars.data_ptr(), None if d_inf is None else d_inf.data_ptr(), scalars.shape[0], _vp(offs), len(offs) - 1,
                               1 if shared else 0, stride, ws.data_ptr(), L["total"], None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    if counters_only:
        return {"counts": ws[L["counts"]: L["counts"] + 4 * L["n_buckets"]].cpu().numpy().view(np.uint32),
                "ovf": [int(v) for v in ws[L["ovf"]: L["ovf"] + 20].cpu().numpy().view(np.uint32)], "L": L}
    # the results lie in front of the item and count buffers: one copy of the head of the workspace
    head = ws[: L["items"]].cpu().numpy()
    u32 = lambda off, n: head[off: off + 4 * n].view(np.uint32)     # noqa: E731
    nb = L["n_buckets"]
    ovf = u32(L["ovf"], 5)
    out = {"counts": u32(L["counts"], nb), "offsets": u32(L["offsets"], nb), "order": u32(L["order"], nb), "sorted": u32(L["sorted"], L["n_items"]),
           "ovf": [int(v) for v in ovf], "L": L}
    recs = []
    for level in range(4):
        n_rec = int(ovf[1 + level])
        assert n_rec <= L["rec_cap"], (level, n_rec, L["rec_cap"])
        off = L["rec"] + 16 * level * L["rec_cap"]
        recs.append(ws[off: off + 16 * n_rec].cpu().numpy().view(np.uint32).reshape(n_rec, 4))
    out["rec"] = recs
    return out
