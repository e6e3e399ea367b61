"""GPU: fold_rounds_kernel (csrc/fold_rounds.hpp) leaves the same bits at every grid.

Its fold workgroups take their tiles from a schedule that depends on the grid alone (csrc/fold_schedule.hpp): with F fold workgroups,
W = 8 F waves and T tiles, every wave folds q = T / W regular tiles in a loop that keeps the next tile's first loads in flight, and the
T % W leftover tiles are dealt to the workgroups and folded by all eight waves of one, their partial limb values added in LDS.  The
prover launches one fold workgroup per CU beside the serial workgroup's; here the kernel is launched at small grids through
tests/cpp/fold_rounds_grid_driver.hip and compared, == on the raw limbs, with blockfold_kernel + sumcheck_small_kernel +
multifold_mfma_kernel<4, 4> on the same inputs, as tests/test_gpu_fold_rounds.py does at the one-tile-per-wave grid: the folded table,
the round polynomials, the challenges, the weights, the transcript state and the partial tables; the per-tile sums' buffer untouched.
Shapes (k, m, k2; F) -- the fold takes a 2^k x m table to m outputs, the rounds run on 2^k2 entries, F fold workgroups:
  (6, 8192, 5; 1)    q = 16, no leftover: the loop and its prefetch alone
  (6, 8192, 5; 3)    q = 5, rem = 8: workgroups with 3, 3 and 2 leftovers
  (6, 8192, 5; 7)    q = 2, rem = 16: more leftovers than workgroups
  (4, 8192, 5; 5)    16 terms: two per wave of a leftover tile, fewer than a register set holds
  (5, 8192, 5; 5)    four per wave
  (8, 8192, 5; 3)    256 terms in two chunks: the strings rebuilt inside the loop, workgroups with different numbers of barriers
  (4, 8448, 5; 4)    132 tiles, q = 4, rem = 4
  (4, 8448, 10; 17)  the one-tile-per-wave grid, q = 0: waves without a tile, the serial kernel's largest LDS request
  (6, 16384, 6; 32)  the one-tile-per-wave grid exactly: q = 1, no leftover
The fills are those of tests/test_gpu_fold_rounds.py; `stored_max` and `top` drive the column sums, and with them the sum over the
eight waves, furthest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tables as T  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5A5A5A5A5A5A5A
# (k, m, k2, F) -> (q, rem) the schedule must give: the branches the shapes are chosen for
SHAPES = {(6, 8192, 5, 1): (16, 0), (6, 8192, 5, 3): (5, 8), (6, 8192, 5, 7): (2, 16), (4, 8192, 5, 5): (3, 8), (5, 8192, 5, 5): (3, 8),
          (8, 8192, 5, 3): (5, 8), (4, 8448, 5, 4): (4, 4), (4, 8448, 10, 17): (0, 132), (6, 16384, 6, 32): (1, 0)}
FILLS = ["random", "uniform_r", "top", "limb_edges", "stored_max", "zero"]


@pytest.fixture(scope="module")
def drv():
    import fold_rounds_grid_driver as D
    D.lib()
    return D


def _table(ora, fill, n, seed):
    return ora.random_fr(n, seed) if fill == "random" else T.fill(fill, n, seed)


def _run(drv, fused, wgs, dev, m, k, k2, ny, state, round0):
    """one form on fresh output buffers -> {name: numpy array}"""
    import torch
    full = lambda rows: torch.full((rows, 4), PATTERN, dtype=torch.int64, device="cuda")   # noqa: E731
    out = {"p1": full(ny << k2), "w2": full((1 << k2) + 1), "rp": full(2 * (round0 + k2) + 1), "ch": full(round0 + k2 + 1),
           "out": full(m + 1), "partials": full(m // 64 + 1), "st": torch.from_numpy(state.copy()).cuda()}
    rc = drv.lib().fold_rounds_grid_driver_run(fused, wgs, dev["table"].data_ptr(), m, k, k2, dev["w"].data_ptr(), dev["fine"].data_ptr(),
                                               out["p1"].data_ptr(), out["w2"].data_ptr(), out["st"].data_ptr(), out["rp"].data_ptr(),
                                               out["ch"].data_ptr(), round0, out["out"].data_ptr(), out["partials"].data_ptr(), 1,
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "launcher returned hipError %d" % rc
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


_inputs = {}   # (k, m, k2, fill) -> (device inputs, state, ny, what the separate launches left): made once, shared by the grids, never written


def _reference(drv, ora, k, m, k2, fill):
    import torch
    key = (k, m, k2, fill)
    if key not in _inputs:
        ny = drv.lib().fold_rounds_grid_driver_slices(k, k2)
        assert 1 <= ny <= 8
        dev = {"table": torch.from_numpy(_table(ora, fill, m << k, 300 + k).view(np.int64)).cuda(),
               "w": torch.from_numpy(T.fill("uniform_r", 1 << k, 310 + k).view(np.int64)).cuda(),          # (any residues serve as weights)
               "fine": torch.from_numpy(_table(ora, fill, 1 << (k + k2), 320 + k).view(np.int64)).cuda()}
        state = np.random.Generator(np.random.PCG64(330 + k)).integers(0, 256, size=drv.info(m)["state_bytes"], dtype=np.uint8)
        sep = _run(drv, 0, 0, dev, m, k, k2, ny, state, k)
        pat = np.int64(PATTERN)
        # the separate form did write everything that is compared, and nothing behind it
        assert (sep["partials"][:-1] != pat).any() and (sep["ch"][k:-1] != pat).any() and (sep["w2"][:-1] != pat).any()
        assert fill == "zero" or (sep["out"][:-1] != pat).any()
        assert (sep["st"] != state).any()
        for name in ("w2", "rp", "ch", "out", "partials"):
            assert (sep[name][-1] == pat).all(), "the element behind `%s` was written" % name
        _inputs[key] = (dev, state, ny, sep)
    return _inputs[key]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("k,m,k2,wgs", sorted(SHAPES))
def test_every_grid_equals_the_separate_launches(drv, ora, k, m, k2, wgs, fill):
    sched = drv.schedule(m // 64, wgs)
    assert (sched["q"], sched["rem"]) == SHAPES[(k, m, k2, wgs)] and sched["waves"] == 8 * wgs
    if wgs == drv.info(m)["one_each"]:                  # one tile per wave, nothing cooperative
        assert (sched["q"], sched["left0"]) in ((0, 0), (1, 0)) and (sched["q"] == 0 or sched["rem"] == 0)
    dev, state, ny, sep = _reference(drv, ora, k, m, k2, fill)
    fus = _run(drv, 1, wgs, dev, m, k, k2, ny, state, k)
    pat = np.int64(PATTERN)
    for name in ("w2", "rp", "ch", "out", "partials"):
        assert (fus[name][-1] == pat).all(), "the element behind `%s` was written" % name
    # bit for bit: the folded table, the round polynomials, the challenges, the weights, the transcript state (and the partial tables)
    for name in ("out", "rp", "ch", "w2", "st", "p1"):
        diff = np.flatnonzero((sep[name] != fus[name]).reshape(len(sep[name]), -1).any(axis=1))
        assert diff.size == 0, "`%s`: %d rows differ, the first at %d" % (name, diff.size, diff[0])
    assert (fus["partials"] == pat).all(), "the fused form touched the per-tile sums"


def test_grid_driver_refuses_what_the_kernels_do_not_take(drv):
    import torch
    buf = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    run = lambda wgs, m, k, k2, first=p: drv.lib().fold_rounds_grid_driver_run(1, wgs, first, m, k, k2, p, p, p, p, p, p, p, 0, p, p, 1, None)   # noqa: E731
    assert run(1, 8192, 4, 5, None) == drv.INVALID       # a null pointer
    assert run(0, 8192, 4, 5) == drv.INVALID             # no fold workgroup
    assert run(17, 8192, 4, 5) == drv.INVALID            # more than one tile per wave needs
    assert run(1, 4096, 4, 5) == drv.INVALID             # fewer outputs than the streaming form takes
    assert run(1, 8192, 3, 5) == drv.INVALID             # the vector form's term count
