"""GPU: blockfold_kernel (csrc/multifold_kernels.hpp) on its own, at every (m, k) the library folds with, against python integers.

The kernel is launched through tests/cpp/blockfold_driver.hip with the grid blockfold_shape gives it.  Its contract: partial[y*m + c],
y < ny, are canonical integers below r whose sum over y mod r is sum_b w_b * T[b*m + c].  The table is in Montgomery form and the
weights carry the factor 2^32 on top, as sumcheck_small_kernel writes them.  Every comparison is == on python integers; the output
buffer is pre-filled with a pattern and carries one guard element that must keep it.
Fills: random; all zero; every limb pattern r - 1 in the table AND in the weights (the largest sum four products per lane reach);
one non-zero entry per term, each in another column with another weight (a slice that reads another term range than its own moves a
product to a wrong weight or drops it).  The largest case is 2^18 entries."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blockfold_driver as DRV  # noqa: E402

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
W_FACTOR = (1 << 32) % R
PATTERN = 0x5A5A5A5A5A5A5A5A
MAX_ENTRIES = 1 << 18
MAX_TERMS = 1 << 10
FILLS = ["random", "zero", "max", "one_per_term"]


def pack(vals, factor=1):
    """canonical ints -> uint64 [n, 4] limbs of v * factor in Montgomery form"""
    f = factor * MONT % R
    raw = b"".join((v * f % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def unpack(a):
    return [int.from_bytes(row.tobytes(), "little") for row in a]


@pytest.fixture(scope="module")
def L():
    return DRV.lib()


@pytest.fixture(scope="module")
def pool():
    """one random table and one set of weights for every shape (a shape takes a prefix), packed once"""
    rng = random.Random(20240611)
    t = [rng.randrange(R) for _ in range(MAX_ENTRIES)]
    w = [rng.randrange(R) for _ in range(MAX_TERMS)]
    for k, at in enumerate(rng.sample(range(MAX_ENTRIES), 12)):
        t[at] = (0, 1, R - 1)[k % 3]
    w[5], w[6], w[7] = 0, 1, R - 1
    return {"t": t, "w": w, "t_packed": pack(t), "w_packed": pack(w, W_FACTOR)}


def case(fill, m, k, pool):
    """(table ints, weight ints, packed table, packed weights)"""
    terms = 1 << k
    n = terms * m
    if fill == "random":
        return pool["t"][:n], pool["w"][:terms], pool["t_packed"][:n], pool["w_packed"][:terms]
    if fill == "zero":
        return [0] * n, pool["w"][:terms], np.zeros((n, 4), dtype=np.uint64), pool["w_packed"][:terms]
    if fill == "max":
        # the values whose stored limbs are r - 1: (r - 1) / 2^256 in the table, (r - 1) / (2^256 2^32) among the weights
        tv, wv = (R - 1) * MONT_INV % R, (R - 1) * MONT_INV * pow(W_FACTOR, -1, R) % R
        tp, wp = np.tile(pack([tv]), (n, 1)), np.tile(pack([wv], W_FACTOR), (terms, 1))
        assert unpack(tp[:1]) == [R - 1] and unpack(wp[:1]) == [R - 1]
        return [tv] * n, [wv] * terms, tp, wp
    assert fill == "one_per_term"
    t = [0] * n
    tp = np.zeros((n, 4), dtype=np.uint64)
    cols = [(37 * b + 11) % m for b in range(terms)]
    vals = [b + 2 for b in range(terms)]
    rows = pack(vals)
    for b in range(terms):
        t[b * m + cols[b]] = vals[b]
        tp[b * m + cols[b]] = rows[b]
    return t, pool["w"][:terms], tp, pool["w_packed"][:terms]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("m,k", DRV.SHAPES)
def test_partials_add_up_to_the_fold(L, pool, m, k, fill):
    import torch
    rc, sh = DRV.shape(m, k)
    assert rc == 0 and 1 <= sh["ny"] <= 8
    ny, terms = sh["ny"], 1 << k
    t, w, tp, wp = case(fill, m, k, pool)
    want = [sum(w[b] * t[b * m + c] for b in range(terms)) % R for c in range(m)]
    d_t = torch.from_numpy(tp.view(np.int64)).cuda()
    d_w = torch.from_numpy(wp.view(np.int64)).cuda()
    out = torch.full((ny * m + 1, 4), PATTERN, dtype=torch.int64, device="cuda")
    status = L.blockfold_driver_run(d_t.data_ptr(), m, k, d_w.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert status == 0, "launcher returned hipError %d" % status
    got = out.cpu().numpy().view(np.uint64)
    assert (got[-1] == np.uint64(PATTERN)).all(), "the element behind the partial tables was written"
    part = unpack(got[:-1])
    assert all(p < R for p in part), "a partial entry is not a canonical integer below r"
    have = [sum(part[y * m + c] for y in range(ny)) % R for c in range(m)]
    bad = [c for c in range(m) if have[c] != want[c]]
    assert not bad, "%d of %d outputs differ, the first at column %d" % (len(bad), m, bad[0])
    if fill == "one_per_term":
        assert sum(1 for v in want if v) > min(m, terms) // 2        # the case does spread its entries
