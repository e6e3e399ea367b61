"""GPU: every kernel of csrc/ntt_kernels.hpp on its own, against python integers (tests/ntt_model.py).

tests/test_gpu_ntt.py compares whole transforms, which pins only the pass plans its sizes take and says nothing about where a wrong
result came from.  Here each kernel is launched through tests/cpp/ntt_driver.hip: the tables are compared by content, the first pass
and every later pass by the state they leave (not only the end result), a pass over its whole legal (s0, T) domain at the smallest n,
with hi > 0, in place and out of place, with every cut n_dst, and a three-pass plan -- which the library forms at 2^23 only -- at
2^14 and 2^15.  Tables and twiddles a kernel consumes come from the model, never from another kernel.  Every comparison is == on every
element as packed limbs; every output buffer is pre-filled with a pattern and carries one guard element that must keep it.
"""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_driver as DRV  # noqa: E402
import ntt_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu
R = NM.R
MONT = (1 << 256) % R
PATTERN = 0x5A5A5A5A5A5A5A5A


# ---- plumbing: python ints <-> device tensors of Montgomery limbs --------------------------------------------------------------
def pack(vals):
    """canonical ints -> uint64 [n, 4] Montgomery limbs, with integers only"""
    raw = b"".join((v % R * MONT % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def dev(vals):
    import torch
    return torch.from_numpy(pack(vals).view(np.int64)).cuda()


def dev_or_dummy(vals):
    """a launcher refuses a null pointer: an empty input is one allocated element that is never read"""
    return dev(vals) if len(vals) else dev([0])


def hp(a):
    return a.ctypes.data


def outbuf(n):
    """n elements and one guard, all pattern"""
    import torch
    return torch.full((n + 1, 4), PATTERN, dtype=torch.int64, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def launched(status):
    assert status == 0, "launcher returned hipError %d" % status


def check_packed(buf, exp, what):
    """buf == exp (packed limbs, one row per element) and then one guard row of pattern"""
    got = buf.cpu().numpy().view(np.uint64)
    assert got.shape[0] == exp.shape[0] + 1, what
    if not np.array_equal(got[:-1], exp):
        bad = np.nonzero((got[:-1] != exp).any(axis=1))[0]
        raise AssertionError("%s: %d of %d elements differ, the first at index %d" % (what, len(bad), exp.shape[0], bad[0]))
    assert (got[-1] == np.uint64(PATTERN)).all(), what + ": the element behind the output was written"


def check(buf, want, what):
    check_packed(buf, pack(want), what)


def rand(n, seed):
    """n random elements with 0, 1 and R - 1 among them"""
    rng = random.Random(seed)
    v = [rng.randrange(R) for _ in range(n)]
    for k, at in enumerate(rng.sample(range(n), min(n // 2, 6))):
        v[at] = (0, 1, R - 1)[k % 3]
    return v


@pytest.fixture(scope="module")
def L():
    return DRV.lib()


_tables = {}


def model_tw1(log_n, inverse):
    key = ("tw1", log_n, inverse)
    if key not in _tables:
        _tables[key] = dev(NM.first_table(log_n, inverse))
    return _tables[key]


def model_W(log_n, inverse):
    key = ("W", log_n, inverse)
    if key not in _tables:
        _tables[key] = dev(NM.twiddle_table(log_n, inverse))
    return _tables[key]


# ---- the tables by content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
def test_twiddle_table(L, inverse):
    log_n = 14
    w, pw = NM.omega(log_n, inverse), []
    for _ in range(log_n - 1):
        pw.append(w)
        w = w * w % R
    d_pw, out = dev(pw), outbuf(1 << (log_n - 1))
    launched(L.ntt_driver_twiddle(d_pw.data_ptr(), log_n - 1, out.data_ptr(), stream()))
    check(out, NM.twiddle_table(log_n, inverse), "W")


@pytest.mark.parametrize("inverse", [False, True])
def test_first_table(L, inverse):
    log_n = 14
    out = outbuf(255)
    launched(L.ntt_driver_first_table(model_W(log_n, inverse).data_ptr(), log_n, out.data_ptr(), stream()))
    check(out, NM.first_table(log_n, inverse), "tw1")


@pytest.mark.parametrize("log_n,s0,T", [(14, 8, 6), (14, 8, 3), (16, 12, 4)])
@pytest.mark.parametrize("inverse", [False, True])
def test_pass_table(L, log_n, s0, T, inverse):
    scale = pack([NM.inv(1 << log_n)])
    for scaled in (False, True):
        out = outbuf(((1 << T) - 1) << s0)
        launched(L.ntt_driver_pass_table(model_W(log_n, inverse).data_ptr(), log_n, s0, T, hp(scale), int(scaled), out.data_ptr(), stream()))
        check(out, NM.pass_table(log_n, s0, T, inverse, scaled), "pass table (%d,%d) scaled=%s" % (s0, T, scaled))


# ---- the first pass alone: gather (bit reversal, zero padding, optional factor) and stages 0..7 ------------------------------------
@pytest.mark.parametrize("log_n", [12, 14])
@pytest.mark.parametrize("with_in2", [False, True])
def test_first8(L, log_n, with_in2):
    n = 1 << log_n
    x, y = rand(n, 300 + log_n), rand(n, 301 + log_n)
    for inverse, n_src in [(False, k) for k in (0, 1, 7, n // 8 + 1, n // 2, n - 1, n)] + [(True, n // 8 + 1), (True, n)]:
        xs, ys = x[:n_src], (y[:n_src] if with_in2 else None)
        d_in = dev_or_dummy(xs)
        d_in2 = dev_or_dummy(ys) if with_in2 else None          # exactly n_src elements, as the coset hook passes them
        out = outbuf(n)
        launched(L.ntt_driver_first8(d_in.data_ptr(), n_src, d_in2.data_ptr() if with_in2 else None, out.data_ptr(), log_n,
                                     model_tw1(log_n, inverse).data_ptr(), stream()))
        want = NM.stages(NM.gather(xs, log_n, ys), log_n, NM.omega(log_n, inverse), 0, 8)
        check(out, want, "first8 log_n=%d n_src=%d in2=%s inverse=%s" % (log_n, n_src, with_in2, inverse))


# ---- one later pass alone, over its legal domain at the smallest n ----------------------------------------------------------------
@pytest.mark.parametrize("T", range(1, 8))
@pytest.mark.parametrize("above", [0, 1, 2])                   # stages left above the pass: 1 and 2 give hi > 0
def test_pass(L, T, above):
    import torch
    s0 = max(8, 11 - T)
    log_n = s0 + T + above
    n = 1 << log_n
    a = rand(n, 500 + 10 * T + log_n)
    src_packed = pack(a)
    d_src = torch.from_numpy(src_packed.view(np.int64)).cuda()
    ninv = NM.inv(n)
    scale = pack([ninv])
    for last_scaled in (False, True):
        inverse = last_scaled
        tab = dev(NM.pass_table(log_n, s0, T, inverse, scaled=last_scaled))
        want = pack(NM.stages(a, log_n, NM.omega(log_n, inverse), s0, s0 + T, ninv if last_scaled else None))
        for n_dst in sorted({1, 1 << (11 - T), (1 << (11 - T)) + 1, n // 2 + 1, n - 1, n}):
            for in_place in (False, True):
                if in_place:                                   # beyond n_dst the buffer keeps what it held: the input
                    buf = outbuf(n)
                    buf[:n] = d_src
                    src_ptr, exp = buf.data_ptr(), np.concatenate([want[:n_dst], src_packed[n_dst:]])
                else:                                          # beyond n_dst the destination keeps the pattern
                    buf = outbuf(n)
                    src_ptr = d_src.data_ptr()
                    exp = np.concatenate([want[:n_dst], np.full((n - n_dst, 4), PATTERN, dtype=np.uint64)])
                launched(L.ntt_driver_pass(src_ptr, buf.data_ptr(), log_n, s0, T, tab.data_ptr(), hp(scale), int(last_scaled), n_dst, stream()))
                check_packed(buf, exp, "pass (%d,%d) log_n=%d scaled=%s n_dst=%d in_place=%s" % (s0, T, log_n, last_scaled, n_dst, in_place))
        if not last_scaled:                                    # the source of an out-of-place pass is read only
            assert np.array_equal(d_src.cpu().numpy().view(np.uint64), src_packed)


# ---- a plan of three passes, the form the library takes from 2^23 on --------------------------------------------------------------
@pytest.mark.parametrize("log_n,plan", [(14, [(8, 4), (12, 1), (13, 1)]), (15, [(8, 3), (11, 2), (13, 2)])])
@pytest.mark.parametrize("inverse", [False, True])
def test_three_pass_chain(L, log_n, plan, inverse):
    n = 1 << log_n
    x = rand(n, 700 + log_n)
    w, ninv = NM.omega(log_n, inverse), NM.inv(n)
    scale = pack([ninv])
    d_x, scratch, dst = dev(x), outbuf(n), outbuf(n)
    launched(L.ntt_driver_first8(d_x.data_ptr(), n, None, scratch.data_ptr(), log_n, model_tw1(log_n, inverse).data_ptr(), stream()))
    state = NM.stages(NM.gather(x, log_n), log_n, w, 0, 8)
    check(scratch, state, "after the first eight stages")
    for p, (s0, T) in enumerate(plan):
        last = p + 1 == len(plan)
        scaled = last and inverse
        tab = dev(NM.pass_table(log_n, s0, T, inverse, scaled))
        out = dst if last else scratch                         # the middle passes run in place
        launched(L.ntt_driver_pass(scratch.data_ptr(), out.data_ptr(), log_n, s0, T, tab.data_ptr(), hp(scale), int(scaled), n, stream()))
        state = NM.stages(state, log_n, w, s0, s0 + T, ninv if scaled else None)
        check(out, state, "after pass (%d,%d)" % (s0, T))
    assert plan[-1][0] + plan[-1][1] == log_n and state == NM.transform(x, log_n, inverse)


# ---- the path below 2^12 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 3, 10, 11])
@pytest.mark.parametrize("inverse", [False, True])
def test_small_path(L, log_n, inverse):
    n = 1 << log_n
    x = rand(n, 900 + log_n)
    w = NM.omega(log_n, inverse)
    d_in, out = dev(x), outbuf(n)
    launched(L.ntt_driver_first_stages(d_in.data_ptr(), out.data_ptr(), log_n, model_W(log_n, inverse).data_ptr(), stream()))
    state = NM.stages(NM.gather(x, log_n), log_n, w, 0, min(log_n, 10))
    check(out, state, "first_stages")
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64), pack(x))
    if log_n == 11:                                            # the only form ntt_inplace launches: stage 10 alone
        launched(L.ntt_driver_mid_stages(out.data_ptr(), log_n, 10, 1, model_W(log_n, inverse).data_ptr(), stream()))
        state = NM.stages(state, log_n, w, 10, 11)
        check(out, state, "mid_stages (10,1)")
    unscaled = NM.transform(x, log_n, inverse)
    assert state == ([v * n % R for v in unscaled] if inverse else unscaled)
