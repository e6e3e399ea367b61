"""CPU: tests/ntt_model.py (the stage-by-stage reference of tests/test_gpu_ntt_kernels.py) against the golden model and the C oracle,
and the oracle's closed-form checker for the transform of a geometric sequence against both.  A reference that is wrong would let a
wrong kernel through, so each piece is pinned here first."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_model as NM  # noqa: E402

R = NM.R
M = NM.M


def rand(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("log_n", range(0, 14))
def test_stage_model_is_the_transform(ora, log_n):
    n = 1 << log_n
    x = rand(n, 100 + log_n)
    fwd, bwd = NM.transform(x, log_n), NM.transform(x, log_n, inverse=True)
    assert fwd == M.domain_fft(x, n) and bwd == M.domain_ifft(x, n)
    xm = ora.fr_from_ints(x)
    assert np.array_equal(ora.fr_from_ints(fwd), ora.domain_fft(xm, n))
    assert np.array_equal(ora.fr_from_ints(bwd), ora.domain_ifft(xm, n))


@pytest.mark.parametrize("log_n,n_src", [(3, 0), (3, 1), (5, 7), (9, 300), (12, 2049), (12, 4095)])
def test_stage_model_pads_short_input(ora, log_n, n_src):
    n = 1 << log_n
    x = rand(n_src, 7 * log_n + n_src)
    xm = ora.fr_from_ints(x) if n_src else np.empty((0, 4), dtype=np.uint64)
    assert np.array_equal(ora.fr_from_ints(NM.transform(x, log_n)), ora.domain_fft(xm, n))
    assert np.array_equal(ora.fr_from_ints(NM.transform(x, log_n, inverse=True)), ora.domain_ifft(xm, n))


@pytest.mark.parametrize("log_n,cuts", [(13, (8, 11)), (13, (8, 9, 12)), (12, (8,)), (11, (10,)), (6, (1, 2, 5)), (14, (8, 12, 13))])
def test_partial_stages_compose_to_the_whole(log_n, cuts):
    """8 + 3 + 2 and friends: running the stages in pieces, as the passes do, is running them all"""
    for inverse in (False, True):
        w = NM.omega(log_n, inverse)
        a = NM.gather(rand(1 << log_n, 31 * log_n + len(cuts)), log_n)
        whole = NM.stages(a, log_n, w, 0, log_n)
        part, at = a, 0
        for c in list(cuts) + [log_n]:
            part = NM.stages(part, log_n, w, at, c)
            at = c
        assert part == whole


def test_last_scale_is_the_inverse_transforms_factor():
    log_n, x = 9, rand(1 << 9, 5)
    w = NM.omega(log_n, True)
    a = NM.stages(NM.gather(x, log_n), log_n, w, 0, 8)
    assert NM.stages(a, log_n, w, 8, 9, NM.inv(1 << log_n)) == M.domain_ifft(x, 1 << log_n)


def test_gather_multiplies_before_it_pads():
    x, y = rand(5, 1), rand(5, 2)
    g = NM.gather(x, 3, y)
    assert [g[NM.bitrev(i, 3)] for i in range(8)] == [a * b % R for a, b in zip(x, y)] + [0, 0, 0]


@pytest.mark.parametrize("inverse", [False, True])
def test_tables_follow_their_definitions(inverse):
    log_n = 12
    w = NM.omega(log_n, inverse)
    assert pow(w, 1 << log_n, R) == 1 and pow(w, 1 << (log_n - 1), R) == R - 1
    assert (NM.omega(log_n) * NM.omega(log_n, True)) % R == 1
    W = NM.twiddle_table(log_n, inverse)
    assert len(W) == 1 << (log_n - 1) and all(W[i] == pow(w, i, R) for i in (0, 1, 2, 1000, 2047))
    tw1 = NM.first_table(log_n, inverse)
    assert len(tw1) == 255
    for t in range(8):
        for j in (0, (1 << t) - 1, (1 << t) // 2):
            assert tw1[(1 << t) - 1 + j] == pow(w, j << (log_n - t - 1), R)
    ni = NM.inv(1 << log_n)
    for s0, T in ((8, 4), (9, 2), (10, 1), (11, 1)):
        if s0 + T > log_n:
            continue
        plain, scaled = NM.pass_table(log_n, s0, T, inverse), NM.pass_table(log_n, s0, T, inverse, scaled=True)
        assert len(plain) == ((1 << T) - 1) << s0
        for t in range(T):
            for ml in {0, (1 << t) - 1}:
                for lo in (0, 1, (1 << s0) - 1):
                    e = pow(w, ((ml << s0) | lo) << (log_n - s0 - t - 1), R)
                    at = (((1 << t) - 1) << s0) + (ml << s0) + lo
                    assert plain[at] == e
                    assert scaled[at] == (e * ni % R if t == T - 1 else e)


def test_tables_are_the_twiddles_the_stages_use():
    """a pass (s0, T) computed with its table's entries instead of W gives the same state"""
    log_n, s0, T = 11, 8, 3
    w = NM.omega(log_n)
    a = NM.stages(NM.gather(rand(1 << log_n, 77), log_n), log_n, w, 0, s0)
    tab = NM.pass_table(log_n, s0, T)
    b = list(a)
    for t in range(T):
        m = 1 << (s0 + t)
        for k in range(0, 1 << log_n, 2 * m):
            for j in range(m):                         # j = (ml << s0) | lo
                tt = b[k + j + m] * tab[(((1 << t) - 1) << s0) + j] % R
                b[k + j + m], b[k + j] = (b[k + j] - tt) % R, (b[k + j] + tt) % R
    assert b == NM.stages(a, log_n, w, s0, s0 + T)


# ---- the closed form ----------------------------------------------------------------------------------------------------------
A = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3 % R


def test_powers_helper(ora):
    got = ora.fr_powers(ora.fr_from_ints([A])[0], 10000)         # more than two chunks, a ragged last one
    assert ora.fr_to_ints(got[:3]) == [1, A, A * A % R]
    for j in (4095, 4096, 4097, 8192, 9999):
        assert ora.fr_to_ints(got[j:j + 1]) == [pow(A, j, R)]


@pytest.mark.parametrize("log_n", [10, 14])
def test_geometric_checker(ora, log_n):
    n = 1 << log_n
    assert pow(A, n, R) != 1
    am = ora.fr_from_ints([A])[0]
    x = ora.fr_powers(am, n)
    fwd, bwd = ora.domain_fft(x, n), ora.domain_ifft(x, n)
    assert ora.ntt_geometric_mismatches(fwd, am, False) == (0, n)
    assert ora.ntt_geometric_mismatches(bwd, am, True) == (0, n)
    if log_n == 10:                                    # the python statement of the identity agrees
        assert NM.geometric_mismatches(ora.fr_to_ints(fwd), A) == [] and NM.geometric_mismatches(ora.fr_to_ints(bwd), A, True) == []
    assert len(set(map(bytes, fwd))) == n              # all outputs distinct: a permuted output cannot pass
    # one flipped limb: exactly that index
    for out, inverse, at in ((fwd, False, n - 3), (bwd, True, 4097 % n), (fwd, False, 0)):
        hurt = out.copy()
        hurt[at, 2] ^= np.uint64(1)
        assert ora.ntt_geometric_mismatches(hurt, am, inverse) == (1, at)
    # two outputs swapped: both
    sw = fwd.copy()
    sw[[5, 6]] = sw[[6, 5]]
    assert ora.ntt_geometric_mismatches(sw, am, False) == (2, 5)
    # the transform of another sequence, and a direction taken for the other: every index
    other = ora.fr_from_ints([A + 1])[0]
    assert ora.ntt_geometric_mismatches(ora.domain_fft(ora.fr_powers(other, n), n), am, False) == (n, 0)
    assert ora.ntt_geometric_mismatches(fwd, am, True)[0] == n
