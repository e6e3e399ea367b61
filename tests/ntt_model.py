"""The radix-2 transform of csrc/ntt_kernels.hpp in python integers, stage by stage, and the contents of its twiddle tables.

Test infrastructure: imports neither oracle/ nor the package.  Values are canonical integers mod R.  The transform is serial_fft
(polynomial/src/utils.rs:281-315): a bit-reversal permutation, then log_n decimation-in-time stages; stage s pairs i0 and i0 + 2^s
inside blocks of 2^(s+1) with the twiddle w^(j << (log_n - s - 1)), j = i0 mod 2^s.  `stages` applies any run of consecutive stages to
an array that is already in bit-reversed order, which is what every kernel after the gather does: the first pass applies stages 0..7,
a later pass (s0, T) stages s0..s0+T-1.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import model as M  # noqa: E402

R = M.R
FIRST_STAGES = 8


def inv(v):
    return pow(v, -1, R)


def omega(log_n, inverse=False):
    w = M.root_of_unity(1 << log_n)
    return inv(w) if inverse else w


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def powers(w, count):
    out, p = [], 1
    for _ in range(count):
        out.append(p)
        p = p * w % R
    return out


def gather(x, log_n, in2=None):
    """the bit-reversed, zero-padded input of the stages: a[o] = x[rev(o)] (* in2[rev(o)]) where rev(o) < len(x), else 0"""
    n = 1 << log_n
    assert len(x) <= n and (in2 is None or len(in2) == len(x))
    out = [0] * n
    for o in range(n):
        src = bitrev(o, log_n)
        if src < len(x):
            out[o] = x[src] * in2[src] % R if in2 is not None else x[src] % R
    return out


def stages(a, log_n, w, s_from, s_to, last_scale=None):
    """stages s_from .. s_to - 1 of the size-2^log_n transform with root w, applied to a copy of `a` (bit-reversed order in, the same
    positions out).  last_scale: every output of stage s_to - 1 is multiplied by it (the inverse transform's 1/n)"""
    n = 1 << log_n
    assert len(a) == n and 0 <= s_from <= s_to <= log_n
    a = list(a)
    W = powers(w, max(n >> 1, 1))
    for s in range(s_from, s_to):
        m, shift = 1 << s, log_n - s - 1
        for k in range(0, n, 2 * m):
            for j in range(m):
                t = a[k + j + m] * W[j << shift] % R
                u = a[k + j]
                a[k + j + m] = (u - t) % R
                a[k + j] = (u + t) % R
    if last_scale is not None and s_to > s_from:
        a = [v * last_scale % R for v in a]
    return a


def transform(x, log_n, inverse=False):
    """Domain::fft / ifft of x zero-padded to 2^log_n"""
    n = 1 << log_n
    return stages(gather(x, log_n), log_n, omega(log_n, inverse), 0, log_n, inv(n) if inverse and log_n else None)


# ---- the tables, from their definitions ----------------------------------------------------------------------------------------
def twiddle_table(log_n, inverse=False):
    """W[i] = w^i, i < max(n / 2, 1)"""
    return powers(omega(log_n, inverse), max(1 << log_n >> 1, 1))


def first_table(log_n, inverse=False):
    """tw1[(1 << t) - 1 + j] = w^(j << (log_n - t - 1)), t < 8, j < 2^t: 255 entries"""
    w = omega(log_n, inverse)
    out = [None] * ((1 << FIRST_STAGES) - 1)
    for t in range(FIRST_STAGES):
        for j in range(1 << t):
            out[(1 << t) - 1 + j] = pow(w, j << (log_n - t - 1), R)
    return out


def pass_table(log_n, s0, T, inverse=False, scaled=False):
    """T[t][ml][lo] = w^(((ml << s0) | lo) << (log_n - s0 - t - 1)) at offset (2^t - 1) 2^s0 + (ml << s0) + lo; scaled: the entries of
    stage T - 1 times n^-1"""
    w = omega(log_n, inverse)
    ni = inv(1 << log_n)
    out = []
    for t in range(T):
        step = pow(w, 1 << (log_n - s0 - t - 1), R)
        row = powers(step, 1 << (s0 + t))             # index (ml << s0) | lo runs over 0 .. 2^(s0 + t) - 1
        if scaled and t == T - 1:
            row = [v * ni % R for v in row]
        out.extend(row)
    assert len(out) == ((1 << T) - 1) << s0
    return out


# ---- the closed form the large sizes are checked by ----------------------------------------------------------------------------
def geometric_mismatches(out, a, inverse=False):
    """indices i with scale * out[i] * (a w^i - 1) != a^n - 1 -- out is the transform of [a^j] exactly when there is none and
    a^n != 1 (then no a w^i is 1)"""
    n = len(out)
    log_n = n.bit_length() - 1
    w, scale = omega(log_n, inverse), (n if inverse else 1)
    rhs = (pow(a, n, R) - 1) % R
    bad, aw = [], a % R
    for i in range(n):
        if scale * out[i] * (aw - 1) % R != rhs:
            bad.append(i)
        aw = aw * w % R
    return bad
