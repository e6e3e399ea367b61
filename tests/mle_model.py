"""Integer model of the kernels of csrc/mle_kernels.hpp and of eq_weights / eval_weights / sum_records (csrc/multifold_kernels.hpp): what
every launcher of tests/cpp/mle_kernels_driver.hip must write, in plain python integers on CANONICAL values.

Tables cross the boundary with tests/tables.py (`canonical`: stored limbs -> ints, `stored`: int -> stored limbs); `pack` / `unpack` here
are those two over a whole table.  tests/test_mle_model_cpu.py holds this model to the CPU oracle before it judges a kernel.
This module imports neither the oracle nor the package under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tables as T  # noqa: E402

R = T.R
W_FACTOR = (1 << 32) % R          # the fold weights of the k-variable fold carry it (multifold_kernels.hpp)


def pack(vals):
    """canonical ints -> uint64 [n, 4] stored limbs"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.stack([T.stored(v) for v in vals])


def unpack(table):
    return T.canonical(table)


# ---- fold ------------------------------------------------------------------------------------------------
def fold_lo_index(j, log_half):
    """the input index of the `lo` partner of output j when the pairs lie 2^log_half apart: (j / half) * 2 half + j % half"""
    half = 1 << log_half
    return (j // half) * 2 * half + j % half


def fold(t, r, log_half):
    """out[j] = lo + r (hi - lo), lo = t[fold_lo_index(j)], hi = t[that + 2^log_half]; len(t) = 2 n_out"""
    half = 1 << log_half
    out = []
    for j in range(len(t) // 2):
        i = fold_lo_index(j, log_half)
        out.append((t[i] + r * (t[i + half] - t[i])) % R)
    return out


def half_sums(t):
    """(sum of t[j], j < n // 2; sum of the rest): a one-entry table has an empty lower half"""
    h = len(t) // 2
    return sum(t[:h]) % R, sum(t[h:]) % R


def fold_tail(t, pts):
    """variable 0 folded with every point in turn"""
    for r in pts:
        t = fold(t, r, (len(t) // 2).bit_length() - 1)
    return list(t)


# ---- outer and elementwise operations ------------------------------------------------------------------
def distinct(a, b, mul):
    return [(x * y if mul else x + y) % R for x in a for y in b]


def elementwise(op, a, b=None, scalar=None):
    if op == 0:
        return [(x + y) % R for x, y in zip(a, b)]
    if op == 1:
        return [(x - y) % R for x, y in zip(a, b)]
    return [x * scalar % R for x in a]


def to_bytes(t):
    return b"".join(v.to_bytes(32, "big") for v in t)


def repeat(t, shift, n_out):
    """shift = 0: the table over and over (add_to_front); else every entry 2^shift times (add_to_back)"""
    return [t[(i >> shift) if shift else (i % len(t))] for i in range(n_out)]


# ---- MultilinearKZG::open --------------------------------------------------------------------------------
def open_step(t, z):
    """(quotient, remainder): q[j] = t[j + n/2] - t[j], rem[j] = t[j] + z q[j]"""
    h = len(t) // 2
    q = [(t[j + h] - t[j]) % R for j in range(h)]
    return q, [(t[j] + z * q[j]) % R for j in range(h)]


def open_steps(t, pts):
    """(the quotients of every round in level order, the remainder after every round)"""
    quotients, rems = [], []
    for z in pts:
        q, t = open_step(t, z)
        quotients += q
        rems.append(t)
    return quotients, rems


# ---- the Horner suffix scan --------------------------------------------------------------------------------
def horner_suffix(c, z):
    """V_i = sum_{j >= i} c_j z^(j - i), i < n: V_0 = p(z), V_1 .. V_{n-1} the quotient of p(x) - p(z) by x - z"""
    v, out = 0, [0] * len(c)
    for i in range(len(c) - 1, -1, -1):
        v = (c[i] + z * v) % R
        out[i] = v
    return out


def horner_suffix_sparse(nonzero, z, at):
    """the same for a polynomial given by its non-zero coefficients {index: value}, at the indices `at` only"""
    items = sorted(nonzero.items())
    return [sum(c * pow(z, j - i, R) for j, c in items if j >= i) % R for i in at]


def dense_degree(c):
    """the index of the last non-zero coefficient, 0 if there is none"""
    return max([i for i, v in enumerate(c) if v % R], default=0)


# ---- circuit tables ------------------------------------------------------------------------------------------
def circuit_layer(inp, gates):
    """gates: (type, in0, in1); type 0 adds, any other multiplies"""
    return [(inp[a] * inp[b] if t else inp[a] + inp[b]) % R for t, a, b in gates]


def wiring_ones(gates, shift, size):
    """(add, mul) tables of `size` entries: a one at (g << 2 shift) | (in0 << shift) | in1 of gate g, in the table of its type"""
    add, mul = [0] * size, [0] * size
    for g, (t, a, b) in enumerate(gates):
        (mul if t else add)[(g << (2 * shift)) | (a << shift) | b] = 1
    return add, mul


# ---- the weights of `evaluation` ---------------------------------------------------------------------------
def eq_table(pts):
    """eq_b(pts) = prod_i (b_i ? r_i : 1 - r_i), b < 2^k, the FIRST point at the most significant bit of b"""
    out = [1]
    for r in pts:
        out = [w * f % R for w in out for f in ((1 - r) % R, r)]
    return out


def eq_weights(pts, first, k):
    """what eq_weights_kernel writes: the eq table of pts[first .. first + k) times 2^32"""
    return [w * W_FACTOR % R for w in eq_table(pts[first:first + k])]


def eval_weights(pts, k1, k2, s):
    """(w1 with the factor 2^32, wa, wb plain): the first k1 points, the next k2 - s, the last s"""
    return eq_weights(pts, 0, k1), eq_table(pts[k1:k1 + k2 - s]), eq_table(pts[k1 + k2 - s:k1 + k2])


def evaluation_split(log_n):
    """(k1, k2, s) that zkhip_mle_evaluation derives for a table of 2^log_n >= 2^17 entries"""
    k1 = min(8, log_n - 13)
    k2 = log_n - k1
    return k1, k2, k2 // 2


def sum_records(t):
    return sum(t) % R
