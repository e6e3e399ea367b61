"""The model the dense-points tests compare with: Lagrange interpolation over BLS12-381 Fr in Python integers, the transform
domain's generator, and what each stage of zkhip_dense_points stores -- evaluation records per segment, partial products of the weights,
(Num, Den) records and their combine (tests/test_dense_points_model_cpu.py holds these to each other and to the oracle).  Imports neither
the oracle nor the package under test."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def lagrange_coefficients_many(xs, ys_list):
    """for each ys of ys_list: the coefficients (low degree first, n of them) of the polynomial of degree < n through (xs[i], ys[i]),
    in Python integers mod r: sum_i y_i / D_i * M(X) / (X - x_i) with the master polynomial M = prod (X - x_j), D_i = prod_{j != i}
    (x_i - x_j), each quotient by synthetic division.  The quotients and the D_i are formed once for all ys."""
    n = len(xs)
    master = [1]
    for x in xs:
        nxt = [0] * (len(master) + 1)
        for k, c in enumerate(master):
            nxt[k + 1] = (nxt[k + 1] + c) % R
            nxt[k] = (nxt[k] - c * x) % R
        master = nxt
    outs = [[0] * n for _ in ys_list]
    for i in range(n):
        d = 1
        for j in range(n):
            if j != i:
                d = d * (xs[i] - xs[j]) % R
        dinv = pow(d, -1, R)
        quotient = [0] * n
        carry = 0
        for k in range(n, 0, -1):                         # master / (X - x_i), top down
            carry = (master[k] + carry * xs[i]) % R
            quotient[k - 1] = carry
        for out, ys in zip(outs, ys_list):
            s = ys[i] * dinv % R
            if s:
                for k in range(n):
                    out[k] = (out[k] + s * quotient[k]) % R
    return outs


def lagrange_coefficients(xs, ys):
    return lagrange_coefficients_many(xs, [ys])[0]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def root_of_unity(size):
    """F::get_root_of_unity(size) of a power of two: 7^((r - 1) / size)"""
    return pow(7, (R - 1) // size, R)


# ---- what each stage of zkhip_dense_points stores (csrc/dense_points_kernels.hpp), on canonical integers ------------------------------
def segment(n, seg_len, seg):
    """[lo, hi) of segment `seg` of an inner range of n: empty beyond the range"""
    lo = min(seg * seg_len, n)
    return lo, min(lo + seg_len, n)


def eval_records(coeffs, xs, seg_len, segs):
    """records[seg][p] = sum over k in the segment of c_k xs[p]^k; an empty segment gives 0"""
    out = []
    for seg in range(segs):
        lo, hi = segment(len(coeffs), seg_len, seg)
        part = coeffs[lo:hi]
        out.append([horner(part, x) * pow(x, lo, R) % R if part else 0 for x in xs])
    return out


def weight_records(xs, seg_len, segs):
    """records[seg][i] = prod over j in the segment, j != i, of (xs[i] - xs[j]); an empty segment gives 1"""
    n = len(xs)
    out = []
    for seg in range(segs):
        lo, hi = segment(n, seg_len, seg)
        row = []
        for i, x in enumerate(xs):
            d = 1
            for j in range(lo, hi):
                if j != i:
                    d = d * (x - xs[j]) % R
            row.append(d)
        out.append(row)
    return out


def weights(xs):
    """D_i = prod_{j != i} (x_i - x_j): the product of a node's records, whatever the cut"""
    return weight_records(xs, max(len(xs), 1), 1)[0]


def invert(d):
    """the device's Fermat inverse: 0 -> 0"""
    return pow(d, R - 2, R)


def weights_inv(xs):
    return [invert(d) for d in weights(xs)]


def domain_records(xs, ys, winv, N, seg_len, segs):
    """records[seg][t] = (Num, Den) at z = w^t, w = root_of_unity(N), from (0, 1) over the segment's nodes in order:
    Num <- Num (z - x_i) + y_i winv_i Den, Den <- Den (z - x_i).  An empty segment gives (0, 1)."""
    w = root_of_unity(N)
    out = []
    for seg in range(segs):
        lo, hi = segment(len(xs), seg_len, seg)
        sx = xs[lo:hi]
        ss = [y * v % R for y, v in zip(ys[lo:hi], winv[lo:hi])]
        row, z = [], 1
        for _t in range(N):
            num, den = 0, 1
            for x, s in zip(sx, ss):
                d = z - x
                num = (num * d + s * den) % R
                den = den * d % R
            row.append((num, den))
            z = z * w % R
        out.append(row)
    return out


def domain_fold(records):
    """per t, the records of segments A then B combined as (Num_A Den_B + Num_B Den_A, Den_A Den_B), from the first segment on"""
    out = list(records[0])
    for nxt in records[1:]:
        out = [((na * db + nb * da) % R, da * db % R) for (na, da), (nb, db) in zip(out, nxt)]
    return out


def rotate_problem(xs, ys, winv, N, k, c):
    """the interpolation problem moved by g = w^k and scaled by c: nodes g x_i, values c y_i, and 1 / D_i / g^(n - 1), which are the
    new nodes' own weights when winv were the old ones'.  Its polynomial is c P(X / g)."""
    g = pow(root_of_unity(N), k, R)
    back = pow(g, -(len(xs) - 1), R)
    return [g * x % R for x in xs], [c * y % R for y in ys], [back * v % R for v in winv]


def rotate_domain_records(records, N, n, k, c, seg_len):
    """domain_records of rotate_problem(...) from those of the problem itself, without walking the nodes again: with z' = g z every
    difference z' - g x_i is g (z - x_i), so after a segment of m nodes lane t + k holds Den' = g^m Den and, s_i' being
    c g^-(n - 1) s_i, Num' = c g^-(n - 1) g^(m - 1) Num of lane t (by induction over the recurrence)."""
    g = pow(root_of_unity(N), k, R)
    c2 = c * pow(g, -(n - 1), R) % R
    out = []
    for seg, rec in enumerate(records):
        lo, hi = segment(n, seg_len, seg)
        f_num, f_den = c2 * pow(g, hi - lo - 1, R) % R, pow(g, hi - lo, R)
        row = [None] * N
        for t, (num, den) in enumerate(rec):
            row[(t + k) % N] = (num * f_num % R, den * f_den % R)
        out.append(row)
    return out
