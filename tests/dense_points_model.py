"""The model the dense-points tests compare with: Lagrange interpolation over BLS12-381 Fr in Python integers, and the transform
domain's generator.  Imports neither the oracle nor the package under test."""
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
