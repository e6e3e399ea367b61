"""An INDEPENDENT model of the BLS12-381 optimal ate pairing: python ints only.

It imports neither `oracle/` nor the package under test; G1, the SRS, commit and open come from tests/golden/model.py.
It is written from the textbook definitions, not from the device code:
  - Fq2 = Fq[u]/(u^2 + 1); Fq12 is held as Fq2[w]/(w^6 - xi), xi = u + 1 (the same field as the tower
    Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v): v = w^2);
  - G2 is the M-type twist y^2 = x^3 + 4 xi, untwisted into E(Fq12) by (x, y) -> (x / w^2, y / w^3);
  - the Miller loop runs over |x| in AFFINE coordinates with the textbook line y_P - y_T - lambda (x_P - x_T);
  - the final exponentiation is one plain pow with exponent (p^12 - 1) / r; x < 0 inverts the result in GT.
GT values are returned as 12 canonical ints in arkworks field order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import model as M  # noqa: E402

P = M.P
R = M.R
X_ABS = 0xD201000000010000                         # |x|, x < 0
XI = (1, 1)
G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))
FINAL_EXP = (P ** 12 - 1) // R


# ---- Fq2 -------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    t = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * t % P, -a[1] * t % P)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


F2_ZERO, F2_ONE = (0, 0), (1, 0)
XI_INV = f2_inv(XI)


# ---- Fq12 as six Fq2 coefficients of w^0..w^5 ---------------------------------------------------------------------
def f12_one():
    return [F2_ONE] + [F2_ZERO] * 5


def f12_mul(a, b):
    acc = [F2_ZERO] * 11
    for i in range(6):
        if a[i] == F2_ZERO:
            continue
        for j in range(6):
            if b[j] != F2_ZERO:
                acc[i + j] = f2_add(acc[i + j], f2_mul(a[i], b[j]))
    return [f2_add(acc[k], f2_mul(acc[k + 6], XI)) if k < 5 else acc[k] for k in range(6)]


def f12_pow(a, e):
    out, base = f12_one(), a
    while e:
        if e & 1:
            out = f12_mul(out, base)
        e >>= 1
        if e:
            base = f12_mul(base, base)
    return out


def f12_to_tower(a):
    """w-basis -> arkworks order: c0 = (a0, a2, a4), c1 = (a1, a3, a5) since w^2 = v"""
    out = []
    for k in (0, 2, 4, 1, 3, 5):
        out.extend(a[k])
    return out


# ---- G2 on the twist (affine tuples of Fq2, None = infinity) ----------------------------------------------------
B2 = f2_scale(XI, 4)


def g2_on_curve(q):
    if q is None:
        return True
    x, y = q
    return f2_sub(f2_mul(y, y), f2_add(f2_mul(f2_mul(x, x), x), B2)) == F2_ZERO


def g2_neg(q):
    return None if q is None else (q[0], ((-q[1][0]) % P, (-q[1][1]) % P))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if f2_add(y1, y2) == F2_ZERO:
            return None
        lam = f2_mul(f2_scale(f2_mul(x1, x1), 3), f2_inv(f2_scale(y1, 2)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), x1), x2)
    return x3, f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1)


def g2_mul(q, k, reduce=True):
    if reduce:
        k %= R
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, q)
        q = g2_add(q, q)
        k >>= 1
    return acc


def g2_mul_raw(q, k):
    """k * q without reducing k mod r (the subgroup check)"""
    return g2_mul(q, k, reduce=False)


def multilinear_srs_g2(tau):                        # trusted_setup.rs:37-45
    return [g2_mul(G2, t) for t in tau]


def univariate_srs_g2(tau, max_degree):             # univariate_kzg.rs:18-35
    return [g2_mul(G2, pow(tau, i, R)) for i in range(max_degree + 1)]


# ---- pairing -------------------------------------------------------------------------------------------------------
def _line(lam, xt, yt, p):
    """y_P - y_T - lam (x_P - x_T) at T = (xt / w^2, yt / w^3), lam = lam' / w:
       = y_P + ((lam' xt - yt) / xi) w^3 - (lam' x_P / xi) w^5"""
    xp, yp = p
    out = [F2_ZERO] * 6
    out[0] = (yp % P, 0)
    out[3] = f2_mul(f2_sub(f2_mul(lam, xt), yt), XI_INV)
    out[5] = f2_mul(f2_scale(lam, (-xp) % P), XI_INV)
    return out


def miller_loop(p, q):
    """f_{|x|, psi(q)}(p), not yet inverted for x < 0"""
    if p is None or q is None:
        return f12_one()
    f, t = f12_one(), q
    for bit in bin(X_ABS)[3:]:
        xt, yt = t
        lam = f2_mul(f2_scale(f2_mul(xt, xt), 3), f2_inv(f2_scale(yt, 2)))
        f = f12_mul(f12_mul(f, f), _line(lam, xt, yt, p))
        t = g2_add(t, t)
        if bit == "1":
            xt, yt = t
            lam = f2_mul(f2_sub(q[1], yt), f2_inv(f2_sub(q[0], xt)))
            f = f12_mul(f, _line(lam, xt, yt, p))
            t = g2_add(t, q)
    return f


def final_exponentiation(f):
    g = f12_pow(f, FINAL_EXP)
    return f12_pow(g, R - 1)                      # x < 0: the inverse in GT (g^r = 1)


def multi_pairing(pairs):
    """prod_k e(p_k, q_k) as one final exponentiation of the product of the Miller loops (w-basis Fq12)"""
    f = f12_one()
    for p, q in pairs:
        f = f12_mul(f, miller_loop(p, q))
    return final_exponentiation(f)


def pairing(p, q):
    return multi_pairing([(p, q)])


def gt_is_one(g):
    return g == f12_one()


# ---- KZG verify, as the reference writes it ------------------------------------------------------------------------
def multilinear_verify(commit, z, evaluation, proofs, srs_g2):
    """MultilinearKZG::verify (multilinear_kzg.rs:90-112, utils.rs:42-60): e(C - v G1, G2) == prod e(pi_i, tau_i G2 - z_i G2)"""
    assert len(srs_g2) == len(z) == len(proofs)
    lhs = pairing(M.g1_add(commit, M.g1_mul(M.G1, (-evaluation) % R)), G2)
    rhs = multi_pairing([(pi, g2_add(t, g2_neg(g2_mul(G2, zi)))) for pi, t, zi in zip(proofs, srs_g2, z)])
    return lhs == rhs


def univariate_verify(commit, z, evaluation, proof, srs_g2):
    """UnivariateKZG::verify (univariate_kzg.rs:83-104): e(C - v G1, G2) == e(pi, tau G2 - z G2)"""
    lhs = pairing(M.g1_add(commit, M.g1_mul(M.G1, (-evaluation) % R)), G2)
    rhs = pairing(proof, g2_add(srs_g2[1], g2_neg(g2_mul(G2, z))))
    return lhs == rhs
