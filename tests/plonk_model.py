"""An INDEPENDENT model of the reference's PLONK (plonk/src/protocol/*.rs, transcripts/merlin/src/lib.rs): python ints and hashlib.

It imports neither `oracle/` nor the package under test; Fr, G1 and the domain come from tests/golden/model.py, the pairing from
tests/pairing_model.py.  The five rounds are restated LITERALLY: DenseUnivariatePolynomial with its schoolbook product, its long
division and the quirks of its operators (dense_univariate.rs:88-124, 210-360), four separate `/ zh_poly` quotients in round 3,
the Merlin transcript whose challenge() resets the hasher.  Commitments are p(tau) * G from a known tau (what an MSM against
tau^i G yields).  For large n, `fast_*` offers the O(n) route: with tau known every commitment except the three t parts is an
evaluation at tau (barycentric over the domain plus the blinding in closed form), and the t parts are tied together by
[t_low] + tau^n [t_mid] + tau^2n [t_high] = t(tau) G.
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairing_model as PM  # noqa: E402

M = PM.M
R = M.R
K1, K2 = 2, 3                                       # compiler/utils.rs:28-36

PROOF_FIELDS = ["as_commitment", "bs_commitment", "cs_commitment", "accumulator_commitment", "t_low", "t_mid", "t_high",
                "a_s_poly_zeta", "b_s_poly_zeta", "c_s_poly_zeta", "sigma1_poly_zeta", "sigma2_poly_zeta",
                "w_accumulator_poly_zeta", "w_zeta_commitment", "w_zeta_omega_commitment"]
POINT_FIELDS = [f for f in PROOF_FIELDS if not f.endswith("_zeta")]
CPI_FIELDS = ["q_m", "q_l", "q_r", "q_o", "q_c", "sigma_1", "sigma_2", "sigma_3"]      # the order of VerifierPreprocessedInput::vpi


# ---- transcripts/merlin/src/lib.rs ------------------------------------------------------------------------------------
def fp_to_string(v):
    """ark-ff 0.4.2 Display for Fp: the canonical integer in decimal with leading zeros trimmed (zero prints as "")"""
    return str(v).lstrip("0")


def point_to_string(pt):
    """ark-ec 0.4.2 Display for an affine short-Weierstrass point"""
    return "infinity" if pt is None else "(%s, %s)" % (fp_to_string(pt[0]), fp_to_string(pt[1]))


class MerlinTranscript:
    def __init__(self, label):                      # :12-21
        self.hasher = hashlib.sha256()
        self.hasher.update(b"Merlin Transcript")
        self.hasher.update(label)

    def append_message(self, label, message):       # :23-28
        self.hasher.update(label)
        self.hasher.update(len(message).to_bytes(8, "little"))
        self.hasher.update(message)

    def append_scalar(self, label, scalar):         # :30-35 serialize_compressed: 32 bytes little-endian
        self.append_message(label, (scalar % R).to_bytes(32, "little"))

    def append_point(self, label, point):           # :37-41
        self.append_message(label, point_to_string(point).encode())

    def challenge(self, label):                     # :43-49 finalize_reset, then the label goes into the EMPTY hasher
        digest = self.hasher.digest()
        self.hasher = hashlib.sha256()
        self.hasher.update(label)
        return int.from_bytes(digest, "big") % R


class PlonkRoundTranscript:                         # plonk/src/protocol/transcript.rs
    def __init__(self):
        self.transcript = MerlinTranscript(b"plonk_protocol")

    def first_round(self, a, b, c):
        for p in (a, b, c):
            self.transcript.append_point(b"first_round", p)

    def second_round(self, acc):
        self.transcript.append_point(b"second_round", acc)

    def third_round(self, lo, mid, hi):
        for p in (lo, mid, hi):
            self.transcript.append_point(b"third_round", p)

    def fourth_round(self, *scalars):
        for s in scalars:
            self.transcript.append_scalar(b"fourth_round", s)

    def fifth_round(self, w, ww):
        for p in (w, ww):
            self.transcript.append_point(b"fifth_round", p)

    def challenge_round(self, label):
        return self.transcript.challenge(label)


def compute_verifier_challenges(proof):             # protocol/utils.rs:56-96
    t = PlonkRoundTranscript()
    t.first_round(proof["as_commitment"], proof["bs_commitment"], proof["cs_commitment"])
    beta = t.challenge_round(b"beta")
    gamma = t.challenge_round(b"gamma")
    t.second_round(proof["accumulator_commitment"])
    alpha = t.challenge_round(b"alpha")
    t.third_round(proof["t_low"], proof["t_mid"], proof["t_high"])
    zeta = t.challenge_round(b"zeta")
    t.fourth_round(*[proof[f] for f in PROOF_FIELDS[7:13]])
    nu = t.challenge_round(b"nu")
    t.fifth_round(proof["w_zeta_commitment"], proof["w_zeta_omega_commitment"])
    mu = t.challenge_round(b"mu")
    return beta, gamma, alpha, zeta, nu, mu


# ---- DenseUnivariatePolynomial, operator by operator ------------------------------------------------------------------
class Poly:
    def __init__(self, c):
        self.c = [x % R for x in c]

    def is_zero(self):                              # :39-41 an EMPTY vector
        return not self.c

    def degree(self):                               # :199-207
        return M.dense_degree(self.c)

    def evaluate(self, x):                          # :184-196
        return sum(c * pow(x, i, R) for i, c in enumerate(self.c)) % R

    def __mul__(self, o):
        if isinstance(o, Poly):                     # :210-233 schoolbook over degree() + 1 coefficients
            if self.is_zero() or o.is_zero():
                return Poly([])
            da, db = self.degree(), o.degree()
            out = [0] * (da + db + 1)
            for i in range(da + 1):
                if self.c[i]:
                    for j in range(db + 1):
                        out[i + j] = (out[i + j] + self.c[i] * o.c[j]) % R
            return Poly(out)
        if self.is_zero() or o % R == 0:            # :235-251
            return Poly([])
        return Poly([c * o for c in self.c])

    def __add__(self, o):
        if isinstance(o, Poly):                     # :253-279 the longer DEGREE decides whose length the sum has
            a, b = (self, o) if self.degree() >= o.degree() else (o, self)
            return Poly([a.c[i] + (b.c[i] if i < len(b.c) else 0) for i in range(len(a.c))])
        if self.is_zero():                          # :281-295
            return Poly([o])
        return Poly([self.c[0] + o] + self.c[1:])

    def __neg__(self):                              # :363-374
        return Poly([-c for c in self.c])

    def __sub__(self, o):
        if isinstance(o, Poly):                     # :348-355
            return self + (-o)
        if self.is_zero():                          # :316-330 (sic: the scalar itself, not its negative)
            return Poly([o])
        return Poly([self.c[0] - o] + self.c[1:])

    def __truediv__(self, o):                       # :382-388 over divide_with_q_and_r :88-124
        if self.is_zero():
            return Poly([])
        assert not o.is_zero(), "Dividing by zero polynomial"
        return Poly(M.dense_divide(self.c, o.c))


def roots_of_unity(n):                              # compiler/utils.rs:42-49
    w, out = M.root_of_unity(n), [1]
    for _ in range(1, n):
        out.append(out[-1] * w % R)
    return out


def to_coefficient_poly(values, n):                 # evaluation.rs:47-56 over Domain::ifft
    return Poly(M.domain_ifft(list(values), n))


def zh_values(n):                                   # protocol/utils.rs:41-48
    return [R - 1] + [0] * (n - 1) + [1]


def l1_values(n):
    return [1] + [0] * (n - 1)


def create_monomial(degree, coeff, constant):       # protocol/utils.rs:98-107
    c = [0] * (degree + 1)
    c[degree] = coeff
    c[0] = constant
    return Poly(c)


def apply_w(poly, w):                               # protocol/utils.rs:26-39
    return Poly([c * pow(w, i, R) for i, c in enumerate(poly.c)])


def g1_mul(pt, k):
    """(k mod r) * pt, equal to M.g1_mul on every input (tests/test_plonk_cpu.py), in Jacobian coordinates: one inversion per product
    where the affine ladder spends one per step.  A verdict of this model is some twenty of these; a test asks for sixteen verdicts."""
    P = M.P
    k %= R
    if pt is None or k == 0:
        return None
    x2, y2 = pt
    X, Y, Z = x2, y2, 1
    for bit in bin(k)[3:]:
        if Z:                                                                 # double (a = 0)
            A, B = X * X % P, Y * Y % P
            C = B * B % P
            D = 2 * ((X + B) * (X + B) - A - C) % P
            E = 3 * A % P
            X3 = (E * E - 2 * D) % P
            X, Y, Z = X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P
        if bit == "1":                                                        # add the affine point
            if not Z:
                X, Y, Z = x2, y2, 1
                continue
            ZZ = Z * Z % P
            H, r = (x2 * ZZ - X) % P, (y2 * Z % P * ZZ - Y) % P
            if H == 0:
                if r:
                    X, Y, Z = 1, 1, 0
                    continue
                return M.g1_mul(pt, k)                                        # the running point equals pt: not within the ladder of k < r
            HH = H * H % P
            HHH, V = H * HH % P, X * HH % P
            X3 = (r * r - HHH - 2 * V) % P
            X, Y, Z = X3, (r * (V - X3) - Y * HHH) % P, Z * H % P
    if not Z:
        return None
    zi = pow(Z, P - 2, P)
    return X * zi % P * zi % P, Y * zi % P * zi % P * zi % P


def commit_tau(poly, tau, n_srs=None):
    """UnivariateKZG::commitment against tau^i G: p(tau) G (an SRS shorter than the polynomial is the reference's index panic)"""
    if n_srs is not None and len(poly.c) > n_srs:
        raise IndexError("powers_of_tau_in_g1[%d]" % n_srs)
    return g1_mul(M.G1, poly.evaluate(tau))


def vpi(cpi, tau):                                  # verifier.rs:24-36
    n = cpi["group_order"]
    out = {f: commit_tau(to_coefficient_poly(cpi[f], n), tau) for f in CPI_FIELDS}
    out["x_2"] = PM.g2_mul(PM.G2, tau)
    return out


def accumulator(cpi, wit, beta, gamma):             # prover.rs:125-155
    n = cpi["group_order"]
    w = roots_of_unity(n)
    acc = [1] * n
    for i in range(1, n):
        k = i - 1
        num = (wit["a"][k] + beta * w[k] + gamma) * (wit["b"][k] + beta * K1 * w[k] + gamma) * (wit["c"][k] + beta * K2 * w[k] + gamma) % R
        den = (wit["a"][k] + beta * cpi["sigma_1"][k] + gamma) * (wit["b"][k] + beta * cpi["sigma_2"][k] + gamma) \
            * (wit["c"][k] + beta * cpi["sigma_3"][k] + gamma) % R
        acc[i] = acc[k] * num % R * M.inv(den) % R
    return acc


def prove(cpi, wit, tau, blinding, n_srs=None, want_challenges=False):
    """PlonkProver::prove (prover.rs:39-96) with the 11 random scalars given in the order the reference draws them"""
    n = cpi["group_order"]
    r1, r2, r3 = blinding[0:6], blinding[6:9], blinding[9:11]
    tr = PlonkRoundTranscript()
    C = lambda p: commit_tau(p, tau, n_srs)
    co = lambda v: to_coefficient_poly(v, n)
    zh = Poly(zh_values(n))
    # round 1 (:98-123)
    a_s = Poly([r1[1], r1[0]]) * zh + co(wit["a"])
    b_s = Poly([r1[3], r1[2]]) * zh + co(wit["b"])
    c_s = Poly([r1[5], r1[4]]) * zh + co(wit["c"])
    proof = {"as_commitment": C(a_s), "bs_commitment": C(b_s), "cs_commitment": C(c_s)}
    tr.first_round(proof["as_commitment"], proof["bs_commitment"], proof["cs_commitment"])
    # round 2 (:125-175)
    beta = tr.challenge_round(b"beta")
    gamma = tr.challenge_round(b"gamma")
    acc_poly = Poly(M.domain_ifft(accumulator(cpi, wit, beta, gamma), n))
    z = acc_poly + Poly([r2[0], r2[1], r2[2]]) * zh
    proof["accumulator_commitment"] = C(z)
    tr.second_round(proof["accumulator_commitment"])
    # round 3 (:177-258)
    w = M.root_of_unity(n)
    alpha = tr.challenge_round(b"alpha")
    l1 = co(l1_values(n))
    zw = apply_w(z, w)
    qm, ql, qr, qo, qc = (co(cpi[f]) for f in ("q_m", "q_l", "q_r", "q_o", "q_c"))
    s1, s2, s3 = (co(cpi[f]) for f in ("sigma_1", "sigma_2", "sigma_3"))
    pi = co(wit["public_poly"])
    t = ((a_s * b_s * qm + a_s * ql + b_s * qr + c_s * qo + pi + qc) / zh) \
        + ((((a_s + create_monomial(1, beta, gamma)) * (b_s + create_monomial(1, beta * 2, gamma))
             * (c_s + create_monomial(1, beta * 3, gamma)) * z) * alpha) / zh) \
        - (((((a_s + s1 * beta) + gamma) * ((b_s + s2 * beta) + gamma) * ((c_s + s3 * beta) + gamma) * zw) * alpha) / zh) \
        + ((((z - 1) * l1) * (alpha * alpha % R)) / zh)
    t_low, t_mid, t_high = Poly(t.c[0:n]), Poly(t.c[n:2 * n]), Poly(t.c[2 * n:])      # split_poly_in_3
    xn = Poly([0] * n + [1])
    b10, b11 = r3
    t_low = t_low + xn * b10
    t_mid = t_mid + (xn * b11 - b10)
    t_high = t_high + ((-b11) % R)
    proof.update(t_low=C(t_low), t_mid=C(t_mid), t_high=C(t_high))
    tr.third_round(proof["t_low"], proof["t_mid"], proof["t_high"])
    # round 4 (:260-293)
    zeta = tr.challenge_round(b"zeta")
    az, bz, cz = a_s.evaluate(zeta), b_s.evaluate(zeta), c_s.evaluate(zeta)
    zwz, s1z, s2z = zw.evaluate(zeta), s1.evaluate(zeta), s2.evaluate(zeta)
    proof.update(a_s_poly_zeta=az, b_s_poly_zeta=bz, c_s_poly_zeta=cz, sigma1_poly_zeta=s1z, sigma2_poly_zeta=s2z,
                 w_accumulator_poly_zeta=zwz)
    tr.fourth_round(az, bz, cz, s1z, s2z, zwz)
    # round 5 (:295-376)
    nu = tr.challenge_round(b"nu")
    r_poly = (qm * az * bz + ql * az + qr * bz + qo * cz + pi.evaluate(zeta) + qc) \
        + (((z * ((az + beta * zeta + gamma) % R) * ((bz + beta * 2 * zeta + gamma) % R) * ((cz + beta * 3 * zeta + gamma) % R))
            - (((s3 * beta) + cz + gamma) * ((az + beta * s1z + gamma) % R) * ((bz + beta * s2z + gamma) % R) * zwz)) * alpha) \
        + (((z - 1) * l1.evaluate(zeta)) * (alpha * alpha % R)) \
        - ((t_low + t_mid * pow(zeta, n, R) + t_high * pow(zeta, 2 * n, R)) * zh.evaluate(zeta))
    w_zeta = (r_poly + (a_s - az) * nu + (b_s - bz) * pow(nu, 2, R) + (c_s - cz) * pow(nu, 3, R)
              + (s1 - s1z) * pow(nu, 4, R) + (s2 - s2z) * pow(nu, 5, R)) / Poly([-zeta, 1])
    w_zeta_omega = (z - zwz) / Poly([-(zeta * w), 1])
    proof.update(w_zeta_commitment=C(w_zeta), w_zeta_omega_commitment=C(w_zeta_omega))
    tr.fifth_round(proof["w_zeta_commitment"], proof["w_zeta_omega_commitment"])
    mu = tr.challenge_round(b"mu")
    return (proof, (beta, gamma, alpha, zeta, nu, mu)) if want_challenges else proof


def _msm(pairs):
    acc = None
    for pt, k in pairs:
        acc = M.g1_add(acc, g1_mul(pt, k))
    return acc


def verifier_points(n, proof, v, public_poly):
    """the G1 arguments of the two pairings of PlonkVerifier::verify (verifier.rs:62-172): (left, right)"""
    beta, gamma, alpha, zeta, nu, mu = compute_verifier_challenges(proof)
    zh_zeta = (pow(zeta, n, R) - 1) % R
    w = M.root_of_unity(n)
    l1_zeta = to_coefficient_poly(l1_values(n), n).evaluate(zeta)
    pi_zeta = to_coefficient_poly(public_poly, n).evaluate(zeta)
    az, bz, cz = proof["a_s_poly_zeta"], proof["b_s_poly_zeta"], proof["c_s_poly_zeta"]
    zwz, s1z, s2z = proof["w_accumulator_poly_zeta"], proof["sigma1_poly_zeta"], proof["sigma2_poly_zeta"]
    a2 = alpha * alpha % R
    r0 = (pi_zeta - l1_zeta * a2 - alpha * ((az + s1z * beta + gamma) * (bz + s2z * beta + gamma) % R * (cz + gamma) % R * zwz)) % R
    t_comb = _msm([(proof["t_low"], 1), (proof["t_mid"], pow(zeta, n, R)), (proof["t_high"], pow(zeta, 2 * n, R))])
    d1 = _msm([(v["q_m"], az * bz), (v["q_l"], az), (v["q_r"], bz), (v["q_o"], cz), (v["q_c"], 1),
               (proof["accumulator_commitment"], (az + zeta * beta + gamma) * (bz + 2 * zeta * beta + gamma) % R
                * (cz + 3 * zeta * beta + gamma) % R * alpha + l1_zeta * a2 + mu),
               (v["sigma_3"], -((az + s1z * beta + gamma) * (bz + s2z * beta + gamma) % R * alpha % R * beta % R * zwz)),
               (t_comb, -zh_zeta)])
    f1 = _msm([(d1, 1), (proof["as_commitment"], nu), (proof["bs_commitment"], pow(nu, 2, R)), (proof["cs_commitment"], pow(nu, 3, R)),
               (v["sigma_1"], pow(nu, 4, R)), (v["sigma_2"], pow(nu, 5, R))])
    e1 = g1_mul(M.G1, nu * az + pow(nu, 2, R) * bz + pow(nu, 3, R) * cz + pow(nu, 4, R) * s1z + pow(nu, 5, R) * s2z + mu * zwz - r0)
    wz, wzw = proof["w_zeta_commitment"], proof["w_zeta_omega_commitment"]
    left = _msm([(wz, 1), (wzw, mu)])
    right = _msm([(wz, zeta), (wzw, w * mu % R * zeta), (f1, 1), (e1, -1)])
    return left, right


def verify(n, proof, v, public_poly):
    left, right = verifier_points(n, proof, v, public_poly)
    return PM.pairing(left, v["x_2"]) == PM.pairing(right, PM.G2)


def verify_tau(n, proof, v, public_poly, tau):
    """the same verdict without a pairing when tau is known: e(L, tau G2) == e(Rt, G2)  <=>  tau L == Rt (G1, G2 of prime order)"""
    left, right = verifier_points(n, proof, v, public_poly)
    return g1_mul(left, tau) == right if left is not None else right is None


def tamper(proof, field):
    """the proof with one field changed: a point gets G added, a scalar one"""
    out = dict(proof)
    out[field] = (proof[field] + 1) % R if field.endswith("_zeta") else M.g1_add(proof[field], M.G1)
    return out


# ---- satisfied circuits by construction ---------------------------------------------------------------------------------
def random_circuit(n, rng, vrng=None, n_public=2):
    """A satisfied circuit of n rows (the last quarter padding) with a copy-constraint permutation built from the variables' uses:
    cells of equal VARIABLE (not merely equal value) are linked in a cycle, labels w^i, 2 w^i, 3 w^i as make_s_polynomials writes them.
    `rng` draws the structure (wiring, selectors), `vrng` the free values: one structure with two value streams = two witnesses."""
    vrng = vrng or rng
    w = roots_of_unity(n)
    rows = n - max(1, n // 4)
    values = [vrng.randrange(R) for _ in range(4)]                    # variable id -> value
    a_id, b_id, c_id = [None] * n, [None] * n, [None] * n
    cols = {f: [0] * n for f in ("q_l", "q_r", "q_m", "q_o", "q_c")}
    public = [0] * n
    for i in range(rows):
        if i < n_public:                                              # "x public": q_l = 1, PI = -x
            values.append(vrng.randrange(R))
            a_id[i] = len(values) - 1
            cols["q_l"][i] = 1
            public[i] = (-values[a_id[i]]) % R
            continue
        a_id[i], b_id[i] = rng.randrange(len(values)), rng.randrange(len(values))
        ql, qr, qm, qc = (rng.randrange(R) if rng.random() < 0.7 else 0 for _ in range(4))
        av, bv = values[a_id[i]], values[b_id[i]]
        values.append((-(ql * av + qr * bv + qm * av * bv + qc)) % R)       # q_o = 1: the output wire takes what closes the gate
        c_id[i] = len(values) - 1
        cols["q_l"][i], cols["q_r"][i], cols["q_m"][i], cols["q_c"][i], cols["q_o"][i] = ql, qr, qm, qc, 1
    val = lambda k: 0 if k is None else values[k]
    wit = {"a": [val(k) for k in a_id], "b": [val(k) for k in b_id], "c": [val(k) for k in c_id], "public_poly": public}
    uses = {}
    for col, ids in enumerate((a_id, b_id, c_id)):
        for row, k in enumerate(ids):
            uses.setdefault(k, []).append((col, row))
    sig = [[0] * n for _ in range(3)]
    for cells in uses.values():
        for i, (col, row) in enumerate(cells):
            ncol, nrow = cells[(i + 1) % len(cells)]
            sig[ncol][nrow] = (col + 1) * w[row] % R
    cpi = dict(cols, group_order=n, sigma_1=sig[0], sigma_2=sig[1], sigma_3=sig[2])
    return cpi, wit


def gate_identity_holds(cpi, wit):
    return all((cpi["q_l"][i] * wit["a"][i] + cpi["q_r"][i] * wit["b"][i] + cpi["q_m"][i] * wit["a"][i] * wit["b"][i]
                + cpi["q_o"][i] * wit["c"][i] + wit["public_poly"][i] + cpi["q_c"][i]) % R == 0 for i in range(cpi["group_order"]))


# ---- the O(n) route ---------------------------------------------------------------------------------------------------
def batch_inv(vals):
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    inv = M.inv(acc)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * vals[i] % R
    return out


class FastDomain:
    """barycentric evaluation of a column given on the n-th roots of unity: f(x) = (x^n - 1) / n * sum_i f_i w^i / (x - w^i)"""

    def __init__(self, n):
        self.n, self.w = n, roots_of_unity(n)

    def weights(self, x):
        inv = batch_inv([(x - wi) % R for wi in self.w])
        s = (pow(x, self.n, R) - 1) * M.inv(self.n) % R
        return [s * wi % R * iv % R for wi, iv in zip(self.w, inv)]

    @staticmethod
    def at(values, weights):
        return sum(v * k for v, k in zip(values, weights) if v) % R


def fast_accumulator(cpi, wit, beta, gamma):
    n = cpi["group_order"]
    w = roots_of_unity(n)
    nums = [(wit["a"][k] + beta * w[k] + gamma) * (wit["b"][k] + beta * K1 * w[k] + gamma) % R * (wit["c"][k] + beta * K2 * w[k] + gamma) % R
            for k in range(n)]
    dens = batch_inv([(wit["a"][k] + beta * cpi["sigma_1"][k] + gamma) * (wit["b"][k] + beta * cpi["sigma_2"][k] + gamma) % R
                      * (wit["c"][k] + beta * cpi["sigma_3"][k] + gamma) % R for k in range(n)])
    acc = [1] * n
    for i in range(1, n):
        acc[i] = acc[i - 1] * nums[i - 1] % R * dens[i - 1] % R
    return acc


def fast_check(cpi, wit, tau, blinding, proof):
    """O(n) checks of a proof made with KNOWN tau and blinding; returns the list of what failed (empty: all hold).  The challenges
    come from the proof's own points (the three t parts cannot be derived in O(n)); everything else is recomputed."""
    n = cpi["group_order"]
    r1, r2 = blinding[0:6], blinding[6:9]
    beta, gamma, alpha, zeta, nu, mu = compute_verifier_challenges(proof)
    dom = FastDomain(n)
    w = dom.w[1]
    G = lambda k: g1_mul(M.G1, k)
    acc = fast_accumulator(cpi, wit, beta, gamma)
    cols = dict(a=wit["a"], b=wit["b"], c=wit["c"], pi=wit["public_poly"], acc=acc, **{f: cpi[f] for f in CPI_FIELDS})

    def at(x):
        k = dom.weights(x)
        v = {name: FastDomain.at(col, k) for name, col in cols.items()}
        zh = (pow(x, n, R) - 1) % R
        v["a"] = (v["a"] + (r1[0] * x + r1[1]) * zh) % R
        v["b"] = (v["b"] + (r1[2] * x + r1[3]) * zh) % R
        v["c"] = (v["c"] + (r1[4] * x + r1[5]) * zh) % R
        v["z"] = (v["acc"] + (r2[0] + r2[1] * x + r2[2] * x * x) * zh) % R
        v["zh"], v["l1"] = zh, zh * M.inv(n * (x - 1)) % R
        return v

    bad = []
    T, Tw, Z, Zw = at(tau), at(tau * w % R), at(zeta), at(zeta * w % R)
    for f, k in (("as_commitment", "a"), ("bs_commitment", "b"), ("cs_commitment", "c"), ("accumulator_commitment", "z")):
        if proof[f] != G(T[k]):
            bad.append(f)
    num = (T["a"] * T["b"] * T["q_m"] + T["a"] * T["q_l"] + T["b"] * T["q_r"] + T["c"] * T["q_o"] + T["pi"] + T["q_c"]
           + alpha * (T["a"] + beta * tau + gamma) * (T["b"] + 2 * beta * tau + gamma) * (T["c"] + 3 * beta * tau + gamma) * T["z"]
           - alpha * (T["a"] + beta * T["sigma_1"] + gamma) * (T["b"] + beta * T["sigma_2"] + gamma) * (T["c"] + beta * T["sigma_3"] + gamma) * Tw["z"]
           + alpha * alpha * (T["z"] - 1) * T["l1"]) % R
    t_tau = num * M.inv(T["zh"]) % R
    t_comb = _msm([(proof["t_low"], 1), (proof["t_mid"], pow(tau, n, R)), (proof["t_high"], pow(tau, 2 * n, R))])
    if t_comb != G(t_tau):
        bad.append("t_low + tau^n t_mid + tau^2n t_high")
    want = dict(a_s_poly_zeta=Z["a"], b_s_poly_zeta=Z["b"], c_s_poly_zeta=Z["c"], sigma1_poly_zeta=Z["sigma_1"],
                sigma2_poly_zeta=Z["sigma_2"], w_accumulator_poly_zeta=Zw["z"])
    bad += [f for f, v in want.items() if proof[f] != v]
    az, bz, cz, s1z, s2z, zwz = (want[f] for f in PROOF_FIELDS[7:13])
    # (tau - zeta) W_zeta = r(tau) G + nu-combination, with the t parts' unknown logarithms taken from their commitments
    r_known = (T["q_m"] * az * bz + T["q_l"] * az + T["q_r"] * bz + T["q_o"] * cz + Z["pi"] + T["q_c"]
               + alpha * (T["z"] * (az + beta * zeta + gamma) * (bz + 2 * beta * zeta + gamma) * (cz + 3 * beta * zeta + gamma)
                          - (beta * T["sigma_3"] + cz + gamma) * (az + beta * s1z + gamma) * (bz + beta * s2z + gamma) * zwz)
               + alpha * alpha * (T["z"] - 1) * Z["l1"]
               + nu * (T["a"] - az) + pow(nu, 2, R) * (T["b"] - bz) + pow(nu, 3, R) * (T["c"] - cz)
               + pow(nu, 4, R) * (T["sigma_1"] - s1z) + pow(nu, 5, R) * (T["sigma_2"] - s2z)) % R
    t_zeta = _msm([(proof["t_low"], 1), (proof["t_mid"], pow(zeta, n, R)), (proof["t_high"], pow(zeta, 2 * n, R))])
    if g1_mul(proof["w_zeta_commitment"], (tau - zeta) % R) != M.g1_add(G(r_known), g1_mul(t_zeta, (-Z["zh"]) % R)):
        bad.append("w_zeta_commitment")
    if g1_mul(proof["w_zeta_omega_commitment"], (tau - zeta * w) % R) != G((T["z"] - zwz) % R):
        bad.append("w_zeta_omega_commitment")
    return bad
