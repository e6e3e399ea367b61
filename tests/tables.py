"""Tables for the parity tests that random data cannot give: full-range and extreme STORED values (the arithmetic fills) and
tables with structure (the shape fills).  `oracle.random_fr` clears the top two bits of every stored element, so it never produces a
stored value in [2^254, r) -- about 45 % of the field -- nor a limb of 0 or 0xFFFFFFFF, a constant table, a 0/1 table or a table whose
sum or first-round difference vanishes.

fill(kind, n, seed) -> numpy uint64 [n, 4]: little-endian limbs of the stored (Montgomery) form, what the provers and the oracle read.
canonical(table)    -> python ints (the values the stored limbs stand for), for tests/golden/model.py.

Everything is generated with whole-array numpy operations (rejection sampling on the limbs): a 2^21-entry table takes a fraction of a second.
This module imports neither the oracle nor the package under test."""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = (1 << 256) % R                                  # the stored form of 1
_R_LIMBS = [(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
_EDGE_LIMBS = np.array([0, 1, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint64)

FILLS_ARITH = ["uniform_r", "top", "stored_max", "limb_edges"]
FILLS_SHAPE = ["zero", "one", "minus_one", "bits", "bytes", "one_hot", "halves_cancel", "halves_equal"]
FILLS = FILLS_ARITH + FILLS_SHAPE


def _limbs(v):
    """one value 0 <= v < 2^256 -> uint64 [4]"""
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def stored(v):
    """canonical python int -> its stored limbs, uint64 [4]"""
    return _limbs((v % R) * MONT % R)


def below_r(a):
    """bool [n]: the 256-bit value of each row is < r (limb by limb from the top)"""
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for i in (3, 2, 1, 0):
        ri = np.uint64(_R_LIMBS[i])
        lt |= eq & (a[:, i] < ri)
        eq &= a[:, i] == ri
    return lt


def at_least_2_254(a):
    return (a[:, 3] >> np.uint64(62)) != 0


def negate(a):
    """r - a limb by limb with borrow, 0 -> 0: the stored form of the negated value (the Montgomery map is linear)"""
    out = np.empty_like(a)
    borrow = np.zeros(len(a), dtype=np.uint64)
    for i in range(4):
        ri = np.uint64(_R_LIMBS[i])
        d = ri - a[:, i]                                              # wraps mod 2^64
        b1 = (a[:, i] > ri).astype(np.uint64)
        out[:, i] = d - borrow
        b2 = (d < borrow).astype(np.uint64)
        borrow = b1 | b2
    out[~a.any(axis=1)] = 0
    return out


def _rejection(rng, n, draw, accept):
    """n rows of draw(rng, m) that are < r; `accept` = the share of draws that are"""
    parts, have = [], 0
    while have < n:
        c = draw(rng, int((n - have) / accept * 1.02) + 16)
        c = c[below_r(c)]
        parts.append(c)
        have += len(c)
    return np.ascontiguousarray(np.concatenate(parts)[:n])


def _draw_255(rng, m):
    a = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)                          # r < 2^255
    return a


def _draw_top(rng, m):
    a = _draw_255(rng, m)
    a[:, 3] |= np.uint64(1 << 62)                                     # uniform on [2^254, 2^255)
    return a


def _draw_edges(rng, m):
    i = rng.integers(0, len(_EDGE_LIMBS), size=(m, 8), dtype=np.uint8)
    i[:, 7] = rng.integers(0, 2, size=m, dtype=np.uint8)              # r's top 32-bit limb is 0x73EDA753: 0 and 1 always pass there, the other three never
    h = _EDGE_LIMBS[i]
    return h[:, 0::2] | (h[:, 1::2] << np.uint64(32))


def _uniform(rng, n):
    return _rejection(rng, n, _draw_255, R / 2 ** 255)


def fill(kind, n, seed):
    rng = np.random.Generator(np.random.PCG64([seed, FILLS.index(kind)]))
    if kind == "uniform_r":
        return _uniform(rng, n)
    if kind == "top":
        return _rejection(rng, n, _draw_top, (R - 2 ** 254) / 2 ** 254)
    if kind == "stored_max":
        return np.tile(_limbs(R - 1), (n, 1))
    if kind == "limb_edges":
        return _rejection(rng, n, _draw_edges, 1.0)
    if kind == "zero":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "one":
        return np.tile(stored(1), (n, 1))
    if kind == "minus_one":
        return np.tile(stored(R - 1), (n, 1))
    if kind == "bits":
        return np.stack([stored(0), stored(1)])[rng.integers(0, 2, size=n)]
    if kind == "bytes":
        return np.stack([stored(v) for v in range(256)])[rng.integers(0, 256, size=n)]
    if kind == "one_hot":
        a = np.zeros((n, 4), dtype=np.uint64)
        v = _uniform(rng, 1)[0]
        a[int(rng.integers(0, n))] = v if v.any() else stored(1)
        return a
    if kind in ("halves_cancel", "halves_equal"):
        if n < 2:
            return _uniform(rng, n)
        lo = _uniform(rng, n // 2)
        return np.ascontiguousarray(np.concatenate([lo, negate(lo) if kind == "halves_cancel" else lo]))
    raise KeyError(kind)


def rotation(kinds, lead, count):
    """`count` fills of `kinds`, starting at `lead` and going round: the factors of a product differ, and every fill leads one case"""
    i = kinds.index(lead)
    return [kinds[(i + q) % len(kinds)] for q in range(count)]


# the zero-coefficient families of a [2, 2] claim (sparse_univariate.rs:55 drops a vanishing coefficient at interpolation), term by term
ZERO_COEFF_FAMILIES = {
    # both terms are linear in the round's variable (a constant factor): the x^2 coefficient vanishes in every round -> 2 monomials
    "linear": [("uniform_r", "one"), ("top", "one")],
    # round one: the first factor of each term does not depend on the variable (2 monomials); once folded at a challenge it does (3)
    "first_round": [("halves_equal", "uniform_r"), ("halves_equal", "top")],
    # claimed sum 0 and p(0) = -p(1) in round one; one term linear, one vanishing altogether -> 2 monomials
    "zero_sum": [("halves_cancel", "one"), ("uniform_r", "zero")],
}


def zero_coeff_lens(family, n_rounds):
    """the number of monomials of every round polynomial of that family"""
    return [2] + [3 if family == "first_round" else 2] * (n_rounds - 1)


def zero_coeff_tables(family, log_n, seed=500):
    """[4, n, 4]: the tables of a [2, 2] claim"""
    kinds = [f for term in ZERO_COEFF_FAMILIES[family] for f in term]
    return np.stack([fill(f, 1 << log_n, seed + q) for q, f in enumerate(kinds)])


def cancelling_tables(log_n, seed=600):
    """[4, n, 4]: (a, 1) + (-a, 1).  Each term is linear and every coefficient of one cancels the other's: the zeros are KEPT after the
    addition (sparse_univariate.rs:159-203), two monomials (0, x^0), (0, x^1) per round"""
    a = fill("uniform_r", 1 << log_n, seed)
    one = fill("one", 1 << log_n, 0)
    return np.stack([a, one, negate(a), one])


def sumcheck_with_claimed_sum(ora, evals, claimed):
    """Sumcheck::prove (sumcheck/src/sumcheck.rs:29-61) absorbing a sum the caller GIVES (zero when poly_sum() never ran), restated round
    by round on the oracle's own half sums, fold and transcript -> (round_polys [n_vars, 2, 4], challenges [n_vars, 4]).  With the true sum
    this is ora.sumcheck_prove (tests/test_structured_tables_cpu.py)."""
    t = ora.Transcript()
    t.commit(ora.fr_to_bytes_be(claimed))
    cur, rps, chs = np.ascontiguousarray(evals), [], []
    while len(cur) > 1:
        hs = ora.mle_half_sums(cur)
        t.commit(ora.fr_to_bytes_be(hs[0]) + ora.fr_to_bytes_be(hs[1]))
        r = t.evaluate_challenge_into_field()
        rps.append(hs)
        chs.append(r)
        cur = ora.mle_partial_evaluation(cur, r, 0, mt=len(cur) >= 1 << 16)
    return np.array(rps, dtype=np.uint64).reshape(-1, 2, 4), np.array(chs, dtype=np.uint64).reshape(-1, 4)


def to_int(row):
    """the 256-bit STORED value of one row"""
    return sum(int(l) << (64 * i) for i, l in enumerate(row))


def canonical(table):
    """stored limbs [n, 4] -> canonical python ints"""
    rinv = pow(MONT, -1, R)
    return [to_int(row) * rinv % R for row in np.asarray(table, dtype=np.uint64).reshape(-1, 4)]
