"""The tables of one GKR layer's sumcheck in the linear-time form (gkr.hip, "a layer's sumcheck in time linear in its width"; the entry
points zkhip_gkr_layer_tables / zkhip_gkr_layer_tables_sharded) restated on Python integers, and the cases the suites run them at.

Field elements are Python ints mod r.  Nothing here imports numpy arithmetic on field values, the oracle or the library under test: the
model is pinned by tests/test_gkr_table_cases_cpu.py against the oracle's DENSE wiring tables (layers 1-3) and against the layer's claim
(every layer of the case list), and tests/test_gpu_gkr_layer_tables.py holds the kernels to it, limb for limb.

A layer is [(type, in0, in1)] with type "add" | "mul"; layer l of a circuit has 2^l gates over the 2^(l+1) values V below it.
  weights   w_g = alpha eq_g(r_b) + beta eq_g(r_c), eq over max(l, 1) index bits, MSB first; with r_c None (the first layer's proof)
            w_g = eq_g(r_b): alpha and beta are NOT applied (include/zkhip.h: "ignored when h_rc is NULL")
  phase 0   Ha0[x] = sum_{add, in0 = x} w_g    Ha1[x] = sum_{add, in0 = x} w_g V[in1]    Hm[x] = sum_{mul, in0 = x} w_g V[in1]
  phase 1   eq_x(u) over l + 1 bits, V(u) = sum_x eq_x(u) V[x],  Aa[c] = sum_{add, in1 = c} w_g eq_{in0}(u),  Am[c] likewise over mul,
            T1[c] = V(u) + V[c],  T2[c] = V(u) V[c]
  shard     entry j of every output of rank `rank` of `world` is row j * world + rank"""
import collections
import functools
import random

import tables as T
from gkr_cases import A, M, random_circuit, scrambled_circuit

R = T.R


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def eq_table(pts):
    """eq_x(pts) for all x < 2^len(pts); pts[0] goes with the MOST significant bit of x"""
    t = [1]
    for p in pts:
        q = (1 - p) % R
        t = [e * f % R for e in t for f in (q, p)]
    return t


def gate_weights(layer, n_gates, r_b, r_c, alpha, beta):
    n = max(layer, 1)
    assert len(r_b) == n and (r_c is None or len(r_c) == n) and n_gates <= 1 << n
    eb = eq_table(r_b)
    if r_c is None:
        return eb[:n_gates]                                   # one point: alpha and beta are ignored
    ec = eq_table(r_c)
    return [(alpha * eb[g] + beta * ec[g]) % R for g in range(n_gates)]


def phase0(gates, V, w):
    """-> Ha0, Ha1, Hm (len(V) entries each)"""
    ha0, ha1, hm = ([0] * len(V) for _ in range(3))
    for g, (t, i0, i1) in enumerate(gates):
        if t == A:
            ha0[i0] = (ha0[i0] + w[g]) % R
            ha1[i0] = (ha1[i0] + w[g] * V[i1]) % R
        else:
            hm[i0] = (hm[i0] + w[g] * V[i1]) % R
    return ha0, ha1, hm


def phase1(gates, V, w, u):
    """-> V(u), Aa, T1, Am, T2"""
    assert 1 << len(u) == len(V)
    eq_u = eq_table(u)
    vu = sum(e * v for e, v in zip(eq_u, V)) % R
    aa, am = [0] * len(V), [0] * len(V)
    for g, (t, i0, i1) in enumerate(gates):
        out = aa if t == A else am
        out[i1] = (out[i1] + w[g] * eq_u[i0]) % R
    return vu, aa, [(vu + v) % R for v in V], am, [vu * v % R for v in V]


def shard(table, world, rank):
    """rows j * world + rank, j = 0 .. len / world"""
    assert len(table) % world == 0 and 0 <= rank < world
    return [table[j * world + rank] for j in range(len(table) // world)]


def limbs(vals):
    """canonical ints -> stored limbs, uint64 [n, 4]: tables.stored of every value, through bytes (a 2^15-entry table in a few ms)"""
    import numpy as np
    raw = b"".join((v % R * T.MONT % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints(table):
    """stored limbs [n, 4] -> canonical ints: tables.canonical, through bytes"""
    import numpy as np
    raw = np.ascontiguousarray(table, dtype=np.uint64).astype("<u8").tobytes()
    rinv = pow(T.MONT, -1, R)
    return [int.from_bytes(raw[o:o + 32], "little") * rinv % R for o in range(0, len(raw), 32)]


# ---- circuits -------------------------------------------------------------------------------------------------------------------------
DEPTH = 15                                     # layers 0 .. 14: the widest table has 2^15 entries
MAX_ENTRIES = 1 << 15
CIRCUITS = ["random", "scrambled", "identity", "fan_in0", "fan_in1", "all_add", "all_mul", "b_eq_c"]
LAYERS = [0, 1, 2, 5, 11, 12, 13, 14]
#  0: one gate, one point of one coordinate         1: one gate variable, two points            2, 5: small layers
# 11: eq(u) over 12 bits in the chain form, <eq, V> from several workgroups + the finish kernel
# 12: weights over 12 bits in the chain form, eq(u) over 13 bits from halves (n_hi = 1)
# 13: weights from halves, both points scaled (n_hi = 1)                       14: n_hi = 2, the part tables split 1 + 1


@functools.lru_cache(maxsize=None)
def circuit(kind, depth=DEPTH):
    """a full circuit (layer l: 2^l gates over 2^(l+1) values), as a tuple of tuples of (type, in0, in1)"""
    if kind == "random":
        layers = random_circuit(depth)
    elif kind == "scrambled":
        layers = scrambled_circuit(depth, 4101)
    else:
        rng = random.Random(4200 + CIRCUITS.index(kind))
        layers = []
        for l in range(depth):
            n_in = 2 << l
            layer = []
            for g in range(1 << l):
                t, i0, i1 = rng.choice((A, M)), rng.randrange(n_in), rng.randrange(n_in)
                if kind == "identity":
                    t, i0, i1 = A, g, g                      # Ha0[x] = w_x: the gate weights, entry by entry
                elif kind == "fan_in0":
                    i0 = 0                                   # row 0 of the grouping by in0 holds every gate
                elif kind == "fan_in1":
                    i1 = 0
                elif kind == "all_add":
                    t = A
                elif kind == "all_mul":
                    t = M
                elif kind == "b_eq_c":
                    i1 = i0
                layer.append((t, i0, i1))
            layers.append(layer)
    return tuple(tuple(layer) for layer in layers)


def as_lists(layers):
    return [list(layer) for layer in layers]


def bad_label_circuit():
    """depth 4; one gate of layer 2 labels value 8 of the 8 below it.  -> (layers, the bad layer, a layer above it that is served)"""
    layers = as_lists(circuit("scrambled", 4))
    t, _, i1 = layers[2][1]
    layers[2][1] = (t, 8, i1)
    return layers, 2, 3


# ---- points, weights of the points, values ----------------------------------------------------------------------------------------------
POINTS = ["random", "zeros", "ones", "minus_ones", "mixed", "same"]
AB = ["random", "one_zero", "zero_one", "zero_zero", "minus_ones"]
FILLS = ["evaluation", "random_fr", "zero", "minus_one", "one_hot", "stored_max"]    # evaluation: the layer's values of a random input


def points(family, n, seed):
    """-> (r_b, r_c), n coordinates each.  The edge families put r_b on the edge; r_c is there too for an odd seed, random otherwise."""
    rng = random.Random(7000 + seed)
    rnd = lambda: [rng.randrange(R) for _ in range(n)]   # noqa: E731
    if family == "random":
        return rnd(), rnd()
    if family == "same":
        p = rnd()
        return p, list(p)
    if family == "mixed":
        cyc = lambda off: [(0, 1, R - 1, rng.randrange(R))[(j + off) % 4] for j in range(n)]   # noqa: E731
        return cyc(0), cyc(1)
    edge = {"zeros": 0, "ones": 1, "minus_ones": R - 1}[family]
    return [edge] * n, ([edge] * n if seed % 2 else rnd())


def alpha_beta(kind, seed):
    rng = random.Random(7500 + seed)
    return {"random": (rng.randrange(R), rng.randrange(R)), "one_zero": (1, 0), "zero_one": (0, 1), "zero_zero": (0, 0),
            "minus_ones": (R - 1, R - 1)}[kind]


def input_seed(kind):
    """the seed of random_fr for the 2^DEPTH input values of circuit `kind` (fill "evaluation")"""
    return 7900 + CIRCUITS.index(kind)


def fill_values(fill, n, seed, random_fr):
    """stored limbs [n, 4] of every fill but "evaluation" (which the suites take from the circuit's evaluation)"""
    if fill == "random_fr":
        return random_fr(n, 7700 + seed)
    return T.fill(fill, n, 7700 + seed)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
# one_point: h_rc NULL.  Every case draws its points, alpha / beta and values from `seed`.
Case = collections.namedtuple("Case", "circuit layer points ab fill one_point seed")


def case_id(c):
    return "%d-%s-l%d-%s-%s-%s%s" % (c.seed, c.circuit, c.layer, c.points, c.ab, c.fill, "-one_point" if c.one_point else "")


def case_inputs(c):
    """-> (r_b, r_c or None, alpha, beta) as ints"""
    r_b, r_c = points(c.points, max(c.layer, 1), c.seed)
    alpha, beta = alpha_beta(c.ab, c.seed)
    return r_b, (None if c.one_point else r_c), alpha, beta


def _phase0_cases():
    out = []

    def add(circ, layer, pts, ab, fill, one_point=False):
        out.append(Case(circ, layer, pts, ab, fill, one_point or layer == 0, len(out)))
    q = 0
    # every listed layer on scrambled and identity wiring: random points and one other family, going round
    for circ in ("scrambled", "identity"):
        for layer in LAYERS:
            for pts in ("random", POINTS[1 + q % 5]):
                add(circ, layer, pts, AB[q % 5], FILLS[q % 6])
                q += 1
    # identity exposes the weights entry by entry: every family of points in the chain form, at its widest, and in the halves form
    for layer in (1, 5, 12, 13, 14):
        for pts in POINTS:
            add("identity", layer, pts, "random" if pts != "same" else "minus_ones", "evaluation")
    # every other wiring, on both sides of the threshold between the two weight forms
    for circ in ("random", "fan_in0", "fan_in1", "all_add", "all_mul", "b_eq_c"):
        for layer in (2, 5, 12, 13):
            add(circ, layer, POINTS[q % 6], AB[q % 5], FILLS[q % 6])
            q += 1
    for ab in AB:
        for layer in (1, 5, 13):
            add("scrambled", layer, "random", ab, "evaluation")
    for fill in FILLS:
        for layer in (2, 11, 13):
            add("scrambled", layer, "mixed", "random", fill)
    # one point: alpha and beta must not be applied, whatever they are -- layer 0 (where the prover is), and both weight forms above it
    for pts in ("random", "zeros", "ones", "minus_ones"):
        for ab in ("random", "minus_ones", "zero_zero"):
            add("scrambled", 0, pts, ab, "random_fr")
    for layer in (1, 5, 12, 13):
        add("scrambled", layer, "random", "minus_ones", "evaluation", one_point=True)
        add("identity", layer, "mixed", "zero_zero", "random_fr", one_point=True)
    return out


def _phase1_cases():
    out = []
    q = 0
    # 2, 5: one workgroup.  11: <eq, V> from several workgroups + the finish kernel.  12, 13, 14: eq(u) from halves, n_hi = 1, 2, 3
    for circ, layers in (("scrambled", (1, 2, 5, 11, 12, 13, 14)), ("identity", (2, 11, 12)), ("fan_in1", (2, 5, 11, 12)), ("fan_in0", (5, 12)),
                         ("b_eq_c", (2, 5, 12)), ("all_add", (5, 11)), ("all_mul", (5, 12)), ("random", (2, 11))):
        for layer in layers:
            out.append(Case(circ, layer, POINTS[q % 6], AB[q % 5], ("evaluation", "random_fr")[q % 2], False, 1000 + len(out)))
            q += 1
    out.append(Case("scrambled", 0, "random", "minus_ones", "random_fr", True, 1000 + len(out)))
    return out


PHASE0_CASES = _phase0_cases()
PHASE1_CASES = _phase1_cases()
# (circuit, layer, world): every rank, both phases
SHARD_WORLDS = (2, 4, 8)
SHARD_CASES = [Case(circ, layer, ("random", "mixed", "same")[q % 3], ("random", "minus_ones")[q % 2], ("evaluation", "random_fr")[q % 2], False, 2000 + q)
               for q, (circ, layer) in enumerate((c, l) for c in ("scrambled", "fan_in0", "b_eq_c") for l in (2, 5, 12))]
