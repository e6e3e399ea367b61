"""The integer model of a GKR layer's linear-size sumcheck tables (tests/gkr_table_cases.py) against the CPU oracle: the reference's
DENSE wiring tables folded with the oracle's own partial evaluation (layers 0-3), the layer's claim through the oracle's circuit
evaluation and MLE evaluation (every case the GPU suite runs), the rank-interleaved shards, and the case lists themselves."""
import functools
import random

import numpy as np
import pytest

import gkr_table_cases as G
import tables as T

R = G.R


@functools.lru_cache(maxsize=None)
def _evaluation(kind):
    from oracle import oracle as ora
    return ora.circuit_evaluation(G.as_lists(G.circuit(kind)), ora.random_fr(1 << G.DEPTH, G.input_seed(kind)))


def _values(ora, c):
    """the stored limbs of the case's V, and the layer's output on it by the oracle (2^layer entries)"""
    gates = list(G.circuit(c.circuit)[c.layer])
    if c.fill == "evaluation":
        ev = _evaluation(c.circuit)
        return ev[c.layer + 1], ev[c.layer]
    V = G.fill_values(c.fill, 2 << c.layer, c.seed, ora.random_fr)
    return V, ora.circuit_evaluation([gates], V)[0]


def _mle_at(ora, table, pts):
    return T.canonical(ora.mle_evaluation(table, G.limbs(pts)))[0]


def _fold_front(ora, table, pts):
    """the first len(pts) variables of `table` (stored limbs) bound to pts, by the oracle -> canonical ints"""
    return T.canonical(ora.mle_partial_evaluations(table, G.limbs(pts), [0] * len(pts)))


DENSE = [(kind, layer, pts, ab) for q, (kind, layer) in enumerate((k, l) for k in G.CIRCUITS for l in (0, 1, 2, 3))
         for pts, ab in ((G.POINTS[q % 6], G.AB[q % 5]), ("random", "random"))]


@pytest.mark.parametrize("kind,layer,pts,ab", DENSE, ids=["%s-l%d-%s-%s" % d for d in DENSE])
def test_model_is_the_dense_tables_folded(ora, kind, layer, pts, ab):
    """add~ / mul~ over (a, b, c) (Circuit::add_mult_mle) folded at r_b and r_c over a and combined with alpha, beta is the (b, c) table the
    reference's prover sums over: the model's phase 1 tables are that table folded at u over b, its phase 0 tables that table summed over c
    against the V terms, row by row.  Layer 0 has one point and no alpha (gkr/src/utils.rs:12-56)."""
    layers = G.as_lists(G.circuit(kind, 4))
    gates = layers[layer]
    seed = 300 + 7 * G.CIRCUITS.index(kind) + layer
    s, n_rows = layer + 1, 2 << layer
    r_b, r_c = G.points(pts, max(layer, 1), seed)
    alpha, beta = G.alpha_beta(ab, seed)
    if layer == 0:
        r_c = None
    rng = random.Random(seed)
    V = [rng.randrange(R) for _ in range(n_rows)]
    u = [rng.randrange(R) for _ in range(s)]
    dense = ora.circuit_add_mult_mle(layers, layer)
    bc = []
    for tab in dense:
        at_b = _fold_front(ora, tab, r_b)
        bc.append(at_b if r_c is None else [(alpha * x + beta * y) % R for x, y in zip(at_b, _fold_front(ora, tab, r_c))])
    add_bc, mul_bc = bc
    assert len(add_bc) == n_rows * n_rows
    w = G.gate_weights(layer, len(gates), r_b, r_c, alpha, beta)
    ha0, ha1, hm = G.phase0(gates, V, w)
    vu, aa, t1, am, t2 = G.phase1(gates, V, w, u)
    assert aa == _fold_front(ora, G.limbs(add_bc), u) and am == _fold_front(ora, G.limbs(mul_bc), u)
    assert vu == _mle_at(ora, G.limbs(V), u)
    assert t1 == [(vu + v) % R for v in V] and t2 == [vu * v % R for v in V]
    for b in range(n_rows):
        row_a, row_m = add_bc[b * n_rows:(b + 1) * n_rows], mul_bc[b * n_rows:(b + 1) * n_rows]
        assert sum(a * (V[b] + V[c]) for c, a in enumerate(row_a)) % R == (ha0[b] * V[b] + ha1[b]) % R
        assert sum(m * V[b] * V[c] for c, m in enumerate(row_m)) % R == hm[b] * V[b] % R
        # and term by term
        assert sum(row_a) % R == ha0[b] and sum(a * V[c] for c, a in enumerate(row_a)) % R == ha1[b]
        assert sum(m * V[c] for c, m in enumerate(row_m)) % R == hm[b]


ALL_CASES = G.PHASE0_CASES + G.PHASE1_CASES + G.SHARD_CASES


@pytest.mark.parametrize("c", ALL_CASES, ids=[G.case_id(c) for c in ALL_CASES])
def test_tables_carry_the_layers_claim(ora, c):
    """sum_x Ha0 V + Ha1 + Hm V = alpha V~_out(r_b) + beta V~_out(r_c) (one point: V~_out(r_b)), V_out the oracle's evaluation of the layer on
    V.  The phase 1 tables at an arbitrary u sum to the phase 0 terms folded at u, and over the vertices u of the cube (layers <= 2) to the
    claim again.  The wiring's structure shows in the tables themselves."""
    gates = list(G.circuit(c.circuit)[c.layer])
    r_b, r_c, alpha, beta = G.case_inputs(c)
    V_l, out_l = _values(ora, c)
    assert len(V_l) == 2 << c.layer and len(out_l) == len(gates) == 1 << c.layer
    V = G.ints(V_l)
    w = G.gate_weights(c.layer, len(gates), r_b, r_c, alpha, beta)
    ha0, ha1, hm = G.phase0(gates, V, w)
    if c.layer == 0:
        out_l = np.concatenate([out_l, np.zeros((1, 4), dtype=np.uint64)])      # w_0 = [output, 0] (protocol.rs:30-33)
    claim = _mle_at(ora, out_l, r_b) if r_c is None else (alpha * _mle_at(ora, out_l, r_b) + beta * _mle_at(ora, out_l, r_c)) % R
    assert sum(a * v + l + m * v for a, l, m, v in zip(ha0, ha1, hm, V)) % R == claim
    rng = random.Random(c.seed)
    u = [rng.randrange(R) for _ in range(c.layer + 1)]
    vu, aa, t1, am, t2 = G.phase1(gates, V, w, u)
    assert vu == _mle_at(ora, V_l, u)
    # the rounds over c continue the rounds over b: their total is the (b, c) sum with b bound to u, i.e. the phase 0 terms with every
    # factor folded at u -- Ha0~(u) V(u) + Ha1~(u) + Hm~(u) V(u) -- which is the claim itself once u runs over the cube's vertices
    fold = lambda t: sum(e * x for e, x in zip(G.eq_table(u), t)) % R   # noqa: E731
    assert sum(a * x + m * y for a, x, m, y in zip(aa, t1, am, t2)) % R == (fold(ha0) * vu + fold(ha1) + fold(hm) * vu) % R
    if c.layer <= 2:
        total = 0
        for x in range(2 << c.layer):
            _, aa_x, t1_x, am_x, t2_x = G.phase1(gates, V, w, [(x >> (c.layer - j)) & 1 for j in range(c.layer + 1)])
            total += sum(a * p + m * q for a, p, m, q in zip(aa_x, t1_x, am_x, t2_x))
        assert total % R == claim
    if c.circuit == "identity":
        assert ha0 == w + [0] * len(w) and ha1 == [x * v % R for x, v in zip(w, V)] + [0] * len(w)
    if c.circuit in ("identity", "all_add"):
        assert not any(hm) and not any(am)
    if c.circuit == "all_mul":
        assert not any(ha0) and not any(ha1) and not any(aa)
    if c.circuit == "fan_in0":
        assert not any(ha0[1:]) and not any(ha1[1:]) and not any(hm[1:]) and ha0[0] == sum(x for x, g in zip(w, gates) if g[0] == G.A) % R
    if c.circuit == "fan_in1":
        assert not any(aa[1:]) and not any(am[1:])
    if c.ab == "zero_zero" and r_c is not None:
        assert not any(w) and not any(ha0 + ha1 + hm + aa + am)
    if r_c is not None and c.points == "zeros" and c.ab == "one_zero":
        assert w == [1] + [0] * (len(w) - 1)


def test_one_point_weights_ignore_alpha_and_beta():
    for layer in (0, 1, 5):
        n = max(layer, 1)
        r_b, _ = G.points("random", n, layer)
        w = G.gate_weights(layer, 1 << layer, r_b, None, R - 1, 12345)
        assert w == G.eq_table(r_b)[: 1 << layer] == G.gate_weights(layer, 1 << layer, r_b, None, 1, 0)
        assert w == G.gate_weights(layer, 1 << layer, r_b, [0] * n, 1, 0)       # = the two-point form at (alpha, beta) = (1, 0)


def test_limb_conversions_are_the_table_helpers():
    for kind in ("uniform_r", "top", "stored_max", "limb_edges", "zero", "minus_one", "one_hot"):
        t = T.fill(kind, 33, 9)
        vals = G.ints(t)
        assert vals == T.canonical(t) and np.array_equal(G.limbs(vals), t)
        assert np.array_equal(G.limbs(vals), np.stack([T.stored(v) for v in vals])) and G.limbs(vals).dtype == np.uint64
    assert G.limbs([]).shape == (0, 4) and G.ints(np.zeros((0, 4), dtype=np.uint64)) == []


def test_eq_table_edges():
    assert G.eq_table([0, 0, 0]) == [1] + [0] * 7 and G.eq_table([1, 1, 1]) == [0] * 7 + [1]
    assert G.eq_table([1, 0, 0]) == [0, 0, 0, 0, 1, 0, 0, 0]                     # the first point is the most significant bit
    assert G.eq_table([R - 1] * 2) == [4, R - 2, R - 2, 1]                       # 1 - (r - 1) = 2
    rng = random.Random(5)
    p = [rng.randrange(R) for _ in range(6)]
    assert sum(G.eq_table(p)) % R == 1


@pytest.mark.parametrize("world", G.SHARD_WORLDS)
def test_shards_interleave_back(world):
    c = G.SHARD_CASES[1]
    gates = list(G.circuit(c.circuit)[c.layer])
    r_b, r_c, alpha, beta = G.case_inputs(c)
    rng = random.Random(world)
    V = [rng.randrange(R) for _ in range(2 << c.layer)]
    u = [rng.randrange(R) for _ in range(c.layer + 1)]
    w = G.gate_weights(c.layer, len(gates), r_b, r_c, alpha, beta)
    for table in G.phase0(gates, V, w) + (V,) + G.phase1(gates, V, w, u)[1:]:
        shards = [G.shard(table, world, rank) for rank in range(world)]
        assert all(len(s) == len(table) // world for s in shards)
        back = [None] * len(table)
        for rank, s in enumerate(shards):
            assert s == table[rank::world]
            for j, v in enumerate(s):
                back[j * world + rank] = v
        assert back == table
    assert [len(G.shard(list(range(8)), 8, rank)) for rank in range(8)] == [1] * 8       # w_len == world: one row per rank


def test_case_lists_cover_what_they_name():
    p0 = G.PHASE0_CASES
    assert {c.circuit for c in p0} == set(G.CIRCUITS) and {c.layer for c in p0} == set(G.LAYERS) == {0, 1, 2, 5, 11, 12, 13, 14}
    assert {c.points for c in p0} == set(G.POINTS) and {c.ab for c in p0} == set(G.AB) and {c.fill for c in p0} == set(G.FILLS)
    assert set(G.FILLS) == {"evaluation", "random_fr", "zero", "minus_one", "one_hot", "stored_max"}
    for kind in ("scrambled", "identity"):
        assert {c.layer for c in p0 if c.circuit == kind} == set(G.LAYERS)
    assert all(c.one_point for c in p0 + G.PHASE1_CASES if c.layer == 0)
    assert any(c.one_point and c.layer == 0 and c.ab == "minus_ones" for c in p0)            # the one-point contract for alpha
    assert {c.layer for c in p0 if c.one_point} >= {0, 12, 13}                                # ... in both weight forms
    assert {c.layer for c in G.PHASE1_CASES} >= {2, 5, 11, 12}
    assert {(c.circuit, c.layer) for c in G.SHARD_CASES} == {(k, l) for k in ("scrambled", "fan_in0", "b_eq_c") for l in (2, 5, 12)}
    assert G.SHARD_WORLDS == (2, 4, 8)
    every = p0 + G.PHASE1_CASES + G.SHARD_CASES
    assert all(2 << c.layer <= G.MAX_ENTRIES == 1 << 15 for c in every)
    assert len({c.seed for c in every}) == len(every) and len({G.case_id(c) for c in p0}) == len(p0)
    n_calls = len(p0) + len(G.PHASE1_CASES) + 2 * len(G.SHARD_CASES) * sum(G.SHARD_WORLDS)
    assert 200 <= n_calls <= 600
    for kind in G.CIRCUITS:
        layers = G.circuit(kind)
        assert len(layers) == G.DEPTH and all(len(layer) == 1 << l for l, layer in enumerate(layers))
        assert all(0 <= g[1] < 2 << l and 0 <= g[2] < 2 << l for l, layer in enumerate(layers) for g in layer)
    assert all(g == (G.A, i, i) for layer in G.circuit("identity") for i, g in enumerate(layer))
    assert all(g[1] == 0 for layer in G.circuit("fan_in0") for g in layer) and all(g[2] == 0 for layer in G.circuit("fan_in1") for g in layer)
    assert all(g[1] == g[2] for layer in G.circuit("b_eq_c") for g in layer)
    assert {g[0] for g in G.circuit("b_eq_c")[5]} == {G.A, G.M} == {g[0] for g in G.circuit("fan_in0")[5]}
    assert {g[0] for layer in G.circuit("all_add") for g in layer} == {G.A} and {g[0] for layer in G.circuit("all_mul") for g in layer} == {G.M}
    bad, at, above = G.bad_label_circuit()
    assert any(g[1] >= 2 << at for g in bad[at]) and all(g[1] < 2 << above and g[2] < 2 << above for g in bad[above])
