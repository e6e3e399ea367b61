"""GPU parity: circuit evaluation, wiring tables and GKRProtocol::prove vs the CPU oracle's restatement
(oracle/gkr.c, pinned by the reference's circuit / GKR tests); names follow circuit/src/circuit.rs and
gkr/src/protocol.rs tests.  The GPU proof must be bit-identical to the oracle's and pass its restated verifier."""
import numpy as np
import pytest

from gkr_cases import CIRCUIT_2, CIRCUIT_3, GKR_1, GKR_2, gkr_proof_mismatches, random_circuit, scrambled_circuit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("case", [GKR_1, CIRCUIT_2, CIRCUIT_3])
def test_circuit_evaluation(zk, case):   # circuit.rs:139-260
    ev = zk.Circuit.from_tuples(case["layers"]).evaluation(zk.Fr.from_ints(case["input"]))
    assert [zk.Fr.to_ints(_host(e)) for e in ev] == case["evaluation"]


def test_circuit_evaluation_index_panic(zk):
    with pytest.raises(IndexError):
        zk.Circuit.from_tuples([[("add", 0, 4)]]).evaluation(zk.Fr.from_ints([1, 2, 3, 4]))


@pytest.mark.parametrize("layer_index", [0, 1, 2])
def test_get_add_n_mul_mle(zk, ora, layer_index):   # circuit.rs:262-518
    c = zk.Circuit.from_tuples(CIRCUIT_3["layers"])
    add, mul = c.add_mult_mle(layer_index)
    want_add, want_mul = ora.circuit_add_mult_mle(CIRCUIT_3["layers"], layer_index)
    assert np.array_equal(_host(add.evaluations), want_add) and np.array_equal(_host(mul.evaluations), want_mul)
    assert add.n_vars == [3, 5, 8][layer_index]
    if layer_index == 1:
        assert zk.Fr.to_ints(mul.evaluation(zk.Fr.from_ints([1, 1, 0, 1, 1]))) == [1]
        assert zk.Fr.to_ints(add.evaluation(zk.Fr.from_ints([0, 0, 0, 0, 1]))) == [1]


def _to_oracle_proof(zk, ora, proof):
    p = ora.GkrProof()
    p.n_proofs = len(proof.sumcheck_proofs)
    for k, sp in enumerate(proof.sumcheck_proofs):
        p.sums[4 * k:4 * k + 4] = [int(v) for v in sp.sum]
        p.n_rounds[k] = len(sp.round_polys)
        for r, rp in enumerate(sp.round_polys):
            s = p.round_polys[k][r]
            s.len = len(rp.coeffs)
            for m in range(len(rp.coeffs)):
                s.coeff[4 * m:4 * m + 4] = [int(v) for v in rp.coeffs[m]]
                s.pow[4 * m:4 * m + 4] = [int(v) for v in rp.pows[m]]
        p.wb[4 * k:4 * k + 4] = [int(v) for v in proof.wb_s[k]]
        p.wc[4 * k:4 * k + 4] = [int(v) for v in proof.wc_s[k]]
    p.w0[0:8] = [int(v) for v in _host(proof.w_0_mle.evaluations).reshape(-1)]
    return p


def _check_against_oracle(zk, ora, layers, inp):
    circuit = zk.Circuit.from_tuples(layers)
    ev = circuit.evaluation(inp)
    want_ev = ora.circuit_evaluation(layers, inp)
    assert all(np.array_equal(_host(a), b) for a, b in zip(ev, want_ev))
    proof = zk.GKRProtocol.prove(circuit, ev)
    step = zk.GKRProtocol.prove_stepwise(circuit, ev)          # same prover, one mirror call per reference line
    assert [sp.to_bytes() for sp in step.sumcheck_proofs] == [sp.to_bytes() for sp in proof.sumcheck_proofs]
    assert all(np.array_equal(a, b) for a, b in zip(step.wb_s + step.wc_s, proof.wb_s + proof.wc_s))
    want = ora.gkr_prove(layers, want_ev)
    assert len(proof.sumcheck_proofs) == want.n_proofs == len(layers)
    for k, sp in enumerate(proof.sumcheck_proofs):
        w_sum, w_rps, w_wb, w_wc = want.layer(k)
        assert np.array_equal(sp.sum, w_sum)
        assert sp.to_bytes() == ora.multi_composed_proof_bytes(w_rps)
        assert np.array_equal(proof.wb_s[k], w_wb) and np.array_equal(proof.wc_s[k], w_wc)
    assert gkr_proof_mismatches(ora, proof, want) == []
    assert gkr_proof_mismatches(ora, proof, ora.gkr_prove_sparse(layers, want_ev)) == []
    assert ora.gkr_verify(layers, inp, _to_oracle_proof(zk, ora, proof))
    return proof


def test_gkr_protocol_1(zk, ora):   # protocol.rs:209-232
    _check_against_oracle(zk, ora, GKR_1["layers"], zk.Fr.from_ints(GKR_1["input"]))


def test_gkr_protocol_2(zk, ora):   # protocol.rs:234-286
    circuit = zk.Circuit.from_tuples(GKR_2["layers"])
    ev = circuit.evaluation(zk.Fr.from_ints(GKR_2["input"]))
    assert zk.Fr.to_ints(_host(ev[0])) == [224]
    proof = _check_against_oracle(zk, ora, GKR_2["layers"], zk.Fr.from_ints(GKR_2["input"]))
    bad = list(GKR_2["input"]); bad[3] += 1
    assert not ora.gkr_verify(GKR_2["layers"], zk.Fr.from_ints(bad), _to_oracle_proof(zk, ora, proof))


def test_gkr_shape_panics(zk):
    circuit = zk.Circuit.from_tuples(CIRCUIT_2["layers"])       # two output gates: w_0 would have 3 entries
    with pytest.raises(AssertionError):
        zk.GKRProtocol.prove(circuit, circuit.evaluation(zk.Fr.from_ints(CIRCUIT_2["input"])))


@pytest.mark.parametrize("depth", [3, 6, 8])   # 8: wiring tables of 2^23 entries, the largest the dense representation allows in practice
def test_gkr_random_circuit(zk, ora, depth):   # Circuit::random (circuit.rs:99-122), gkr/benches
    _check_against_oracle(zk, ora, random_circuit(depth), ora.random_fr(2 ** depth, 40 + depth))


@pytest.mark.parametrize("layers,inp,tau", [
    (GKR_1["layers"], GKR_1["input"], [54, 90]),                       # succint_protocol.rs:282-306 (test_succint_gkr_protocol_1)
    (random_circuit(3), [4, 3, 7, 6, 6, 1, 2, 5], [5, 6, 7, 8, 9]),    # SRS larger than the input layer: add_to_back blow-up
])
def test_succint_gkr_prove(zk, ora, layers, inp, tau):
    """SuccintGKRProtocol::prove: GKR proof + commitment to the input layer (blown up to the SRS size) + openings at
    the last layer's b and c.  The pairing verifier is out of scope; the commitment and both openings are compared with
    the oracle's naive restatements, the opened values with w_b / w_c, and the sumcheck part with the oracle's verifier."""
    circuit = zk.Circuit.from_tuples(layers)
    inp_f, tau_f = zk.Fr.from_ints(inp), zk.Fr.from_ints(tau)
    ev = circuit.evaluation(inp_f)
    srs = zk.TrustedSetup.setup(tau_f)
    commitment, proof = zk.SuccintGKRProtocol.prove(circuit, ev, srs)
    assert ora.gkr_verify(layers, inp_f, _to_oracle_proof(zk, ora, proof))
    blow = len(tau) - (len(inp).bit_length() - 1)
    poly = ora.mle_add_to_back(inp_f, blow)
    osrs = ora.kzg_multilinear_srs_g1(tau_f)
    want_c = ora.g1_to_affine(ora.kzg_commitment(poly, osrs, True))
    assert np.array_equal(commitment.xy, want_c[:12]) and commitment.infinity == bool(want_c[12])
    ch = proof._challenges[-1]
    half = len(ch) // 2
    for pts, opening, w_val in ((ch[:half], proof.proof_wb_opening, proof.wb_s[-1]), (ch[half:], proof.proof_wc_opening, proof.wc_s[-1])):
        z = np.concatenate([pts, np.zeros((len(tau) - len(pts), 4), dtype=np.uint64)])
        want_ev, want_proofs = ora.kzg_open(poly, z, osrs)
        assert np.array_equal(opening.evaluation, want_ev) and np.array_equal(opening.evaluation, w_val)
        for got, want in zip(opening.proofs, want_proofs):
            a = ora.g1_to_affine(want)
            assert got.infinity == bool(a[12]) and (got.infinity or np.array_equal(got.xy, a[:12]))


@pytest.mark.parametrize("depth", [10, 11, 16])
def test_gkr_beyond_the_dense_tables(zk, ora, depth):
    """zkhip_gkr_prove builds neither the dense 2^(3l+2)-entry wiring tables nor the dense 2^(2l+2)-entry (b, c) tables of
    the layer sumchecks (depth 16: 2^47 and 2^32 entries): every table is as wide as the layer.  No dense prover exists to
    compare with at these depths (depth <= 8 is compared bit for bit above); the proof must pass the restated verifier
    (whose own checks of the wiring stop at layer one, as in gkr/src/protocol.rs:119-196) and a wrong input must fail it."""
    layers = random_circuit(depth)
    inp = ora.random_fr(2 ** depth, 60 + depth)
    circuit = zk.Circuit.from_tuples(layers)
    ev = circuit.evaluation(inp)
    want_ev = ora.circuit_evaluation(layers, inp)
    assert all(np.array_equal(_host(a), b) for a, b in zip(ev, want_ev))
    proof = zk.GKRProtocol.prove(circuit, ev)
    assert len(proof.sumcheck_proofs) == depth and len(proof.sumcheck_proofs[-1].round_polys) == 2 * depth
    op = _to_oracle_proof(zk, ora, proof)
    assert ora.gkr_verify(layers, inp, op)
    bad = inp.copy()
    bad[5, 0] ^= np.uint64(1)
    assert not ora.gkr_verify(layers, bad, op)


@pytest.mark.parametrize("depth", [9, 10, 12, 13, 16])
def test_gkr_bit_exact_beyond_the_dense_tables(zk, ora, depth):
    """Bit for bit against the reference's layer prover restated on sparse containers (oracle/gkr_sparse.c: the (b, c)-table
    prover of protocol.rs:61-108 / multi_composed_sumcheck.rs:64-121 in O(gates) per round, pinned on the dense restatement at
    every depth that one reaches).  At these depths the layers' sumchecks run through the mid-size kernels in their GKR role
    (rounds one ahead of the transcript, two-round stages, additive table, continued transcript) -- which the restated verifier
    cannot see: gkr/src/protocol.rs:154-181 never checks a layer's final claim against the wiring for layers >= 2.
    Depth 20 (BASELINE configs[3]): tests/test_gpu_baseline_sizes.py."""
    layers = random_circuit(depth)
    inp = ora.random_fr(2 ** depth, 60 + depth)
    circuit = zk.Circuit.from_tuples(layers)
    ev = circuit.evaluation(inp)
    want_ev = ora.circuit_evaluation(layers, inp)
    want = ora.gkr_prove_sparse(layers, want_ev)
    assert gkr_proof_mismatches(ora, zk.GKRProtocol.prove(circuit, ev), want) == []
    if depth in (9, 12, 16):
        for stages in (False, True):                              # the sharded prover's sessions, one rank
            assert gkr_proof_mismatches(ora, zk.GKRProtocol.prove_sharded(circuit, ev, use_stages=stages), want) == []


@pytest.mark.parametrize("depth,seed", [(4, 11), (7, 12), (10, 13), (12, 14), (14, 15)])
def test_gkr_bit_exact_scrambled_wiring(zk, ora, depth, seed):
    """Gate types mixed inside a layer, inputs shared between gates, b == c, unused inputs (Circuit::random has none of these):
    CSR rows of uneven length, both product terms live in every layer, zero coefficients that must be dropped per term."""
    layers = scrambled_circuit(depth, seed)
    inp = ora.random_fr(2 ** depth, 900 + seed)
    if seed % 2:
        inp[1] = 0
    circuit = zk.Circuit.from_tuples(layers)
    ev = circuit.evaluation(inp)
    want_ev = ora.circuit_evaluation(layers, inp)
    assert all(np.array_equal(_host(a), b) for a, b in zip(ev, want_ev))
    want = ora.gkr_prove_sparse(layers, want_ev)
    assert gkr_proof_mismatches(ora, zk.GKRProtocol.prove(circuit, ev), want) == []
    assert gkr_proof_mismatches(ora, zk.GKRProtocol.prove_sharded(circuit, ev, use_stages=True), want) == []
    assert ora.gkr_verify(layers, inp, want)


def test_gkr_device_circuit_reused_across_inputs(zk, ora):
    """One Circuit, several inputs: the device-resident circuit (zkhip_circuit_create) is built on the first proof and reused;
    every proof must still be the oracle's for its input.  A bad gate label surfaces when the prover reaches its layer."""
    layers = random_circuit(6)
    circuit = zk.Circuit.from_tuples(layers)
    handles = []
    for seed in (1, 2, 3):
        inp = ora.random_fr(2 ** 6, 700 + seed)
        ev = circuit.evaluation(inp)
        proof = zk.GKRProtocol.prove(circuit, ev)
        handles.append(circuit._device.handle.value)
        want = ora.gkr_prove(layers, ora.circuit_evaluation(layers, inp))
        for k, sp in enumerate(proof.sumcheck_proofs):
            w_sum, w_rps, w_wb, w_wc = want.layer(k)
            assert np.array_equal(sp.sum, w_sum) and sp.to_bytes() == ora.multi_composed_proof_bytes(w_rps)
            assert np.array_equal(proof.wb_s[k], w_wb) and np.array_equal(proof.wc_s[k], w_wc)
        assert ora.gkr_verify(layers, inp, _to_oracle_proof(zk, ora, proof))
    assert len(set(handles)) == 1
    # an out-of-range label in layer 2 (inputs of layer 2 label 8 values): the reference indexes out of bounds there
    bad = [list(layer) for layer in random_circuit(3)]
    g = bad[2][1]
    bad[2][1] = (g[0], 8, g[2])
    ok = zk.Circuit.from_tuples(random_circuit(3))
    ev = ok.evaluation(ora.random_fr(8, 9))
    with pytest.raises(IndexError):
        zk.GKRProtocol.prove(zk.Circuit.from_tuples(bad), ev)


@pytest.mark.parametrize("stages", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 4, 8, 12])
def test_gkr_prove_sharded_world_1_matches_prove(zk, ora, depth, stages):
    """The sharded prover's code path (zkhip_gkr_prove_sharded: the layer tables from the builder behind zkhip_gkr_layer_tables_sharded,
    enqueued inside the library, the rounds over b and over c as two zkhip_mc_* sessions with an additive table and a continued
    transcript) on one rank: the proof must be zkhip_gkr_prove's, bit for bit.  The public table entry points themselves are held to an
    integer model in tests/test_gpu_gkr_layer_tables.py."""
    layers = random_circuit(depth)
    circuit = zk.Circuit.from_tuples(layers)
    inp = ora.random_fr(2 ** depth, 800 + depth)
    ev = circuit.evaluation(inp)
    want = zk.GKRProtocol.prove(circuit, ev)
    got = zk.GKRProtocol.prove_sharded(circuit, ev, use_stages=stages)      # stages: two rounds per exchange (zkhip_mc_stage_*)
    assert len(got.sumcheck_proofs) == depth
    for a, b in zip(got.sumcheck_proofs, want.sumcheck_proofs):
        assert np.array_equal(a.sum, b.sum) and a.to_bytes() == b.to_bytes()
    assert all(np.array_equal(a, b) for a, b in zip(got.wb_s, want.wb_s))
    assert all(np.array_equal(a, b) for a, b in zip(got.wc_s, want.wc_s))
    assert np.array_equal(_host(got.w_0_mle.evaluations), _host(want.w_0_mle.evaluations))
    if 3 <= depth <= 8:
        assert ora.gkr_verify(layers, inp, _to_oracle_proof(zk, ora, got))


def test_gate_replaced_in_place_proves_the_edited_circuit(zk, ora):
    """The reference reads &Circuit on every call (gkr/src/protocol.rs:21-25); the mirror keeps the circuit resident in HBM.  Gates are
    immutable and a layer's gate list counts its mutations, so a gate REPLACED in place (same shape) reaches the device copy: the next
    proof is the edited circuit's, for both provers."""
    depth = 6
    circuit = zk.Circuit.random(depth)
    inp = ora.random_fr(2 ** depth, 4400)
    before = zk.GKRProtocol.prove(circuit, circuit.evaluation(inp))
    with pytest.raises(AttributeError):
        circuit.layers[3].layer[2].inputs = (0, 0)                        # no silent in-place edits of a gate
    old = circuit.layers[3].layer[2]
    circuit.layers[3].layer[2] = zk.Gate("mul" if old.gate_type == "add" else "add", (old.inputs[1], old.inputs[0]))
    ev = circuit.evaluation(inp)
    after = zk.GKRProtocol.prove(circuit, ev)
    fresh_layers = [[(g.gate_type, g.inputs[0], g.inputs[1]) for g in layer.layer] for layer in circuit.layers]
    fresh = zk.Circuit.from_tuples(fresh_layers)
    want = zk.GKRProtocol.prove(fresh, fresh.evaluation(inp))
    assert [p.to_bytes() for p in after.sumcheck_proofs] == [p.to_bytes() for p in want.sumcheck_proofs]
    assert [p.to_bytes() for p in after.sumcheck_proofs] != [p.to_bytes() for p in before.sumcheck_proofs]
    assert ora.gkr_verify(fresh_layers, inp, _to_oracle_proof(zk, ora, after))
    sharded = zk.GKRProtocol.prove_sharded(circuit, ev, use_stages=True)
    assert [p.to_bytes() for p in sharded.sumcheck_proofs] == [p.to_bytes() for p in want.sumcheck_proofs]
    # a whole layer replaced, and appended gates, are seen too
    circuit.layers[2] = zk.CircuitLayer([zk.Gate("add", (g.inputs[1], g.inputs[0])) for g in circuit.layers[2].layer])
    again = zk.GKRProtocol.prove(circuit, circuit.evaluation(inp))
    fresh2 = zk.Circuit.from_tuples([[(g.gate_type, g.inputs[0], g.inputs[1]) for g in layer.layer] for layer in circuit.layers])
    assert [p.to_bytes() for p in again.sumcheck_proofs] == [p.to_bytes() for p in zk.GKRProtocol.prove(fresh2, fresh2.evaluation(inp)).sumcheck_proofs]


def test_gkr_fresh_context_in_a_destroyed_ones_memory(zk, ora):
    """A context is destroyed and the next one -- whose scratch may be the very memory the old one proved in, outer-transcript ring flags
    and all, with session tokens that restart at 1 -- proves ANOTHER input of the same shape: every proof bit-exact and accepted by the
    restated verifier (the flags are cleared per proof; a stale flag equal to the live token would let the hasher absorb the previous
    proof's round items)."""
    from zk_cryptography_amd import _native as N
    for depth in (8, 5):
        layers = random_circuit(depth)
        for seed in range(4):
            _check_against_oracle(zk, ora, layers, ora.random_fr(2 ** depth, 8800 + 10 * depth + seed))
            N.Context.get(0).destroy()                   # the next proof runs on a fresh context (Context.get creates it)
    # an explicitly destroyed context takes its device circuits with it: nothing dereferences the freed context later
    circuit = zk.Circuit.from_tuples(random_circuit(4))
    inp = ora.random_fr(16, 8899)
    zk.GKRProtocol.prove(circuit, circuit.evaluation(inp))
    dev = circuit._device
    N.Context.get(0).destroy()
    assert not dev.alive() and not dev.handle
    del dev
    _check_against_oracle(zk, ora, random_circuit(4), inp)


@pytest.mark.parametrize("depth,n_proofs,lanes", [(6, 5, 0), (9, 16, 8), (12, 3, 2), (4, 1, 0)])
def test_gkr_prove_batch_equals_the_single_proofs(zk, ora, depth, n_proofs, lanes):
    """zkhip_gkr_prove_batch: n independent proofs of one circuit from ONE call (internal lanes; gkr/benches/gkr_benchmark.rs:11-27) -- every
    proof bit-identical to the oracle's and to GKRProtocol.prove's, whatever the number of lanes; a second batch reuses the lanes."""
    layers = random_circuit(depth) if depth != 9 else scrambled_circuit(depth, 77)
    circuit = zk.Circuit.from_tuples(layers)
    inputs = [ora.random_fr(2 ** depth, 9300 + 31 * depth + b) for b in range(n_proofs)]
    evs = [circuit.evaluation(inp) for inp in inputs]
    for rep in range(2):
        proofs = zk.GKRProtocol.prove_batch(circuit, evs, max_lanes=lanes)
        assert len(proofs) == n_proofs
        for inp, ev, proof in zip(inputs, evs, proofs):
            want = ora.gkr_prove_sparse(layers, ora.circuit_evaluation(layers, inp))
            assert gkr_proof_mismatches(ora, proof, want) == []
    single = zk.GKRProtocol.prove(circuit, evs[-1])
    assert [sp.to_bytes() for sp in single.sumcheck_proofs] == [sp.to_bytes() for sp in proofs[-1].sumcheck_proofs]
    assert zk.GKRProtocol.prove_batch(circuit, []) == []


def test_gkr_batch_on_a_warm_lane_checks_the_layer_lengths(zk, ora):
    """zkhip_gkr_prove_batch by the raw ABI, one lane: after three calls the lane replays the circuit's launch chain as a recorded graph,
    which never reaches the per-layer length check of the plain chain.  A fourth call with one h_layer_len halved -- still a power of
    two, but not the circuit's -- must be ZKHIP_ERR_SHAPE before anything is staged, every output untouched, exactly as on a circuit
    the lane has never seen; the lane then proves the right lengths again, bit for bit."""
    import ctypes as C
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd.composed import MAX_MONO
    depth = 5
    layers = random_circuit(depth)
    circuit = zk.Circuit.from_tuples(layers)
    inp = ora.random_fr(2 ** depth, 9700)
    ev = [t.contiguous() for t in circuit.evaluation(inp)]
    ctx = N.Context.get(ev[0].device.index)
    nl, stride = depth, 2 * depth
    ptrs = (C.c_void_p * (nl + 1))(*[t.data_ptr() for t in ev])
    good = [t.shape[0] for t in ev]
    halved = list(good)
    halved[3] //= 2
    F64, F32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(cir, lens):
        out = dict(sums=np.full((nl, 4), F64), n_rounds=np.full(nl, F32), rp_lens=np.full((nl, stride), F32),
                   rps=np.full((nl, stride, MAX_MONO, 2, 4), F64), wb=np.full((nl, 4), F64), wc=np.full((nl, 4), F64), w0=np.full((2, 4), F64),
                   chal=np.full((nl, stride, 4), F64))
        status = np.full(1, 0x5A5A5A5A, dtype=np.int32)
        dev = zk.GKRProtocol._device_circuit(cir, ctx)
        st = N.lib().zkhip_gkr_prove_batch(dev.handle, C.c_uint32(1), C.c_uint32(1), ptrs, (C.c_size_t * (nl + 1))(*lens), vp(out["sums"]), vp(out["n_rounds"]),
                                           vp(out["rp_lens"]), vp(out["rps"]), vp(out["wb"]), vp(out["wc"]), vp(out["w0"]), vp(out["chal"]), vp(status))
        return st, int(status[0]), out

    def untouched(out):
        return all((a == (F32 if a.dtype == np.uint32 else F64)).all() for a in out.values())

    single = zk.GKRProtocol.prove(circuit, ev)
    assert gkr_proof_mismatches(ora, single, ora.gkr_prove(layers, ora.circuit_evaluation(layers, inp))) == []

    def is_the_proof(out):
        return (np.array_equal(out["sums"], np.stack([sp.sum for sp in single.sumcheck_proofs])) and np.array_equal(out["wb"], np.stack(single.wb_s))
                and np.array_equal(out["wc"], np.stack(single.wc_s)) and np.array_equal(out["w0"], _host(single.w_0_mle.evaluations))
                and all(np.array_equal(out["chal"][k, : 2 * (k + 1)], single._challenges[k]) for k in range(nl)))

    for _ in range(3):          # plain chain, recorded chain, replayed graph
        st, own, out = call(circuit, good)
        assert st == N.ZKHIP_OK and own == N.ZKHIP_OK and is_the_proof(out)
    st, own, out = call(circuit, halved)
    assert st == N.ERR_SHAPE and own == N.ERR_SHAPE
    assert untouched(out)
    cold = zk.Circuit.from_tuples(layers)           # a circuit of its own: the lane holds no graph of it
    st, own, out = call(cold, halved)
    assert st == N.ERR_SHAPE and own == N.ERR_SHAPE
    assert untouched(out)
    st, own, out = call(circuit, good)
    assert st == N.ZKHIP_OK and own == N.ZKHIP_OK and is_the_proof(out)
