"""zkhip_gkr_layer_tables / zkhip_gkr_layer_tables_sharded by the raw ABI against the integer model of tests/gkr_table_cases.py (pinned on
the CPU by tests/test_gkr_table_cases_cpu.py), `==` on the stored limbs.  The entry point takes r_b, r_c, alpha and beta BY VALUE: the one
seam where gkr_gate_weights_kernel, gkr_eq_halves_kernel + gkr_eq_expand_kernel (two points, scaled), gkr_gate_rows_kernel (both phases,
rank-interleaved rows), gkr_eq_table_kernel and gkr_dot_finish_kernel run at chosen points -- edge coordinates, r_b == r_c, vanishing
alpha / beta, wirings with one gate type or one row that holds every gate -- which the challenges of a whole proof never give.
Every output is allocated one row longer than it is and prefilled: what lies behind the last row must come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import gkr_table_cases as G

pytestmark = pytest.mark.gpu
PATTERN = 0xA5A5A5A5A5A5A5A5


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Env:
    def __init__(self, zk, ora):
        import torch
        from zk_cryptography_amd import _native as N
        self.zk, self.ora, self.N, self.torch = zk, ora, N, torch
        self.lib = N.lib()
        self.ctx = N.Context.get(torch.cuda.current_device())
        self._circuits, self._evaluations = {}, {}

    def handle(self, kind, layers=None):
        """the device-resident circuit `kind` (layers: a circuit of the caller's own, kept under that name)"""
        if kind not in self._circuits:
            circuit = self.zk.Circuit.from_tuples(layers if layers is not None else G.as_lists(G.circuit(kind)))
            self._circuits[kind] = (circuit, self.zk.GKRProtocol._device_circuit(circuit, self.ctx))
        return self._circuits[kind][1].handle

    def values(self, c):
        """stored limbs [2^(layer+1), 4] of the case's V"""
        if c.fill != "evaluation":
            return G.fill_values(c.fill, 2 << c.layer, c.seed, self.ora.random_fr)
        if c.circuit not in self._evaluations:
            self.handle(c.circuit)
            ev = self._circuits[c.circuit][0].evaluation(self.ora.random_fr(1 << G.DEPTH, G.input_seed(c.circuit)))
            self._evaluations[c.circuit] = [t.cpu().numpy().view(np.uint64) for t in ev]
        return self._evaluations[c.circuit][c.layer + 1]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

    def tables(self, handle, layer, d_w, w_len, r_b, r_c, alpha, beta, phase, world=1, rank=0, plain=False, rows=None, null=(), with_wu=None):
        """One call -> (status, the four outputs as uint64 [rows + 1, 4], h_wu as uint64 [4]).  plain: zkhip_gkr_layer_tables (world 1).
        null: the names of arguments passed as NULL."""
        rows = w_len // max(world, 1) if rows is None else rows
        fill = int(np.uint64(PATTERN).view(np.int64))
        outs = [self.torch.full((rows + 1, 4), fill, dtype=self.torch.int64, device="cuda") for _ in range(4)]
        wu = np.full(4, PATTERN, dtype=np.uint64)
        optrs = (C.c_void_p * 4)(*[t.data_ptr() for t in outs])
        rb, al, be = G.limbs(r_b), G.limbs([alpha]), G.limbs([beta])
        rc = G.limbs(r_c) if r_c is not None else None
        pick = lambda name, v: None if name in null else v   # noqa: E731
        if with_wu is None:
            with_wu = phase == 1
        args = [handle, C.c_uint32(layer), pick("d_w", C.c_void_p(d_w.data_ptr())), C.c_size_t(w_len), pick("h_rb", _vp(rb)),
                None if rc is None else _vp(rc), pick("h_alpha", _vp(al)), pick("h_beta", _vp(be)), C.c_int(phase)]
        tail = [pick("d_out", optrs), _vp(wu) if with_wu else None]
        if plain:
            assert world == 1 and rank == 0
            st = self.lib.zkhip_gkr_layer_tables(*args, *tail)
        else:
            st = self.lib.zkhip_gkr_layer_tables_sharded(*args, C.c_uint32(world), C.c_uint32(rank), *tail)
        return st, [t.cpu().numpy().view(np.uint64) for t in outs], wu

    def challenges_of_the_rounds_over_b(self, ha0, V_l, hm):
        """MultiComposedSumcheckProver.prove_partial on [Ha0, V], [Hm, V]: a proof that continues no other records its challenges at the
        head of the context's challenge buffer (composed.hip: ZK_SMALL_CHALLENGES, out_base 0), where phase 1 reads them -> u as ints"""
        zk = self.zk
        V = [zk.Multilinear(V_l), zk.Multilinear(V_l)]
        poly = [zk.ComposedMultilinear([zk.Multilinear(G.limbs(ha0)), V[0]]), zk.ComposedMultilinear([zk.Multilinear(G.limbs(hm)), V[1]])]
        Vi = G.ints(V_l)
        claimed = sum((a + m) * v for a, m, v in zip(ha0, hm, Vi)) % G.R
        _, ch = zk.MultiComposedSumcheckProver.prove_partial(poly, G.limbs([claimed])[0])
        assert ch.shape == (len(Vi).bit_length() - 1, 4)
        return G.ints(ch)


@pytest.fixture(scope="module")
def env(ora):
    import zk_cryptography_amd as zk
    return _Env(zk, ora)


@functools.lru_cache(maxsize=None)
def _untouched(rows):
    return np.full((rows, 4), PATTERN, dtype=np.uint64)


def _model(env, c):
    gates = G.circuit(c.circuit)[c.layer]
    V_l = env.values(c)
    assert V_l.shape == (2 << c.layer, 4)
    V = G.ints(V_l)
    r_b, r_c, alpha, beta = G.case_inputs(c)
    w = G.gate_weights(c.layer, len(gates), r_b, r_c, alpha, beta)
    return gates, V_l, V, (r_b, r_c, alpha, beta), w


@pytest.mark.parametrize("c", G.PHASE0_CASES, ids=[G.case_id(c) for c in G.PHASE0_CASES])
def test_phase0_tables_are_the_models(env, c):
    """Ha0, Ha1, Hm of the whole layer.  One point (h_rc NULL): the weights are eq_g(r_b) whatever h_alpha and h_beta hold."""
    gates, V_l, V, inputs, w = _model(env, c)
    want = G.phase0(gates, V, w)
    n = len(V)
    st, outs, _ = env.tables(env.handle(c.circuit), c.layer, env.dev(V_l), n, *inputs, 0, plain=c.seed % 2 == 0)
    assert st == env.N.ZKHIP_OK
    for name, got, exp in zip(("Ha0", "Ha1", "Hm"), outs, want):
        assert np.array_equal(got[:n], G.limbs(exp)), name
        assert np.array_equal(got[n:], _untouched(1)), name + ": the row behind the table"
    assert np.array_equal(outs[3], _untouched(n + 1))             # d_out[3] is the shard of V: not written at world 1
    if c.circuit in ("identity", "all_add"):
        assert not outs[2][:n].any()                              # exact zeros, not merely the model's
    if c.circuit == "all_mul":
        assert not outs[0][:n].any() and not outs[1][:n].any()
    if c.circuit == "identity":
        assert np.array_equal(outs[0][: n // 2], G.limbs(w))      # the gate weights themselves, entry by entry


@pytest.mark.parametrize("c", G.PHASE1_CASES, ids=[G.case_id(c) for c in G.PHASE1_CASES])
def test_phase1_tables_are_the_models(env, c):
    """After the rounds over b of the layer's own claim: h_wu = V(u) at the challenges that proof RETURNED (so those are the ones read),
    Aa, V(u) + V, Am, V(u) V."""
    gates, V_l, V, inputs, w = _model(env, c)
    ha0, _, hm = G.phase0(gates, V, w)
    u = env.challenges_of_the_rounds_over_b(ha0, V_l, hm)
    vu, aa, t1, am, t2 = G.phase1(gates, V, w, u)
    n = len(V)
    st, outs, wu = env.tables(env.handle(c.circuit), c.layer, env.dev(V_l), n, *inputs, 1, plain=c.seed % 2 == 0)
    assert st == env.N.ZKHIP_OK
    assert np.array_equal(wu, G.limbs([vu])[0])
    for name, got, exp in zip(("Aa", "T1", "Am", "T2"), outs, (aa, t1, am, t2)):
        assert np.array_equal(got[:n], G.limbs(exp)), name
        assert np.array_equal(got[n:], _untouched(1)), name + ": the row behind the table"
    if c.circuit in ("identity", "all_add"):
        assert not outs[2][:n].any()
    if c.circuit == "all_mul":
        assert not outs[0][:n].any()


@pytest.mark.parametrize("world", G.SHARD_WORLDS)
@pytest.mark.parametrize("c", G.SHARD_CASES, ids=[G.case_id(c) for c in G.SHARD_CASES])
def test_every_rank_builds_its_interleaved_rows(env, c, world):
    """Rows j * world + rank of every table, w_len / world entries per output, for every rank of the world; phase 0 also hands out the
    rank's rows of V.  Uneven rows, one row that holds every gate, b == c.  At w_len == world every rank builds one row."""
    gates, V_l, V, inputs, w = _model(env, c)
    n = len(V)
    rows = n // world
    assert rows >= 1
    ha0, ha1, hm = G.phase0(gates, V, w)
    handle, d_w = env.handle(c.circuit), env.dev(V_l)
    u = env.challenges_of_the_rounds_over_b(ha0, V_l, hm)
    vu, aa, t1, am, t2 = G.phase1(gates, V, w, u)
    for rank in range(world):
        st, outs, _ = env.tables(handle, c.layer, d_w, n, *inputs, 0, world, rank)
        assert st == env.N.ZKHIP_OK
        for name, got, exp in zip(("Ha0", "Ha1", "Hm", "V"), outs, (ha0, ha1, hm, V)):
            assert got.shape == (rows + 1, 4)
            assert np.array_equal(got[:rows], G.limbs(G.shard(exp, world, rank))), (name, rank)
            assert np.array_equal(got[rows:], _untouched(1)), (name, rank)
        st, outs, wu = env.tables(handle, c.layer, d_w, n, *inputs, 1, world, rank)
        assert st == env.N.ZKHIP_OK
        assert np.array_equal(wu, G.limbs([vu])[0]), rank
        for name, got, exp in zip(("Aa", "T1", "Am", "T2"), outs, (aa, t1, am, t2)):
            assert np.array_equal(got[:rows], G.limbs(G.shard(exp, world, rank))), (name, rank)
            assert np.array_equal(got[rows:], _untouched(1)), (name, rank)


def test_refusals_write_nothing(env, ora):
    """Every refused call leaves the four outputs and h_wu as they were."""
    N = env.N
    layer, n = 5, 64
    handle = env.handle("scrambled")
    c = G.Case("scrambled", layer, "random", "random", "random_fr", False, 3000)
    V_l = G.fill_values("random_fr", 2 * n, c.seed, ora.random_fr)          # long enough for the doubled length
    d_w = env.dev(V_l)
    inputs = G.case_inputs(c)

    def refused(want, layer=layer, w_len=n, phase=0, world=1, rank=0, plain=False, **kw):
        st, outs, wu = env.tables(handle, layer, d_w, w_len, *inputs, phase, world, rank, plain=plain, rows=2 * n, **kw)
        assert st == want, (st, want, layer, w_len, phase, world, rank, kw)
        assert all(np.array_equal(o, _untouched(2 * n + 1)) for o in outs) and np.array_equal(wu, np.full(4, PATTERN, dtype=np.uint64))

    for phase in (0, 1):
        for world in (0, 3, 6):
            refused(N.ERR_ARG, phase=phase, world=world)
        for world in (1, 2, 8):
            refused(N.ERR_ARG, phase=phase, world=world, rank=world)
        refused(N.ERR_SHAPE, phase=phase, world=128)                        # world > w_len
        refused(N.ERR_SHAPE, phase=phase, layer=2, w_len=8, world=16)
        for plain in (False, True):
            refused(N.ERR_ARG, phase=phase, layer=G.DEPTH, plain=plain)     # layer == n_layers
            refused(N.ERR_SHAPE, phase=phase, w_len=n // 2, plain=plain)
            refused(N.ERR_SHAPE, phase=phase, w_len=2 * n, plain=plain)
            for name in ("d_w", "h_rb", "h_alpha", "h_beta", "d_out"):
                refused(N.ERR_ARG, phase=phase, plain=plain, null=(name,))
    for plain in (False, True):
        refused(N.ERR_ARG, phase=2, plain=plain, with_wu=True)
        refused(N.ERR_ARG, phase=-1, plain=plain, with_wu=True)
        refused(N.ERR_ARG, phase=1, plain=plain, with_wu=False)             # phase 1 has to say where V(u) goes
    # the call itself is good: served with the very arguments the refusals varied
    gates = G.circuit("scrambled")[layer]
    V = G.ints(V_l[:n])
    want = G.phase0(gates, V, G.gate_weights(layer, len(gates), *inputs))
    st, outs, _ = env.tables(handle, layer, d_w, n, *inputs, 0)
    assert st == N.ZKHIP_OK and all(np.array_equal(o[:n], G.limbs(e)) for o, e in zip(outs, want))


def test_a_label_out_of_range_refuses_its_layer_only(env, ora):
    """zkhip_circuit_create accepts the circuit; the layer with the label is ZKHIP_ERR_INDEX in both phases, nothing written, and a layer
    above it is served."""
    N = env.N
    layers, bad, good = G.bad_label_circuit()
    handle = env.handle("bad_label", layers)
    for layer in (bad, good):
        n = 2 << layer
        V_l = ora.random_fr(n, 3100 + layer)
        r_b, r_c = G.points("random", layer, 3100)
        alpha, beta = G.alpha_beta("random", 3100)
        if layer == good:
            V = G.ints(V_l)
            w = G.gate_weights(layer, len(layers[layer]), r_b, r_c, alpha, beta)
            want = G.phase0(layers[layer], V, w)
            want1 = G.phase1(layers[layer], V, w, env.challenges_of_the_rounds_over_b(want[0], V_l, want[2]))
        for phase in (0, 1):
            for world, rank in ((1, 0), (2, 1)):
                st, outs, wu = env.tables(handle, layer, env.dev(V_l), n, r_b, r_c, alpha, beta, phase, world, rank)
                if layer == bad:
                    assert st == N.ERR_INDEX
                    assert all(np.array_equal(o, _untouched(n // world + 1)) for o in outs) and np.array_equal(wu, np.full(4, PATTERN, dtype=np.uint64))
                else:
                    assert st == N.ZKHIP_OK
                    assert phase == 0 or np.array_equal(wu, G.limbs(want1[:1])[0])
                    assert all(np.array_equal(o[: n // world], G.limbs(G.shard(e, world, rank))) for o, e in zip(outs, want if phase == 0 else want1[1:]))
