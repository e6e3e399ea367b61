"""GPU: every entry point of the Python mirror beside proofs, commits and sessions in flight on ONE context (tests/inflight_cases.py
holds the table and runs the cells; include/zkhip.h, "Calls beside work in flight", is the rule).

Per cell: begin the holder; call the other -- it raises ZkhipError with status ZKHIP_ERR_BUSY or returns, bit for bit, what it
returns on an idle context, as the table says; collect the holder -- every proof and commitment is the oracle's; call the other
again on the idle context -- the idle result.  At the end of a holder's test a fresh Sumcheck.prove and a fresh
MultilinearKZG.commitment on the same context are the oracle's.  The idle result of every other call is computed once per module and
held against the oracle (ora.*), tests/plonk_model.py and tests/pairing_model.py there.  No tolerances.

H3 runs in a process of its own (ZKHIP_OVERLAP_MIN_LOG is read once per process): this file as a program."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import inflight_cases as IC  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


@pytest.fixture(scope="module")
def env(zk, ora):
    e = IC.make_env(zk, ora, holders=[h for h in IC.HOLDERS if h not in IC.CHILD_HOLDERS])
    IC.compute_idle(e)          # every other call on the idle context, held against the oracle or model
    return e


def _report(rep):
    print("%s: %.3f s for %d cells" % (rep["holder"], rep["seconds"], len(rep["cells"])))
    print("  busy:   %s" % " ".join(o for o, c in rep["cells"].items() if c == IC.BUSY))
    print("  serves: %s" % " ".join(o for o, c in rep["cells"].items() if c == IC.SERVES))
    for b in rep["bad"]:
        print("  BAD %s" % b)


def _run_child(job, extra_env, timeout):
    """This file as a program in a process of its own with `extra_env` set -> what the job returned"""
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(job)], env=dict(os.environ, **extra_env), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit("a child of %s hung: nothing more is started on this device\n%s" % (os.path.basename(__file__), (e.stdout or b"").decode()[-3000:]), 1)
    text = out.stdout.decode()
    if out.returncode < 0 or out.returncode in (134, 139):
        pytest.exit("a child of %s was killed (%d): nothing more is started on this device\n%s" % (os.path.basename(__file__), out.returncode, text[-3000:]), 1)
    assert out.returncode == 0, text[-3000:]
    return json.loads(text.strip().splitlines()[-1])


@pytest.mark.parametrize("holder", [h for h in IC.HOLDERS if h not in IC.CHILD_HOLDERS])
def test_every_other_call_beside(env, holder):
    try:
        rep = IC.run_holder(env, holder)
    except IC.DeviceFault as fault:
        pytest.exit("%s: nothing more is started on this device" % fault, 1)
    _report(rep)
    assert rep["bad"] == []
    assert rep["cells"] == {o: IC.TABLE[(holder, o)][0] for o in IC.OTHERS}


@pytest.mark.parametrize("holder", sorted(IC.CHILD_HOLDERS))
def test_every_other_call_beside_in_a_process_of_its_own(env, holder):
    """the deferred folds of H3 are flushed by whatever the caller does next: the child's idle results are this process's, bit for bit"""
    rep = _run_child({"holder": holder}, IC.CHILD_HOLDERS[holder], 300)
    _report(rep)
    assert rep["bad"] == []
    assert rep["cells"] == {o: IC.TABLE[(holder, o)][0] for o in IC.OTHERS}
    assert rep["idle"] == env.idle
    assert rep["deferred_seen"], "no proof of the holder had its second half held back: the holder is not what the table describes"


# ---- the entry points whose header promises untouched outputs on refusal, by the raw ABI -------------------------------------------
def _sentinel_calls(env):
    """[(name, call() -> status, the host and device buffers that must still hold the sentinel)] for the seven batched entry points"""
    import torch
    from zk_cryptography_amd import plonk
    e, N = env, env.N
    lib, h = N.lib(), env.ctx.handle
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u32, sz = C.c_uint32, C.c_size_t
    host = lambda *shape: np.full(shape, FILL)     # noqa: E731
    dev = lambda *shape: torch.full(shape, -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")     # the same 64-bit pattern   # noqa: E731
    calls = []
    # zkhip_sumcheck_prove_batch, zkhip_composed_prove_batch: 4 tables of 2^8 entries, 2 products of two
    ptrs = (C.c_void_p * 4)(*[p.evaluations.data_ptr() for p in e.pb8])
    s, rp, ch = host(4, 4), host(4, 8, 2, 4), host(4, 8, 4)
    calls.append(("zkhip_sumcheck_prove_batch", lambda: lib.zkhip_sumcheck_prove_batch(h, u32(4), ptrs, sz(256), None, vp(s), vp(rp), vp(ch)), [s, rp, ch]))
    crp, cch = host(2, 8, 3, 4), host(2, 8, 4)
    calls.append(("zkhip_composed_prove_batch", lambda: lib.zkhip_composed_prove_batch(h, u32(2), ptrs, u32(2), sz(256), vp(crp), vp(cch)), [crp, cch]))
    # zkhip_domain_transform_batch, zkhip_univariate_multiply_batch: device outputs
    src = torch.from_numpy(np.ascontiguousarray(e.fb).view(np.int64)).cuda()
    dst = dev(3, 256, 4)
    calls.append(("zkhip_domain_transform_batch", lambda: lib.zkhip_domain_transform_batch(h, u32(3), N.ptr(src), sz(100), sz(100), N.ptr(dst), sz(256), u32(8),
                                                                                          C.c_int(0)), [dst]))
    a = torch.from_numpy(np.stack(e.mba).view(np.int64)).cuda()
    b = torch.from_numpy(np.stack(e.mbb).view(np.int64)).cuda()
    prod = dev(3, 52, 4)
    calls.append(("zkhip_univariate_multiply_batch", lambda: lib.zkhip_univariate_multiply_batch(h, u32(3), N.ptr(a), sz(33), sz(33), N.ptr(b), sz(20), sz(20),
                                                                                                N.ptr(prod), sz(52)), [prod]))
    # zkhip_plonk_prove_batch, zkhip_plonk_verify_batch
    key = plonk._key_for(e.pl_c, e.pl_srs)
    cols = [[plonk._column(v) for v in (w.a, w.b, w.c, w.public_poly)] for w in e.pl_wobj]
    wp = [(C.c_void_p * 3)(*[row[j].data_ptr() for row in cols]) for j in range(4)]
    bl = np.stack([e.zk.Fr.from_ints(x) for x in e.pl_bl])
    xy, inf, ev, pch, st = host(3, 9, 12), np.full((3, 9), 0xA5, dtype=np.uint8), host(3, 6, 4), host(3, 6, 4), np.full(3, 0x5A5A5A5A, dtype=np.int32)
    calls.append(("zkhip_plonk_prove_batch", lambda: lib.zkhip_plonk_prove_batch(key.handle, u32(3), wp[0], wp[1], wp[2], wp[3], vp(bl), vp(xy), vp(inf), vp(ev),
                                                                                vp(pch), vp(st)), [xy, inf, ev, pch, st, cols]))
    vxy, vinf = plonk._points_arrays(e.pl_vpi._commitments())
    vkey = plonk._vkey_for(e.ctx, e.pl_n, vxy, vinf, e.pl_srs)
    pxy, pinf, pev = np.zeros((3, 9, 12), dtype=np.uint64), np.zeros((3, 9), dtype=np.uint8), np.zeros((3, 6, 4), dtype=np.uint64)
    for i, proof in enumerate(e.pl_proofs):
        pxy[i], pinf[i], pev[i] = proof._arrays()
    pubs = [plonk._column(p) for p in e.pl_pubs]
    pp = (C.c_void_p * 3)(*[t.data_ptr() for t in pubs])
    ok, pair_xy, pair_inf = np.full(3, 0xA5, dtype=np.uint8), host(3, 2, 12), np.full((3, 2), 0xA5, dtype=np.uint8)
    calls.append(("zkhip_plonk_verify_batch", lambda: lib.zkhip_plonk_verify_batch(vkey.handle, sz(3), vp(pxy), vp(pinf), vp(pev), pp, vp(ok), vp(pair_xy),
                                                                                  vp(pair_inf)), [ok, pair_xy, pair_inf, pubs]))
    # zkhip_kzg_open_batch: two openings of 2^6 entries through the level tables
    fxy, finf = e.srs6.folded()
    tables = e.srs6.level_tables
    ep = (C.c_void_p * 2)(e.p6.evaluations.data_ptr(), e.p6b.evaluations.data_ptr())
    z = np.ascontiguousarray(np.stack([e.pts6, e.pts6b]).reshape(12, 4))
    oev, oxy, oinf = host(2, 4), host(2, 6, 12), np.full((2, 6), 0xA5, dtype=np.uint8)
    calls.append(("zkhip_kzg_open_batch", lambda: lib.zkhip_kzg_open_batch(h, u32(2), ep, sz(64), vp(z), sz(6), N.ptr(e.srs6.powers_of_tau_in_g1), N.ptr(e.srs6.inf),
                                                                          sz(64), N.ptr(fxy), N.ptr(finf), N.ptr(tables), vp(oev), vp(oxy), vp(oinf)), [oev, oxy, oinf]))
    assert [c[0] for c in calls] == list(IC.PROMISE_UNTOUCHED)

    # ---- the entry points that used to write, clear or stage before they were refused (profiles/inflight/NOTES.md)
    K, G = e.K, e.zk.GKRProtocol
    byte = lambda *shape: np.full(shape, 0xA5, dtype=np.uint8)     # noqa: E731
    uev, uxy, uinf = host(4), host(12), byte(1)
    uz = np.ascontiguousarray(e.uz, dtype=np.uint64)
    calls.append(("zkhip_univariate_kzg_open", lambda: lib.zkhip_univariate_kzg_open(h, N.ptr(e.upoly.coefficients), sz(64), vp(uz), N.ptr(e.usrs.powers_of_tau_in_g1),
                                                                                    N.ptr(e.usrs.inf), sz(64), vp(uev), vp(uxy), vp(uinf)), [uev, uxy, uinf]))
    gdev = G._device_circuit(e.cir4, e.ctx)
    gtab = [t.contiguous() for t in e.ev4[0]]
    gptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in gtab])
    glens = (C.c_size_t * 5)(*[t.shape[0] for t in gtab])
    g32 = lambda *shape: np.full(shape, 0xA5A5A5A5, dtype=np.uint32)     # noqa: E731
    gs, gn, gl, gr, gwb, gwc, gw0, gch = host(4, 4), g32(4), g32(4, 8), host(4, 8, 7, 2, 4), host(4, 4), host(4, 4), host(2, 4), host(4, 8, 4)
    calls.append(("zkhip_gkr_prove_circuit", lambda: lib.zkhip_gkr_prove_circuit(gdev.handle, gptrs, glens, vp(gs), vp(gn), vp(gl), vp(gr), vp(gwb), vp(gwc), vp(gw0),
                                                                                vp(gch)), [gs, gn, gl, gr, gwb, gwc, gw0, gch, gtab]))
    tev, txy, tinf = host(4), host(6, 12), byte(6)
    z1 = np.ascontiguousarray(e.pts6, dtype=np.uint64)
    calls.append(("zkhip_kzg_open_tables", lambda: lib.zkhip_kzg_open_tables(h, N.ptr(e.p6.evaluations), sz(64), vp(z1), sz(6), N.ptr(e.srs6.powers_of_tau_in_g1),
                                                                            N.ptr(e.srs6.inf), sz(64), N.ptr(fxy), N.ptr(finf), N.ptr(tables), vp(tev), vp(txy), vp(tinf)),
                  [tev, txy, tinf]))
    prep = e.srs6.prepared_lines(False)
    cxy, cinf = K._g1_arrays([e.commit6])
    qxy, qinf = K._g1_arrays(list(e.open6.proofs))
    qev = np.ascontiguousarray(e.open6.evaluation, dtype=np.uint64).reshape(1, 4)
    vok = byte(1)
    calls.append(("zkhip_kzg_verify_batch", lambda: lib.zkhip_kzg_verify_batch(h, sz(1), u32(6), vp(cxy), vp(cinf), vp(qev), vp(z1), vp(qxy), vp(qinf),
                                                                              N.ptr(e.srs6.powers_of_tau_in_g2), N.ptr(e.srs6.g2_inf), sz(6), N.ptr(prep), vp(vok)), [vok]))
    sxy, sinf, sev, sch = host(9, 12), byte(9), host(6, 4), host(6, 4)
    calls.append(("zkhip_plonk_prove", lambda: lib.zkhip_plonk_prove(key.handle, N.ptr(cols[0][0]), N.ptr(cols[0][1]), N.ptr(cols[0][2]), N.ptr(cols[0][3]), vp(bl[0]),
                                                                    vp(sxy), vp(sinf), vp(sev), vp(sch)), [sxy, sinf, sev, sch]))
    sok = byte(1)
    g2 = e.pl_srs.powers_of_tau_in_g2
    calls.append(("zkhip_plonk_verify", lambda: lib.zkhip_plonk_verify(h, sz(e.pl_n), vp(vxy), vp(vinf), vp(pxy[0]), vp(pinf[0]), vp(pev[0]), N.ptr(pubs[0]), N.ptr(g2),
                                                                      N.ptr(e.pl_srs.g2_inf), sz(len(g2)), vp(sok)), [sok]))
    gt, i0, i1 = e.cir3.layers[1]._arrays()
    lib.zkhip_gkr_mle_size.restype = C.c_size_t
    size = lib.zkhip_gkr_mle_size(u32(1))
    dadd, dmul = dev(size, 4), dev(size, 4)
    calls.append(("zkhip_circuit_add_mult_mle", lambda: lib.zkhip_circuit_add_mult_mle(h, vp(gt), vp(i0), vp(i1), sz(len(gt)), u32(1), N.ptr(dadd), N.ptr(dmul)), [dadd, dmul]))
    assert [c[0] for c in calls[len(IC.PROMISE_UNTOUCHED):]] == list(IC.PROMISED_SINCE)
    return calls


def _still_sentinel(buf):
    import torch
    if isinstance(buf, list):           # inputs kept alive, not outputs
        return True
    if isinstance(buf, torch.Tensor):
        return bool((buf == (0xA5 if buf.dtype == torch.uint8 else -0x5A5A5A5A5A5A5A5B)).all().item())
    if buf.dtype == np.uint8:
        return bool((buf == 0xA5).all())
    if buf.dtype == np.int32:
        return bool((buf == 0x5A5A5A5A).all())
    if buf.dtype == np.uint32:
        return bool((buf == 0xA5A5A5A5).all())
    return bool((buf == FILL).all())


@pytest.mark.parametrize("holder", ["H4", "H6"])
def test_raw_refusals_leave_the_outputs_alone(env, holder):
    """zkhip_sumcheck_prove_batch, zkhip_composed_prove_batch, zkhip_domain_transform_batch, zkhip_univariate_multiply_batch,
    zkhip_plonk_prove_batch, zkhip_plonk_verify_batch, zkhip_kzg_open_batch -- and the entry points that used to write before they were
    refused: zkhip_univariate_kzg_open, zkhip_gkr_prove_circuit, zkhip_kzg_open_tables, zkhip_kzg_verify_batch, zkhip_plonk_prove,
    zkhip_plonk_verify, zkhip_circuit_add_mult_mle -- beside a commit in flight (H4) and a live session (H6): ZKHIP_ERR_BUSY, every word
    of every output still the sentinel, the holder's result the oracle's; once the holder has ended the same call, on the same buffers,
    succeeds."""
    for name, call, outputs in _sentinel_calls(env):
        state = IC.BEGIN[holder](env)
        try:
            status = call()
            env.ctx.synchronize()
        finally:
            held = IC.COLLECT[holder](env, state)
        assert status == env.N.ERR_BUSY, (name, status)
        assert all(_still_sentinel(b) for b in outputs), name
        assert held == [], (name, held)
        assert call() == env.N.ZKHIP_OK, name
        env.ctx.synchronize()
        assert not all(_still_sentinel(b) for b in outputs if not isinstance(b, list)), name
    assert IC.fresh_work_mismatches(env) == []


def _unbound_calls(env):
    """Entry points of the header's two lists that the cells of the table do not call beside a lent workspace -- no mirror method binds
    them, or the mirror's method is refused at an earlier call of its own -- by the raw ABI, every input built beforehand:
    -> ([(name, call() -> status, outputs)] that must refuse, [(name, call() -> (status, result))] that must serve)"""
    import torch
    from zk_cryptography_amd import plonk
    e, N = env, env.N
    K, lib, h = e.K, N.lib(), env.ctx.handle
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u32, sz = C.c_uint32, C.c_size_t
    host = lambda *shape: np.full(shape, FILL)     # noqa: E731
    byte = lambda *shape: np.full(shape, 0xA5, dtype=np.uint8)     # noqa: E731
    g32 = lambda *shape: np.full(shape, 0xA5A5A5A5, dtype=np.uint32)     # noqa: E731
    dev = lambda *shape: torch.full(shape, -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")     # noqa: E731
    dev8 = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")     # noqa: E731
    refuse, serve = [], []
    # zkhip_gkr_prove: the one-shot form (uploads the circuit for one proof)
    arrays = [layer._arrays() for layer in e.cir4.layers]
    gt, i0, i1 = (np.ascontiguousarray(np.concatenate([a[j] for a in arrays])) for j in range(3))
    ng = (C.c_size_t * 4)(*[len(a[0]) for a in arrays])
    gtab = [t.contiguous() for t in e.ev4[0]]
    gptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in gtab])
    glens = (C.c_size_t * 5)(*[t.shape[0] for t in gtab])
    gs, gn, gl, gr, gwb, gwc, gw0, gch = host(4, 4), g32(4), g32(4, 8), host(4, 8, 7, 2, 4), host(4, 4), host(4, 4), host(2, 4), host(4, 8, 4)
    refuse.append(("zkhip_gkr_prove", lambda: lib.zkhip_gkr_prove(h, u32(4), ng, vp(gt), vp(i0), vp(i1), gptrs, glens, vp(gs), vp(gn), vp(gl), vp(gr), vp(gwb),
                                                                  vp(gwc), vp(gw0), vp(gch)), [gs, gn, gl, gr, gwb, gwc, gw0, gch, gtab]))
    # zkhip_srs_level_tables (the mirror's precompute_open is refused at the fold in front of it)
    fxy, finf = e.srs6.folded()
    lib.zkhip_srs_level_tables_bytes.restype = C.c_size_t
    lt = dev8(lib.zkhip_srs_level_tables_bytes(sz(64)))
    refuse.append(("zkhip_srs_level_tables", lambda: lib.zkhip_srs_level_tables(h, N.ptr(fxy), N.ptr(finf), sz(64), N.ptr(lt)), [lt]))
    # the G2 halves of the two setups (refused behind their G1 halves in the mirror)
    tau5 = np.ascontiguousarray(e.tau5, dtype=np.uint64)
    mxy, minf = dev(5, 24), dev8(5)
    refuse.append(("zkhip_srs_multilinear_g2", lambda: lib.zkhip_srs_multilinear_g2(h, vp(tau5), u32(5), N.ptr(mxy), N.ptr(minf)), [mxy, minf]))
    utau = np.ascontiguousarray(e.utau, dtype=np.uint64)
    uxy, uinf = dev(4, 24), dev8(4)
    refuse.append(("zkhip_srs_univariate_g2", lambda: lib.zkhip_srs_univariate_g2(h, vp(utau), sz(3), N.ptr(uxy), N.ptr(uinf)), [uxy, uinf]))
    # zkhip_pairing, zkhip_pairing_prepared (refused behind zkhip_g2_prepare in the cell)
    pxy_h, pinf_h = K._g1_arrays([e.pair_p])
    pxy, pinf = torch.from_numpy(pxy_h.view(np.int64)).cuda(), torch.from_numpy(pinf_h).cuda()
    qxy, qinf = K._g2_device([e.pair_q])
    prep = K.g2_prepare([e.pair_q])
    gt1, gt2 = dev(1, 72), dev(1, 72)
    refuse.append(("zkhip_pairing", lambda: lib.zkhip_pairing(h, N.ptr(pxy), N.ptr(pinf), N.ptr(qxy), N.ptr(qinf), sz(1), N.ptr(gt1)), [gt1]))
    refuse.append(("zkhip_pairing_prepared", lambda: lib.zkhip_pairing_prepared(h, N.ptr(pxy), N.ptr(pinf), N.ptr(prep), sz(1), N.ptr(gt2)), [gt2]))
    # zkhip_univariate_kzg_verify_batch with the lines prepared beforehand
    uprep = e.usrs.prepared_lines(True)
    cxy, cinf = K._g1_arrays([e.ucommit])
    oxy, oinf = K._g1_arrays([e.uopen.proof])
    oev = np.ascontiguousarray(e.uopen.evaluation, dtype=np.uint64).reshape(1, 4)
    oz = np.ascontiguousarray(e.uz, dtype=np.uint64).reshape(1, 4)
    uok = byte(1)
    g2 = e.usrs.powers_of_tau_in_g2
    refuse.append(("zkhip_univariate_kzg_verify_batch", lambda: lib.zkhip_univariate_kzg_verify_batch(h, sz(1), vp(cxy), vp(cinf), vp(oev), vp(oz), vp(oxy), vp(oinf),
                                                                                                      N.ptr(g2), N.ptr(e.usrs.g2_inf), sz(len(g2)), N.ptr(uprep), vp(uok)),
                   [uok]))
    # zkhip_ntt: in place, so the data is the output
    data = dev(256, 4)
    refuse.append(("zkhip_ntt", lambda: lib.zkhip_ntt(h, N.ptr(data), u32(8), C.c_int(0)), [data]))
    # zkhip_kzg_open: the form without level tables
    z1 = np.ascontiguousarray(e.pts6, dtype=np.uint64)
    kev, kxy, kinf = host(4), host(6, 12), byte(6)
    refuse.append(("zkhip_kzg_open", lambda: lib.zkhip_kzg_open(h, N.ptr(e.p6.evaluations), sz(64), vp(z1), sz(6), N.ptr(e.srs6.powers_of_tau_in_g1), N.ptr(e.srs6.inf),
                                                                sz(64), N.ptr(fxy), N.ptr(finf), vp(kev), vp(kxy), vp(kinf)), [kev, kxy, kinf]))
    # zkhip_mc_begin: a session; the one that begins on the idle context is released at once
    mptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in e.h7_dev[:2]])
    msz = (C.c_uint32 * 1)(2)
    made = []

    def mc_begin():
        st = C.c_void_p()
        rc = lib.zkhip_mc_begin(h, mptrs, msz, u32(1), sz(1 << 10), u32(1), C.c_int(0), None, C.byref(st))
        made.append(bool(st))
        if st:
            assert lib.zkhip_mc_abort(st) == N.ZKHIP_OK
        return rc
    refuse.append(("zkhip_mc_begin", mc_begin, [made]))
    assert [c[0] for c in refuse] == list(IC.RAW_REFUSED)

    # ---- served: the result beside the holder is the result on the idle context
    vxy, vinf = plonk._points_arrays(e.pl_vpi._commitments())
    pg2 = e.pl_srs.powers_of_tau_in_g2
    proofs = [p._arrays() for p in e.pl_proofs]
    pubs = [plonk._column(p) for p in e.pl_pubs]

    def vkey_create():
        """-> (status, what the key's verdicts are once the holder has ended)"""
        vk = C.c_void_p()
        rc = lib.zkhip_plonk_vkey_create(h, sz(e.pl_n), vp(vxy), vp(vinf), N.ptr(pg2), N.ptr(e.pl_srs.g2_inf), sz(len(pg2)), C.byref(vk))

        def verdicts():
            xy, inf, ev = (np.ascontiguousarray(np.stack([p[j] for p in proofs])) for j in range(3))
            pp = (C.c_void_p * 3)(*[t.data_ptr() for t in pubs])
            ok = np.zeros(3, dtype=np.uint8)
            assert lib.zkhip_plonk_verify_batch(vk, sz(3), vp(xy), vp(inf), vp(ev), pp, vp(ok), None, None) == N.ZKHIP_OK
            assert lib.zkhip_plonk_vkey_destroy(vk) == N.ZKHIP_OK
            return ok.tolist()
        return rc, verdicts
    serve.append(("zkhip_plonk_vkey_create", vkey_create))
    gdev = e.zk.GKRProtocol._device_circuit(e.cir4, e.ctx)
    d_w = e.ev4[0][3].contiguous()
    rb, rc_, al, be = (np.ascontiguousarray(e.pts12[a:b], dtype=np.uint64) for a, b in ((0, 2), (2, 4), (4, 5), (5, 6)))

    def layer_tables():
        out = [dev(8, 4) for _ in range(3)]
        optrs = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
        rc = lib.zkhip_gkr_layer_tables(gdev.handle, u32(2), N.ptr(d_w), sz(8), vp(rb), vp(rc_), vp(al), vp(be), C.c_int(0), optrs, None)
        return rc, lambda: IC.canon(out)
    serve.append(("zkhip_gkr_layer_tables", layer_tables))

    def circuit_create():
        """-> (status, the sums and w_b of a proof on the new circuit once the holder has ended)"""
        cir = C.c_void_p()
        rc = lib.zkhip_circuit_create(h, u32(4), ng, vp(gt), vp(i0), vp(i1), C.byref(cir))

        def proof():
            s_, n_, l_, r_, wb_, wc_, w0_, ch_ = host(4, 4), g32(4), g32(4, 8), host(4, 8, 7, 2, 4), host(4, 4), host(4, 4), host(2, 4), host(4, 8, 4)
            assert lib.zkhip_gkr_prove_circuit(cir, gptrs, glens, vp(s_), vp(n_), vp(l_), vp(r_), vp(wb_), vp(wc_), vp(w0_), vp(ch_)) == N.ZKHIP_OK
            lib.zkhip_circuit_destroy(cir)
            return IC.canon([s_, wb_, wc_, w0_, ch_])
        return rc, proof
    serve.append(("zkhip_circuit_create", circuit_create))
    assert [c[0] for c in serve] == list(IC.RAW_SERVED)
    return refuse, serve


@pytest.mark.parametrize("holder", ["H4", "H6"])
def test_raw_calls_the_table_does_not_reach_beside_a_lent_workspace(env, holder):
    """zkhip_gkr_prove, zkhip_srs_level_tables, zkhip_srs_multilinear_g2, zkhip_srs_univariate_g2, zkhip_pairing, zkhip_pairing_prepared,
    zkhip_univariate_kzg_verify_batch, zkhip_ntt, zkhip_kzg_open, zkhip_mc_begin: ZKHIP_ERR_BUSY beside the holder with every output the
    sentinel, ZKHIP_OK afterwards.  zkhip_plonk_vkey_create, zkhip_gkr_layer_tables, zkhip_circuit_create: served beside the holder, and
    what they made is what they make on the idle context."""
    refuse, serve = _unbound_calls(env)
    for name, call, outputs in refuse:
        state = IC.BEGIN[holder](env)
        try:
            status = call()
            env.ctx.synchronize()
        finally:
            held = IC.COLLECT[holder](env, state)
        assert status == env.N.ERR_BUSY, (name, status)
        assert all(_still_sentinel(b) for b in outputs if not (isinstance(b, list) and b and isinstance(b[0], bool))), name
        assert held == [], (name, held)
        assert call() == env.N.ZKHIP_OK, name
        env.ctx.synchronize()
        if name == "zkhip_mc_begin":
            assert outputs[0] == [False, True]           # no session beside the holder, one afterwards
        else:
            assert not all(_still_sentinel(b) for b in outputs if not isinstance(b, list)), name
    for name, call in serve:
        status, result = call()
        env.ctx.synchronize()
        assert status == env.N.ZKHIP_OK, (name, status)
        idle = result()
        state = IC.BEGIN[holder](env)
        try:
            status, result = call()
            env.ctx.synchronize()
        finally:
            held = IC.COLLECT[holder](env, state)
        assert status == env.N.ZKHIP_OK, (name, status)
        assert held == [], (name, held)
        assert result() == idle, name
        if name == "zkhip_plonk_vkey_create":
            assert idle == [1, 1, 1]
    assert IC.fresh_work_mismatches(env) == []


# ---- a process of its own -------------------------------------------------------------------------------------------------------------
def _job_holder(holder):
    import zk_cryptography_amd as zk
    from oracle import oracle as ora
    ora.lib()
    e = IC.make_env(zk, ora, holders=[holder])
    IC.compute_idle(e, check=False)      # held against the oracle in the parent, whose digests these must equal
    rep = IC.run_holder(e, holder)
    rep["idle"] = e.idle
    # the holder is what the table says: of four proofs begun, the last one's big fold is still held back -- zkhip_ctx_synchronize is
    # what launches it (the fold is the only kernel of that name between the two profile calls)
    N = e.N
    lib, h = N.lib(), e.ctx.handle
    pend = IC.BEGIN[holder](e)
    N.check(lib.zkhip_profile_enable(h, 1), "profile_enable")
    try:
        e.ctx.synchronize()
        folds = 0
        for name in (b"multifold", b"multifold_small"):
            cnt = C.c_uint64(0)
            N.check(lib.zkhip_profile_read(h, name, None, C.byref(cnt), None), "profile_read")
            folds += cnt.value
    finally:
        N.check(lib.zkhip_profile_enable(h, 0), "profile_enable")
    rep["deferred_seen"] = folds > 0
    rep["bad"] += IC.COLLECT[holder](e, pend)
    return rep


if __name__ == "__main__":
    job = json.loads(sys.argv[1])
    print(json.dumps(_job_holder(job["holder"])))
