"""GPU parity of the serial prover kernel's prologue paths and of the way a proof reaches the host (the sequence word in the
pinned result slot, zkhip_ctx::wait_proof): every proof bit-exact against the CPU oracle on sum, round polynomials and challenges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


_WANT = {}


def _table(ora, log_n, seed):
    """(table, the oracle's proof of it), computed once per (size, seed)"""
    key = (log_n, seed)
    if key not in _WANT:
        ev = ora.random_fr(1 << log_n, seed)
        _WANT[key] = (ev, ora.sumcheck_prove(ev))
    return _WANT[key]


def _same(got, want):
    (proof, ch), (s, rp, och) = got, want
    return np.array_equal(proof.sum, s) and np.array_equal(proof.univariate_poly, rp) and np.array_equal(ch, och)


def _prover(zk, ev, want, opening):
    """The three ways a proof's transcript opens (SmallArgs::first): with the sum of the prover's own tree, with a sum the host
    hands in, with the sum poly_sum() left on the device."""
    sc = zk.Sumcheck(zk.Multilinear(ev))
    if opening == "own":
        sc._sum_deferred = True                      # no claimed sum, no block sums: lo + hi of the first round
    elif opening == "host":
        sc.sum = want[0]
    else:
        sc.poly_sum()
    return sc


@pytest.mark.parametrize("opening", ["own", "host", "device"])
@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 10])
def test_serial_kernel_alone(zk, ora, log_n, opening):
    """One launch takes the whole proof.  2^1 and 2^2 have no level 2 / level 3 below the root (the rounds' `depth` branches), 2^10 is the
    largest tree the kernel holds."""
    ev, want = _table(ora, log_n, 8100 + log_n)
    assert _same(_prover(zk, ev, want, opening).prove(), want)


@pytest.mark.parametrize("opening", ["own", "host", "device"])
def test_stage_plan_one_stage(zk, ora, opening):
    """2^11: chunk sums, one serial launch on grouped leaves with fold weights, the fold, the closing launch."""
    ev, want = _table(ora, 11, 8111)
    assert _same(_prover(zk, ev, want, opening).prove(), want)


def _overlapped_2_19():
    """Runs in a process of its own (the switch is read once): the overlapped plan at 2^19 -- the strided leaves with two and with eight
    partial tables, the launch that writes fold weights, and the closing launch, which copies 11 earlier rounds into the pinned slot."""
    import zk_cryptography_amd as zk
    from oracle import oracle as ora
    ora.lib()
    ev, want = _table(ora, 19, 8119)
    ok = [_same(_prover(zk, ev, want, opening).prove(), want) for opening in ("own", "host", "device")]
    ok.append(_same(_prover(zk, ev, want, "device").prove(), want))          # the slot and the scratch a second time
    return ok


def test_overlapped_plan_at_2_19():
    import json, os, subprocess, sys
    env = dict(os.environ, ZKHIP_OVERLAP_MIN_LOG="19")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert json.loads(text.strip().splitlines()[-1]) == [True] * 4


def test_hand_off_of_synchronous_proofs(zk, ora):
    """64 synchronous proofs through one result slot: two different 2^10 tables and a 2^3 table in turn.  A word seen early or left over
    from the proof before would hand out that proof, or a short proof with a long one's tail behind it."""
    cases = [_table(ora, 10, 8210), _table(ora, 10, 8211), _table(ora, 3, 8203)]
    provers = []
    for ev, want in cases:
        sc = zk.Sumcheck(zk.Multilinear(ev))
        sc.poly_sum()
        provers.append(sc)
    for i in range(64):
        assert _same(provers[i % 3].prove(), cases[i % 3][1]), i


def _begin(zk, ev):
    sc = zk.Sumcheck(zk.Multilinear(ev))
    sc.poly_sum()
    return sc.prove_begin()


def _abandon(h):
    """zkhip_sumcheck_prove_end with null outputs: the proof is waited out, nothing is collected"""
    from zk_cryptography_amd import _native as N
    t, h._ticket = h._ticket, None
    N.check(N.lib().zkhip_sumcheck_prove_end(h._poly._ctx.handle, t, None, None, None), "sumcheck_prove_end")


def test_hand_off_of_proofs_in_flight(zk, ora):
    """Eight proofs in flight at 2^11, collected youngest first and from the middle, two tickets abandoned; then the same eight slots
    again with every table in another slot.  (Their last kernels store the slots' words like any other; the synchronous proof at the
    end goes through slot 0 behind two of them and must wait for its own value.)"""
    cases = [_table(ora, 11, 8300 + j) for j in range(8)]
    hs = [_begin(zk, ev) for ev, _ in cases]
    for j in (7, 3, 4):
        assert _same(hs[j].wait(), cases[j][1]), j
    _abandon(hs[2])
    _abandon(hs[5])
    for j in (0, 6, 1):
        assert _same(hs[j].wait(), cases[j][1]), j
    hs = [_begin(zk, cases[(j + 3) % 8][0]) for j in range(8)]
    for j in (4, 0, 7, 2, 5, 1, 6, 3):
        assert _same(hs[j].wait(), cases[(j + 3) % 8][1]), j
    ev, want = cases[0]
    assert _same(_prover(zk, ev, want, "device").prove(), want)              # every ticket is free again


def test_hand_off_with_the_profile_on(zk, ora):
    """With the library's profile enabled the collector takes the event: the proof is right and the timeline lists every launch."""
    import ctypes as C
    from zk_cryptography_amd import _native as N
    ev, want = _table(ora, 11, 8111)
    sc = _prover(zk, ev, want, "own")
    ctx, lib, mx = N.Context.get(), N.lib(), 64
    N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        got = sc.prove()
        names, st, sp, cnt = C.create_string_buffer(32 * mx), (C.c_double * mx)(), (C.c_double * mx)(), C.c_uint32(0)
        N.check(lib.zkhip_profile_timeline(ctx.handle, mx, names, st, sp, C.byref(cnt)), "profile_timeline")
    finally:
        N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    assert _same(got, want)
    listed = [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(cnt.value)]
    assert listed == ["chunk_sums", "sumcheck_small", "multifold_small", "sumcheck_small"]
    assert all(sp[i] >= st[i] for i in range(cnt.value))                    # every launch's events have completed
    assert _same(_prover(zk, ev, want, "own").prove(), want)                 # ... and back on the word


if __name__ == "__main__":
    import json, os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(_overlapped_2_19()))
