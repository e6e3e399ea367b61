"""GPU: the big fold of the overlapped plan and the serial rounds beside it as ONE launch (csrc/fold_rounds.hpp).

Kernel level: fold_rounds_kernel is launched directly through tests/cpp/fold_rounds_driver.hip and compared, == on the raw limbs, with
the three launches it stands for on the same inputs (blockfold_kernel, sumcheck_small_kernel, multifold_mfma_kernel<4, 4>): the folded
table, the round polynomials, the challenges, the fold weights of the next stage and the transcript state.  The per-tile sums, which
the fused form does not compute, lie in a buffer of their own filled with a pattern that it must leave alone.
Shapes (k, m, k2) -- the fold takes a 2^k x m table to m outputs, the rounds run on 2^k2 entries:
  (4, 8192, 5)   the smallest the matrix-core form takes, 2^17 entries: 128 tiles, 16 fold workgroups of eight waves
  (5, 8192, 5)
  (6, 16384, 6)  the term count of the 2^24 proof
  (4, 8448, 10)  132 tiles: eight waves do not divide them, the last workgroup has four waves without a tile; and the serial
                 kernel's largest LDS request (2^10 entries with weights)
Prover level, in a child process with ZKHIP_OVERLAP_MIN_LOG=22 (the switch is read once): the synchronous proof at 2^22 (k1 = 4,
k2 = 10) and 2^23 against the oracle, with and without poly_sum(), absorbing the true sum, a host value and a device value; the launch
scopes of that proof; and two proofs in flight, which keep the fork and its names.  This file run as a program is that child."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tables as T  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5A5A5A5A5A5A5A
SHAPES = [(4, 8192, 5), (5, 8192, 5), (6, 16384, 6), (4, 8448, 10)]
FILLS = ["random", "uniform_r", "top", "limb_edges", "stored_max", "zero"]

# the launch scopes of one synchronous proof in host enqueue order, the library deriving every sum itself
FUSED_PROOF = ["fine_sums", "coarse_sums", "sumcheck_small", "blockfold", "multifold", "multifold_rounds", "blockfold", "sumcheck_small"]
# ... and of a proof in flight (fewer than three): the fork as before, the matrix-core fold under its one name
FORKED_PROOF = ["fine_sums", "coarse_sums", "sumcheck_small", "blockfold", "multifold", "sumcheck_small", "blockfold", "sumcheck_small"]


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv():
    import fold_rounds_driver as D
    D.lib()
    return D


def _table(ora, fill, n, seed):
    return ora.random_fr(n, seed) if fill == "random" else T.fill(fill, n, seed)


def _run(drv, fused, dev, m, k, k2, ny, state, round0):
    """one form on fresh output buffers -> {name: numpy array}"""
    import torch
    full = lambda rows: torch.full((rows, 4), PATTERN, dtype=torch.int64, device="cuda")   # noqa: E731
    out = {"p1": full(ny << k2), "w2": full((1 << k2) + 1), "rp": full(2 * (round0 + k2) + 1), "ch": full(round0 + k2 + 1),
           "out": full(m + 1), "partials": full(m // 64 + 1), "st": torch.from_numpy(state.copy()).cuda()}
    rc = drv.lib().fold_rounds_driver_run(fused, dev["table"].data_ptr(), m, k, k2, dev["w"].data_ptr(), dev["fine"].data_ptr(),
                                          out["p1"].data_ptr(), out["w2"].data_ptr(), out["st"].data_ptr(), out["rp"].data_ptr(),
                                          out["ch"].data_ptr(), round0, out["out"].data_ptr(), out["partials"].data_ptr(), 1,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "launcher returned hipError %d" % rc
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("k,m,k2", SHAPES)
def test_fused_launch_equals_the_separate_launches(drv, ora, k, m, k2, fill):
    import torch
    info = drv.info()
    assert info["lanes"] == 64 * info["waves"] and info["lanes"] >= 512
    ny = drv.lib().fold_rounds_driver_slices(k, k2)
    assert 1 <= ny <= 8
    n, round0 = m << k, k
    dev = {"table": torch.from_numpy(_table(ora, fill, n, 300 + k).view(np.int64)).cuda(),
           "w": torch.from_numpy(T.fill("uniform_r", 1 << k, 310 + k).view(np.int64)).cuda(),          # (any residues serve as weights)
           "fine": torch.from_numpy(_table(ora, fill, 1 << (k + k2), 320 + k).view(np.int64)).cuda()}
    state = np.random.Generator(np.random.PCG64(330 + k)).integers(0, 256, size=info["state_bytes"], dtype=np.uint8)
    sep = _run(drv, 0, dev, m, k, k2, ny, state, round0)
    fus = _run(drv, 1, dev, m, k, k2, ny, state, round0)
    pat = np.int64(PATTERN)
    # the separate form did write everything that is compared, and nothing behind it
    assert (sep["partials"][:-1] != pat).any() and (sep["ch"][round0:-1] != pat).any() and (sep["w2"][:-1] != pat).any()
    assert fill == "zero" or (sep["out"][:-1] != pat).any()
    assert (sep["st"] != state).any()
    for name in ("w2", "rp", "ch", "out", "partials"):
        assert (sep[name][-1] == pat).all() and (fus[name][-1] == pat).all(), "the element behind `%s` was written" % name
    assert (sep["rp"][:2 * round0] == pat).all() and (sep["ch"][:round0] == pat).all()
    # bit for bit: the folded table, the round polynomials, the challenges, the weights, the transcript state (and the partial tables)
    for name in ("out", "rp", "ch", "w2", "st", "p1"):
        diff = np.flatnonzero((sep[name] != fus[name]).reshape(len(sep[name]), -1).any(axis=1))
        assert diff.size == 0, "`%s`: %d rows differ, the first at %d" % (name, diff.size, diff[0])
    assert (fus["partials"] == pat).all(), "the fused form touched the per-tile sums"


def test_driver_refuses_what_the_kernels_do_not_take(drv):
    import torch
    buf = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    run = lambda m, k, k2, first=p: drv.lib().fold_rounds_driver_run(1, first, m, k, k2, p, p, p, p, p, p, p, 0, p, p, 1, None)   # noqa: E731
    assert run(8192, 4, 5, None) == drv.INVALID          # a null pointer
    assert run(4096, 4, 5) == drv.INVALID                # fewer outputs than the streaming form takes
    assert run(8192 + 64, 4, 5) == drv.INVALID           # no whole workgroups of the separate fold
    assert run(8192, 3, 5) == drv.INVALID                # the vector form's term count
    assert run(8192, 4, 11) == drv.INVALID               # more entries than the serial kernel keeps


# ---- prover level -----------------------------------------------------------------------------------------------------------------
CLAIMED = T.stored(0x1234567890ABCDEF)                   # a sum the caller gives: absorbed as it is


def _same(*pairs):
    return all(np.array_equal(a, b) for a, b in pairs)


def _prover_mismatches(zk, ora, ev, claimed_too):
    """the synchronous proof in every way a caller reaches it -> the ways that differ from the oracle"""
    import torch
    bad = []
    s, rp, och = ora.sumcheck_prove(ev)
    poly = zk.Multilinear(ev)
    sc = zk.Sumcheck(poly)
    sc.poly_sum()                                        # the fine sums; the true sum is the root of the prover's own tree
    proof, ch = sc.prove()
    if not _same((proof.sum, s), (proof.univariate_poly, rp), (ch, och)):
        bad.append("poly_sum + prove")
    sc = zk.Sumcheck(poly)
    sc._sum_deferred = True                              # no poly_sum(), no claimed sum: the library derives every sum itself
    proof, ch = sc.prove()
    if not _same((proof.sum, s), (proof.univariate_poly, rp), (ch, och)):
        bad.append("prove alone, true sum")
    if claimed_too:
        rp1, ch1 = T.sumcheck_with_claimed_sum(ora, ev, CLAIMED)
        sc = zk.Sumcheck(poly)
        sc.sum = CLAIMED                                 # from the host, no poly_sum()
        proof, ch = sc.prove()
        if not _same((proof.sum, CLAIMED), (proof.univariate_poly, rp1), (ch, ch1)):
            bad.append("prove alone, host sum")
        sc = zk.Sumcheck(poly)
        sc.poly_sum()
        d_sum = torch.from_numpy(CLAIMED.view(np.int64).copy()).cuda()
        sc._sum_dev, sc._sum_ptr, sc._sum_deferred = d_sum, d_sum.data_ptr(), False     # from the device, beside poly_sum()'s block sums
        proof, ch = sc.prove()
        if not _same((proof.sum, CLAIMED), (proof.univariate_poly, rp1), (ch, ch1)):
            bad.append("poly_sum + prove, device sum")
    return bad


def _job(zk, ora, job):
    from test_gpu_sumcheck import _enqueue_order, _unsummed, _same_as_oracle
    log_n, fill = job["log_n"], job["fill"]
    ev = _table(ora, fill, 1 << log_n, 400 + log_n)
    got = {"bad": _prover_mismatches(zk, ora, ev, job["claimed"])}
    if job["names"]:
        proof, names = _enqueue_order(zk, _unsummed(zk, ev).prove)
        got["names"] = names if _same_as_oracle(ora, ev, proof) else ["proof differs"]
        scs = [_unsummed(zk, ev), _unsummed(zk, ev)]
        proofs, names2 = _enqueue_order(zk, lambda: [h.wait() for h in [sc.prove_begin() for sc in scs]])
        got["names_in_flight"] = names2 if all(_same_as_oracle(ora, ev, p) for p in proofs) else ["proof differs"]
    return got


def _run_child(job, timeout=300):
    """This file as a program in a process of its own with the overlapped plan from 2^22 on -> what the job returned"""
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(job)], env=dict(os.environ, ZKHIP_OVERLAP_MIN_LOG="22"),
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit("a child of %s hung: nothing more is started on this device\n%s" % (os.path.basename(__file__), (e.stdout or b"").decode()[-3000:]), 1)
    text = out.stdout.decode()
    if out.returncode < 0 or out.returncode in (134, 139):
        pytest.exit("a child of %s was killed (%d): nothing more is started on this device\n%s" % (os.path.basename(__file__), out.returncode, text[-3000:]), 1)
    assert out.returncode == 0, text[-3000:]
    return json.loads(text.strip().splitlines()[-1])


@pytest.mark.parametrize("fill", ["random", "top"])
def test_synchronous_proof_at_2_22(fill):
    """k1 = 4, k2 = 10: the serial kernel's largest LDS request beside the fold"""
    got = _run_child({"log_n": 22, "fill": fill, "claimed": True, "names": fill == "random"})
    print(got)
    assert got["bad"] == []
    if fill == "random":
        assert got["names"] == FUSED_PROOF
        assert got["names_in_flight"] == 2 * FORKED_PROOF


def test_synchronous_proof_at_2_23():
    got = _run_child({"log_n": 23, "fill": "random", "claimed": False, "names": False})
    print(got)
    assert got["bad"] == []


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import zk_cryptography_amd as zk_
    from oracle import oracle as ora_
    ora_.lib()
    print(json.dumps(_job(zk_, ora_, json.loads(sys.argv[1]))))
