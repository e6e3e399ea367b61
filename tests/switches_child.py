"""The process tests/test_gpu_switches.py starts once per group of switches (they are read once per process):
    python switches_child.py <group> <file with the parent's default openings>
Every workload below runs with the library's profile on, is compared bit for bit with the CPU oracle (the openings: with the default
path's proofs from the parent), and the profile's launch counts must show the form the switch selects."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import zk_cryptography_amd as zk                    # noqa: E402
from zk_cryptography_amd import _native as N        # noqa: E402
from oracle import oracle as ora                    # noqa: E402
from gkr_cases import gkr_proof_mismatches, random_circuit    # noqa: E402

NAMES = ("composed_pipe_round", "composed_tail", "composed_round", "gkr_small_mid", "gkr_small_end", "gkr_mid", "gkr_end", "multifold",
         "multifold_valu", "multifold_small", "fine_sums", "msm_small", "msm_accumulate")


def profiled(work):
    """work() with the profile on -> (its result, {name: launches})"""
    ctx = N.Context.get()
    N.check(N.lib().zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        result = work()
        counts = {}
        for name in NAMES:
            cnt = C.c_uint64()
            N.check(N.lib().zkhip_profile_read(ctx.handle, name.encode(), None, C.byref(cnt), None), "profile_read")
            counts[name] = cnt.value
    finally:
        N.check(N.lib().zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    print({k: v for k, v in counts.items() if v}, flush=True)
    return result, counts


def composed_k2(log_n=16):
    t = np.stack([ora.random_fr(1 << log_n, 8100 + q) for q in range(2)])
    (proof, ch), counts = profiled(lambda: zk.ComposedSumcheck(zk.ComposedMultilinear(list(t))).prove())
    rp, och = ora.composed_prove(t)
    assert np.array_equal(proof.round_polys, rp) and np.array_equal(ch, och)
    return counts


def gkr(depth=9):
    layers = random_circuit(depth)
    inp = ora.random_fr(2 ** depth, 8200 + depth)
    circuit = zk.Circuit.from_tuples(layers)
    ev = circuit.evaluation(inp)
    proof, counts = profiled(lambda: zk.GKRProtocol.prove(circuit, ev))
    assert gkr_proof_mismatches(ora, proof, ora.gkr_prove_sparse(layers, ora.circuit_evaluation(layers, inp))) == []
    return counts


def fold4(log_n=17):
    a, pts = ora.random_fr(1 << log_n, 8300), ora.random_fr(4, 8301)
    got, counts = profiled(lambda: zk.Multilinear(a).partial_evaluations(pts, [0] * 4).to_numpy())
    assert np.array_equal(got, ora.mle_partial_evaluations(a, pts, [0] * 4))
    return counts


def sumcheck(log_n=18):
    ev = ora.random_fr(1 << log_n, 8400)

    def work():
        sc = zk.Sumcheck(zk.Multilinear(ev))
        sc.poly_sum()
        return sc.prove()
    (proof, ch), counts = profiled(work)
    s, rp, och = ora.sumcheck_prove(ev)
    assert np.array_equal(proof.sum, s) and np.array_equal(proof.univariate_poly, rp) and np.array_equal(ch, och)
    return counts


def fine_block_sums(log_n=18, log_blocks=10):
    """zkhip_mle_block_sums at the overlapped plan's granularity (blocks of 256 entries), which poly_sum() takes from 2^24 entries on"""
    import torch
    n, ev = 1 << log_n, ora.random_fr(1 << log_n, 8450)
    poly = zk.Multilinear(ev)
    buf = torch.empty(((1 << log_blocks) + 1, 4), dtype=torch.int64, device=poly.evaluations.device)
    total = np.empty(4, dtype=np.uint64)
    _, counts = profiled(lambda: N.check(N.lib().zkhip_mle_block_sums(poly._ctx.handle, poly.evaluations.data_ptr(), n, log_blocks, buf.data_ptr(),
                                                                       total.ctypes.data), "block_sums"))
    got = buf.cpu().numpy().view(np.uint64)
    blocks = ev.reshape(1 << log_blocks, n >> log_blocks, 4)
    assert np.array_equal(got[:-1], np.stack([ora.mle_sum(b) for b in blocks]))
    assert np.array_equal(got[-1], ora.mle_sum(ev)) and np.array_equal(total, got[-1])
    return counts


def commit_table(n=256):
    tau, sc = ora.random_fr(8, 8500), ora.random_fr(n, 8501)
    srs = zk.TrustedSetup.setup(tau).precompute()
    com, counts = profiled(lambda: zk.MultilinearKZG.commitment(zk.Multilinear(sc), srs))
    want = ora.g1_to_affine(ora.kzg_commitment(sc, ora.kzg_multilinear_srs_g1(tau), True))
    assert com.infinity == bool(want[12]) and np.array_equal(com.xy, want[:12])
    return counts


def opening_inputs(log_n):
    return ora.random_fr(log_n, 8600 + log_n), ora.random_fr(log_n, 8700 + log_n), ora.random_fr(1 << log_n, 8800 + log_n)


def opening(log_n):
    """MultilinearKZG::open on the plain SRS, folded per call: the batched commit of the bucket path at every size -> (xy, inf, evaluation)"""
    tau, z, vals = opening_inputs(log_n)
    srs = zk.TrustedSetup.setup(tau)
    proof = zk.MultilinearKZG.open(zk.Multilinear(vals), z, srs, cache_folded_srs=False)
    return np.stack([p.xy for p in proof.proofs]), np.array([p.infinity for p in proof.proofs]), np.asarray(proof.evaluation)


def opening_like(ref, log_n):
    (xy, inf, ev), counts = profiled(lambda: opening(log_n))
    assert np.array_equal(inf, ref["inf%d" % log_n]) and np.array_equal(ev, ref["ev%d" % log_n])
    assert np.array_equal(xy[~inf], ref["xy%d" % log_n][~inf]) and not inf.all()
    return counts


def group_a(ref):
    assert (os.environ["ZKHIP_PIPE"], os.environ["ZKHIP_MF"], os.environ["ZKHIP_MSM_SMALL"]) == ("0", "0", "0")
    c = composed_k2()                 # default: the rounds from 2^15 entries down to the tail are composed_pipe_round launches
    assert c["composed_pipe_round"] == 0 and c["composed_round"] >= 1 and c["composed_tail"] == 1, c
    c = gkr()                         # ZKHIP_PIPE=0 is the host transcript too: no layer ends on the device
    assert c["gkr_small_end"] == 0 and c["gkr_end"] == 0 and c["composed_pipe_round"] == 0 and c["composed_tail"] >= 9, c
    c = fold4()                       # m = 2^13 outputs of 2^4 terms: the streaming shape, whose form ZKHIP_MF chooses
    assert c["multifold"] == 1 and c["multifold_valu"] == 1 and c["multifold_small"] == 0, c
    c = commit_table()                # default: one msm_small launch
    assert c["msm_small"] == 0 and c["msm_accumulate"] == 1, c


def group_b(ref):
    assert os.environ["ZKHIP_GKR_HOST_TRANSCRIPT"] == "1" and os.environ["ZKHIP_PIPE_WGS"] == "64"
    c = gkr()
    assert c["gkr_small_end"] == 0 and c["gkr_end"] == 0 and c["composed_tail"] >= 9, c
    # ZKHIP_FINE_LDS=0, ZKHIP_MF_OCC=2 set the LDS requests of fine_sums and of the matrix-core fold.  poly_sum + prove at 2^18 launches
    # neither (block sums at 2^8 blocks, folds of 2^10 outputs); the smallest shapes that do: the stage plan's first fold at 2^21 (2^13
    # outputs of 2^8 terms) and the block sums at the overlapped plan's granularity
    c = sumcheck(18)
    assert c["fine_sums"] == 0 and c["multifold"] == 0 and c["multifold_small"] >= 1, c
    c = sumcheck(21)
    assert c["multifold"] >= 1 and c["multifold_valu"] == 0, c
    c = fine_block_sums()
    assert c["fine_sums"] == 1, c
    c = composed_k2()                 # ZKHIP_PIPE_WGS=64 caps the grid of the pipelined rounds
    assert c["composed_pipe_round"] >= 2 and c["composed_tail"] == 1, c
    c = opening_like(ref, 12)         # ZKHIP_MSM_BATCH_DELTA=2: the widths of the batch's geometry
    assert c["msm_small"] == 0 and c["msm_accumulate"] == 1, c
    c = opening_like(ref, 15)         # ZKHIP_OPEN_PIPELINES=1: rounds ABOVE 2^14 quotients leave the batch, and 2^15 entries have none ...
    assert c["msm_small"] == 0 and c["msm_accumulate"] == 1, c
    c = opening_like(ref, 16)         # ... at 2^16 the round of 2^15 quotients is a commit of its own beside the batch
    assert c["msm_small"] == 0 and c["msm_accumulate"] == 2, c


def group_c(ref):
    assert os.environ["ZKHIP_GKR_FUSE_SMALL"] == "0"
    c = gkr()                         # default: every layer of depth 9 (<= 512 rows) takes the fused launches
    assert c["gkr_small_mid"] == 0 and c["gkr_small_end"] == 0 and c["gkr_mid"] == 9 and c["gkr_end"] == 9, c


def group_default(ref):
    """No switch set: what the other groups' counts are measured against."""
    assert not [k for k in os.environ if k.startswith("ZKHIP_") and k not in ("ZKHIP_LIB", "ZKHIP_DIAG_LIB")]
    c = composed_k2()
    assert c["composed_pipe_round"] >= 2 and c["composed_tail"] == 1, c
    c = gkr()
    assert c["gkr_small_mid"] == 9 and c["gkr_small_end"] == 9 and c["gkr_mid"] == 0 and c["gkr_end"] == 0, c
    c = fold4()
    assert c["multifold"] == 1 and c["multifold_valu"] == 0, c
    c = commit_table()
    assert c["msm_small"] == 1 and c["msm_accumulate"] == 0, c
    c = opening_like(ref, 16)
    assert c["msm_accumulate"] == 1, c


if __name__ == "__main__":
    {"A": group_a, "B": group_b, "C": group_c, "default": group_default}[sys.argv[1]](np.load(sys.argv[2]))
    print("switches ok")
