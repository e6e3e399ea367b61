"""KZG verify on the GPU: one JSON line.

  single_ms_n8 / single_ms_n20     one MultilinearKZG.verify (prepared lines already built), median ms
  batch_n20_B{64,256,1024}         MultilinearKZG.verify_batch at n = 20: ms, openings/s, pairings/s (n + 1 pairings per opening)
  batch_speedup_n20_B256           256 single verify calls / one batch of 256
  univariate_B{256,1024}           UnivariateKZG.verify_batch: ms, openings/s, pairings/s (2 per opening)
  prepare_ms_n20                   zkhip_kzg_prepare of [G2, tau_1 G2 .. tau_20 G2] (21 points, with their curve and subgroup checks)
  g2_srs_ms_n20 / g2_srs_ms_uni1024  the G2 half of setup(n = 20) / generate_srs(max_degree = 1023)

Every call returns host verdicts, so it synchronises; times are wall clock around the call.
usage: python tools/perf_verify.py [--reps K]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    import zk_cryptography_amd as zk
    from zk_cryptography_amd import _native as N

    out = {"metric": "kzg_verify", "device": torch.cuda.get_device_name(0)}
    ml = {}
    for nv in (8, 20):
        srs = zk.TrustedSetup.setup(zk.Fr.random(nv, 1), g2=True)
        poly = zk.Multilinear(zk.Fr.random(1 << nv, 2))
        z = zk.Fr.random(nv, 3)
        commit = zk.MultilinearKZG.commitment(poly, srs)
        proof = zk.MultilinearKZG.open(poly, z, srs)
        assert zk.MultilinearKZG.verify(commit, z, proof, srs)      # builds the prepared lines, warms up
        out["single_ms_n%d" % nv] = round(_med(lambda: zk.MultilinearKZG.verify(commit, z, proof, srs), a.reps), 3)
        ml[nv] = (srs, commit, z, proof)

    srs, commit, z, proof = ml[20]
    for B in (64, 256, 1024):
        cs, zs, ps = [commit] * B, [z] * B, [proof] * B
        ok = zk.MultilinearKZG.verify_batch(cs, zs, ps, srs)
        assert ok.all()
        ms = _med(lambda: zk.MultilinearKZG.verify_batch(cs, zs, ps, srs), a.reps)
        out["batch_n20_B%d_ms" % B] = round(ms, 3)
        out["batch_n20_B%d_openings_per_s" % B] = round(B / ms * 1e3, 1)
        out["batch_n20_B%d_pairings_per_s" % B] = round(21 * B / ms * 1e3, 1)
    out["batch_speedup_n20_B256"] = round(256 * out["single_ms_n20"] / out["batch_n20_B256_ms"], 1)

    usrs = zk.UnivariateKZG.generate_srs(zk.Fr.random(1, 4)[0], 1023, g2=True)
    upoly = zk.DenseUnivariatePolynomial(zk.Fr.random(1024, 5))
    uz = zk.Fr.random(1, 6)[0]
    ucommit = zk.UnivariateKZG.commitment(upoly, usrs)
    uproof = zk.UnivariateKZG.open(upoly, uz, usrs)
    assert zk.UnivariateKZG.verify(ucommit, uz, uproof, usrs)
    out["univariate_single_ms"] = round(_med(lambda: zk.UnivariateKZG.verify(ucommit, uz, uproof, usrs), a.reps), 3)
    for B in (256, 1024):
        cs, zs, ps = [ucommit] * B, [uz] * B, [uproof] * B
        assert zk.UnivariateKZG.verify_batch(cs, zs, ps, usrs).all()
        ms = _med(lambda: zk.UnivariateKZG.verify_batch(cs, zs, ps, usrs), a.reps)
        out["univariate_B%d_ms" % B] = round(ms, 3)
        out["univariate_B%d_openings_per_s" % B] = round(B / ms * 1e3, 1)
        out["univariate_B%d_pairings_per_s" % B] = round(2 * B / ms * 1e3, 1)

    import ctypes as C
    g2, inf = srs.powers_of_tau_in_g2, srs.g2_inf
    N.lib().zkhip_g2_prepared_bytes.restype = C.c_size_t
    buf = torch.empty(N.lib().zkhip_g2_prepared_bytes(C.c_size_t(21)), dtype=torch.uint8, device=g2.device)
    ctx = N.Context.get(g2.device.index)
    out["prepare_ms_n20"] = round(_med(lambda: N.check(N.lib().zkhip_kzg_prepare(ctx.handle, N.ptr(g2), N.ptr(inf), C.c_size_t(20), N.ptr(buf)),
                                                       "prepare"), a.reps), 3)
    tau = np.ascontiguousarray(zk.Fr.random(20, 7))
    qxy = torch.empty((1024, 24), dtype=torch.int64, device="cuda")
    qinf = torch.empty(1024, dtype=torch.uint8, device="cuda")
    out["g2_srs_ms_n20"] = round(_med(lambda: N.check(N.lib().zkhip_srs_multilinear_g2(ctx.handle, tau.ctypes.data_as(C.c_void_p), C.c_uint32(20),
                                                                                      N.ptr(qxy), N.ptr(qinf)), "g2 srs"), a.reps), 3)
    t1 = np.ascontiguousarray(zk.Fr.random(1, 8))
    out["g2_srs_ms_uni1024"] = round(_med(lambda: N.check(N.lib().zkhip_srs_univariate_g2(ctx.handle, t1.ctypes.data_as(C.c_void_p), C.c_size_t(1023),
                                                                                          N.ptr(qxy), N.ptr(qinf)), "g2 srs"), a.reps), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
