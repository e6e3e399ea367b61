"""PLONK verify on the GPU, one proof or a batch: one JSON line.

For n = 2^12 and 2^16 (--sizes), in one process after warm-up:
  single_ms_n*             PlonkVerifier.verify (zkhip_plonk_verify: host G1 ladders, lines prepared per call, two pairings), median ms
  batch_n*_B*              PlonkVerifier.verify_batch at B = 1, 16, 64, 256, 1024: api_ms (the python call, which packs the proofs),
                           abi_ms (zkhip_plonk_verify_batch on packed arrays), proofs_per_s (of abi_ms)
  per_proof_ratio_n*_B64   single_ms / (api_ms of B = 64 / 64): how many times cheaper a proof is in a batch of 64
  split_ms_n*_B*           the library's profile counters of one profiled call: pi (the PI pass and its finishing pass), terms, combine,
                           miller_loops, final_exp; host_challenges (the Merlin transcripts alone: B x zkhip_plonk_challenges) and
                           host_and_idle (what abi_ms exceeds the kernel sum by: challenges, scalars, copies, launches)
  kzg_n20_B256_ms          MultilinearKZG.verify_batch at n_vars = 20, B = 256 in the same process: the yardstick (21 ladders and 21
                           Miller loops per opening against 20 and 2 here)
  ratio_to_kzg_n*_B256     api_ms of B = 256 / kzg_n20_B256_ms (both through their python calls)

The circuit is c = a * b on every row with the identity permutation (tools/perf_plonk.py's); a batch is B copies of one proof with one
column: the verifier's work does not depend on the values.  Every call returns host verdicts, so it synchronises.
usage: python tools/perf_plonk_verify.py [--reps K] [--sizes 12,16] [--batches 1,16,64,256,1024] [--no-kzg]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"pi": "plonk_verify_pi", "terms": "plonk_verify_terms", "combine": "plonk_verify_combine", "miller_loops": "pairing_miller_loops",
           "final_exp": "pairing_final_exp"}


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
    ap.add_argument("--sizes", default="12,16")
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--no-kzg", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import zk_cryptography_amd as zk
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    from zk_cryptography_amd.field import R_MOD

    lib = N.lib()
    vp = C.c_void_p
    out = {"metric": "plonk_verify", "device": torch.cuda.get_device_name(0)}
    batches = [int(s) for s in a.batches.split(",")]
    for log_n in [int(s) for s in a.sizes.split(",")]:
        n = 1 << log_n
        ctx = N.Context.get()
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()
        wa, wb = dev(zk.Fr.synthetic(n, 1)), dev(zk.Fr.synthetic(n, 2))
        wc = torch.empty_like(wa)
        N.check(lib.zkhip_pointwise_mul(ctx.handle, N.ptr(wa), N.ptr(wb), C.c_size_t(n), N.ptr(wc)), "a * b")
        x = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
        x[1] = dev(zk.Fr.from_ints([1]))[0]
        s1 = torch.empty_like(wa)
        N.check(lib.zkhip_domain_transform(ctx.handle, N.ptr(x), C.c_size_t(2), N.ptr(s1), C.c_uint32(log_n), C.c_int(0)), "w^i")
        s2, s3 = torch.empty_like(wa), torch.empty_like(wa)
        N.check(lib.zkhip_mle_elementwise(ctx.handle, C.c_int(0), N.ptr(s1), N.ptr(s1), None, C.c_size_t(n), C.c_size_t(n), N.ptr(s2)), "2 w^i")
        N.check(lib.zkhip_mle_elementwise(ctx.handle, C.c_int(0), N.ptr(s2), N.ptr(s1), None, C.c_size_t(n), C.c_size_t(n), N.ptr(s3)), "3 w^i")
        zero = torch.zeros_like(wa)
        const = lambda v: dev(zk.Fr.from_ints([v])).repeat(n, 1).contiguous()
        cpi = zk.CommonPreprocessedInput(n, zero, zero, const(1), const(R_MOD - 1), zero, s1, s2, s3)
        wit = zk.Witness(wa, wb, wc, zero)
        srs = zk.UnivariateKZG.generate_srs(zk.Fr.synthetic(1, 3)[0], n + 5, g2=True)
        proof = zk.PlonkProver(cpi, srs).prove(wit, blinding=[7 + i for i in range(11)])
        v = zk.VerifierPreprocessedInput.vpi(srs, cpi)
        verifier = zk.PlonkVerifier(n, proof, srs, v)
        assert verifier.verify(zero)
        single = _med(lambda: verifier.verify(zero), a.reps)
        out["single_ms_n%d" % log_n] = round(single, 3)
        vxy, vinf = plonk._points_arrays(v._commitments())
        key = plonk._vkey_for(ctx, n, vxy, vinf, srs)
        pxy, pinf, pev = proof._arrays()
        for B in batches:
            proofs = [proof] * B
            assert zk.PlonkVerifier.verify_batch(n, proofs, srs, v, zero) == [True] * B
            api = _med(lambda: zk.PlonkVerifier.verify_batch(n, proofs, srs, v, zero), a.reps)
            xy, inf, ev = np.tile(pxy, (B, 1, 1)), np.tile(pinf, (B, 1)), np.tile(pev, (B, 1, 1))
            ptrs = (C.c_void_p * B)(*([zero.data_ptr()] * B))
            ok = np.zeros(B, dtype=np.uint8)
            call = lambda: N.check(lib.zkhip_plonk_verify_batch(key.handle, C.c_size_t(B), xy.ctypes.data_as(vp), inf.ctypes.data_as(vp),
                                                                ev.ctypes.data_as(vp), ptrs, ok.ctypes.data_as(vp), None, None), "verify_batch")
            call()
            assert ok.all()
            abi = _med(call, a.reps)
            tag = "n%d_B%d" % (log_n, B)
            out["batch_" + tag] = {"api_ms": round(api, 3), "abi_ms": round(abi, 3), "proofs_per_s": round(B / abi * 1e3, 1)}
            N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile")
            call()
            split, total = {}, 0.0
            for name, kernel in KERNELS.items():
                t = C.c_double(0)
                N.check(lib.zkhip_profile_read(ctx.handle, kernel.encode(), C.byref(t), None, None), "profile_read")
                split[name] = round(t.value, 3)
                total += t.value
            N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile")
            ch = np.zeros((6, 4), dtype=np.uint64)

            def challenges():
                for _ in range(B):
                    lib.zkhip_plonk_challenges(pxy.ctypes.data_as(vp), pinf.ctypes.data_as(vp), pev.ctypes.data_as(vp), ch.ctypes.data_as(vp))
            split["host_challenges"] = round(_med(challenges, a.reps), 3)
            split["host_and_idle"] = round(max(0.0, abi - total), 3)
            out["split_ms_" + tag] = split
        if 64 in batches:
            out["per_proof_ratio_n%d_B64" % log_n] = round(single / (out["batch_n%d_B64" % log_n]["api_ms"] / 64), 1)
        del key, srs, cpi
        torch.cuda.empty_cache()
    if not a.no_kzg:
        nv, B = 20, 256
        msrs = zk.TrustedSetup.setup(zk.Fr.random(nv, 1), g2=True)
        poly = zk.Multilinear(zk.Fr.random(1 << nv, 2))
        z = zk.Fr.random(nv, 3)
        commit = zk.MultilinearKZG.commitment(poly, msrs)
        opening = zk.MultilinearKZG.open(poly, z, msrs)
        cs, zs, ps = [commit] * B, [z] * B, [opening] * B
        assert zk.MultilinearKZG.verify_batch(cs, zs, ps, msrs).all()
        kzg = _med(lambda: zk.MultilinearKZG.verify_batch(cs, zs, ps, msrs), a.reps)
        out["kzg_n20_B256_ms"] = round(kzg, 3)
        for log_n in [int(s) for s in a.sizes.split(",")]:
            if 256 in batches:
                out["ratio_to_kzg_n%d_B256" % log_n] = round(out["batch_n%d_B256" % log_n]["api_ms"] / kzg, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
