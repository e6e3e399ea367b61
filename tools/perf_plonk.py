"""PLONK prove on the GPU: one JSON line.

For n = 2^12, 2^16, 2^18, 2^20 (--sizes), after warm-up, with the key built (and the shifted-SRS table, --table):
  prove_ms_n*            zkhip_plonk_prove, median wall-clock ms (the call returns the proof, so it synchronises)
  split_ms_n*            the library's own profile counters of one profiled prove, kernel time summed per group: commits (msm_*),
                         transforms (ntt_*), grand_product, quotient (+ split), linearisation (+ the two divisions), other (the
                         evaluations).  Commits run three in flight, so their kernel times overlap: the groups need not add up
                         to the wall time; `host_and_idle` is what the wall time exceeds the kernel sum by (or 0).
  commits_alone_ms_n*    the same nine commits alone through zkhip_kzg_commit_begin / _end, three in flight, in the same process
  ratio_to_commits_n*    prove / commits alone
  scaling_18_over_16     t(2^18) / t(2^16): near 4 for quasi-linear work

The circuit is c = a * b on every row (q_m = 1, q_o = -1) with random a, b and the identity permutation: a satisfied witness that
costs nothing to build; the prover's work does not depend on the values.
usage: python tools/perf_plonk.py [--reps K] [--sizes 12,16,18,20] [--table]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"commits": ("msm_",), "transforms": ("ntt_",), "grand_product": ("plonk_grand_product",),
          "quotient": ("plonk_quotient", "plonk_split"), "linearisation": ("plonk_linearise", "plonk_divide"), "other": ("plonk_evaluate",)}
KERNELS = ["msm_convert_points", "msm_sort", "msm_overflow", "msm_order", "msm_accumulate", "msm_segment", "msm_terms", "msm_small",
           "ntt_first8", "ntt_pass", "ntt_first_stages", "ntt_mid_stages", "plonk_grand_product", "plonk_quotient", "plonk_split",
           "plonk_linearise", "plonk_divide", "plonk_evaluate"]


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
    ap.add_argument("--sizes", default="12,16,18,20")
    ap.add_argument("--table", action="store_true", help="build the shifted-SRS table for every size (1.6 GiB at 2^20)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import zk_cryptography_amd as zk
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd.field import R_MOD
    from zk_cryptography_amd.kzg import _commit_begin

    lib = N.lib()
    out = {"metric": "plonk_prove", "device": torch.cuda.get_device_name(0), "table": bool(a.table)}
    times = {}
    for log_n in [int(s) for s in a.sizes.split(",")]:
        n = 1 << log_n
        ctx = N.Context.get()
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()
        wa, wb = dev(zk.Fr.synthetic(n, 1)), dev(zk.Fr.synthetic(n, 2))
        wc = torch.empty_like(wa)
        N.check(lib.zkhip_pointwise_mul(ctx.handle, N.ptr(wa), N.ptr(wb), C.c_size_t(n), N.ptr(wc)), "a * b")
        x = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
        x[1] = dev(zk.Fr.from_ints([1]))[0]
        s1 = torch.empty_like(wa)                                  # the evaluations of X over the domain: w^i
        N.check(lib.zkhip_domain_transform(ctx.handle, N.ptr(x), C.c_size_t(2), N.ptr(s1), C.c_uint32(log_n), C.c_int(0)), "w^i")
        s2, s3 = torch.empty_like(wa), torch.empty_like(wa)
        N.check(lib.zkhip_mle_elementwise(ctx.handle, C.c_int(0), N.ptr(s1), N.ptr(s1), None, C.c_size_t(n), C.c_size_t(n), N.ptr(s2)), "2 w^i")
        N.check(lib.zkhip_mle_elementwise(ctx.handle, C.c_int(0), N.ptr(s2), N.ptr(s1), None, C.c_size_t(n), C.c_size_t(n), N.ptr(s3)), "3 w^i")
        zero = torch.zeros_like(wa)
        const = lambda v: dev(zk.Fr.from_ints([v])).repeat(n, 1).contiguous()
        cpi = zk.CommonPreprocessedInput(n, zero, zero, const(1), const(R_MOD - 1), zero, s1, s2, s3)
        wit = zk.Witness(wa, wb, wc, zero)
        srs = zk.UnivariateKZG.generate_srs(zk.Fr.synthetic(1, 3)[0], n + 5, g2=True)
        if a.table:
            srs.precompute()
        prover = zk.PlonkProver(cpi, srs)
        bl = [7 + i for i in range(11)]
        proof = prover.prove(wit, blinding=bl)                     # warm-up: key, twiddles, workspaces
        v = zk.VerifierPreprocessedInput.vpi(srs, cpi)
        assert zk.PlonkVerifier(n, proof, srs, v).verify(wit.public_poly)
        ms = _med(lambda: prover.prove(wit, blinding=bl), a.reps)
        times[log_n] = ms
        out["prove_ms_n%d" % log_n] = round(ms, 3)
        N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile")
        prover.prove(wit, blinding=bl)
        split, total = dict.fromkeys(GROUPS, 0.0), 0.0
        for k in KERNELS:
            t = C.c_double(0)
            N.check(lib.zkhip_profile_read(ctx.handle, k.encode(), C.byref(t), None, None), "profile_read")
            for g, prefixes in GROUPS.items():
                if k.startswith(prefixes):
                    split[g] += t.value
                    total += t.value
        N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile")
        split["host_and_idle"] = max(0.0, ms - total)
        out["split_ms_n%d" % log_n] = {g: round(t, 3) for g, t in split.items()}
        # the same nine commits alone: (n + 2) x 3, n + 3, (n + 6, n + 1, n + 1), (n + 5, n + 2), three in flight
        scal = dev(zk.Fr.synthetic(n + 6, 4))
        table = srs.table

        def commits():
            for group in ((n + 2, n + 2, n + 2), (n + 3,), (n + 6, n + 1, n + 1), (n + 5, n + 2)):
                pend = [_commit_begin(srs.powers_of_tau_in_g1, srs.inf, len(srs), scal, m, False, table) for m in group]
                for p in pend:
                    p.wait()
        commits()
        cms = _med(commits, a.reps)
        out["commits_alone_ms_n%d" % log_n] = round(cms, 3)
        out["ratio_to_commits_n%d" % log_n] = round(ms / cms, 3)
        del prover, cpi, srs
        torch.cuda.empty_cache()
    if 16 in times and 18 in times:
        out["scaling_18_over_16"] = round(times[18] / times[16], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
