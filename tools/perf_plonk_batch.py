"""Measurement: PlonkProver.prove_batch (zkhip_plonk_prove_batch) against the loop of zkhip_plonk_prove on the same key, witnesses and
blindings, per circuit size n and batch B.  Both are warmed, then timed in alternating windows, every window closed by a device
synchronise and long enough (--window seconds) to dwarf the timer; the figure is the median of --repeats windows per proof and the
spread is (max - min) / median over them.  At (8, 64) and (2^11, 64) one profiled batch call is split by the library's own launch
scopes.  Prints ONE JSON line (profiles/plonk_batch/perf_line.json).

Every size is measured by a child process of its own under `timeout -k 10`, one after the other; the first child that fails ends the
run (nothing more is started on the device behind a fault or a hang), and the line then holds the sizes measured so far and the failure.

The circuit is c = a * b on every row (q_m = 1, q_o = -1) with the identity permutation, as tools/perf_plonk.py: a satisfied witness
that costs nothing to build.  A batch proves that one witness B times, each proof with a blinding of its own.

    python tools/perf_plonk_batch.py [--sizes 8,256,2048,4096,65536] [--batches 1,2,16,64] [--window 0.2] [--repeats 3] [--limit 240]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP_BYTES = 2 << 30                     # the work areas of one batch stay under this: B is capped by it
PROFILED = ((8, 64), (2048, 64))


def circuit(zk, N, lib, ctx, n):
    import numpy as np
    import torch
    from zk_cryptography_amd.field import R_MOD
    log_n = n.bit_length() - 1
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
    return cpi, zk.Witness(wa, wb, wc, zero)


def child(a):
    import numpy as np
    import torch
    import zk_cryptography_amd as zk
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    n = int(a.child)
    lib, ctx = N.lib(), N.Context.get()
    cpi, wit = circuit(zk, N, lib, ctx, n)
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.synthetic(1, 3)[0], n + 5, g2=True)
    prover = zk.PlonkProver(cpi, srs)
    key = plonk._key_for(cpi, srs)
    cols = [plonk._column(v) for v in (wit.a, wit.b, wit.c, wit.public_poly)]
    D = 1
    while D < 3 * n + 6:
        D <<= 1
    fit = max(1, CAP_BYTES // (32 * (13 * (n + 8) + 6 * D)))
    vp = C.c_void_p
    rows, profiles = [], {}
    for batch in sorted({min(int(v), fit) for v in a.batches.split(",")}):
        bl = zk.Fr.from_ints([1000 * b + i + 7 for b in range(batch) for i in range(11)]).reshape(batch, 11, 4)
        ptrs = [(C.c_void_p * batch)(*[cols[j].data_ptr()] * batch) for j in range(4)]
        xy, inf = np.zeros((batch, 9, 12), dtype=np.uint64), np.zeros((batch, 9), dtype=np.uint8)
        ev, ch = np.zeros((batch, 6, 4), dtype=np.uint64), np.zeros((batch, 6, 4), dtype=np.uint64)
        status = np.zeros(batch, dtype=np.int32)
        sxy, sinf, sev, sch = xy.copy(), inf.copy(), ev.copy(), ch.copy()

        def batched():
            N.check(lib.zkhip_plonk_prove_batch(key.handle, C.c_uint32(batch), ptrs[0], ptrs[1], ptrs[2], ptrs[3], bl.ctypes.data_as(vp),
                                                xy.ctypes.data_as(vp), inf.ctypes.data_as(vp), ev.ctypes.data_as(vp), ch.ctypes.data_as(vp),
                                                status.ctypes.data_as(vp)), "prove_batch")

        def loop():
            for b in range(batch):
                N.check(lib.zkhip_plonk_prove(key.handle, N.ptr(cols[0]), N.ptr(cols[1]), N.ptr(cols[2]), N.ptr(cols[3]), bl[b].ctypes.data_as(vp),
                                              sxy[b].ctypes.data_as(vp), sinf[b].ctypes.data_as(vp), sev[b].ctypes.data_as(vp), sch[b].ctypes.data_as(vp)),
                        "prove")

        def window(fn, reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t

        reps = {}
        for name, fn in (("batch", batched), ("loop", loop)):
            window(fn, 1)                                              # warm-up: key, tables, work areas, clocks
            reps[name] = max(1, int(a.window / window(fn, 1)) + 1)
        assert np.array_equal(xy, sxy) and np.array_equal(ev, sev) and np.array_equal(ch, sch)      # the same proofs, or the figures mean nothing
        took = {"batch": [], "loop": []}
        for _ in range(a.repeats):
            for name, fn in (("batch", batched), ("loop", loop)):
                took[name].append(window(fn, reps[name]))
        row = {"n": n, "batch": batch, "chunk": int(lib.zkhip_plonk_batch_chunk(key.handle)), "short_commits": srs.table is not None}
        for name in ("batch", "loop"):
            per = sorted(t / reps[name] / batch for t in took[name])
            med = per[len(per) // 2]
            row[name + "_ms_per_proof"] = round(med * 1e3, 4)
            row[name + "_spread"] = round((per[-1] - per[0]) / med, 4)
            row[name + "_window_s"] = round(min(took[name]), 3)
        row["speedup"] = round(row["loop_ms_per_proof"] / row["batch_ms_per_proof"], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)             # progress; the result is the one line on stdout
        if (n, batch) in PROFILED:
            mx = 1024
            N.check(lib.zkhip_profile_enable(ctx.handle, 1), "profile")
            try:
                t0 = time.perf_counter()
                batched()
                wall = time.perf_counter() - t0
                names, st, sp, cnt = C.create_string_buffer(32 * mx), (C.c_double * mx)(), (C.c_double * mx)(), C.c_uint32(0)
                N.check(lib.zkhip_profile_timeline(ctx.handle, mx, names, st, sp, C.byref(cnt)), "profile_timeline")
            finally:
                N.check(lib.zkhip_profile_enable(ctx.handle, 0), "profile")
            scopes = {}
            for i in range(min(cnt.value, mx)):
                name = names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode()
                ms, k = scopes.get(name, (0.0, 0))
                scopes[name] = (ms + (sp[i] - st[i]) / 1e3, k + 1)
            profiles["n%d_b%d" % (n, batch)] = {"wall_ms": round(wall * 1e3, 3), "launch_scopes": int(cnt.value),
                                                "scope_ms": {k: [round(v[0], 4), v[1]] for k, v in sorted(scopes.items())}}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows, "profiles": profiles}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,256,2048,4096,65536")
    ap.add_argument("--batches", default="1,2,16,64")
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    out = {"tool": "perf_plonk_batch", "window_s": a.window, "repeats": a.repeats, "rows": [], "profiles": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--batches", a.batches,
               "--window", str(a.window), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                                   # nothing more on the device behind a failure
            out["stopped"] = {"n": n, "returncode": r.returncode}
            break
        part = json.loads(r.stdout.strip().splitlines()[-1])
        out["device"] = part["device"]
        out["rows"] += part["rows"]
        out["profiles"].update(part["profiles"])
    print(json.dumps(out), flush=True)
    return 1 if "stopped" in out else 0


if __name__ == "__main__":
    sys.exit(main())
