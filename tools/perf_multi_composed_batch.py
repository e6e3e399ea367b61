"""us per proof: MultiComposedSumcheckProver.prove_partial_batch against a loop of prove_partial, by term shape, size and batch, in
ONE process, through the Python mirror and through the raw C ABI (every argument prepared beforehand: what a C or C++ caller pays).
The legs are timed in turn, repetition by repetition, after a warm-up of every shape (what else runs on the host then touches all of
them alike); every figure is the median over the repetitions with its quartiles; wall time around work that ends in a
synchronisation.  The batch's outputs are compared with the loop's on the same inputs first: a difference fails the run.
prove_batch (partial = 0: the table bytes are hashed on the host first) is timed at two sizes beside prove_partial_batch and beside
hashlib's SHA-256 over the same number of bytes, which bounds that route.
Every GPU step runs under an alarm of its own: a step that hangs ends the process.
usage (GPU box): python tools/perf_multi_composed_batch.py [--out FILE] [--json FILE] [--reps N] [--batches B ...] [--shapes S ...]
The table replaces what stands between the two marker lines of FILE (default profiles/multi_composed_batch/NOTES.md); the rest of
FILE is kept.  The JSON line (default profiles/multi_composed_batch/perf_line.json) holds every figure."""
import argparse, ctypes as C, hashlib, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N

BEGIN, END = "<!-- perf_multi_composed_batch: begin -->", "<!-- perf_multi_composed_batch: end -->"
SHAPES = ("2,2:4", "2,2:8", "2,2:10", "2,2:12", "2,2:14", "2,3:8", "2,3:12")
BATCHES = (1, 2, 4, 16, 64, 256, 1024)
FULL = ("2,2:8", "2,2:12")          # prove_batch, B = 64
P = zk.MultiComposedSumcheckProver


def step(seconds, work):
    """work() under its own time limit (SIGALRM's default action ends the process: nothing more is started on the GPU after a hang)"""
    signal.alarm(seconds)
    try:
        return work()
    finally:
        signal.alarm(0)


def timed_in_turn(works, reps):
    ts = {k: [] for k in works}
    for _ in range(reps):
        for k, w in works.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w()
            ts[k].append(time.perf_counter() - t0)
    return ts


def quartiles_us(ts, B):
    q = statistics.quantiles(ts, n=4)
    return [round(1e6 * v / B, 3) for v in (q[0], statistics.median(ts), q[2])]


def tables(count, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat = torch.randint(0, 2 ** 62, (count * n, 4), dtype=torch.int64, device="cuda", generator=g)
    return [zk.Multilinear(flat[i * n:(i + 1) * n]) for i in range(count)]


def claims_of(tabs, sizes, B):
    T, out = sum(sizes), []
    for b in range(B):
        at, terms = b * T, []
        for k in sizes:
            terms.append(zk.ComposedMultilinear(tabs[at:at + k]))
            at += k
        out.append(terms)
    return out


def raw(tabs, sizes, B, log_n, sums, partial, batched):
    """the batch, or the loop of single calls, through the C ABI"""
    T = sum(sizes)
    lib, h = N.lib(), tabs[0]._ctx.handle
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    sz = (C.c_uint32 * len(sizes))(*sizes)
    lens = np.zeros((B, log_n), dtype=np.uint32)
    rp, ch = np.zeros((B, log_n, 7, 2, 4), dtype=np.uint64), np.zeros((B, log_n, 4), dtype=np.uint64)
    s = np.ascontiguousarray(sums[:B])
    if batched:
        ptrs = (C.c_void_p * (B * T))(*[t.evaluations.data_ptr() for t in tabs[:B * T]])
        ready = (h, C.c_uint32(B), ptrs, sz, C.c_uint32(len(sizes)), C.c_size_t(1 << log_n), vp(s), C.c_int(partial), vp(lens), vp(rp), vp(ch))
        call = lambda _alive=(s, lens, rp, ch): N.check(lib.zkhip_multi_composed_prove_batch(*ready), "batch")   # noqa: E731
    else:
        each = [((C.c_void_p * T)(*[t.evaluations.data_ptr() for t in tabs[b * T:(b + 1) * T]]), vp(s[b]), vp(lens[b]), vp(rp[b]), vp(ch[b])) for b in range(B)]

        nt, nn, pp = C.c_uint32(len(sizes)), C.c_size_t(1 << log_n), C.c_int(partial)

        def call(_alive=(s, lens, rp, ch)):       # (the pointers in `each` do not keep their arrays alive)
            for p, sb, lb, rb, cb in each:
                N.check(lib.zkhip_multi_composed_prove(h, p, sz, nt, nn, sb, pp, lb, rb, cb), "single")
    return call, (lens, rp, ch)


def same_mirror(a, b):
    assert len(a) == len(b)
    for (pa, ca), (pb, cb) in zip(a, b):
        assert pa.to_bytes() == pb.to_bytes() and np.array_equal(ca, cb) and np.array_equal(pa.sum, pb.sum)


def same_raw(a, b):
    (la, ra, ca), (lb, rb, cb) = a, b
    assert np.array_equal(la, lb) and np.array_equal(ca, cb)
    keep = np.arange(7)[None, None, :] < la[:, :, None]          # the monomials of a round up to its length
    assert np.array_equal(ra[keep], rb[keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_composed_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "multi_composed_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--shapes", type=str, nargs="*", default=list(SHAPES), help="K,K,..:log_n ...")
    ap.add_argument("--full", type=str, nargs="*", default=list(FULL), help="shapes for prove_batch at B = 64")
    args = ap.parse_args()
    assert args.reps >= 7, "the median of at least seven repetitions"
    rows, full_rows = [], []
    fmt = lambda v: "%.2f / %.2f / %.2f" % tuple(v)   # noqa: E731
    lines = ["| term sizes | entries per table | B | loop of `prove_partial`, us per proof (q1 / median / q3) | `prove_partial_batch` | loop through the C ABI | batch through the C ABI | loop / batch (mirror) | loop / batch (C ABI) | batch kernel |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for spec in args.shapes:
        sizes, log_n = [int(v) for v in spec.split(":")[0].split(",")], int(spec.split(":")[1])
        T, bmax = sum(sizes), max(args.batches)
        tabs = step(300, lambda: tables(bmax * T, 1 << log_n, 70 + 8 * T + log_n))
        claims = claims_of(tabs, sizes, bmax)
        sums = np.zeros((bmax, 4), dtype=np.uint64)      # every proof absorbs a zero sum: the prover does not check it
        bmin = N.lib().zkhip_multi_composed_batch_min((C.c_uint32 * len(sizes))(*sizes), C.c_uint32(len(sizes)), C.c_size_t(1 << log_n))
        for B in args.batches:
            raw_loop, out_loop = raw(tabs, sizes, B, log_n, sums, 1, False)
            raw_batch, out_batch = raw(tabs, sizes, B, log_n, sums, 1, True)
            works = {"loop": lambda: [P.prove_partial(c, s) for c, s in zip(claims[:B], sums[:B])],
                     "batch": lambda: P.prove_partial_batch(claims[:B], sums[:B]), "loop_raw": raw_loop, "batch_raw": raw_batch}
            got = {name: step(300, w) for name, w in works.items()}                 # warm-up of every leg, and the same proofs
            same_mirror(got["batch"], got["loop"])
            same_raw(out_batch, out_loop)
            ts = step(900, lambda: timed_in_turn(works, args.reps))
            q = {name: quartiles_us(v, B) for name, v in ts.items()}
            rows.append({"term_sizes": sizes, "log_n": log_n, "batch": B, "on_kernel": bool(bmin and B >= bmin), "us_per_proof": q})
            lines.append("| %s | 2^%d | %d | %s | %s | %s | %s | %.2f | %.2f | %s |" % (sizes, log_n, B, fmt(q["loop"]), fmt(q["batch"]), fmt(q["loop_raw"]), fmt(q["batch_raw"]),
                                                                                q["loop"][1] / q["batch"][1], q["loop_raw"][1] / q["batch_raw"][1],
                                                                                "yes" if bmin and B >= bmin else "no"))
            print(lines[-1], flush=True)
        del tabs, claims
    flines = ["| term sizes | entries per table | B | `prove_partial_batch`, us per proof (q1 / median / q3) | `prove_batch` | loop of `prove` | hashlib SHA-256 of the same bytes | (prove_batch - prove_partial_batch) / prove_batch |",
              "|---|---|---|---|---|---|---|---|"]
    for spec in args.full:
        sizes, log_n, B = [int(v) for v in spec.split(":")[0].split(",")], int(spec.split(":")[1]), 64
        T = sum(sizes)
        tabs = step(300, lambda: tables(B * T, 1 << log_n, 90 + 8 * T + log_n))
        claims, sums = claims_of(tabs, sizes, B), np.zeros((B, 4), dtype=np.uint64)
        blob = [bytes(T * (32 << log_n)) for _ in range(B)]
        works = {"partial_batch": lambda: P.prove_partial_batch(claims, sums), "full_batch": lambda: P.prove_batch(claims, sums),
                 "full_loop": lambda: [P.prove(c, s) for c, s in zip(claims, sums)], "hashlib": lambda: [hashlib.sha256(x).digest() for x in blob]}
        got = {name: step(300, w) for name, w in works.items()}
        same_mirror(got["full_batch"], got["full_loop"])
        ts = step(900, lambda: timed_in_turn(works, args.reps))
        q = {name: quartiles_us(v, B) for name, v in ts.items()}
        share = (q["full_batch"][1] - q["partial_batch"][1]) / q["full_batch"][1]
        full_rows.append({"term_sizes": sizes, "log_n": log_n, "batch": B, "us_per_proof": q, "table_bytes_route_share": round(share, 3)})
        flines.append("| %s | 2^%d | %d | %s | %s | %s | %s | %.2f |" % (sizes, log_n, B, fmt(q["partial_batch"]), fmt(q["full_batch"]), fmt(q["full_loop"]), fmt(q["hashlib"]), share))
        print(flines[-1], flush=True)
        del tabs, claims
    record = {"tool": "perf_multi_composed_batch", "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "figures": "us per proof: first quartile, median, third quartile", "rows": rows, "prove_batch_rows": full_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(json.dumps(record) + "\n")
    print(json.dumps(record), flush=True)
    text = "\n".join([BEGIN, "", "First quartile / median / third quartile of %d repetitions, the columns timed in turn in one process, `%s`."
                      % (args.reps, torch.cuda.get_device_name(0)), ""] + lines + ["", "`prove_batch` (partial = 0), B = 64:", ""] + flines + ["", END])
    old = open(args.out).read() if os.path.exists(args.out) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text + old[old.index(END) + len(END):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + text + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(new)


if __name__ == "__main__":
    main()
