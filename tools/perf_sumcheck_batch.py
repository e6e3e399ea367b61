"""us per proof: Sumcheck.prove_batch / ComposedSumcheck.prove_batch against what a caller can do without them, by size and batch, in
ONE process: a loop of single prove() calls and, for the basic prover, eight proofs in flight through prove_begin() / wait().  The
three are timed in turn, repetition by repetition (what else runs on the host then touches all of them alike); every figure is the
median over the repetitions with its quartiles.  Every proof absorbs the default (zero) sum: the cheapest single call there is.
Every GPU step runs under an alarm of its own: a step that hangs ends the process.
usage (GPU box): python tools/perf_sumcheck_batch.py [--out FILE] [--json FILE] [--reps N] [--batches B ...]
The table replaces what stands between the two marker lines of FILE (default profiles/sumcheck_batch/NOTES.md); the rest of FILE is
kept.  The JSON line (default profiles/sumcheck_batch/perf_line.json) holds every figure."""
import argparse, collections, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk

BEGIN, END = "<!-- perf_sumcheck_batch: begin -->", "<!-- perf_sumcheck_batch: end -->"
BASIC_LOGS = (4, 8, 12, 14, 16)
COMPOSED = ((2, 4), (2, 8), (2, 10), (2, 12), (5, 4), (5, 8), (5, 10), (5, 12))
BATCHES = (1, 2, 64, 256, 1024)
IN_FLIGHT = 8


def step(seconds, work):
    """work() under its own time limit (SIGALRM's default action ends the process: nothing more is started on the GPU after a hang)"""
    signal.alarm(seconds)
    try:
        return work()
    finally:
        signal.alarm(0)


def timed_in_turn(works, reps):
    """{name: [seconds per repetition]}: one repetition of every entry of `works` after the other, `reps` times (each ends in a
    stream synchronisation of its own)"""
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


def in_flight(polys):
    pend, out = collections.deque(), []
    for p in polys:
        if len(pend) == IN_FLIGHT:
            out.append(pend.popleft().wait())
        pend.append(zk.Sumcheck(p).prove_begin())
    while pend:
        out.append(pend.popleft().wait())
    return out


def same(a, b, basic):
    for (pa, ca), (pb, cb) in zip(a, b):
        ra, rb = (pa.univariate_poly, pb.univariate_poly) if basic else (pa.round_polys, pb.round_polys)
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    return len(a) == len(b)


def raw_batch(tabs, B, k, log_n, basic):
    """the same batch through the C ABI with every argument prepared beforehand: what a C or C++ caller pays (the Python mirror
    builds B proof objects around it)"""
    import ctypes as C
    from zk_cryptography_amd import _native as N
    ptrs = (C.c_void_p * (B * k))(*[t.evaluations.data_ptr() for t in tabs[:B * k]])
    s, zeros = np.empty((B, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
    rp, ch = np.empty((B, log_n, k + 1, 4), dtype=np.uint64), np.empty((B, log_n, 4), dtype=np.uint64)
    h, vp = tabs[0]._ctx.handle, lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if basic:
        return lambda: N.check(N.lib().zkhip_sumcheck_prove_batch(h, C.c_uint32(B), ptrs, C.c_size_t(1 << log_n), vp(zeros), vp(s), vp(rp), vp(ch)), "batch")
    return lambda: N.check(N.lib().zkhip_composed_prove_batch(h, C.c_uint32(B), ptrs, C.c_uint32(k), C.c_size_t(1 << log_n), vp(rp), vp(ch)), "batch")


def tables(count, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat = torch.randint(0, 2 ** 62, (count * n, 4), dtype=torch.int64, device="cuda", generator=g)
    return [zk.Multilinear(flat[i * n:(i + 1) * n]) for i in range(count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sumcheck_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--basic", type=int, nargs="*", default=list(BASIC_LOGS))
    ap.add_argument("--composed", type=str, nargs="*", default=["%d:%d" % kc for kc in COMPOSED], help="K:log_n ...")
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 repetitions"
    bmax = max(args.batches)
    rows = []
    lines = ["| prover | entries per table | B | loop of `prove`, us per proof (q1 / median / q3) | %d in flight | `prove_batch` | the same call through the C ABI | loop / batch | in flight / batch |" % IN_FLIGHT,
             "|---|---|---|---|---|---|---|---|---|"]

    def measure(label, k, log_n, works_of):
        for B in args.batches:
            works = works_of(B)
            got = {name: step(300, w) for name, w in works.items()}                 # warm-up of every shape, and the same proofs
            assert all(same(got["batch"], v, k == 0) for v in got.values() if v is not None)
            ts = step(900, lambda: timed_in_turn(works, args.reps))
            q = {name: quartiles_us(v, B) for name, v in ts.items()}
            rows.append({"prover": label, "k": max(k, 1), "log_n": log_n, "batch": B, "us_per_proof": q})
            fmt = lambda v: "%.2f / %.2f / %.2f" % tuple(v)   # noqa: E731
            fl = q.get("in_flight")
            lines.append("| %s | 2^%d | %d | %s | %s | %s | %s | %.2f | %s |" % (label, log_n, B, fmt(q["loop"]), fmt(fl) if fl else "-", fmt(q["batch"]),
                                                                             fmt(q["batch_raw"]), q["loop"][1] / q["batch"][1],
                                                                             "%.2f" % (fl[1] / q["batch"][1]) if fl else "-"))
            print(lines[-1], flush=True)

    for log_n in args.basic:
        polys = step(300, lambda: tables(bmax, 1 << log_n, 3 + log_n))
        zeros = np.zeros((bmax, 4), dtype=np.uint64)
        measure("basic", 0, log_n, lambda B: {"loop": lambda: [zk.Sumcheck(p).prove() for p in polys[:B]],
                                               "in_flight": lambda: in_flight(polys[:B]),
                                               "batch": lambda: zk.Sumcheck.prove_batch(polys[:B], zeros[:B]),
                                               "batch_raw": raw_batch(polys, B, 1, log_n, True)})
        del polys
    for spec in args.composed:
        k, log_n = (int(v) for v in spec.split(":"))
        flat = step(300, lambda: tables(bmax * k, 1 << log_n, 50 + 8 * k + log_n))
        cps = [zk.ComposedMultilinear(flat[b * k:(b + 1) * k]) for b in range(bmax)]
        measure("composed K = %d" % k, k, log_n, lambda B: {"loop": lambda: [zk.ComposedSumcheck(cp).prove() for cp in cps[:B]],
                                                            "batch": lambda: zk.ComposedSumcheck.prove_batch(cps[:B]),
                                                            "batch_raw": raw_batch(flat, B, k, log_n, False)})
        del flat, cps
    record = {"tool": "perf_sumcheck_batch", "device": torch.cuda.get_device_name(0), "reps": args.reps, "in_flight": IN_FLIGHT,
              "figures": "us per proof: first quartile, median, third quartile", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(json.dumps(record) + "\n")
    text = "\n".join([BEGIN, "", "First quartile / median / third quartile of %d repetitions, the columns timed in turn in one process, `%s`."
                      % (args.reps, torch.cuda.get_device_name(0)), ""] + lines + ["", END])
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
