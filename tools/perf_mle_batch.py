"""us per evaluation: Multilinear.evaluation_batch / zkhip_mle_evaluation_batch against what a caller can do without them -- a loop of
single evaluation() calls -- by size and batch, in ONE process, through the Python mirror and through the C ABI with every argument
prepared beforehand.  The four are timed in turn, repetition by repetition (what else runs on the host then touches all of them
alike); every call ends in its own synchronisation and the host clock stands around it.  Every figure is the median over the
repetitions with its quartiles; the spread of a row is the widest quartile distance of its columns.
Every GPU step runs under an alarm of its own: a step that hangs ends the process.
usage (GPU box): python tools/perf_mle_batch.py [--out FILE] [--json FILE] [--reps N] [--batches B ...] [--logs L ...] [--trace]
The table replaces what stands between the two marker lines of FILE (default profiles/mle_batch/NOTES.md); the rest of FILE is kept.
The JSON line (default profiles/mle_batch/perf_line.json) holds every figure."""
import argparse, ctypes as C, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N
if os.environ.get("ZKHIP_LIB"):          # another build of the library, for same-box A/Bs of compile-time choices (tools/bench_with_lib.py)
    N.LIB_PATH = os.path.abspath(os.environ["ZKHIP_LIB"])

BEGIN, END = "<!-- perf_mle_batch: begin -->", "<!-- perf_mle_batch: end -->"
LOGS = (4, 8, 12, 14, 16)
BATCHES = (1, 2, 64, 1024)


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


def raw_calls(polys, pts, B, log_n):
    """(loop of zkhip_mle_evaluation, zkhip_mle_evaluation_batch) with every argument built beforehand: what a C caller pays"""
    lib, h, n = N.lib(), polys[0]._ctx.handle, C.c_size_t(1 << log_n)
    out = np.empty((B, 4), dtype=np.uint64)
    ptrs = (C.c_void_p * B)(*[p.evaluations.data_ptr() for p in polys[:B]])
    singles = [(C.c_void_p(p.evaluations.data_ptr()), pts[b].ctypes.data_as(C.c_void_p), out[b].ctypes.data_as(C.c_void_p)) for b, p in enumerate(polys[:B])]
    vp, nv, op = pts.ctypes.data_as(C.c_void_p), C.c_size_t(log_n), out.ctypes.data_as(C.c_void_p)

    def loop():
        for t, p, o in singles:
            N.check(lib.zkhip_mle_evaluation(h, t, n, p, nv, o), "evaluation")
        return out.copy()

    def batch():
        N.check(lib.zkhip_mle_evaluation_batch(h, B, ptrs, n, vp, nv, op), "evaluation_batch")
        return out.copy()
    return loop, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mle_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--trace", action="store_true", help="only the batch through the C ABI, 2 + 10 calls per shape, nothing written: the run to put under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    if args.trace:
        for log_n in args.logs:
            polys = step(300, lambda: tables(max(args.batches), 1 << log_n, 3 + log_n))
            pts = zk.Fr.synthetic(max(args.batches) * log_n, 0x5EED000000003001 + log_n).reshape(-1, log_n, 4)
            for B in args.batches:
                _loop, batch = raw_calls(polys, pts, B, log_n)
                step(300, lambda: [batch() for _ in range(12)])
            del polys
        return
    assert args.reps >= 20, "the median of at least 20 repetitions"
    bmax = max(args.batches)
    rows = []
    lines = ["| entries per table | B | regime | loop of `evaluation`, us per evaluation (q1 / median / q3) | `evaluation_batch` | loop through the C ABI | batch through the C ABI | spread | loop / batch (mirror) | loop / batch (C ABI) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    fmt = lambda v: "%.2f / %.2f / %.2f" % tuple(v)   # noqa: E731
    for log_n in args.logs:
        n = 1 << log_n
        polys = step(300, lambda: tables(bmax, n, 3 + log_n))
        pts = zk.Fr.synthetic(bmax * log_n, 0x5EED000000003001 + log_n).reshape(bmax, log_n, 4)
        kmin = N.lib().zkhip_mle_evaluation_batch_min(n)
        for B in args.batches:
            raw_loop, raw_batch = raw_calls(polys, pts, B, log_n)
            works = {"loop": lambda: np.stack([p.evaluation(pts[b]) for b, p in enumerate(polys[:B])]),
                     "batch": lambda: zk.Multilinear.evaluation_batch(polys[:B], pts[:B]),
                     "loop_raw": raw_loop, "batch_raw": raw_batch}
            got = {name: step(300, w) for name, w in works.items()}                 # warm-up of every shape, and the same values
            assert all(np.array_equal(got["loop"], v) for v in got.values())
            ts = step(900, lambda: timed_in_turn(works, args.reps))
            q = {name: quartiles_us(v, B) for name, v in ts.items()}
            spread = max(v[2] - v[0] for v in q.values())
            regime = "single path" if (B == 1 or kmin == 0 or B < kmin) else ("resident" if log_n <= 12 else "2^%d blocks" % (log_n - 12))
            rows.append({"log_n": log_n, "batch": B, "regime": regime, "us_per_evaluation": q, "spread_us": round(spread, 3)})
            lines.append("| 2^%d | %d | %s | %s | %s | %s | %s | %.2f | %.2f | %.2f |" % (log_n, B, regime, fmt(q["loop"]), fmt(q["batch"]), fmt(q["loop_raw"]),
                                                                                      fmt(q["batch_raw"]), spread, q["loop"][1] / q["batch"][1],
                                                                                      q["loop_raw"][1] / q["batch_raw"][1]))
            print(lines[-1], flush=True)
        del polys
    record = {"tool": "perf_mle_batch", "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "figures": "us per evaluation: first quartile, median, third quartile", "rows": rows}
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
