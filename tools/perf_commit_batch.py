"""ms per polynomial of B commitments against one SRS, three ways, by size, batch and plain points / shifted-SRS table, in ONE process:
  (a) a loop of zkhip_kzg_commit / zkhip_kzg_commit_table;
  (b) the same commits three in flight (zkhip_kzg_commit_begin / _end): the best a caller had before the batch call;
  (c) zkhip_kzg_commit_polys, and beside it the Python mirror (MultilinearKZG.commitment_batch) of the same call.
The three legs alternate repetition by repetition; a cell reports their medians and the spread (quartile 3 - quartile 1, the largest
of the three legs) -- a batch "wins" where (c) is below the better of (a) and (b) by more than that spread.  The route and the chunks the
planner chose (zkhip_commit_polys_plan_info) stand beside every cell.  Every GPU step runs under an alarm of its own: a step that hangs
ends the process.
usage (GPU box): python tools/perf_commit_batch.py [--out FILE] [--json FILE] [--reps N] [--batches B ...] [--plain-only | --table-only] [log_n ...]
The table replaces what stands between the two marker lines of FILE (default profiles/commit_batch/NOTES.md); the rest of FILE is kept."""
import argparse, ctypes as C, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N

BEGIN, END = "<!-- perf_commit_batch: begin -->", "<!-- perf_commit_batch: end -->"
ROUTES = ("single commits", "short", "bucket")
SCALAR_BYTES_MAX = 1 << 30          # B is capped where 32 n B bytes of scalars pass this


def step(seconds, work):
    """work() under its own time limit (SIGALRM's default action ends the process: nothing more is started on the GPU after a hang)"""
    signal.alarm(seconds)
    try:
        return work()
    finally:
        signal.alarm(0)


def timed(work):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    work()                                      # every leg ends in a synchronisation of its own
    return 1e3 * (time.perf_counter() - t0)


def quartile_spread(ts):
    q = statistics.quantiles(ts, n=4)
    return q[2] - q[0]


class Legs:
    def __init__(self, srs, polys, table):
        self.srs, self.polys, self.table = srs, polys, table
        self.ctx = N.Context.get(srs.powers_of_tau_in_g1.device.index)
        self.n = len(srs)
        self.lib = N.lib()
        vp = C.c_void_p
        self.pts, self.inf = vp(srs.powers_of_tau_in_g1.data_ptr()), vp(srs.inf.data_ptr())
        self.tab = vp(srs.table.data_ptr()) if table else None
        b = len(polys)
        self.xy = np.zeros((b, 12), dtype=np.uint64)
        self.oinf = np.zeros(b, dtype=np.uint8)
        self.ptrs = (vp * b)(*[p.evaluations.data_ptr() for p in polys])
        self.lens = (C.c_size_t * b)(*[self.n] * b)

    def out(self, k):
        return C.c_void_p(self.xy.ctypes.data + 96 * k), C.c_void_p(self.oinf.ctypes.data + k)

    def loop(self):
        n = C.c_size_t(self.n)
        for k, p in enumerate(self.polys):
            sc = C.c_void_p(p.evaluations.data_ptr())
            if self.table:
                st = self.lib.zkhip_kzg_commit_table(self.ctx.handle, self.tab, self.inf, n, sc, n, C.c_int(1), *self.out(k))
            else:
                st = self.lib.zkhip_kzg_commit(self.ctx.handle, self.pts, self.inf, n, sc, n, C.c_int(1), *self.out(k))
            N.check(st, "commit")

    def in_flight(self):
        n, pend = C.c_size_t(self.n), []
        for k, p in enumerate(self.polys):
            if len(pend) == 3:
                j, t = pend.pop(0)
                N.check(self.lib.zkhip_kzg_commit_end(self.ctx.handle, t, *self.out(j)), "commit_end")
            t = C.c_uint32(0)
            N.check(self.lib.zkhip_kzg_commit_begin(self.ctx.handle, None if self.table else self.pts, self.tab, self.inf, n,
                                                    C.c_void_p(p.evaluations.data_ptr()), n, C.c_int(1), C.byref(t)), "commit_begin")
            pend.append((k, t))
        for j, t in pend:
            N.check(self.lib.zkhip_kzg_commit_end(self.ctx.handle, t, *self.out(j)), "commit_end")

    def batch(self):
        vp = C.c_void_p
        N.check(self.lib.zkhip_kzg_commit_polys(self.ctx.handle, None if self.table else self.pts, self.tab, self.inf, C.c_size_t(self.n),
                                                C.c_uint32(len(self.polys)), self.ptrs, self.lens, C.c_int(1), vp(self.xy.ctypes.data),
                                                vp(self.oinf.ctypes.data)), "commit_polys")

    def mirror(self):
        return zk.MultilinearKZG.commitment_batch(self.polys, self.srs)

    def plan(self):
        route, n_chunks = C.c_uint32(0), C.c_uint32(0)
        counts = (C.c_uint32 * len(self.polys))()
        N.check(self.lib.zkhip_commit_polys_plan_info(C.c_size_t(self.n), self.lens, C.c_uint32(len(self.polys)), C.c_int(1 if self.table else 0),
                                                      C.byref(route), C.byref(n_chunks), counts, None), "plan_info")
        return ROUTES[route.value], list(counts[:n_chunks.value])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commit_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "commit_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 2, 3, 8, 64, 256])
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--table-only", action="store_true")
    ap.add_argument("log_n", type=int, nargs="*", default=[8, 12, 13, 14, 16, 18, 20])
    args = ap.parse_args()
    assert args.reps >= 8, "quartiles of at least 8 repetitions"
    head = ["| scalars | B | points | route (chunks) | (a) loop | (b) three in flight | (c) batch call | mirror of (c) | spread | better of (a), (b) / (c) |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    lines, records = [], []
    for log_n in args.log_n:
        n = 1 << log_n
        batches = [b for b in args.batches if 32 * n * b <= SCALAR_BYTES_MAX]
        srs = step(300, lambda: zk.TrustedSetup.setup(zk.Fr.random(log_n, 5)))
        g = torch.Generator(device="cuda").manual_seed(3)
        polys = [zk.Multilinear(torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)) for _ in range(max(batches))]
        for table in ([False] if args.plain_only else [True] if args.table_only else [False, True]):
            if table:
                step(300, srs.precompute)
            for B in batches:
                legs = Legs(srs, polys[:B], table)
                route, chunks = legs.plan()
                # warm-up, and the same commitments from every leg
                step(300, legs.loop); want = (legs.xy.copy(), legs.oinf.copy())
                for leg in (legs.in_flight, legs.batch):
                    legs.xy[:] = 0; legs.oinf[:] = 7
                    step(300, leg)
                    assert (legs.oinf == want[1]).all() and (legs.xy == want[0]).all()
                got = step(300, legs.mirror) if (table or n > zk.TrustedSetup.SMALL_SRS) else None      # (the mirror gives a small SRS its table)
                assert got is None or all((gk.xy == want[0][k]).all() for k, gk in enumerate(got))
                ts = {"loop": [], "in_flight": [], "batch": [], "mirror": []}
                for _ in range(args.reps):                       # the legs alternate
                    ts["loop"].append(step(300, lambda: timed(legs.loop)))
                    ts["in_flight"].append(step(300, lambda: timed(legs.in_flight)))
                    ts["batch"].append(step(300, lambda: timed(legs.batch)))
                    if got is not None:
                        ts["mirror"].append(step(300, lambda: timed(legs.mirror)))
                med = {k: statistics.median(v) / B if v else None for k, v in ts.items()}
                spread = max(quartile_spread(ts[k]) for k in ("loop", "in_flight", "batch")) / B
                best = min(med["loop"], med["in_flight"])
                rec = {"log_n": log_n, "batch": B, "table": table, "route": route, "chunks": chunks, "ms_per_poly": med, "spread_ms_per_poly": spread,
                       "ratio": best / med["batch"], "reps": args.reps}
                records.append(rec)
                lines.append("| 2^%d | %d | %s | %s (%s) | %.4f | %.4f | %.4f | %s | %.4f | %.2f |" % (
                    log_n, B, "table" if table else "plain", route, " ".join(str(c) for c in chunks), med["loop"], med["in_flight"], med["batch"],
                    "%.4f" % med["mirror"] if med["mirror"] is not None else "-", spread, best / med["batch"]))
                print(lines[-1], flush=True)
        del polys, srs
        torch.cuda.empty_cache()
    text = "\n".join([BEGIN, "", "ms per polynomial; medians of %d alternating repetitions per leg, one process, `%s`; spread = the largest quartile "
                      "range of the three legs." % (args.reps, torch.cuda.get_device_name(0)), ""] + head + lines + ["", END])
    old = open(args.out).read() if os.path.exists(args.out) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text + old[old.index(END) + len(END):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + text + "\n"
    for path in (args.out, args.json):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(new)
    with open(args.json, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
