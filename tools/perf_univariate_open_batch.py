"""ms per opening of B univariate KZG openings against one SRS, two ways, by size, batch and plain points / shifted-SRS table, in ONE
process:
  (a) a loop of zkhip_univariate_kzg_open (plain points: the single call takes no table) -- the yardstick;
  (b) zkhip_univariate_kzg_open_batch, with plain points and, where the SRS has a table, with the table; beside it the Python mirror
      (UnivariateKZG.open_batch) of the same call.
The legs alternate repetition by repetition; a cell reports their medians and the spread (quartile 3 - quartile 1, the larger of the
two legs) -- the batch "wins" where (b) is below (a) by more than that spread.  Every GPU step runs under an alarm of its own: a step
that hangs ends the process.
usage (GPU box): python tools/perf_univariate_open_batch.py [--out FILE] [--json FILE] [--reps N] [--batches B ...] [log_n ...]
The table replaces what stands between the two marker lines of FILE (default profiles/univariate_open_batch/NOTES.md); the rest of
FILE is kept."""
import argparse, ctypes as C, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N

BEGIN, END = "<!-- perf_univariate_open_batch: begin -->", "<!-- perf_univariate_open_batch: end -->"
TABLE_MAX_LOG = 16                  # the table of a larger SRS is not built here (2^16 points: 100 MiB)


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
    def __init__(self, srs, polys, zs, table):
        self.srs, self.polys, self.zs, self.table = srs, polys, zs, table
        self.ctx = N.Context.get(srs.powers_of_tau_in_g1.device.index)
        self.lib = N.lib()
        vp = C.c_void_p
        self.pts, self.inf = vp(srs.powers_of_tau_in_g1.data_ptr()), vp(srs.inf.data_ptr())
        self.tab = vp(srs.table.data_ptr()) if table else None
        b = len(polys)
        self.z = np.ascontiguousarray(zs[:b], dtype=np.uint64)
        self.ev = np.zeros((b, 4), dtype=np.uint64)
        self.xy = np.zeros((b, 12), dtype=np.uint64)
        self.oinf = np.zeros(b, dtype=np.uint8)
        self.ptrs = (vp * b)(*[p.coefficients.data_ptr() for p in polys])
        self.lens = (C.c_size_t * b)(*[len(p) for p in polys])

    def loop(self):
        vp, n_points = C.c_void_p, C.c_size_t(len(self.srs))
        for k, p in enumerate(self.polys):
            st = self.lib.zkhip_univariate_kzg_open(self.ctx.handle, vp(p.coefficients.data_ptr()), C.c_size_t(len(p)), vp(self.z.ctypes.data + 32 * k),
                                                    self.pts, self.inf, n_points, vp(self.ev.ctypes.data + 32 * k), vp(self.xy.ctypes.data + 96 * k),
                                                    vp(self.oinf.ctypes.data + k))
            N.check(st, "open")

    def batch(self):
        vp = C.c_void_p
        N.check(self.lib.zkhip_univariate_kzg_open_batch(self.ctx.handle, len(self.polys), self.ptrs, self.lens, vp(self.z.ctypes.data),
                                                         None if self.table else self.pts, self.tab, self.inf, len(self.srs), vp(self.ev.ctypes.data),
                                                         vp(self.xy.ctypes.data), vp(self.oinf.ctypes.data)), "open_batch")

    def mirror(self):
        return zk.UnivariateKZG.open_batch(self.polys, list(self.z), self.srs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "univariate_open_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "univariate_open_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batches", type=int, nargs="*", default=[2, 8, 64])
    ap.add_argument("log_n", type=int, nargs="*", default=[8, 12, 14, 16])
    args = ap.parse_args()
    assert args.reps >= 8, "quartiles of at least 8 repetitions"
    head = ["| coefficients | B | points | (a) loop of open | (b) batch call | mirror of (b) | spread | (a) / (b) |", "|---|---|---|---|---|---|---|---|"]
    lines, records = [], []
    for log_n in args.log_n:
        n = 1 << log_n
        srs = step(300, lambda: zk.UnivariateKZG.generate_srs(zk.Fr.random(1, 5)[0], n - 1))
        g = torch.Generator(device="cuda").manual_seed(3)
        polys = [zk.DenseUnivariatePolynomial(torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)) for _ in range(max(args.batches))]
        zs = zk.Fr.random(max(args.batches), 7)
        for table in ([False, True] if log_n <= TABLE_MAX_LOG else [False]):
            if table:
                step(300, srs.precompute)
            for B in args.batches:
                legs = Legs(srs, polys[:B], zs, table)
                # warm-up, and the same openings from both legs and the mirror
                step(300, legs.loop); want = (legs.ev.copy(), legs.xy.copy(), legs.oinf.copy())
                legs.ev[:] = 0; legs.xy[:] = 0; legs.oinf[:] = 7
                step(300, legs.batch)
                assert (legs.ev == want[0]).all() and (legs.oinf == want[2]).all() and (legs.xy == want[1]).all()
                got = step(300, legs.mirror)
                assert all((gk.proof.xy == want[1][k]).all() and (gk.evaluation == want[0][k]).all() for k, gk in enumerate(got))
                ts = {"loop": [], "batch": [], "mirror": []}
                for _ in range(args.reps):                       # the legs alternate
                    ts["loop"].append(step(300, lambda: timed(legs.loop)))
                    ts["batch"].append(step(300, lambda: timed(legs.batch)))
                    ts["mirror"].append(step(300, lambda: timed(legs.mirror)))
                med = {k: statistics.median(v) / B for k, v in ts.items()}
                spread = max(quartile_spread(ts[k]) for k in ("loop", "batch")) / B
                rec = {"log_n": log_n, "batch": B, "table": table, "ms_per_opening": med, "spread_ms_per_opening": spread, "ratio": med["loop"] / med["batch"],
                       "reps": args.reps}
                records.append(rec)
                lines.append("| 2^%d | %d | %s | %.4f | %.4f | %.4f | %.4f | %.2f |" % (log_n, B, "table" if table else "plain", med["loop"], med["batch"],
                                                                                        med["mirror"], spread, med["loop"] / med["batch"]))
                print(lines[-1], flush=True)
        del polys, srs
        torch.cuda.empty_cache()
    text = "\n".join([BEGIN, "", "ms per opening; medians of %d alternating repetitions per leg, one process, `%s`; spread = the larger quartile "
                      "range of the two legs.  The mirror uses the SRS's table when it has one (an SRS of at most 4096 points builds its own)."
                      % (args.reps, torch.cuda.get_device_name(0)), ""] + head + lines + ["", END])
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
