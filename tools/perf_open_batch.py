"""ms per opening: a loop of MultilinearKZG.open against one MultilinearKZG.open_batch, by size and batch, in ONE process, with the
library's profile of a batch of 64 (device time per launch, host fold).  Sizes 2^8 and 2^12 take the batched short path, 2^16 the
sequential fallback (no speedup claimed there).  Every GPU step runs under an alarm of its own: a step that hangs ends the process.
usage (GPU box): python tools/perf_open_batch.py [--out FILE] [--reps N] [log_n ...]
The table replaces what stands between the two marker lines of FILE (default profiles/open_batch/NOTES.md); the rest of FILE is kept."""
import argparse, ctypes as C, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N

BEGIN, END = "<!-- perf_open_batch: begin -->", "<!-- perf_open_batch: end -->"
SCOPES = ("open_batch_steps", "open_batch_planes", "open_batch_reduce", "open_batch_fold")
BATCHES = (1, 2, 16, 64)


def step(seconds, work):
    """work() under its own time limit (SIGALRM's default action ends the process: nothing more is started on the GPU after a hang)"""
    signal.alarm(seconds)
    try:
        return work()
    finally:
        signal.alarm(0)


def median_ms(work, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        work()                                  # both calls end in a stream synchronisation of their own
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def profile(work):
    ctx = N.Context.get()
    N.check(N.lib().zkhip_profile_enable(ctx.handle, 1), "profile_enable")
    try:
        work()
        out = {}
        for name in SCOPES:
            ms, cnt = C.c_double(), C.c_uint64()
            N.check(N.lib().zkhip_profile_read(ctx.handle, name.encode(), C.byref(ms), C.byref(cnt), None), "profile_read")
            out[name] = (ms.value, cnt.value)
    finally:
        N.check(N.lib().zkhip_profile_enable(ctx.handle, 0), "profile_enable")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_batch", "NOTES.md"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("log_n", type=int, nargs="*", default=[8, 12, 16])
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 repetitions"
    lines = ["| entries | B | loop of `open`, ms per opening | `open_batch`, ms per opening | ratio |", "|---|---|---|---|---|"]
    prof_lines = []
    for log_n in args.log_n:
        n, bmax = 1 << log_n, max(BATCHES)
        srs = step(300, lambda: zk.TrustedSetup.setup(zk.Fr.random(log_n, 5)).precompute_open())
        g = torch.Generator(device="cuda").manual_seed(3)
        polys = [zk.Multilinear(torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)) for _ in range(bmax)]
        points = [zk.Fr.random(log_n, 100 + b) for b in range(bmax)]
        for B in BATCHES:
            loop = lambda: [zk.MultilinearKZG.open(p, z, srs) for p, z in zip(polys[:B], points[:B])]        # noqa: E731
            batch = lambda: zk.MultilinearKZG.open_batch(polys[:B], points[:B], srs)                        # noqa: E731
            a, b = step(120, loop), step(120, batch)                                                        # warm-up, and the same proofs
            assert all((x.evaluation == y.evaluation).all() and x.proofs == y.proofs for x, y in zip(a, b))
            t_loop = step(300, lambda: median_ms(loop, args.reps)) / B
            t_batch = step(300, lambda: median_ms(batch, args.reps)) / B
            lines.append("| 2^%d | %d | %.4f | %.4f | %.2f |" % (log_n, B, t_loop, t_batch, t_loop / t_batch))
            print(lines[-1], flush=True)
        if n <= zk.TrustedSetup.SMALL_SRS:
            t0 = time.perf_counter()
            pr = step(120, lambda: profile(lambda: zk.MultilinearKZG.open_batch(polys, points, srs)))
            wall = 1e3 * (time.perf_counter() - t0)
            prof_lines.append("2^%d, B = %d, one profiled call (%.3f ms with the profile on): " % (log_n, bmax, wall) +
                              ", ".join("%s %.3f ms (%d)" % (k, v[0], v[1]) for k, v in pr.items()))
            print(prof_lines[-1], flush=True)
    text = "\n".join([BEGIN, "", "Median of %d repetitions per step, one process, `%s`." % (args.reps, torch.cuda.get_device_name(0)), ""] + lines + [""] +
                     ["Profile (device time between events per launch; `open_batch_fold` is the host fold, bracketed by events on the idle stream):", ""] +
                     ["- " + s for s in prof_lines] + ["", END])
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
