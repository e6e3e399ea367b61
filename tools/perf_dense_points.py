"""zkhip_dense_points on one MI355X: evaluation at m points against what a caller can do without it -- a loop of m single
DenseUnivariatePolynomial.evaluate calls --, and interpolation (no counterpart to compare with) in milliseconds and field products
per second beside the VALU issue peak bench.py uses.  One process; the columns of a row are timed in turn, repetition by repetition;
every call ends in its own synchronisation and the host clock stands around it.  Every figure is the median over the repetitions with
its quartiles.  Every GPU step runs under an alarm of its own: a step that hangs ends the process.
usage (GPU box): python tools/perf_dense_points.py [--out FILE] [--json FILE] [--reps N]
The tables replace what stands between the two marker lines of FILE (default profiles/dense_points/NOTES.md); the rest of FILE is kept.
The JSON line (default profiles/dense_points/perf_line.json) holds every figure."""
import argparse, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zk_cryptography_amd as zk
from zk_cryptography_amd import _native as N

BEGIN, END = "<!-- perf_dense_points: begin -->", "<!-- perf_dense_points: end -->"
EVAL_LOGS, EVAL_POINTS = (8, 12, 16), (1, 64, 4096)
INTERP = ((1, 1 << 8), (1, 1 << 10), (1, 1 << 12), (1, 1 << 14), (64, 17), (64, 256))
VALU_PEAK = 1024 * 2.4e9 / 4.9        # wave-instructions per second (bench.py: 1024 SIMDs, one v_mad_u64_u32 per 4.9 cycles)
VALU_PER_PRODUCT = 380                # the NTT butterfly's count (one Montgomery product, one add, one sub; bench.py `roofline_alu`)


def step(seconds, work):
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
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return ts


def quartiles(ts, scale):
    q = statistics.quantiles(ts, n=4)
    return [round(scale * v, 4) for v in (q[0], statistics.median(ts), q[2])]


def fr(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 2 ** 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)


def plan(op, batch, n_in, n_x):
    import ctypes as C
    info = (C.c_uint32 * 8)()
    N.check(N.lib().zkhip_dense_points_plan_info(op, batch, n_in, n_x, info), "plan_info")
    return {"segments": info[1], "launches": info[3], "scratch_bytes": info[4] + (info[5] << 32)}


def interp_products(batch, n):
    """field products of an interpolation with shared nodes: n per node for D_i, once per call; three per (node, domain point) and job for
    (Num, Den); the inverses and the transform apart"""
    big = 1 << max((n - 1).bit_length(), 0)
    return n * n + batch * 3 * n * big


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_points", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dense_points", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 repetitions"
    fmt = lambda v: "%.3g / %.3g / %.3g" % tuple(v)   # noqa: E731
    ev_rows, ev_lines = [], ["| coefficients | m | segments | loop of `evaluate(point)`, us per point (q1 / median / q3) | `evaluate([m, 4])`, host points in, host values out | device points in, device values out | loop / 2-D form | G products/s (device form) | of the VALU issue peak |",
                             "|---|---|---|---|---|---|---|---|---|"]
    for log_n in EVAL_LOGS:
        n = 1 << log_n
        poly = zk.DenseUnivariatePolynomial(step(300, lambda: fr(n, 5 + log_n)))
        for m in EVAL_POINTS:
            d_pts = fr(m, 50 + m)
            h_pts = d_pts.cpu().numpy().view(np.uint64)
            works = {"loop": lambda: np.stack([poly.evaluate(h_pts[k]) for k in range(m)]),
                     "host": lambda: poly.evaluate(h_pts),
                     "device": lambda: poly.evaluate(d_pts)}
            got = {name: step(300, w) for name, w in works.items()}                   # warm-up of every shape, and the same values
            assert np.array_equal(got["loop"], got["host"]) and np.array_equal(got["loop"], got["device"].cpu().numpy().view(np.uint64))
            ts = step(900, lambda: timed_in_turn(works, args.reps))
            q = {name: quartiles(v, 1e6 / m) for name, v in ts.items()}
            rate = n * m / (statistics.median(ts["device"]))
            frac = rate * VALU_PER_PRODUCT / 64 / VALU_PEAK
            p = plan(N.DENSE_EVALUATE, 1, n, m)
            ev_rows.append({"log_n": log_n, "m": m, "plan": p, "us_per_point": q, "products_per_s": rate, "valu_frac": round(frac, 4)})
            ev_lines.append("| 2^%d | %d | %d | %s | %s | %s | %.2f | %.2f | %.3f |" % (log_n, m, p["segments"], fmt(q["loop"]), fmt(q["host"]), fmt(q["device"]),
                                                                                 q["loop"][1] / q["host"][1], rate / 1e9, frac))
            print(ev_lines[-1], flush=True)
    in_rows, in_lines = [], ["| B | n | segments | launches per chunk | `interpolate_batch`, ms per call (q1 / median / q3) | G products/s | of the VALU issue peak |", "|---|---|---|---|---|---|---|"]
    for B, n in INTERP:
        ys = fr(B * n, 70 + n).reshape(B, n, 4)
        xs = fr(n, 71 + n)                                                            # shared nodes; distinct with overwhelming probability
        works = {"interpolate": lambda: zk.DenseUnivariatePolynomial.interpolate_batch(ys, xs)}
        step(300, works["interpolate"])
        ts = step(900, lambda: timed_in_turn(works, args.reps))["interpolate"]
        q = quartiles(ts, 1e3)
        rate = interp_products(B, n) / statistics.median(ts)
        frac = rate * VALU_PER_PRODUCT / 64 / VALU_PEAK
        p = plan(N.DENSE_INTERPOLATE, B, n, n)
        in_rows.append({"batch": B, "n": n, "plan": p, "ms": q, "products_per_s": rate, "valu_frac": round(frac, 4)})
        in_lines.append("| %d | %d | %d | %d | %s | %.2f | %.3f |" % (B, n, p["segments"], p["launches"], fmt(q), rate / 1e9, frac))
        print(in_lines[-1], flush=True)
    record = {"tool": "perf_dense_points", "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "figures": "first quartile, median, third quartile; evaluation in us per point, interpolation in ms per call",
              "valu_peak_wave_instructions_per_s": VALU_PEAK, "valu_per_product": VALU_PER_PRODUCT, "evaluate": ev_rows, "interpolate": in_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(json.dumps(record) + "\n")
    text = "\n".join([BEGIN, "", "First quartile / median / third quartile of %d repetitions, the columns timed in turn in one process, `%s`; host clock around calls that end "
                      "in a synchronisation.  Products per second count n_in m products (evaluation) and n^2 + 3 B n N (interpolation, shared nodes: "
                      "the n^2 of the weights once per call); the share of the issue peak takes %d VALU instructions per product."
                      % (args.reps, torch.cuda.get_device_name(0), VALU_PER_PRODUCT), ""] + ev_lines + [""] + in_lines + ["", END])
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
