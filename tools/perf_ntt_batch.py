"""Measurement: zkhip_domain_transform_batch against the loop of zkhip_domain_transform on the same inputs, per transform size, batch
and direction.  Both are timed in this process after a warm-up, alternating, every window closed by a device synchronise and long
enough (--window seconds) to dwarf the timer; the figure is the median of --repeats windows and the spread is (max - min) / median over
them.  Prints ONE JSON line (profiles/ntt_batch/perf_line.json).

    python tools/perf_ntt_batch.py [--log-n 8,10,...] [--batches 1,4,...] [--window 0.25] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from zk_cryptography_amd import _native as N  # noqa: E402

VALU_PEAK = 1024 * 2.4e9 / 4.9          # wave-instructions per second, as tools/perf_ntt.py
BUTTERFLY_INSTR = 360
CAP_BYTES = 2 << 30                     # source plus destination stay under this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="8,10,12,14,16,18,20")
    ap.add_argument("--batches", default="1,4,16,64,256")
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    lib, ctx = N.lib(), N.Context.get(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for log_n in [int(v) for v in a.log_n.split(",")]:
        n = 1 << log_n
        fit = max(1, (CAP_BYTES - 1) // (64 * n))
        for batch in sorted({min(int(v), fit) for v in a.batches.split(",")}):
            x = torch.randint(0, 2 ** 62, (batch, n, 4), dtype=torch.int64, device="cuda", generator=g)    # every limb < 2^62: reduced residues
            y = torch.empty_like(x)
            h, px, py = ctx.handle, x.data_ptr(), y.data_ptr()
            for inverse in (0, 1):
                args_b = (h, C.c_uint32(batch), C.c_void_p(px), C.c_size_t(n), C.c_size_t(n), C.c_void_p(py), C.c_size_t(n), C.c_uint32(log_n),
                          C.c_int(inverse))
                args_s = [(h, C.c_void_p(px + 32 * n * b), C.c_size_t(n), C.c_void_p(py + 32 * n * b), C.c_uint32(log_n), C.c_int(inverse))
                          for b in range(batch)]

                def batched():
                    N.check(lib.zkhip_domain_transform_batch(*args_b), "transform_batch")

                def loop():
                    for s in args_s:
                        N.check(lib.zkhip_domain_transform(*s), "transform")

                def window(fn, reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(reps):
                        fn()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t

                reps = {}
                for name, fn in (("batch", batched), ("loop", loop)):
                    window(fn, 2)                                              # warm-up: tables, workspace, clocks
                    reps[name] = max(2, int(a.window * 1.1 / (window(fn, 3) / 3)) + 1)
                took = {"batch": [], "loop": []}
                for _ in range(a.repeats):
                    for name, fn in (("batch", batched), ("loop", loop)):
                        took[name].append(window(fn, reps[name]))
                row = {"log_n": log_n, "batch": batch, "inverse": inverse}
                for name in ("batch", "loop"):
                    per = sorted(t / reps[name] / batch for t in took[name])
                    med = per[len(per) // 2]
                    row[name + "_us_per_transform"] = round(med * 1e6, 3)
                    row[name + "_spread"] = round((per[-1] - per[0]) / med, 4)
                    row[name + "_window_s"] = round(min(took[name]), 3)
                row["speedup"] = round(row["loop_us_per_transform"] / row["batch_us_per_transform"], 3)
                bf = n / 2 * log_n / (row["batch_us_per_transform"] * 1e-6)
                row["batch_gbutterflies_per_s"] = round(bf / 1e9, 3)
                row["batch_valu_share"] = round(bf * BUTTERFLY_INSTR / 64 / VALU_PEAK, 4)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)         # progress; the result is the one line on stdout
            del x, y
    print(json.dumps({"tool": "perf_ntt_batch", "device": torch.cuda.get_device_name(0), "window_s": a.window, "repeats": a.repeats,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
