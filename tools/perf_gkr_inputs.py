"""us per input: the reference bench's iteration (gkr/benches/gkr_benchmark.rs:19-26: circuit.evaluation(&input), then
GKRProtocol::prove) over B inputs of one circuit, in ONE process, four legs per shape:
  eval_loop     a loop of Circuit.evaluation                       eval_batch    Circuit.evaluation_batch (zkhip_circuit_evaluate_batch)
  loop_prove    that loop, then GKRProtocol.prove_batch            prove_inputs  GKRProtocol.prove_inputs (the two calls)
and the evaluation through the raw C ABI, outputs allocated and pointers prepared beforehand (eval_batch_raw: what a C caller pays).
The legs are timed in turn, repetition by repetition, after a warm-up of every shape; every figure is the median over the
repetitions with its quartiles; wall time around work that ends in a synchronisation.  The batch's tables are compared with the
loop's on the same inputs first: a difference fails the run.  Every GPU step runs under an alarm of its own: a step that hangs
ends the process.  The width T is compiled in: ZKHIP_LIB=path runs the tool against another build of the library
(-DZK_CEB_TAIL_LOG=8 or 12), one process per build; --tail-log names the build in the output.
usage (GPU box): python tools/perf_gkr_inputs.py [--out FILE] [--json FILE] [--reps N] [--shapes DEPTH:B ...] [--tail-log T] [--no-prove]
The table replaces what stands between the two marker lines of FILE (default profiles/circuit_eval_batch/NOTES.md; the markers
carry the tail width, so the builds of a comparison keep a table each); the rest of FILE is kept."""
import argparse, ctypes as C, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from zk_cryptography_amd import _native as N
if os.environ.get("ZKHIP_LIB"):
    N.LIB_PATH = os.path.abspath(os.environ["ZKHIP_LIB"])
import zk_cryptography_amd as zk

SHAPES = ("8:1", "8:8", "8:32", "20:1", "20:8", "20:24")


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
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return ts


def quartiles_us(ts, B):
    q = statistics.quantiles(ts, n=4)
    return [round(1e6 * v / B, 3) for v in (q[0], statistics.median(ts), q[2])]


def raw_batch(circuit, inputs):
    """zkhip_circuit_evaluate_batch with every argument prepared beforehand -> (call, the arena it writes, its pointer table)"""
    ctx = N.Context.get(inputs[0].device.index)
    dev = zk.GKRProtocol._device_circuit(circuit, ctx)
    lens = list(dev.shape)
    B, per = len(inputs), sum(lens)
    arena = torch.empty((B, per, 4), dtype=torch.int64, device="cuda")
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    ptrs = np.zeros((B, len(lens) + 1), dtype=np.uint64)
    for b in range(B):
        ptrs[b, :-1] = arena.data_ptr() + 32 * (b * per + offs)
        ptrs[b, -1] = inputs[b].data_ptr()
    fn, h, n_in, p = N.lib().zkhip_circuit_evaluate_batch, dev.handle.value, inputs[0].shape[0], ptrs.ctypes.data
    return (lambda _alive=(arena, ptrs, inputs): N.check(fn(h, B, n_in, p, None), "evaluate_batch")), arena, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuit_eval_batch", "NOTES.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "circuit_eval_batch", "perf_line.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", type=str, nargs="*", default=list(SHAPES), help="DEPTH:B ...")
    ap.add_argument("--tail-log", type=int, default=None, help="log2 of the width T the library under test was built with (default: the header's)")
    ap.add_argument("--no-prove", action="store_true", help="the two evaluation legs only (the T comparison)")
    args = ap.parse_args()
    assert args.reps >= 7, "the median of at least seven repetitions"
    if args.tail_log is None:
        import re
        with open(os.path.join(ROOT, "zk-cryptography_amd", "csrc", "circuit_eval_plan.hpp")) as f:
            args.tail_log = int(re.search(r"#define ZK_CEB_TAIL_LOG (\d+)", f.read()).group(1))
    block = "perf_gkr_inputs%s T=2^%d" % (" --no-prove" if args.no_prove else "", args.tail_log)
    begin, end = "<!-- %s: begin -->" % block, "<!-- %s: end -->" % block
    fmt = lambda v: "%.1f / %.1f / %.1f" % tuple(v)   # noqa: E731
    # --no-prove: the loop runs once, for the comparison of the outputs, and is not timed (at depth 20 it is most of a run)
    legs = ["eval_batch", "eval_batch_raw"] if args.no_prove else ["eval_loop", "eval_batch", "eval_batch_raw", "loop_prove", "prove_inputs"]
    lines = ["| depth | B | " + " | ".join("`%s`, us per input (q1 / median / q3)" % l if i == 0 else "`%s`" % l for i, l in enumerate(legs)) +
             ("" if args.no_prove else " | eval_loop / eval_batch | eval_loop q1 - eval_batch q3 | loop_prove / prove_inputs") + " |",
             "|---|---|" + "---|" * (len(legs) + (0 if args.no_prove else 3))]
    rows, circuits = [], {}
    for spec in args.shapes:
        depth, B = (int(v) for v in spec.split(":"))
        if depth not in circuits:
            circuits[depth] = step(600, lambda: zk.Circuit.random(depth))
        circuit = circuits[depth]
        g = torch.Generator(device="cuda").manual_seed(1000 * depth + B)
        inputs = [torch.randint(0, 2 ** 62, (1 << depth, 4), dtype=torch.int64, device="cuda", generator=g) for _ in range(B)]
        raw, arena, lens = raw_batch(circuit, inputs)
        works = {"eval_loop": lambda: [circuit.evaluation(i) for i in inputs], "eval_batch": lambda: circuit.evaluation_batch(inputs), "eval_batch_raw": raw}
        if not args.no_prove:
            works["loop_prove"] = lambda: zk.GKRProtocol.prove_batch(circuit, [circuit.evaluation(i) for i in inputs])
            works["prove_inputs"] = lambda: zk.GKRProtocol.prove_inputs(circuit, inputs)
        got = {name: step(600, w) for name, w in works.items()}                     # warm-up of every leg, and the same results
        torch.cuda.synchronize()
        for b in range(B):
            at = 0
            for k, n in enumerate(lens + [1 << depth]):
                assert torch.equal(got["eval_loop"][b][k], got["eval_batch"][b][k]), (depth, B, b, k)
                if k < len(lens):
                    assert torch.equal(got["eval_loop"][b][k], arena[b, at:at + n]), (depth, B, b, k, "raw")
                    at += n
        if not args.no_prove:
            for pa, pb in zip(got["loop_prove"], got["prove_inputs"]):
                assert [sp.to_bytes() for sp in pa.sumcheck_proofs] == [sp.to_bytes() for sp in pb.sumcheck_proofs]
        del got
        ts = step(1100, lambda: timed_in_turn({l: works[l] for l in legs}, args.reps))
        q = {name: quartiles_us(v, B) for name, v in ts.items()}
        rows.append({"depth": depth, "batch": B, "us_per_input": q})
        lines.append("| %d | %d | " % (depth, B) + " | ".join(fmt(q[l]) for l in legs) +
                     ("" if args.no_prove else " | %.2f | %.1f | %.2f" % (q["eval_loop"][1] / q["eval_batch"][1], q["eval_loop"][0] - q["eval_batch"][2],
                                                                       q["loop_prove"][1] / q["prove_inputs"][1])) + " |")
        print(lines[-1], flush=True)
        del inputs, arena, raw, works
    record = {"tool": "perf_gkr_inputs", "device": torch.cuda.get_device_name(0), "library": os.path.relpath(N.LIB_PATH, ROOT), "tail_log": args.tail_log,
              "reps": args.reps, "figures": "us per input: first quartile, median, third quartile", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(json.dumps(record) + "\n")
    print(json.dumps(record), flush=True)
    text = "\n".join([begin, "", "T = 2^%d.  First quartile / median / third quartile of %d repetitions, the columns timed in turn in one process, `%s`."
                      % (args.tail_log, args.reps, torch.cuda.get_device_name(0)), ""] + lines + ["", end])
    old = open(args.out).read() if os.path.exists(args.out) else ""
    if begin in old and end in old:
        new = old[:old.index(begin)] + text + old[old.index(end) + len(end):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + text + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(new)


if __name__ == "__main__":
    main()
