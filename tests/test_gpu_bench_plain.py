"""bench.py without --full: warm-up, exactly `steps` timed steps, the outputs of the last one (--dump-outputs) and one JSON line with
the headline only.  The dumped proof is the CPU oracle's proof of the same synthetic table, limb for limb."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _limbs(a):
    """float64 [..., 8] of 32-bit halves (bench.py --dump-outputs) -> uint64 [..., 4] Montgomery limbs"""
    assert a.dtype == np.float64 and a.shape[-1] == 8
    h = a.astype(np.uint64)
    assert np.array_equal(h.astype(np.float64), a) and (h >> np.uint64(32)).max(initial=0) == 0
    return np.ascontiguousarray(h.astype(np.uint32)).view(np.uint64)


def test_bench_plain_run_and_dump_outputs(tmp_path, ora):
    import zk_cryptography_amd as zk
    log_n = 16
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--log-n", str(log_n),
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "field-evals/s" and d["higher_is_better"] is True and d["dtype"] == "u32" and d["metric"].startswith("field-evals/s")
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx((1 << log_n) * 4 / (4 * d["ms_per_step"] * 1e-3), rel=2e-2)
    for extra in ("legs", "batches", "roofline", "pipelined", "cpu_baseline", "msm", "gkr"):       # behind --full
        assert extra not in d
    names = sorted(os.listdir(out_dir))
    assert names == ["challenges.npy", "sum.npy", "univariate_poly.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in names) <= 64 << 20
    ev = zk.Fr.synthetic(1 << log_n, 0x5EED000000000001)          # bench.py's table of rank 0
    s, rp, ch = ora.sumcheck_prove(ev)
    assert np.array_equal(_limbs(np.load(out_dir / "sum.npy")).reshape(-1), np.asarray(s, dtype=np.uint64).reshape(-1))
    assert np.array_equal(_limbs(np.load(out_dir / "univariate_poly.npy")), np.asarray(rp, dtype=np.uint64).reshape(log_n, 2, 4))
    assert np.array_equal(_limbs(np.load(out_dir / "challenges.npy")), np.asarray(ch, dtype=np.uint64).reshape(log_n, 4))
