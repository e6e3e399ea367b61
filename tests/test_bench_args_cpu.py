"""bench.py's options are checked before anything touches the GPU: the legs' options without --full are refused (a plain run would
ignore them and print none of the objects they select), and so is a run without timed steps."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv,needle", [
    (["--no-msm", "--no-gkr"], "--no-msm, --no-gkr"),
    (["--composed-log-n", "15"], "--composed-log-n"),
    (["--no-exchange"], "--no-exchange"),
    (["--steps", "0"], "--steps must be >= 1"),
])
def test_bench_refuses_options_a_plain_run_cannot_honour(argv, needle):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=60)
    assert out.returncode == 2 and needle in out.stderr.decode() and not out.stdout.strip()
