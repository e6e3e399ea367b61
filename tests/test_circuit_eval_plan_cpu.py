"""No GPU: the launch plan and the label bounds of zkhip_circuit_evaluate_batch (csrc/circuit_eval_plan.hpp), which the entry point and
this test share.  tests/cpp/circuit_eval_plan_check.cpp is built with g++ around the header -- it has no HIP in it -- at the committed
width T and at the two other widths of the comparison, under the host sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "circuit_eval_plan_check.cpp")


@pytest.mark.parametrize("tail_log", [None, 8, 12])
def test_plan_and_label_bounds(tmp_path, tail_log):
    exe = str(tmp_path / "circuit_eval_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if tail_log is not None:
        flags.append("-DZK_CEB_TAIL_LOG=%d" % tail_log)
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")
