"""No GPU: the plan of zkhip_mle_evaluation_batch (csrc/mle_batch_plan.hpp), which the entry point, its kernels and this test share.
tests/cpp/mle_batch_plan_check.cpp is built with g++ around the header -- it has no HIP in it -- under the host sanitizers and run
directly.  And the block decomposition the kernels of 2^13 .. 2^16 entries compute, over the oracle: the blocks' evaluations weighted
with eq_q of the leading points add up to the table's evaluation."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "mle_batch_plan_check.cpp")


def test_plan_and_weight_bit_order(tmp_path):
    exe = str(tmp_path / "mle_batch_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")


@pytest.mark.parametrize("log_n", [13, 14])
def test_block_decomposition_over_the_oracle(ora, log_n):
    h = log_n - 12
    table = ora.random_fr(1 << log_n, 400 + log_n)
    pts = ora.random_fr(log_n, 500 + log_n)
    one = ora.fr_from_ints([1])[0]
    total = ora.fr_from_ints([0])[0]
    for q in range(1 << h):
        w = ora.mle_evaluation(table[q << 12:(q + 1) << 12], pts[h:])
        for i in range(h):                                   # point 0 is the most significant index bit
            w = ora.fr_mul(w, pts[i] if (q >> (h - 1 - i)) & 1 else ora.fr_sub(one, pts[i]))
        total = ora.fr_add(total, w)
    assert np.array_equal(total, ora.mle_evaluation(table, pts))
