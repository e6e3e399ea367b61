"""No GPU: the plan of zkhip_dense_points (csrc/dense_points_plan.hpp), which the entry point, its kernels and this test share.
tests/cpp/dense_points_plan_check.cpp is built with g++ around the header -- it has no HIP in it -- under the host sanitizers and run
directly.  And the arithmetic the interpolation kernels run, restated over the oracle's field operations: the (Num, Den) recurrence
over the nodes and the combine of two segments reproduce, at every point of the transform domain, the polynomial a Lagrange model in
Python integers (tests/dense_points_model.py) interpolates; and Horner over segments, each scaled by x^(first coefficient), adds up to the evaluation."""
import os
import subprocess

import numpy as np
import pytest

from dense_points_model import R, lagrange_coefficients, root_of_unity

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "dense_points_plan_check.cpp")


def test_plan_segments_chunks_scratch_and_refusals(tmp_path):
    exe = str(tmp_path / "dense_points_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")


@pytest.mark.parametrize("n", [5, 17])
def test_the_recurrence_and_its_combine_over_the_oracle(ora, n):
    N = 1 << (n - 1).bit_length()
    w = root_of_unity(N)
    assert ora.fr_to_ints(ora.fr_get_root_of_unity(N)) == [w]
    xs = [(0x1234567 * (k + 3) ** 5 + k) % R for k in range(n)]
    xs[1] = pow(w, 3, R)                                                    # one node on the domain: the recurrence has no special case there
    ys = ora.fr_to_ints(ora.random_fr(n, 3100 + n))
    coeffs = ora.fr_from_ints(lagrange_coefficients(xs, ys))
    for i in range(n):                                                      # the model interpolates
        assert ora.fr_to_ints(ora.dense_evaluate(coeffs, ora.fr_from_ints([xs[i]])[0])) == [ys[i]]
    X, zero, one = ora.fr_from_ints(xs), ora.fr_from_ints([0])[0], ora.fr_from_ints([1])[0]
    s = []
    for i in range(n):
        d = one
        for j in range(n):
            if j != i:
                d = ora.fr_mul(d, ora.fr_sub(X[i], X[j]))
        s.append(ora.fr_mul(ora.fr_from_ints([ys[i]])[0], ora.fr_inv(d)))

    def walk(z, lo, hi):
        num, den = zero, one
        for i in range(lo, hi):
            d = ora.fr_sub(z, X[i])
            num = ora.fr_add(ora.fr_mul(num, d), ora.fr_mul(s[i], den))
            den = ora.fr_mul(den, d)
        return num, den

    cut = n // 2 + 1
    for t in range(N):
        z = ora.fr_from_ints([pow(w, t, R)])[0]
        want = ora.dense_evaluate(coeffs, z)
        num, _den = walk(z, 0, n)
        assert np.array_equal(num, want), t
        (na, da), (nb, db) = walk(z, 0, cut), walk(z, cut, n)               # segments A then B
        assert np.array_equal(ora.fr_add(ora.fr_mul(na, db), ora.fr_mul(nb, da)), want), t
        assert np.array_equal(ora.fr_mul(da, db), _den), t


def test_horner_over_segments_over_the_oracle(ora):
    n, seg = 23, 8
    coeffs, x = ora.random_fr(n, 3200), ora.random_fr(1, 3201)[0]
    total = ora.fr_from_ints([0])[0]
    for lo in range(0, n, seg):
        part = ora.dense_evaluate(coeffs[lo:lo + seg], x)
        total = ora.fr_add(total, ora.fr_mul(part, ora.fr_powers(x, lo + 1)[lo]))
    assert np.array_equal(total, ora.dense_evaluate(coeffs, x))
