"""DenseUnivariatePolynomial::{evaluate(points), evaluate_batch, interpolate, interpolate_batch} of the C++ host mirror
(tests/cpp/test_mirror_dense_points.cpp), against the CPU oracle.  CPU: it must compile and link; GPU: it must pass.  Built here with
the compile line of the `test_mirror` target of tests/cpp/Makefile, into a temporary directory."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_mirror_dense_points.cpp")


def _build(tmp_path):
    from zk_cryptography_amd import _native
    from oracle import oracle
    _native.build()
    oracle.build()
    csrc, ora = os.path.join(ROOT, "zk-cryptography_amd", "csrc"), os.path.join(ROOT, "oracle")
    exe = os.path.join(str(tmp_path), "test_mirror_dense_points")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, SRC, "-L" + csrc, "-lzkhip", "-L" + ora, "-lzkoracle",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath," + ora, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_mirror_dense_points_builds(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_mirror_dense_points_passes(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert "dense points mirror: 0 failed" in res.stdout
