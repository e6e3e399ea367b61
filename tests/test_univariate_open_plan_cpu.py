"""No GPU: the chunk planner of zkhip_univariate_kzg_open_batch (csrc/univariate_open_plan.hpp), which the entry point and this test
share.  tests/cpp/univariate_open_plan_check.cpp is built with g++ around the header -- it has no HIP in it -- under the host
sanitizers: every plan covers its jobs exactly once and in order, every chunk keeps the job and scratch bounds, quotients and rows do
not overlap, and the status codes are the single call's."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "univariate_open_plan_check.cpp")


def test_plans_cover_their_batches_within_the_bounds(tmp_path):
    exe = str(tmp_path / "univariate_open_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")


def test_the_header_names_the_planners_bounds():
    import re
    root = os.path.dirname(HERE)
    with open(os.path.join(root, "zk-cryptography_amd", "csrc", "univariate_open_plan.hpp")) as f:
        plan = f.read()
    with open(os.path.join(root, "include", "zkhip.h")) as f:
        header = " ".join(" ".join(re.sub(r"^\s*\*\s?", "", line) for line in f.read().splitlines()).split())
    jobs = int(re.search(r"constexpr uint32_t UOP_CHUNK_JOBS = (\d+);", plan).group(1))
    scratch = int(re.search(r"constexpr size_t UOP_SCRATCH_MAX = \(size_t\)(\d+) << 20;", plan).group(1))
    block = int(re.search(r"constexpr size_t UOP_BLOCK = (\d+);", plan).group(1))
    assert jobs <= 1024 and "#include <hip" not in plan
    assert "at most %d consecutive openings" % jobs in header and "at most %d MiB of quotients" % scratch in header
    assert "at most %d coefficients" % block in header
