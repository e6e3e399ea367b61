"""No GPU: the slot rule and the workspace carve-up of the MSM's short path (csrc/msm_small_plan.hpp), which the four drivers of msm.hip
and this test share.  tests/cpp/msm_small_plan_check.cpp is built with g++ around the header -- it has no HIP in it -- under the host
sanitizers: over single commits, openings (single and in chunks, at every window width), PLONK rounds and short-route classes the plan
is, field for field, what each driver's own rule gave, no lane walks more than the cap, and the byte sizes cover partials and terms."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "msm_small_plan_check.cpp")


def test_plan_is_the_four_rules(tmp_path):
    exe = str(tmp_path / "msm_small_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")
