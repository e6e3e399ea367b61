"""No GPU: the chunk planner of zkhip_kzg_commit_polys (csrc/commit_polys_plan.hpp) and the geometry mode it plans for ("several problems,
one set of points", csrc/msm_geometry.hpp), which the entry point and this test share.  tests/cpp/commit_polys_plan_check.cpp is built
with g++ around the two headers -- neither has HIP in it -- under the host sanitizers: every plan covers its batch in order, every
chunk's geometry builds within the sort's limits and the workspace bound, every sort item lands on its problem's own points, and the
geometries of the modes that existed before are, field for field, what they were."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "commit_polys_plan_check.cpp")


def test_plans_and_geometries(tmp_path):
    exe = str(tmp_path / "commit_polys_plan_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1].startswith("checked ")
