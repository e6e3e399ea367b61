"""No GPU: the tile schedule of fold_rounds_kernel's fold workgroups (csrc/fold_schedule.hpp), which the kernel, the host and this
test share.  tests/cpp/fold_schedule_check.cpp is built with g++ around the header -- it has no HIP in it -- and walks every tile count
T in 1 .. 4200 and every number of fold workgroups F in 1 .. 300: the regular tiles of the waves and the leftover tiles of the
workgroups cover every tile exactly once, q = 0 is one tile per wave, and no workgroup gets more than ceil(rem / F) leftovers."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "fold_schedule_check.cpp")


def test_every_grid_covers_every_tile_once(tmp_path):
    exe = str(tmp_path / "fold_schedule_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    out = subprocess.run([exe, "4200", "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.strip().splitlines()[-1] == "checked %d" % (4200 * 300)
