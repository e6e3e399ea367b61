"""The C++ host mirror (include/zkhip.hpp) runs the reference's own unit tests (same names, inputs and expected
values) plus oracle comparisons.  CPU: it must compile and link; GPU: it must pass."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def _build():
    from oracle import oracle
    from zk_cryptography_amd import _native
    oracle.build()
    _native.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "test_mirror"])
    return os.path.join(CPP, "test_mirror")


def test_cpp_mirror_builds():
    assert os.path.exists(_build())


def test_plonk_kernels_driver_builds_and_links():
    """tests/cpp/plonk_kernels_driver.hip (the launchers of tests/test_gpu_plonk_kernels.py): compiled for gfx950, loadable, every launcher
    exported, and a launcher turns a bad argument away on the host (no GPU is touched on that path)"""
    import sys
    sys.path.insert(0, HERE)
    import plonk_kernels_driver as DRV
    assert os.path.exists(DRV.build())
    L = DRV.lib()
    for name in DRV.LAUNCHERS:
        assert hasattr(L, "plonk_driver_" + name), name
    assert L.plonk_driver_gp_rows() == 1024 and L.plonk_driver_flag_count() == 4
    assert [L.plonk_driver_stream_grid(n) for n in (1, 256, 257, 4096)] == [1, 1, 2, 16]
    assert L.plonk_driver_gp_top(None, 0, None, None) != 0 and L.plonk_driver_powers(None, None, 0, None, 0, None) != 0


@pytest.mark.gpu
def test_cpp_mirror_passes_reference_tests():
    exe = _build()          # `make` is a no-op when the binary is newer than the headers it was built from (a stale one -- older than
                            # oracle/zkoracle.h or include/zkhip.h* -- must never run: the structs it allocates would be the old ones)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert " 0 failed" in res.stdout
