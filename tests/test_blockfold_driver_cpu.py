"""No GPU: tests/cpp/blockfold_driver.hip compiles for gfx950 and loads, blockfold_shape gives every (m, k) the library folds with a
grid that reaches the chip inside the consumers' limits, and the launchers refuse what the shape function does not accept before
they touch a device (on a machine without one a launch would come back with another error than hipErrorInvalidValue)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blockfold_driver as DRV  # noqa: E402


@pytest.fixture(scope="module")
def L():
    return DRV.lib()


def test_driver_builds_for_gfx950_and_loads(L):
    assert os.path.exists(DRV.LIB_PATH)
    assert "--offload-arch=gfx950" in DRV.FLAGS
    assert L.blockfold_driver_block() == 256            # one wave per SIMD


@pytest.mark.parametrize("m,k", DRV.SHAPES)
def test_shape_fills_the_chip_within_the_consumers_limits(L, m, k):
    rc, sh = DRV.shape(m, k)
    assert rc == 0
    assert sh["workgroups"] >= (256 if (m, k) == (256, 10) else 128)
    assert 1 <= sh["per"] <= 4                          # WideAcc's capacity (tests/test_gpu_arith.py)
    assert 1 <= sh["ny"] <= 8                           # loads in flight in the serial kernel's strided prologue
    assert 1 <= sh["slices"] <= 256 >> sh["log_ow"]
    assert sh["slices"] * sh["per"] * sh["ny"] == 1 << k            # every term once
    assert sh["workgroups"] == (m >> sh["log_ow"]) * sh["ny"]
    # the prover's partial tables: 2 x 1024 entries behind the first fold (k <= 6), 32 x 256 behind the second
    assert sh["ny"] * m <= (2048 if k <= 6 else 32 * 256)


def test_the_issue_shape_of_the_tail_fold(L):
    assert DRV.shape(256, 10) == (0, {"log_ow": 3, "slices": 32, "per": 4, "ny": 8, "workgroups": 256})


@pytest.mark.parametrize("m,k", [(0, 3), (3, 3), (255, 6), (768, 6), (1, 3), (4, 3), (256, 0), (1024, 0), (256, 11)])
def test_shapes_outside_the_rule_are_refused(L, m, k):
    """m no power of two; fewer outputs than a workgroup's 8 (log_ow > log2 m); no term; more than 32 x 4 x 8 terms"""
    rc, sh = DRV.shape(m, k)
    assert rc == DRV.INVALID and sh["workgroups"] == 0
    fake = 4096                                          # never dereferenced: the refusal comes first
    assert L.blockfold_driver_run(fake, m, k, fake, fake, None) == DRV.INVALID


def test_null_pointers_are_refused(L):
    fake = 4096
    assert L.blockfold_driver_shape(256, 10, None) == DRV.INVALID
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert L.blockfold_driver_run(args[0], 256, 10, args[1], args[2], None) == DRV.INVALID
