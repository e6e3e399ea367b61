"""The library's environment switches (csrc/tunables.hpp) on the GPU: the forms that bench.py's and the tools'
switches select are reached by no other test.  A switch is read once per process, so each group runs in a fresh child process
(tests/switches_child.py): every result bit for bit the oracle's -- an opening's: the default path's, computed here -- and the launch
counts of the library's profile show that the selected form ran.

Group A: ZKHIP_PIPE=0 (composed K = 2 at 2^16, GKR at depth 9 -- the host transcript with it), ZKHIP_MF=0 (four points on 2^17 entries),
ZKHIP_MSM_SMALL=0 (a commit of 256 scalars on the table).  Group B: ZKHIP_GKR_HOST_TRANSCRIPT=1 (depth 9), ZKHIP_FINE_LDS=0 and
ZKHIP_MF_OCC=2 (poly_sum + prove at 2^18 and, since that size launches neither kernel, at 2^21 and the fine block sums of 2^18 entries),
ZKHIP_PIPE_WGS=64 (composed K = 2 at 2^16), ZKHIP_MSM_BATCH_DELTA=2 (an opening at 2^12), ZKHIP_OPEN_PIPELINES=1 (openings at 2^15 and
at 2^16, the first size with a round above 2^14 quotients).  Group C: ZKHIP_GKR_FUSE_SMALL=0 (depth 9) -- on its own, because the host
transcript of groups A and B never asks for the fused launches.  And the same workloads with no switch set: the counts of the default
forms, which the other groups' differ from."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = {
    "default": {},
    "A": dict(ZKHIP_PIPE="0", ZKHIP_MF="0", ZKHIP_MSM_SMALL="0"),
    "B": dict(ZKHIP_GKR_HOST_TRANSCRIPT="1", ZKHIP_FINE_LDS="0", ZKHIP_MF_OCC="2", ZKHIP_PIPE_WGS="64", ZKHIP_MSM_BATCH_DELTA="2",
              ZKHIP_OPEN_PIPELINES="1"),
    "C": dict(ZKHIP_GKR_FUSE_SMALL="0"),
}


@pytest.fixture(scope="module")
def default_openings(tmp_path_factory):
    """The openings of the child's inputs in this process: the default path (whatever this process was started with, it is not group B)."""
    assert not any(os.environ.get(k) for k in GROUPS["B"])
    import switches_child as child
    ref = {}
    for log_n in (12, 15, 16):
        ref["xy%d" % log_n], ref["inf%d" % log_n], ref["ev%d" % log_n] = child.opening(log_n)
    path = str(tmp_path_factory.mktemp("switches") / "openings.npz")
    np.savez(path, **ref)
    return path


@pytest.mark.parametrize("group", list(GROUPS))
def test_switch_group_in_a_fresh_process(group, default_openings):
    env = {k: v for k, v in os.environ.items() if not (k.startswith("ZKHIP_") and k not in ("ZKHIP_LIB", "ZKHIP_DIAG_LIB"))}
    res = subprocess.run([sys.executable, os.path.join(HERE, "switches_child.py"), group, default_openings], env=dict(env, **GROUPS[group]),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "switches ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
