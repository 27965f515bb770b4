"""Single-product probes and the dense fp64 bound (tests/probes.py) for every conv kernel form of CostRegNet, one
child process per kernel-selection environment (tests/probe_check.py: the environment -> kernel map and the case
table).  The bounds are about 1000x tighter than the per-layer oracle comparisons of test_gpu_parity.py /
test_gpu_fullsize.py: a lost low-order bf16 piece at a tile edge or a dropped split cross term fails here.  Each child also
runs the smallest volumes mvs_conv_layer / mvs_conv11_prob admit (1 x 1 x 1 upwards; probe_check.TINY_*) against the
dense bound, inside a guarded, poisoned arena."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_child  # noqa: E402
from probe_check import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_conv_probes(case):
    r = gpu_child.run(["probe_check.py", case], env=CASES[case]["env"], timeout=300)
    assert r.returncode == 0, f"probe_check {case}: rc {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}"
    ratios = r.json()["ratios"]
    assert ratios and max(ratios.values()) <= 1.0, ratios
