"""Every warp + variance kernel form (warp_variance_kernel, warp_variance16_kernel, warp_variance_tc2_kernel with fp32 and
with 16-bit features, homo_warp_kernel, relative_proj_kernel) against the fp64 reference and the derived bound of
tests/warp_ref.py -- about 50 times tighter than the atol = 5e-4 of test_gpu_parity.py / test_gpu_fullsize.py, on rigs
those never try (fast epipolar motion, roll, all borders and corners, points behind a source camera with NaN voxels).
One child process per kernel-selection environment (tests/warp_ref_check.py: the environment -> kernel map); a failed
child fails its environment and nothing is retried (tests/gpu_child.py).  The tap-cache forms must equal the plain forms bit for bit on
every case, NaN positions included."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_child  # noqa: E402
import warp_ref as W  # noqa: E402
from warp_ref_check import ENVS, IDENTICAL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """envname -> (the environment's child, run on first use, and the directory of its volumes)"""
    work = str(tmp_path_factory.mktemp("warp_ref"))

    def run(envname):
        r = gpu_child.run_once(("warp_ref", envname), ["warp_ref_check.py", envname, work], env=ENVS[envname]["env"],
                               timeout=300)
        return r, os.path.join(work, envname)
    return run


@pytest.mark.parametrize("envname", list(ENVS))
def test_warp_kernels_lie_within_the_fp64_bound(runs, envname):
    r, _ = runs(envname)
    assert r.returncode == 0, f"warp_ref_check {envname}: rc {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}"
    res = r.json()
    want = {f"{c}/{s}" for c in W.CASES for s in ENVS[envname]["storages"]}
    assert want <= set(res["ratios"]), want - set(res["ratios"])
    assert not res["failures"] and res["worst"] <= 1.0, res


@pytest.mark.parametrize("tc", list(IDENTICAL))
def test_tap_cache_volumes_equal_the_plain_kernels_bit_for_bit(runs, tc):
    """same taps, same weights, same fma nesting: EQUAL on every case and storage type, NaN positions included"""
    plain = IDENTICAL[tc]
    ra, dir_a = runs(tc)
    rb, dir_b = runs(plain)
    # 1: a bound failed, the volumes exist
    assert ra.returncode in (0, 1) and rb.returncode in (0, 1), (ra.stderr[-2000:], rb.stderr[-2000:])
    differ = []
    for name in W.CASES:
        for s in ENVS[tc]["storages"]:
            a = np.load(os.path.join(dir_a, f"{name}_{s}.npy"))
            b = np.load(os.path.join(dir_b, f"{name}_{s}.npy"))
            if not np.array_equal(a, b, equal_nan=True):
                differ.append((name, s, int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())))
    assert not differ, differ
