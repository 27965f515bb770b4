"""Every warp + variance kernel form (warp_variance_kernel, warp_variance16_kernel, warp_variance_tc2_kernel with fp32 and
with 16-bit features, homo_warp_kernel, relative_proj_kernel) against the fp64 reference and the derived bound of
tests/warp_ref.py -- about 50 times tighter than the atol = 5e-4 of test_gpu_parity.py / test_gpu_fullsize.py, on rigs
those never try (fast epipolar motion, roll, all borders and corners, points behind a source camera with NaN voxels).
One child process per kernel-selection environment (tests/warp_ref_check.py: the environment -> kernel map); a failed
child fails its environment and nothing is retried.  The tap-cache forms must equal the plain forms bit for bit on
every case, NaN positions included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import warp_ref as W  # noqa: E402
from warp_ref_check import ENVS, IDENTICAL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("warp_ref"))
    done = {}

    def run(envname):
        if envname not in done:
            env = {k: v for k, v in os.environ.items() if not k.startswith("MVS_")}
            env.update(ENVS[envname]["env"])
            try:
                r = subprocess.run([sys.executable, os.path.join(HERE, "warp_ref_check.py"), envname, work], env=env,
                                   capture_output=True, text=True, timeout=300)
                done[envname] = (r.returncode, r.stdout, r.stderr)
            except subprocess.TimeoutExpired as e:
                done[envname] = (-1, str(e.stdout), "timeout: " + str(e.stderr))
        return done[envname] + (os.path.join(work, envname),)
    return run


@pytest.mark.parametrize("envname", list(ENVS))
def test_warp_kernels_lie_within_the_fp64_bound(runs, envname):
    rc, out, err, _ = runs(envname)
    print(out[-8000:])
    print(err[-3000:])
    assert rc == 0, f"warp_ref_check {envname}: rc {rc}\n{out[-4000:]}\n{err[-3000:]}"
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    want = {f"{c}/{s}" for c in W.CASES for s in ENVS[envname]["storages"]}
    assert want <= set(res["ratios"]), want - set(res["ratios"])
    assert not res["failures"] and res["worst"] <= 1.0, res


@pytest.mark.parametrize("tc", list(IDENTICAL))
def test_tap_cache_volumes_equal_the_plain_kernels_bit_for_bit(runs, tc):
    """same taps, same weights, same fma nesting: EQUAL on every case and storage type, NaN positions included"""
    plain = IDENTICAL[tc]
    rc_a, _, err_a, dir_a = runs(tc)
    rc_b, _, err_b, dir_b = runs(plain)
    assert rc_a in (0, 1) and rc_b in (0, 1), (err_a[-2000:], err_b[-2000:])    # 1: a bound failed, the volumes exist
    differ = []
    for name in W.CASES:
        for s in ENVS[tc]["storages"]:
            a = np.load(os.path.join(dir_a, f"{name}_{s}.npy"))
            b = np.load(os.path.join(dir_b, f"{name}_{s}.npy"))
            if not np.array_equal(a, b, equal_nan=True):
                differ.append((name, s, int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())))
    assert not differ, differ
