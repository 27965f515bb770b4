"""The cloud path at the ends of its index arithmetic and at the launch cap of csrc/cloud_common.h (DESIGN.md section 2,
"The cloud path at its limits").  The cases and the checkers are tests/cloud_limits_check.py's; each group runs in a child
process of its own, one after another, through gpu_child.run_once: a group that faults ends the run."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

# group -> the child's time limit in seconds: four times its wall time on the MI355X, rounded up to 10 s
LIMITS = {"trips": 20, "fuse-cap": 20, "dense-564": 20, "voxels": 20, "big-grid": 20, "top-f64": 20, "top-b32f": 20, "fuse-e31": 20,
          "dense-895": 20, "top-f32": 30}


@pytest.mark.parametrize("group", list(LIMITS))
def test_the_cloud_path_at_its_limits(group):
    r = gpu_child.run_once(("cloud-limits", group), ["cloud_limits_check.py", group], timeout=LIMITS[group])
    skipped = r.records("SKIP ")
    if r.returncode == 0 and skipped:
        pytest.skip(skipped[0]["reason"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    cases = r.records("C ")
    assert r.json() == dict(group=group, ok=True, peak_gib=r.json()["peak_gib"]) and cases
    assert all(c["peak_gib"] <= 40.0 for c in cases) and r.json()["peak_gib"] <= 40.0, cases
