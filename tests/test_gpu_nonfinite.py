"""NaN and infinity through every conv kernel form of CostRegNet, the soft-argmin's launch forms and the chain, against
the contract of tests/nonfinite_ref.py: R1 a non-finite reference value is never hidden behind a finite number, R2 every
finite output keeps the kernel's bound, R3 non-finite values spread no further than the form's geometry allows.  One
child process (tests/nonfinite_check.py) per kernel-selection environment of probe_check.CASES, each run once."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_child  # noqa: E402
from probe_check import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


def _child(args, env=None):
    r = gpu_child.run(["nonfinite_check.py"] + args, env=env, timeout=300)
    assert r.returncode == 0, f"nonfinite_check {args}: rc {r.returncode}\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}"
    return r.json()


@pytest.mark.parametrize("case", list(CASES))
def test_conv_layers_keep_and_confine_nonfinite_values(case):
    out = _child(["layers", case], CASES[case]["env"])
    assert out["ratios"] and max(out["ratios"].values()) <= 1.0, out["ratios"]
    for key, (seen, table) in out["spread"].items():
        assert all(s <= t for s, t in zip(seen, table)), (key, seen, table)


def test_softargmin_every_form_keeps_nan_and_drops_minus_inf():
    out = _child(["softargmin"])
    assert all(max(r) <= 1.0 for r in out["ratios"].values()), out["ratios"]


def test_chain_keeps_nan_from_the_volume_and_from_the_warp():
    out = _child(["chain"])
    for key, rep in out["report"].items():
        assert rep["finite_got"] >= 0.5 and (not key.endswith(":f32") or rep["logit_ratio"] <= 1.0), (key, rep)
