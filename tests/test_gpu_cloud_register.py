"""mvs_cloud_register / fusion.register_cloud / fusion.evaluate_cloud(register=...) on the GPU, held to
tests/register_ref.py: the correspondences exactly, the reduced sums within the pairwise-sum bound (bit for bit where
every term is an integer), every step within the solve bound, the whole loop within the propagated bound and with the
reference's iteration count.  The bytes do not depend on the cell size, the run or the stream; the buffers of the entry
point lie between guards and are poisoned.

The checks run in children (tests/register_check.py GROUP, through tests/gpu_child.py), one per group, each started once
and shared by the tests of its group; a check's record carries its figures, which the tests print.

The step kernel serves 8 sources per wave and 4 waves per block, one level-0 partial sum per 32 sources, 256 partial sums
per partial sum of every later level: N = 31, 32, 33 sit around one block's share, 63, 64, 65 around two, 32 * 256 + 1 is
one more than one level-1 partial sum covers and 32 * 256 * 256 + 1 one more than two levels cover."""
import pytest

import gpu_child
import register_check as RC

pytestmark = pytest.mark.gpu
LIMITS = dict(edges=240, sums=240, dense=300, loop=240, evaluate=240)      # seconds; a child takes a small part of it


def record(group, check):
    r = gpu_child.run_once(("register_check", group), ["register_check.py", group], timeout=LIMITS[group])
    recs = {rec["check"]: rec for rec in r.records("R ")}
    assert r.returncode == 0 and set(recs) == {RC.name_of(c) for c in RC.GROUPS[group]}, r.stderr[-3000:]
    rec = recs[check]
    print({k: v for k, v in rec.items() if k != "why"})
    assert rec["ok"], rec["why"]
    return rec


@pytest.mark.parametrize("check", [RC.name_of(c) for c in RC.GROUPS["edges"]])
def test_edges_probes_determinism_refusals_and_guards(check):
    record("edges", check)


def test_the_sums_at_the_boundaries_of_their_tree_lie_within_the_pairwise_bound():
    rec = record("sums", "check_reduction_boundaries")
    assert rec["2097153"] == [65537, 257, 2, 1] and rec["8193"] == [257, 2, 1] and rec["32"] == [1] and rec["worst_ratio"] <= 1.0


@pytest.mark.parametrize("check", [RC.name_of(c) for c in RC.GROUPS["dense"]])
def test_every_step_of_a_dense_pair_against_the_reference_from_the_devices_own_transform(check):
    rec = record("dense", check)
    assert rec["gap"] >= 1e-9 and rec["worst_sum_ratio"] <= 1.0 and rec["worst_step_ratio"] <= 1.0 and rec["inliers"] > 1900


@pytest.mark.parametrize("check", [RC.name_of(c) for c in RC.GROUPS["loop"]])
def test_the_whole_loop_converges_like_the_reference_within_the_propagated_bound(check):
    rec = record("loop", check)
    assert 2 <= rec["iterations"] < 50 and rec["worst_ratio"] <= 1.0


def test_evaluate_cloud_scores_a_moved_cloud_like_the_unmoved_one_after_registering_it():
    rec = record("evaluate", "check_evaluate_cloud")
    assert rec["unregistered"] > rec["base"]
