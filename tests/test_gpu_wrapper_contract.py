"""The wrapper contract (tests/wrapper_contract.py) with real CUDA tensors.

First the table under the same Recorder as the host file: no launch happens, and the verdict of every case must equal
the one the stand-in tensors of tests/test_wrapper_contract_host.py get, which pins the stand-in to the real thing.
Then the only launches of the two files: every case the table expects to be `copied` from a strided view, and that the
Recorder run of the same case judged honest, runs with the real library inside a guarded arena under the three poisons,
and its outputs must be the bytes of the same call on a contiguous clone.  Last, every pointer include/mvs_abi.h states
is per element runs one element into a larger allocation and gives the bytes of the aligned call (the kernels behind
them hold no access wider than a dword in their gfx950 code; no pointer with a wider access is ever misaligned here).
Every address of these launches is honest by construction: the Recorder run of the same case judged it.  The
`other_device` rows need two GPUs."""
import pytest
import torch

import guarded as G
import wrapper_contract as WC

pytestmark = pytest.mark.gpu
CASES = [c.name for c in WC.CASES]
TWO = torch.cuda.is_available() and torch.cuda.device_count() >= 2


def _rows(case, other_device):
    return [(leaf, d) for leaf, d in WC.table_rows(case, "rec") if (d == "other_device") == other_device]


def _verdicts_agree(name, other_device):
    case = WC.CASE[name]
    assert WC.run_case(case, "rec")[0] == WC.run_case(case, "fake")[0] == "honest"
    assert WC.table_rows(case, "rec") == WC.table_rows(case, "fake")
    wrong = []
    for leaf, defect in _rows(case, other_device):
        real, detail, _ = WC.run_case(case, "rec", leaf, defect)
        fake = WC.run_case(case, "fake", leaf, defect)[0]
        want = WC.expectation(case, leaf, defect)
        if real != fake or not WC.agrees(want, real):
            wrong.append(f"{leaf} {defect}: CUDA tensors {real}, stand-in {fake}, expected {want} ({detail})")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("name", CASES)
def test_verdicts_with_cuda_tensors_equal_the_stand_ins(name):
    _verdicts_agree(name, other_device=False)


@pytest.mark.skipif(not TWO, reason="needs 2 GPUs")
@pytest.mark.parametrize("name", CASES)
def test_other_device_verdicts_with_cuda_tensors_equal_the_stand_ins(name):
    _verdicts_agree(name, other_device=True)
    assert WC.run_case(WC.CASE[name], "rec", index=1)[0] == "honest"


def test_the_recorder_launches_nothing_and_leaves_the_modules_as_they_were():
    from scene_3dreconstruction_mvsnet_amd import _lib, module
    world = WC.World(fake=False)
    with WC.installed(world):
        kwargs = WC.CASE["volume_relayout@0"].build(WC.Maker("rec"))
        kwargs["out"].fill_(7.0)
        assert _lib.volume_relayout(**kwargs) is kwargs["out"]
    torch.cuda.synchronize()
    assert [c[0] for c in world.calls] == ["mvs_volume_relayout"] and not world.problems()
    assert bool((kwargs["out"] == 7.0).all())      # the call that would have overwritten it was recorded, not made
    assert _lib.torch is torch and module.torch is torch and hasattr(_lib.load(), "_handle")


# ---- the launches: a strided input gives the bytes of its contiguous clone ---------------------------------------------
# not warp_variance_backward's four: mvs_abi.h says "Float atomics reorder the sums: not bit-reproducible run to run", so
# there are no bytes to compare; the Recorder half above holds its strided rows
COPIED = [(c.name, leaf) for c in WC.CASES for leaf in c.roles
          if c.reproducible and WC.expectation(c, leaf, "strided") == "copied"]


@pytest.fixture(scope="module")
def arena():
    return G.Arena(64 << 20, "cuda")


@pytest.mark.parametrize("name,leaf", COPIED)
def test_a_strided_input_gives_the_bytes_of_its_contiguous_clone(name, leaf, arena):
    case = WC.CASE[name]
    assert WC.run_case(case, "rec", leaf, "strided")[0] == "copied"      # the launch below hands over what this judged
    got, guard_bytes = G.same_under_all_poisons(arena, lambda a: WC.real_outputs(case, leaf, a, strided=True))
    plain = WC.real_outputs(case, leaf, G.Plain("cuda"), strided=False)
    torch.cuda.synchronize()
    G.assert_same_bytes(got, plain, f"{name} with a strided {leaf}")
    assert guard_bytes >= 2 * G.MIN_GUARD and sum(t.numel() for t in got) > 0


# ---- the launches: a per-element pointer one element into a larger allocation ------------------------------------------
PER_ELEMENT = [(c.name, leaf) for c in WC.CASES for leaf in c.per_element]


@pytest.mark.parametrize("name,leaf", PER_ELEMENT)
def test_a_per_element_tensor_one_element_in_gives_the_bytes_of_the_aligned_call(name, leaf, arena):
    case = WC.CASE[name]
    assert WC.run_case(case, "rec", leaf, "misaligned")[0] == "honest"      # handed over as it is, and judged
    got, _ = G.same_under_all_poisons(arena, lambda a: WC.real_outputs(case, leaf, a, strided=False, offset=True))
    plain = WC.real_outputs(case, leaf, G.Plain("cuda"), strided=False)
    torch.cuda.synchronize()
    G.assert_same_bytes(got, plain, f"{name} with {leaf} one element in")
    assert sum(t.numel() for t in got) > 0


def _direct(entry, A, offset):
    """One direct call of an entry point whose outputs the wrappers allocate themselves: every pointer the header
    states is per element one element in (offset) or aligned.  rt, and the depth_values the header asks nothing of,
    stay aligned."""
    from scene_3dreconstruction_mvsnet_amd import _lib
    m = WC.Maker("plain")
    lib, st = _lib.load(), _lib._stream(torch.device("cuda", 0))

    def inp(t):
        return WC._one_element_in(A, t, "in") if offset else A.put(t, "in")

    def out(*shape):
        t = torch.empty(shape, device="cuda")
        return WC._one_element_in(A, t, "out") if offset else A.carve(shape, torch.float32, "out")
    if entry == "mvs_softargmin_conf":
        cost, dv, depth, conf = inp(m.f(8, 7, 9)), A.put(m.depths(8), "in"), out(7, 9), out(7, 9)
        _lib.check(lib.mvs_softargmin_conf(cost.data_ptr(), dv.data_ptr(), depth.data_ptr(), conf.data_ptr(), 8, 7, 9, st))
        return depth, conf
    if entry == "mvs_depth_regression":
        p, dv, depth = inp(m.f(8, 7, 9, lo=0, hi=0.25)), A.put(m.depths(8), "in"), out(7, 9)
        _lib.check(lib.mvs_depth_regression(p.data_ptr(), dv.data_ptr(), depth.data_ptr(), 8, 7, 9, st))
        return depth
    fea, rt, dv, warped = inp(m.f(5, 7, 9)), A.put(m.rt(1), "in"), inp(m.depths(3)), out(5, 3, 7, 9)
    _lib.check(lib.mvs_homo_warp(fea.data_ptr(), rt.data_ptr(), dv.data_ptr(), warped.data_ptr(), 5, 3, 7, 9, st))
    return warped


@pytest.mark.parametrize("entry", ["mvs_softargmin_conf", "mvs_depth_regression", "mvs_homo_warp"])
def test_the_per_element_outputs_the_wrappers_allocate_themselves(entry, arena):
    """depth_out / conf_out of mvs_softargmin_conf, depth_out of mvs_depth_regression, out of mvs_homo_warp (with their
    per-element inputs), at odd sizes: 7 x 9 maps, 5 channels."""
    got, _ = G.same_under_all_poisons(arena, lambda a: _direct(entry, a, offset=True))
    aligned = _direct(entry, G.Plain("cuda"), offset=False)
    torch.cuda.synchronize()
    G.assert_same_bytes(got, (aligned,) if isinstance(aligned, torch.Tensor) else aligned, f"{entry} one element in")
