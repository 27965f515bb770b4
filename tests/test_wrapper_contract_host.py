"""Every Python wrapper that reaches a device entry point, held to the contract of tests/wrapper_contract.py on a
machine without a GPU: stand-in device tensors (host memory that reports a CUDA device), a recording stand-in for the
library, no launch.  A wrapper either refuses before any device call or hands over only honest pointers."""
import os

import pytest
import torch

import wrapper_contract as WC
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib

CASES = [c.name for c in WC.CASES]


# ---- the harness has teeth ---------------------------------------------------------------------------------------------
def _softargmin(cost, dv, depth, conf, D=8, index=0, keep=True):
    """One mvs_softargmin_conf call through the Recorder, the way a wrapper makes it."""
    if not keep:
        dv = dv.clone().data_ptr()      # the temporary dies here, its address travels on
    else:
        dv = dv.data_ptr()
    with torch.cuda.device(torch.device("cuda", index)):
        _lib.load().mvs_softargmin_conf(cost.data_ptr(), dv, depth.data_ptr(), conf.data_ptr(), D, 8, 8,
                                        _lib._stream(torch.device("cuda", index)))


@pytest.mark.parametrize("defect,words", [
    (None, None), ("host", "host tensor"), ("dtype", "float64"), ("short", "28 bytes, the header asks for 32"),
    ("strided", "non-contiguous argument"), ("device", "on device 1"), ("dead", "died before the call"),
    ("null", "is NULL"), ("not_current", "with device 0 current"), ("unknown", "no tensor the wrapper was given or made")])
def test_honest_reports_each_kind_of_dishonest_pointer(defect, words):
    world = WC.World(fake=True)
    with WC.installed(world):
        m = WC.Maker("fake")
        cost, dv, depth, conf = m.f(8, 8, 8), m.depths(8), m.f(8, 8), m.f(8, 8)
        index, keep = 0, True
        if defect == "host":
            dv = torch.zeros(8)
        elif defect == "dtype":
            dv = m.like(dv, dtype=torch.float64)
        elif defect == "short":
            dv = m.depths(7)
        elif defect == "strided":
            dv = m.like(dv, strided=True)
        elif defect == "device":
            dv = m.like(dv, index=1)
        elif defect == "dead":
            keep = False
        elif defect == "null":
            dv = torch.zeros(0)
        elif defect == "not_current":
            cost, dv, depth, conf = (m.like(t, index=1) for t in (cost, dv, depth, conf))
        world.passed = [cost, dv, depth, conf]
        for t in world.passed:
            if not isinstance(t, WC.Dev):
                world.note(t)
        if defect == "unknown":
            dv = torch.zeros(8)      # never shown to the world
        if defect == "not_current":
            _lib.load().mvs_softargmin_conf(cost.data_ptr(), dv.data_ptr(), depth.data_ptr(), conf.data_ptr(), 8, 8, 8,
                                            WC.STREAM_BASE + 1)
        else:
            _softargmin(cost, dv, depth, conf, keep=keep)
    problems = world.problems()
    if defect is None:
        assert problems == [] and [c[0] for c in world.calls] == ["mvs_softargmin_conf"]
    else:
        assert len(problems) == 1 and words in problems[0], problems
        assert "depth_values" in problems[0] or defect == "not_current", problems      # that one is about the call, not a pointer


def test_the_recorder_forwards_what_does_no_device_work_and_launches_nothing_else():
    world = WC.World(fake=True)
    with WC.installed(world) as rec:
        assert rec.mvs_abi_version() == _lib.ABI_VERSION
        assert _lib.query_workspace(3, 32, 8, 8, 8) == WC.dom.workspace_bytes(3, 8, 8, 8)
        with pytest.raises(AttributeError):
            rec.mvs_no_such_entry
    assert set(WC.FORWARDED) | set(WC.DEVICE_ENTRIES) == set(WC.ALL_ENTRIES) and not world.calls
    assert _lib.load() is not rec and _lib.torch is torch


def test_prototypes_and_abi_table_agree_and_every_pointer_has_its_extent():
    flat = {n: args for table in _lib._ABI.values() for n, args in table.items()}
    assert set(WC.PROTOS) == set(flat)
    missing = []
    for name, params in WC.PROTOS.items():
        assert len(params) == len(flat[name]), name
        for (kind, p), ctype in zip(params, flat[name]):
            assert (kind == "ptr") == (ctype in (_lib._vp, _lib._vpp, _lib._szp)), (name, p)
        if name in WC.DEVICE_ENTRIES:
            missing += [f"{name}.{p}" for kind, p in params if kind == "ptr" and p != "stream" and p not in WC.EXTENTS.get(name, {})]
            assert params[-1] == ("ptr", "stream"), name
    assert not missing, missing
    assert set(WC.EXTENTS) == set(WC.DEVICE_ENTRIES)


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_good_call_is_honest_on_either_device(name):
    case = WC.CASE[name]
    for index in (0, 1):      # on device 1 only `with torch.cuda.device(dev)` around allocation and call keeps it honest
        verdict, detail, called = WC.run_case(case, "fake", index=index)
        assert verdict == "honest", (index, detail)
        assert set(case.entries) <= set(called), called


@pytest.mark.parametrize("name", CASES)
def test_every_defect_is_refused_before_any_call_or_handed_over_honestly(name):
    case = WC.CASE[name]
    rows = WC.table_rows(case)
    wrong = []
    for leaf, defect in rows:
        want = WC.expectation(case, leaf, defect)
        verdict, detail, _ = WC.run_case(case, "fake", leaf, defect)
        print(f"{name} {leaf} {defect}: {verdict}")
        if not WC.agrees(want, verdict):
            wrong.append(f"{leaf} {defect}: expected {want}, got {verdict} ({detail})")
    assert not wrong, "\n".join(wrong)
    assert len(rows) >= 5 * len(case.roles)


@pytest.mark.parametrize("name", CASES)
def test_with_every_tensor_on_the_host_the_wrapper_raises_and_nothing_is_recorded(name):
    verdict, detail, called = WC.run_case(WC.CASE[name], "fake", all_host=True)
    assert verdict == "refused" and not called, (verdict, detail, called)


# ---- completeness ------------------------------------------------------------------------------------------------------
def test_every_function_that_names_a_device_entry_point_is_in_the_table():
    named = WC.functions_that_name_a_device_entry_point()
    covered = {f for c in WC.CASES for f in c.covers}
    assert not set(named) - covered, sorted(set(named) - covered)
    assert {"forward_images", "depth_infer", "homo_warping", "depth_regression", "_downsample", "cloud_select"} <= set(named)
    assert not {"filter_compose", "pack_weights", "pack_feature_weights", "query_workspace", "load"} & set(named)
    reached = {e for c in WC.CASES for e in c.entries}
    wanted = {e for es in named.values() for e in es}
    assert wanted <= reached, wanted - reached


def test_every_tensor_parameter_has_every_defect_class_or_a_cited_exemption():
    exemptions = 0
    for case in WC.CASES:
        world = WC.World(fake=True)
        with WC.installed(world):
            kwargs = case.build(WC.Maker("fake"))
        tensors = dict(WC.leaves(kwargs))
        assert set(tensors) == set(case.roles), (case.name, set(tensors) ^ set(case.roles))
        for leaf, t in tensors.items():
            classes = {d.split(":")[0] for d in WC.defects_of(case, leaf, t)}
            assert {"host", "dtype", "strided", "short", "other_device"} <= classes
            assert case.roles[leaf] != "out" or "offset-shape" in classes
        for (leaf, defect), (header, text) in case.exempt.items():
            assert leaf in tensors and defect in WC.defects_of(case, leaf, tensors[leaf]), (case.name, leaf, defect)
            source = " ".join(open(os.path.join(WC.REPO, "include", header)).read().replace(" * ", " ").split())
            assert len(text) >= 20 and " ".join(text.split()) in source, f"{case.name} {leaf} {defect}: {header} does not say {text!r}"
            exemptions += 1
        for key, want in case.expect.items():
            assert key[0] in tensors and key[1] in WC.defects_of(case, key[0], tensors[key[0]]), (case.name, key)
            assert want in WC.EXPECTATIONS or WC.library_case_exists(want), (case.name, key, want)
    print(f"{exemptions} exemptions, each citing its header; {len(WC.all_rows())} rows")
    assert exemptions <= 20


# ---- the product path: what MVSNet hands over --------------------------------------------------------------------------
def _model():
    return MVSNet(refine=False, debug=0).eval()


def _judge(world, entries):
    called = {c[0] for c in world.calls}
    assert not world.problems(), world.problems()
    assert called == set(entries), called


@pytest.mark.parametrize("variant", ["expanded depth_values", "strided proj_matrices", "uint8 HWC slice of a larger batch"])
def test_forward_hands_over_honest_row_views(variant):
    world = WC.World(fake=True)
    with WC.installed(world):
        m = WC.Maker("fake")
        imgs, proj, dv = m.f(2, 3, 3, 32, 32, lo=0, hi=1), m.proj(2, 3), m.depths(8)[None].expand(2, 8)
        if variant == "strided proj_matrices":
            proj = m.like(proj, strided=True)
        if variant.startswith("uint8"):
            imgs = m.u8(4, 3, 32, 32, 3)[1:3]
        world.passed = [imgs, proj, dv]
        out = _model()(imgs, proj, dv)
        assert tuple(out["depth"].shape) == (2, 8, 8)
    _judge(world, ["mvs_forward_images_fmt"])
    assert len(world.calls) == 2


def test_extract_features_and_forward_features_hand_over_honest_row_views():
    world = WC.World(fake=True)
    with WC.installed(world):
        m = WC.Maker("fake")
        model = _model()
        imgs = m.u8(6, 32, 32, 3)[1:5]
        feats = model.extract_features(imgs, chunk=3)
        proj, dv = m.like(m.proj(2, 3), strided=True), m.depths(8)[None].expand(2, 8)
        world.passed = [imgs, proj, dv]
        out = model.forward_features(feats, [[0, 1, 2], [3, 1, 0]], proj, dv)
        assert tuple(out["photometric_confidence"].shape) == (2, 8, 8)
    _judge(world, ["mvs_feature_net_fmt", "mvs_depth_infer_views"])
    assert len(world.calls) == 4
