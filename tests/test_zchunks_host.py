"""The library's launch plans (csrc/launch_plan.h, asked through tests/zchunks.py) on known values, the reach of the
z-chunk case categories, and the planner alone under the host sanitizers (no GPU needed; tests/test_gpu_zchunks.py runs
the cases)."""
import os
import subprocess

import pytest

import gpu_child
import zchunks
from zchunks import LAYER, TAIL, WARP, plan

CFG2 = (192, 128, 160)   # 640 x 512 images, D = 192 (cfg2; cfg5 has the same volume)
CFG3 = (256, 296, 400)   # 1600 x 1184 images, D = 256


def test_known_splits_at_256_cus():
    assert zchunks.conv11_prob(*CFG2, 256)[:3] == (11, 9, 8)
    assert zchunks.conv11_prob(*CFG3, 256)[:3] == (26, 5, 24)
    assert zchunks.conv11_prob(192, 144, 40, 256)[:3] == (5, 20, 1)
    assert zchunks.conv11_prob(16, 8, 8, 256)[:3] == (4, 2, 4)       # the clamp to >= 4 planes
    assert zchunks.conv1z(*CFG2, 256)[:3] == (16, 6, 16)
    assert zchunks.conv1z(*CFG3, 256)[:3] == (128, 1, 128)
    assert zchunks.conv1z(296, 104, 8, 256)[:3] == (5, 30, 3)
    assert zchunks.convz16(2, *CFG3, 256)[:3] == (19, 7, 14)
    assert zchunks.convz16(3, 8, 8, 8, 256) is None                  # Do = 2 < 4: the tile kernel
    assert zchunks.conv0z16(4, 64, 64, 256) is None
    # grids: tiles x chunks (cfg2 conv11_prob: 6 x 9 tiles of 30 x 14 logits)
    assert zchunks.conv11_prob(*CFG2, 256).grid == 6 * 9 * 9


@pytest.mark.parametrize("D,slab,n", [(288, 44, 7), (632, 44, 15), (312, 36, 9), (320, 36, 9), (192, 40, 5),
                                      (256, 40, 7), (640, 44, 15)])
def test_tap_cache_slab(D, slab, n):
    s = zchunks.tc_slab(D, 16, 24)
    assert (s.zc, s.n) == (slab, n)
    assert s.grid == 12 * n         # 384 pixels = 12 blocks of 32
    assert s.n % 8 != 0


@pytest.mark.parametrize("cus", [80, 256, 304])
@pytest.mark.parametrize("name", sorted(zchunks.LAUNCHERS))
def test_every_category_has_a_small_shape(name, cus):
    found = zchunks.cheapest_cases(name, cus)
    missing = set(zchunks.required_categories(name)) - set(found)
    assert not missing, (name, cus, missing)
    fn = zchunks.LAUNCHERS[name]
    for cat, (D, h, w) in found.items():
        assert D % 8 == 0 and h % 8 == 0 and w % 8 == 0
        assert D * h * w <= zchunks.MAX_VOXELS
        assert cat in zchunks.categories(name, fn(D, h, w, cus))
    # the example shapes the categories were first found with are no cheaper than the search's
    if name == "conv11_prob" and cus == 256:
        assert found["last1"][0] * found["last1"][1] * found["last1"][2] <= 192 * 144 * 40


def test_conv1z_reaches_long_chunks_through_persist_cus():
    found = zchunks.cheapest_cases("conv1z", 4, 24)
    assert {"single", "zc0-last1", "zc0-last2", "zc1-last2", "zc2-last1"} <= set(found)
    for D, h, w in found.values():
        assert zchunks.conv1z(D, h, w, 4).zc >= 24


# ---------------------------------------------------------------- the planned forms
# Expected values: the kernel names, grids and workgroup sizes the parent commit of the planner launched on a 256-CU
# MI355X (profiles/launch_plan_kernels_parent.txt: tools/prof_stage.py all 2 <cfg> under a kernel trace) for the launched
# rows, and the parent's launcher code for the rest (layers 9 and 10 behind the fused tail, the switches, the edges).


def layer_plans(shape, storage, cus=256, **switches):
    """{layer: (form, tile)} of layers 0 .. 10 in a volume `shape`"""
    D, h, w = shape
    levels = [0, 0, 1, 1, 2, 2, 3, 3, 2, 1, 0]
    out = {}
    for layer, lv in enumerate(levels):
        p = plan(LAYER, D >> lv, h >> lv, w >> lv, cus, layer=layer, storage=storage, **switches)
        out[layer] = (p.form, p.tile)
    return out


def tail_plan(shape, storage, cus=256, **switches):
    D, h, w = shape
    return plan(TAIL, D // 2, h // 2, w // 2, cus, layer=9, storage=storage, **switches)


def test_default_forms_cfg2_fp32():
    got = layer_plans(CFG2, "f32")
    z = (0, 0, 0)
    assert got == {0: ("Conv0WinoSplit", z), 1: ("Conv1Z", z), 2: ("ConvGSplit", (2, 4, 2)), 3: ("ConvGSplit", (2, 2, 1)),
                   4: ("ConvGSplit", (4, 2, 1)), 5: ("ConvS", z), 6: ("ConvS", z), 7: ("DeconvS", z),
                   8: ("DeconvGSplit", (2, 4, 1)), 9: ("DeconvG", z), 10: ("ProbLds", z)}
    assert plan(LAYER, *CFG2, 256, layer=1).split == (16, 6, 16, 240)             # conv1z_mfma_kernel: 240 blocks
    t = tail_plan(CFG2, "f32")
    assert (t.form, t.split) == ("TailSplit", (11, 9, 8, 486))                    # conv11_prob_split_kernel: 486 blocks
    wp = plan(WARP, *CFG2, 256, N=3)
    assert (wp.form, wp.split, wp.depth_fastest) == ("WarpTc", (40, 5, 32, 640 * 5), 0)   # grid (640, 5)


def test_default_forms_cfg3_bf16():
    got = layer_plans(CFG3, "bf16")
    z = (0, 0, 0)
    assert got == {0: ("Conv0Z16", z), 1: ("ConvZ16", z), 2: ("ConvZ16", z), 3: ("ConvG16", (4, 1, 1)),
                   4: ("ConvG16", (4, 2, 1)), 5: ("ConvG16", (2, 1, 1)), 6: ("ConvG16", (4, 1, 1)),
                   7: ("DeconvG16", (2, 1, 1)), 8: ("DeconvG16", (4, 2, 1)), 9: ("DeconvG16", (1, 4, 2)), 10: ("ProbLds", z)}
    assert plan(LAYER, *CFG3, 256, layer=0, storage="bf16").split == (256, 1, 256, 481)
    assert plan(LAYER, *CFG3, 256, layer=1, storage="bf16").split == (128, 1, 128, 247)
    assert plan(LAYER, 128, 148, 200, 256, layer=2, storage="bf16").split == (19, 7, 14, 931)
    t = tail_plan(CFG3, "bf16")
    assert (t.form, t.split) == ("Tail16", (26, 5, 24, 1470))
    wp = plan(WARP, *CFG3, 256, N=5, storage="bf16")
    assert (wp.form, wp.split, wp.depth_fastest) == ("WarpTc", (40, 7, 16, 3700 * 7), 1)  # grid (7, 3700)


def test_default_forms_cfg5_fp16():
    got = layer_plans(CFG2, "f16")
    z = (0, 0, 0)
    assert got == {0: ("Conv0Z16", z), 1: ("ConvZ16", z), 2: ("ConvG16", (2, 4, 2)), 3: ("ConvG16", (4, 1, 1)),
                   4: ("ConvG16", (4, 2, 1)), 5: ("ConvG16", (1, 1, 1)), 6: ("ConvG16", (1, 1, 1)),
                   7: ("DeconvG16", (1, 1, 1)), 8: ("DeconvG16", (4, 2, 1)), 9: ("DeconvG16", (1, 4, 2)), 10: ("ProbLds", z)}
    assert plan(LAYER, *CFG2, 256, layer=0, storage="f16").split == (64, 3, 64, 240)
    assert plan(LAYER, *CFG2, 256, layer=1, storage="f16").split == (16, 6, 16, 240)
    t = tail_plan(CFG2, "f16")
    assert (t.form, t.split) == ("Tail16", (11, 9, 8, 486))
    wp = plan(WARP, *CFG2, 256, N=4, storage="f16")
    assert (wp.form, wp.split, wp.depth_fastest) == ("WarpTc", (40, 5, 32, 640 * 5), 0)


def test_every_switch_changes_its_form():
    """The one change each of Options' 20 switches makes, against the default rows above."""
    f32 = lambda **sw: layer_plans(CFG2, "f32", **sw)    # noqa: E731
    f16 = lambda **sw: layer_plans(CFG2, "f16", **sw)    # noqa: E731
    z = (0, 0, 0)
    seen = set()

    def changed(base, got, want, *names):
        seen.update(names)
        assert {k: v for k, v in got.items() if base[k] != v} == want, names

    d32, d16 = f32(), f16()
    changed(d32, f32(conv0_wino=0), {0: ("Conv0Mfma", z)}, "conv0_wino")
    changed(d32, f32(conv0_split=0), {0: ("Conv0Wino", z)}, "conv0_split")
    changed(d32, f32(split_layers=0), {2: ("ConvWz", z), 3: ("ConvG", z), 4: ("ConvWz", z), 8: ("DeconvG", z)}, "split_layers")
    changed(f32(split_layers=0), f32(split_layers=0, conv_wino=0), {2: ("ConvG", z), 4: ("ConvG", z)}, "conv_wino")
    changed(d32, f32(conv_wino=0), {})                     # behind the split-operand layers
    changed(d32, f32(force_direct=1), {k: ("Direct", z) for k in range(11)}, "force_direct")
    changed(d16, f16(force_direct=1), {k: ("Direct", z) for k in range(11)})     # (the launcher refuses 16-bit storage)
    changed(d32, f32(split_deconv=3), {7: ("DeconvGSplit", (1, 1, 1))}, "split_deconv")
    changed(d32, f32(split_deconv=0), {8: ("DeconvG", z)})
    changed(d32, f32(conv1z=0), {1: ("ConvGPersist", z)}, "conv1z")
    assert plan(LAYER, *CFG2, 256, layer=1, conv1z=0).split.grid == 256 * 3         # three persistent blocks per CU
    assert plan(LAYER, 8, 8, 8, 256, layer=1).form == "ConvG" and plan(LAYER, 8, 8, 8, 256, layer=1, conv1z=1).form == "Conv1Z"
    assert plan(LAYER, *CFG2, 256, layer=1, persist_cus=4).split == (96, 1, 96, 40)
    assert plan(LAYER, *CFG2, 256, layer=1, conv1z=0, persist_cus=4).split.grid == 4 * 3
    seen.add("persist_cus")
    changed(d16, f16(mfma16=0), {0: ("Conv0Wino", z), 1: ("ConvGPersist", z), 2: ("ConvWz", z), 3: ("ConvG", z), 4: ("ConvWz", z),
                                 5: ("ConvS", z), 6: ("ConvS", z), 7: ("DeconvS", z), 8: ("DeconvG", z), 9: ("DeconvG", z)}, "mfma16")
    assert tail_plan(CFG2, "f16", mfma16=0).form == "TailTwoLaunches"
    changed(d16, f16(convz16=0), {1: ("ConvG16", (2, 2, 2))}, "convz16")
    changed(d16, f16(convz16=1), {2: ("ConvZ16", z), 3: ("ConvZ16", z)})
    changed(d16, f16(conv0z16=0), {0: ("Conv0Tile16", z)}, "conv0z16")
    assert plan(LAYER, 8, 8, 8, 256, layer=0, storage="f16").form == "Conv0Tile16"
    assert plan(LAYER, 8, 8, 8, 256, layer=0, storage="f16", conv0z16=1).form == "Conv0Z16"
    changed(d16, f16(deep_tiles=0), {4: ("ConvG16", (1, 2, 2)), 8: ("DeconvG16", (1, 4, 1))}, "deep_tiles")
    changed(d16, f16(deep_tiles=1), {5: ("ConvG16", (2, 1, 1)), 6: ("ConvG16", (4, 1, 1)), 7: ("DeconvG16", (2, 1, 1))})
    # the tail
    assert tail_plan(CFG2, "f32", fuse_prob=0).form == "TailTwoLaunches" and tail_plan(CFG2, "f16", fuse_prob=0).form == "TailTwoLaunches"
    assert tail_plan(CFG2, "f32", tail_split=0)[:3:2] == ("TailPriv", (11, 9, 8, 486))
    assert tail_plan(CFG2, "f16", tail_split=0).form == "Tail16"
    seen.update(["fuse_prob", "tail_split"])
    # the warp: fp32 feature copy, and the 16-bit copy of MVS_FEAT16=1 (feature element size 2)
    w32 = lambda **sw: plan(WARP, *CFG2, 256, N=3, **sw)                                 # noqa: E731
    w16 = lambda **sw: plan(WARP, *CFG2, 256, N=3, storage="f16", fes=2, **sw)           # noqa: E731
    assert (w32().form, w16().form) == ("WarpTc", "WarpTc")
    assert (w32(warp_tc=0).form, w32(warp_tc=0).depth_fastest, w16(warp_tc=0).form) == ("WarpPlain", 0, "WarpTc")
    assert (w16(warp_tc16=0).form, w16(warp_tc16=0).depth_fastest, w32(warp_tc16=0).form) == ("WarpPlain", 0, "WarpTc")
    assert w32(warp_tc=0, warp_depth_fastest=1).depth_fastest == 1 and w32(warp_depth_fastest=1).depth_fastest == 0
    assert w32(warp_depth_fastest_tc=1).depth_fastest == 1 and w32(warp_tc=0, warp_depth_fastest_tc=1).depth_fastest == 0
    assert plan(WARP, *CFG3, 256, N=5, storage="bf16", warp_depth_fastest_tc=0).depth_fastest == 0
    seen.update(["warp_tc", "warp_tc16", "warp_depth_fastest", "warp_depth_fastest_tc"])
    # MVS_FEAT16 picks the feature copy's element size (mvs_host.hip) and MVS_FEAT_SPLIT01 FeatureNet's kernels: no plan moves
    for name in ("feat16", "feat_split01"):
        assert f16(**{name: 1}) == d16 and f32(**{name: 1}) == d32 and w32(**{name: 1}) == w32()
        assert tail_plan(CFG2, "f16", **{name: 1}) == tail_plan(CFG2, "f16")
        seen.add(name)
    assert seen == set(zchunks.switch_names()) and len(seen) == 20


def test_fall_through_edges():
    z = (0, 0, 0)
    assert plan(LAYER, 12, 16, 16, 256, layer=0).form == "Conv0WinoSplit"
    assert plan(LAYER, 10, 16, 16, 256, layer=0).form == "Conv0Mfma"                      # D % 4 != 0
    assert plan(LAYER, 8, 16, 16, 256, layer=3, storage="bf16", convz16=1).form == "ConvZ16"     # Do = 4
    assert plan(LAYER, 6, 16, 16, 256, layer=3, storage="bf16", convz16=1)[:2] == ("ConvG16", (4, 1, 1))   # Do = 3 < 4
    assert plan(LAYER, 3, 16, 16, 256, layer=2, storage="bf16", convz16=1)[:2] == ("ConvG16", (2, 4, 2))
    assert plan(LAYER, 8, 16, 16, 256, layer=0, storage="bf16", conv0z16=1).form == "Conv0Z16"
    assert plan(LAYER, 7, 16, 16, 256, layer=0, storage="bf16", conv0z16=1)[:2] == ("Conv0Tile16", z)     # D < 8
    assert plan(WARP, 192, 128, 160, 256, N=5).form == "WarpTc"
    assert plan(WARP, 192, 128, 160, 256, N=6).form == "WarpPlain"                        # 2 <= N <= 5
    assert plan(WARP, 192, 128, 160, 256, N=1).form == "WarpPlain"
    # the deep-tile threshold 2 nb >= 3 cus of conv6 (tile 4 x 1 x 1 M-tiles: nb = ceil(D / 4) x ceil(H / 2) x ceil(W / 8))
    deep = lambda nb, cus: plan(LAYER, 4, 2, 8 * nb, cus, layer=6, storage="bf16").tile == (4, 1, 1)   # noqa: E731
    assert not deep(10, 7)      # 2 nb = 3 cus - 1
    assert deep(12, 8)          # 2 nb = 3 cus
    assert deep(11, 7)          # 2 nb = 3 cus + 1
    assert plan(LAYER, 4, 2, 80, 7, layer=6, storage="bf16").tile == (1, 1, 1)


# ---------------------------------------------------------------- the planner alone, under the host sanitizers
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"      # the host compiler of the toolchain that builds the library


def test_plan_sweep_under_host_sanitizers(tmp_path):
    """tests/plan_sweep.cpp: every plan at the ends of the ABI's shape domain, as a stand-alone host program built with
    the address and undefined-behaviour sanitizers (nothing is preloaded, nothing is loaded into Python, no GPU)."""
    assert os.path.exists(CXX), CXX
    exe = tmp_path / "plan_sweep"
    subprocess.run([CXX, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "scene_3dreconstruction_mvsnet_amd", "csrc"),
                    os.path.join(REPO, "tests", "plan_sweep.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 bad" in r.stdout.splitlines()[-1], r.stdout[-500:]


# ---------------------------------------------------------------- zchunk_check.py: what is a verdict and what is not
CHILD = """
import json, sys
sys.path.insert(0, {tests!r})
import zchunk_check as z
from scene_3dreconstruction_mvsnet_amd import _lib
def fails(storage, D, save):
    if D == 8: raise AssertionError("out of tolerance")
    if D == 16: raise _lib.MvsError(2, "a refusal of the library")
    if D == 24: raise RuntimeError({text!r})
z.run_warp = fails      # no case reaches the GPU
sys.argv = ["zchunk_check.py", {cases!r}, {out!r}]
sys.exit(z.main())
"""


def _check_child(tmp_path, depths, text=""):
    import json
    cases, out = tmp_path / "cases.json", tmp_path / "out.json"
    cases.write_text(json.dumps([{"id": f"D{D}", "op": "warp", "storage": "f32", "layer": None, "shape": [D, 16, 24],
                                  "save": None} for D in depths]))
    script = CHILD.format(tests=os.path.join(REPO, "tests"), text=text, cases=str(cases), out=str(out))
    r = gpu_child.run(["-c", script], timeout=300, gpu=False)
    return r, (json.loads(out.read_text()) if out.exists() else {})


def test_zchunk_check_keeps_failures_and_refusals_as_verdicts(tmp_path):
    r, verdicts = _check_child(tmp_path, [8, 16, 32])
    assert r.returncode == 0, r.stderr[-2000:]
    assert [verdicts[k]["ok"] for k in ("D8", "D16", "D32")] == [False, False, True]
    assert "out of tolerance" in verdicts["D8"]["msg"] and "libmvs_hip status 2" in verdicts["D16"]["msg"]


@pytest.mark.parametrize("text", ["HIP error: an illegal memory access was encountered",
                                  "libmvs_hip status 4: conv11_prob launch: unspecified launch failure"],
                         ids=["torch", "library"])
def test_zchunk_check_ends_on_a_hip_error_the_way_the_stop_rule_reads(tmp_path, text):
    """The error is a Python exception made for the test; nothing runs on a GPU."""
    r, verdicts = _check_child(tmp_path, [8, 24, 32], text)
    assert r.returncode != 0 and text in r.stderr
    assert gpu_child.fatal_reason(r.returncode, r.timed_out, r.stderr) is not None
    assert list(verdicts) == ["D8"] and not verdicts["D8"]["ok"]      # the case before it kept its verdict; none ran after
