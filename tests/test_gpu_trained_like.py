"""The inference path on BatchNorm parameters like a trained checkpoint's (tests/golden/gen_trained_golden.py: signed
gamma, one zero gamma per layer, folded |scale| from 0.03 to 95, means as large as the conv output) -- every other GPU
test draws gamma and running_var from [0.5, 1.5] or uses an identity BatchNorm.

1. Every conv kernel form per layer, dense, against fp64 (tests/trained_check.py, one child per kernel-selection
   environment): the cases of test_gpu_conv_probes.py, the shapes of test_gpu_split_tile_pipeline.py, the layers of
   test_gpu_featnet_ref.py; fp32, bf16 and fp16 storage; the bounds of tests/probes.py and tests/featnet_ref.py, which
   scale per element with conv(|x|, |w_fold|) of the element's own channel.  Each child runs the trained-like state and
   the same state with two extreme channels per layer (running_var = 0; scale = 2^-12: fp16-subnormal folded weights).
2. Stages and end to end against the reference fixture fx_trained.npz: warp + variance, CostRegNet, soft-argmin, the
   depth path, MVSNet.forward from images after load_state_dict; 16-bit storage against the matched oracle.

Stage tolerances are the project's first ones (test_gpu_parity.py): volumes 3e-4 max(|want|, 1), depth rel_l1 < 1e-5,
confidence assert_conf_close at 1e-3.  Every stage also prints e_hip = max|hip - ref64| next to the fixture's
e_ref = max|ref32 - ref64|: DESIGN.md section 2 records them.  A stage that missed its first tolerance with
e_hip <= 2 e_ref would be ill-conditioned, not wrong, and its tolerance would become 2 e_ref (the factor: DESIGN.md
section 11.4); none does.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_child  # noqa: E402
import trained_like as T  # noqa: E402
from conftest import assert_conf_close, rel_l1  # noqa: E402
from featnet_check import ENVS  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from probe_check import CASES  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 1. per layer, dense, every kernel form ----------------------------------------------------------------------------
def run_child(mode, name, env):
    r = gpu_child.run(["trained_check.py", mode, name], env=env, timeout=300)
    assert r.returncode == 0, f"trained_check {mode} {name}: rc {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}"
    res = r.json()
    worst = max(res["ratios"], key=res["ratios"].get)
    print(f"{mode} {name}: worst error / bound {res['ratios'][worst]:.4f} at {worst}; {res['seconds']} s")
    for key, (c, top, rel_err, rel_bound, ratio) in sorted(res["channels"].items(), key=lambda kv: -kv[1][4])[:3]:
        print(f"  smallest channel of {key}: channel {c}, max|ref64| {top:.3e}, error / max|ref64| {rel_err:.3e}, "
              f"bound / max|ref64| {rel_bound:.3e}")
    if res["flush16"]:
        print(f"  fp16 extreme channels: worst error / bound {max(v for k, v in res['ratios'].items() if k in res['flush16']):.4f}, "
              f"with the flush term {max(res['flush16'].values()):.4f}")
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_conv_layers_dense_on_trained_like_bn(case):
    res = run_child("layers", case, CASES[case]["env"])
    want = {f"{s}:{l}:dense:{st}" for s in ("trained", "extreme") for l in CASES[case]["layers"] for st in CASES[case]["storages"]}
    assert want <= set(res["ratios"]), want - set(res["ratios"])
    assert not res["failures"] and max(res["ratios"].values()) <= 1.0, res["failures"]


@pytest.mark.parametrize("envname", ["default", "split01"])
def test_feature_layers_dense_on_trained_like_bn(envname):
    """MVS_FEAT16 selects no FeatureNet conv kernel (it narrows the finished features): not run here"""
    res = run_child("featnet", envname, ENVS[envname])
    want = {f"{s}:{k}:dense" for s in ("trained", "extreme") for k in [f"layer{l}" for l in range(8)] + ["fused"]}
    assert want <= set(res["ratios"]), want - set(res["ratios"])
    assert not res["failures"] and max(res["ratios"].values()) <= 1.0, res["failures"]


# ---- 2. stages and end to end against the reference fixture -------------------------------------------------------------
def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def problem():
    fx = T.fixture()
    for v in fx.values():
        v.setflags(write=False)
    return fx, T.costreg_state()


@functools.lru_cache(maxsize=None)
def blob():
    return _lib.pack_weights(problem()[1]).to(DEV)


def report(stage, got, fx, key):
    """prints the three figures of the stage; returns max|got - ref32|"""
    want, ref64 = fx[key][0], fx[key + "_ref64"][0]
    e32, e_hip, e_ref = float(np.abs(got - want).max()), float(np.abs(got - ref64).max()), float(fx["e_ref/" + key])
    print(f"{stage}: max|hip - ref32| {e32:.3e}, e_hip = max|hip - ref64| {e_hip:.3e}, e_ref = max|ref32 - ref64| {e_ref:.3e}, "
          f"max|want| {float(np.abs(want).max()):.4g}")
    return e32


def volume_tolerance(want):
    return 3e-4 * max(float(np.abs(want).max()), 1.0)


def test_warp_variance_matches_the_trained_fixture():
    fx, _ = problem()
    feats, proj, dv = fx["features"][0], fx["proj_matrices"][0], fx["depth_values"][0]
    ws = _lib.alloc_workspace(feats.shape[0], 32, dv.shape[0], feats.shape[2], feats.shape[3], DEV)
    got = _lib.from_c8(_lib.warp_variance(cu(feats), _lib.relative_proj(cu(proj)), cu(dv), ws)).cpu().numpy()
    assert report("warp_variance", got, fx, "variance") <= volume_tolerance(fx["variance"][0])


def test_costreg_matches_the_trained_fixture():
    fx, _ = problem()
    var = fx["variance"][0]
    ws = _lib.alloc_workspace(1, *var.shape, DEV)
    got = _lib.costreg_forward(_lib.to_c8(cu(var)), blob(), ws).cpu().numpy()
    assert report("costreg_forward", got, fx, "cost_reg") <= volume_tolerance(fx["cost_reg"][0])


def check_maps(stage, depth, conf, fx):
    report(stage + " depth", depth, fx, "depth")
    report(stage + " confidence", conf, fx, "photometric_confidence")
    r = rel_l1(depth, fx["depth"][0])
    print(f"{stage}: depth rel_l1 {r:.3e}")
    assert r < 1e-5
    assert_conf_close(conf, fx["photometric_confidence"][0], fx["expected_index"][0], prob=fx["prob_volume"][0], atol=1e-3)


def test_softargmin_conf_matches_the_trained_fixture():
    fx, _ = problem()
    depth, conf = _lib.softargmin_conf(cu(fx["cost_reg"][0]), cu(fx["depth_values"][0]))
    check_maps("softargmin_conf", depth.cpu().numpy(), conf.cpu().numpy(), fx)


def hip_depth_infer(fx, dtype=_lib.MVS_F32):
    feats, proj, dv = fx["features"][0], fx["proj_matrices"][0], fx["depth_values"][0]
    N, C, h, w = feats.shape
    ws = _lib.alloc_workspace(N, C, dv.shape[0], h, w, DEV, dtype)
    depth = torch.empty((h, w), dtype=torch.float32, device=DEV)
    conf = torch.empty_like(depth)
    _lib.depth_infer(cu(feats), cu(proj), cu(dv), blob(), ws, depth, conf, dtype=dtype)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), conf.cpu().numpy()


def test_depth_infer_matches_the_trained_fixture():
    fx, _ = problem()
    check_maps("depth_infer", *hip_depth_infer(fx), fx)


def test_mvsnet_forward_from_images_matches_the_trained_fixture():
    """load_state_dict of the trained-like state, then images in: FeatureNet, _packable_state and the eps the module
    passes to both packers are on this path"""
    fx, _ = problem()
    model = MVSNet(refine=False).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in T.weights().items()})
    model.eval()
    feats = model.extract_features(cu(fx["imgs"][0]))
    assert report("extract_features", feats.cpu().numpy(), fx, "features") <= volume_tolerance(fx["features"][0])
    out = model(cu(fx["imgs"]), cu(fx["proj_matrices"]), cu(fx["depth_values"]))
    assert tuple(out["depth"].shape) == fx["depth"].shape
    check_maps("MVSNet.forward", out["depth"].cpu().numpy()[0], out["photometric_confidence"].cpu().numpy()[0], fx)


@pytest.mark.parametrize("storage", ["f16", "bf16"])
def test_16bit_storage_matches_matched_oracle_on_trained_like_bn(storage):
    """as test_gpu_parity.py::test_16bit_storage_matches_matched_oracle, on the trained-like state"""
    fx, sd = problem()
    depth, conf = hip_depth_infer(fx, dtype=_lib.dtype_code(storage))
    depth_m, conf_m = orc.depth_infer(fx["features"][0], fx["proj_matrices"][0], fx["depth_values"][0], sd, storage=storage)
    r_m, r_ref = rel_l1(depth, depth_m), rel_l1(depth, fx["depth"][0])
    print(f"{storage}: depth rel_l1 against the matched oracle {r_m:.3e}, against the fp32 reference {r_ref:.3e}")
    assert np.isfinite(depth).all() and np.isfinite(conf).all()
    assert r_m < (2e-4 if storage == "f16" else 1e-3)
    assert r_ref < (1e-3 if storage == "f16" else 1e-2)
