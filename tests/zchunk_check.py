#!/usr/bin/env python3
"""Child-process helper of tests/test_gpu_zchunks.py: runs a list of z-chunk / depth-slab cases under whatever
kernel-selection environment the parent set (read once per process) and checks each against the CPU oracle.

    zchunk_check.py CASES.json RESULTS.json

Every case is {"id", "op": "conv11_prob" | "layer" | "warp", "storage", "layer", "shape": [D, h, w], "save"}; the
results file maps each id to {"ok", "msg"} and is rewritten after every case, so the cases that ran before a crash
keep their verdicts.  "warp" cases also save the raw volume to `save` for the parent's bit-equality checks.
"""
import functools
import json
import os
import sys
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gpu_child  # noqa: E402
from conftest import assert_conf_close, rel_l1  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic  # noqa: E402

DEV = "cuda:0"
LAYER_ATOL = 2e-4   # x max|want|: fp32 layers, as test_gpu_fullsize / test_gpu_conv0_tile
EPS = {"f32": 0.0, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}
WARP_N, WARP_H, WARP_W = 5, 16, 24   # 384 pixels: 12 pixel blocks
SD = synthetic.random_costreg_state(seed=31)


@functools.lru_cache(maxsize=None)
def blob():
    return _lib.pack_weights(SD).to(DEV)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def check_fp32(got, want, what):
    scale = max(float(np.abs(want).max()), 1.0)
    np.testing.assert_allclose(got, want, rtol=0, atol=LAYER_ATOL * scale, err_msg=what)
    r = rel_l1(got, want)
    assert r < 2e-6, f"{what}: rel-L1 {r:.3e}"


def run_layer(layer, storage, D, h, w, rng):
    """conv0 .. conv3 on a random input of the layer's size, against the oracle (16-bit: the matched-storage oracle
    and bounds of layer_check.py)."""
    code = _lib.dtype_code(storage)
    q = lambda t: orc.round_storage(t, storage)  # noqa: E731
    ci, _ = _lib._LAYER_CH[layer]
    lvl = 0 if layer <= 1 else 1
    x = q(rng.standard_normal((ci, D >> lvl, h >> lvl, w >> lvl)).astype(np.float32))
    key, bn = _lib.CONV_WEIGHT_KEYS[layer], _lib.BN_PREFIXES[layer]
    stride = 2 if layer in (1, 3) else 1
    got = _lib.from_c8(_lib.conv_layer(layer, _lib.to_c8(cu(x)).to(_lib.TORCH_DTYPES[code]), None, blob(),
                                       dtype=code).float()).cpu().numpy()
    if storage == "f32":
        check_fp32(got, orc.conv3d(x, SD[key], bn=orc._bn(SD, bn), stride=stride), f"layer {layer}")
        return
    wf, sh = orc._fold(SD, key, bn)
    want = q(orc.conv3d(x, q(wf), bias=sh, bn=None, stride=stride, relu=True))
    scale = max(float(np.abs(want).max()), 1.0)
    np.testing.assert_allclose(got, want, rtol=2 * EPS[storage], atol=3e-4 * scale, err_msg=f"layer {layer} {storage}")


def run_conv11_prob(storage, D, h, w, rng):
    """The fused tail prob(conv11(x) + skip) on d9 = (16, D/2, h/2, w/2) and skip = (8, D, h, w); the logits against
    the oracle (fp32: test_cfg2_fused_conv11_prob_matches_oracle's bounds; 16-bit: the matched oracle of
    test_fused_conv11_prob_16bit_matches_oracle), then the maps softargmin makes of them."""
    code = _lib.dtype_code(storage)
    tdt = _lib.TORCH_DTYPES[code]
    q = lambda t: orc.round_storage(t, storage)  # noqa: E731
    x = q(np.abs(rng.standard_normal((16, D // 2, h // 2, w // 2))).astype(np.float32))
    skip = q(np.abs(rng.standard_normal((8, D, h, w))).astype(np.float32))
    got = _lib.conv11_prob(_lib.to_c8(cu(x)).to(tdt), _lib.to_c8(cu(skip)).to(tdt), blob(), dtype=code).cpu().numpy()
    assert np.isfinite(got).all()
    if storage == "f32":
        d11 = skip + orc.deconv3d(x, SD["conv11.0.weight"], bn=orc._bn(SD, "conv11.1"))
    else:
        wf, sh = orc._fold(SD, "conv11.0.weight", "conv11.1", transposed=True)
        wt = np.ascontiguousarray(q(wf).transpose(1, 0, 2, 3, 4))
        d11 = skip + np.maximum(orc.deconv3d(x, wt, bn=None, relu=False) + sh[:, None, None, None], 0.0)
    want = orc.conv3d(d11, SD["prob.weight"], bias=SD["prob.bias"], bn=None, relu=False)[0]
    if storage == "f32":
        check_fp32(got, want, "conv11_prob logits")
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-5 * max(float(np.abs(want).max()), 1.0),
                                   err_msg=f"conv11_prob logits {storage}")
    dv = synthetic.depth_values(D)
    depth, conf, _ = orc.softargmin_conf(got, dv)
    depth_o, conf_o, idx_o, prob_o = orc.softargmin_conf(want, dv, want_prob=True)
    assert rel_l1(depth, depth_o) < 1e-5, rel_l1(depth, depth_o)
    assert_conf_close(conf, conf_o, idx_o, prob=prob_o, atol=1e-4)


def run_warp(storage, D, save):
    """The variance volume of WARP_N views at WARP_H x WARP_W against the oracle (16-bit: the fp32 volume rounded to
    the storage type, from features rounded too when MVS_FEAT16=1 narrows the gather copy), saved raw for the
    parent's comparison with the plain kernel."""
    code = _lib.dtype_code(storage)
    feats = synthetic.random_features(WARP_N, 32, WARP_H, WARP_W, seed=D)
    proj = synthetic.cameras(WARP_N, WARP_H, WARP_W, yaw_deg=1.0)
    dv = synthetic.depth_values(D)
    ws = _lib.alloc_workspace(WARP_N, 32, D, WARP_H, WARP_W, DEV, code)
    var = _lib.warp_variance(cu(feats), _lib.relative_proj(cu(proj)), cu(dv), ws, dtype=code)
    torch.cuda.synchronize()
    raw = var.view(torch.int32 if storage == "f32" else torch.int16).cpu().numpy()
    np.save(save, raw)
    got = _lib.from_c8(var.float()).cpu().numpy()
    assert np.isfinite(got).all()
    if storage == "f32":
        want = orc.variance_volume(feats, proj, dv)
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-4)
    else:
        q = lambda t: orc.round_storage(t, storage)  # noqa: E731
        f = q(feats) if os.environ.get("MVS_FEAT16") == "1" else feats
        np.testing.assert_allclose(got, q(orc.variance_volume(f, proj, dv)), rtol=EPS[storage], atol=5e-4)


def main():
    cases_path, out_path = sys.argv[1:3]
    with open(cases_path) as f:
        cases = json.load(f)
    results = {}
    for case in cases:
        D, h, w = case["shape"]
        rng = np.random.default_rng(D * 7919 + h * 31 + w)
        try:
            if case["op"] == "layer":
                run_layer(case["layer"], case["storage"], D, h, w, rng)
            elif case["op"] == "conv11_prob":
                run_conv11_prob(case["storage"], D, h, w, rng)
            else:
                run_warp(case["storage"], D, case["save"])
            results[case["id"]] = {"ok": True, "msg": ""}
        except (AssertionError, RuntimeError) as e:   # RuntimeError: a status the library returned
            if any(t in str(e) for t in gpu_child.HIP_ERROR_TEXTS):
                raise   # a HIP error is no verdict: the child ends with it on stderr, which gpu_child's stop rule reads
            results[case["id"]] = {"ok": False, "msg": "".join(traceback.format_exception_only(type(e), e))[-4000:]}
        with open(out_path, "w") as f:
            json.dump(results, f)
    env = {k: v for k, v in os.environ.items() if k.startswith("MVS_")}
    print(f"zchunk_check env={env}: {sum(r['ok'] for r in results.values())} of {len(cases)} cases pass")
    return 0


if __name__ == "__main__":
    sys.exit(main())
