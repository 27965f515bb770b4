"""FeatureNet's kernels (csrc/featnet.hip: fconv_mfma_kernel in eight instantiations, fconv01_fused_kernel in three,
c8_to_nchw_kernel, narrow_kernel for f16 / bf16) against the fp64 reference, the single-product probes and the derived
bounds of tests/featnet_ref.py.  One child process per kernel-selection environment (tests/featnet_check.py), started
with a time limit and never retried (tests/gpu_child.py); and the 31-bit size guard of check_image_dims, just inside and at it.

The size-guard cases print their wall time (MEASURED_WALL records it); over two minutes, keep one inside case only.
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import featnet_ref as R  # noqa: E402
import gpu_child  # noqa: E402
from conftest import load_weights  # noqa: E402
from featnet_check import ENVS, INSTANTIATIONS, KEYS  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GIB = float(1 << 30)


@pytest.mark.parametrize("envname", list(ENVS))
def test_featnet_kernels_lie_within_the_fp64_bound(envname):
    r = gpu_child.run_once(("featnet", envname), ["featnet_check.py", envname], env=ENVS[envname], timeout=900)
    assert r.returncode == 0, f"featnet_check {envname}: rc {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}"
    res = r.json()
    assert set(KEYS[envname]) <= set(res["ratios"]), set(KEYS[envname]) - set(res["ratios"])
    assert not res["failures"] and res["worst"] <= 1.0, res


def test_every_kernel_instantiation_has_a_result_key():
    """8 layer kernels, 3 fused formats, c8_to_nchw and both narrow kernels each map to a key some environment reports"""
    assert len(INSTANTIATIONS) == 8 + 3 + 1 + 2
    reported = {k for keys in KEYS.values() for k in keys}
    assert set(INSTANTIATIONS.values()) <= reported


# ---- the size guard: N*H*W*8 < 2^31 (check_image_dims; goff[] in the staging code is a 32-bit int) --------------------
def pixel(n, y, x, c):
    """cheap deterministic uint8 image, the same integer arithmetic in numpy and torch (int64)"""
    return (y * 7 + x * 13 + c * 101 + n * 59 + ((y * x) >> 2) + ((y ^ x) * 3)) & 255


def device_image(N, H, W):
    """uint8 [N,H,W,3] on the device, generated there in row blocks"""
    img = torch.empty((N, H, W, 3), dtype=torch.uint8, device=DEV)
    xs = torch.arange(W, device=DEV, dtype=torch.int64)[None, :, None]
    cs = torch.arange(3, device=DEV, dtype=torch.int64)[None, None, :]
    for n in range(N):
        for y0 in range(0, H, 1024):
            ys = torch.arange(y0, min(H, y0 + 1024), device=DEV, dtype=torch.int64)[:, None, None]
            img[n, y0:y0 + ys.shape[0]] = pixel(n, ys, xs, cs).to(torch.uint8)
    return img


def host_crop(n, y0, y1, x0, x1):
    """fp32 [1,3,y1-y0,x1-x0] of the same image, as the loader would hand it over (x / 255 in fp32)"""
    ys = np.arange(y0, y1, dtype=np.int64)[None, :, None]
    xs = np.arange(x0, x1, dtype=np.int64)[None, None, :]
    cs = np.arange(3, dtype=np.int64)[:, None, None]
    return R.u8_to_f32(pixel(n, ys, xs, cs).astype(np.uint8))[None]


def check_window(st, feats, n, fy0, fx0, H, W, size=8):
    """feats[n, :, fy0:fy0+size, fx0:fx0+size] against the fp64 chain on the image crop that holds the window's whole
    receptive field (derived from FEATURE_LAYERS: R.receptive_field()); at the image border the crop ends there too, so
    the chain's zero padding is the true one.  Returns the worst error / chained bound."""
    rf, stride = R.receptive_field()
    half = rf // 2                                           # a multiple of the feature stride: the phases stay aligned
    assert half % stride == 0
    y0, x0 = max(0, fy0 * stride - half), max(0, fx0 * stride - half)
    y1, x1 = min(H, (fy0 + size - 1) * stride + half + 1), min(W, (fx0 + size - 1) * stride + half + 1)
    ref, E = R.chain_ref_bound(st, host_crop(n, y0, y1, x0, x1), consts={0: R.FUSED_C0})
    oy, ox = fy0 - y0 // stride, fx0 - x0 // stride
    got = feats[n, :, fy0:fy0 + size, fx0:fx0 + size].cpu().numpy()[None]
    return R.ratio(got, ref[:, :, oy:oy + size, ox:ox + size], E[:, :, oy:oy + size, ox:ox + size]), (y0, y1, x0, x1, oy, ox)


def run_inside(N, H, W, images):
    need = (_lib.query_feature_workspace(N, H, W) + N * H * W * 3 + N * 32 * (H // 4) * (W // 4) * 4) / GIB + 3.0
    total = torch.cuda.get_device_properties(DEV).total_memory / GIB
    if total < need:
        pytest.skip("needs %.1f GiB of device memory, the device has %.1f" % (need, total))
    assert N * H * W * 8 < 2 ** 31 <= (N + 1) * H * W * 8 or N == 1
    st = R.fstate(load_weights())
    fb = _lib.pack_feature_weights(st).to(DEV)
    t0 = time.time()
    try:
        img = device_image(N, H, W)
        feats = _lib.feature_net(img, fb)
        torch.cuda.synchronize()
        t1 = time.time()
        h, w = H // 4, W // 4
        windows = [(0, 0), (0, w - 8), (h - 8, 0), (h - 8, w - 8), (h - 8, w // 2 - 3), (h // 2 - 5, w - 8),
                   (h // 3, w // 5), (2 * h // 3 + 1, w // 2 + 3)]
        worst = 0.0
        for n in images:
            for fy0, fx0 in windows:
                r, where = check_window(st, feats, n, fy0, fx0, H, W)
                # bit equality with a small launch on the same crop (same pixels, same kernels, small offsets)
                y0, y1, x0, x1, oy, ox = where
                small = _lib.feature_net(img[n:n + 1, y0:y1, x0:x1].contiguous(), fb)
                same = torch.equal(small[0, :, oy:oy + 8, ox:ox + 8], feats[n, :, fy0:fy0 + 8, fx0:fx0 + 8])
                print("image %d window (%d, %d): error / bound %.3e, equals the small launch: %s" % (n, fy0, fx0, r, same))
                assert r <= 1.0 and same, (n, fy0, fx0, r, same)
                worst = max(worst, r)
        print("N=%d %dx%d: generate + feature_net %.1f s, windows %.1f s, worst ratio %.3e" % (
            N, H, W, t1 - t0, time.time() - t1, worst))
    finally:
        img = feats = small = None
        torch.cuda.empty_cache()


def test_just_inside_the_size_guard():
    """N = 1, 16384 x 16352 (the largest multiple-of-32 pair with H*W*8 < 2^31 and H != W; about 22 GiB of device memory
    with uint8 HWC input): the four corners, the last rows / columns and two interior windows of 8 x 8 feature pixels
    against the fp64 chain on the crop holding their receptive field, and bit-equal to a small launch on that crop.
    Wall time on the MI355X: see MEASURED_WALL below."""
    H, W = 16384, 16352
    assert H * W * 8 < 2 ** 31 <= H * (W + 32) * 8 and H % 32 == 0 and W % 32 == 0
    run_inside(1, H, W, images=(0,))


def test_just_inside_the_size_guard_many_images():
    """N = 51 at 2048 x 2560 (the largest N the guard admits): the LAST image holds the largest offsets"""
    run_inside(51, 2048, 2560, images=(50, 0))


MEASURED_WALL = None        # seconds on the MI355X, both inside cases; not recorded yet (run_inside prints them)


def test_at_the_size_guard_nothing_is_enqueued():
    lib = _lib.load()
    fb = _lib.pack_feature_weights(R.fstate(load_weights())).to(DEV)
    img = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), 123.25, dtype=torch.float32, device=DEV)
    s = _lib._stream(DEV)
    for N, H, W in ((1, 16384, 16384), (52, 2048, 2560), (1, 16384, 16352 + 32)):
        assert N * H * W * 8 >= 2 ** 31
        n = ctypes.c_size_t(77)
        assert lib.mvs_query_feature_workspace(N, H, W, ctypes.byref(n)) == 1 and n.value == 77      # MVS_ERR_BAD_SHAPE
        for fmt in (0, 1, 2):
            assert lib.mvs_feature_net_fmt(img.data_ptr(), fmt, fb.data_ptr(), out.data_ptr(), ws.data_ptr(), 1 << 40,
                                           N, H, W, s) == 1
            assert lib.mvs_feature_conv01_fmt(img.data_ptr(), fmt, out.data_ptr(), fb.data_ptr(), N, H, W, s) == 1
        for layer in range(8):
            assert lib.mvs_feature_layer(layer, img.data_ptr(), out.data_ptr(), fb.data_ptr(), N, H, W, s) == 1
        assert b"31-bit" in lib.mvs_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 123.25).all()) and bool((ws == 0).all())
