"""conv0's default fp32 kernel (conv0_w48t: persistent producer / consumer blocks on a 4 (z) x 8 (y) x 32 (x) tile,
conv0_split.hip) at shapes that reach every edge of its tile, against the CPU oracle with the per-layer bounds of
test_gpu_fullsize.py::test_cfg2_every_layer_matches_oracle[0]: H not a multiple of 8, W not a multiple of 32, D = 4 / 8 /
48, and tile counts below the CU count (one tile per block) and above it (blocks loop over 2-3 or 5-6 tiles, with and
without the XCD-banded tile order).  Plus the heavy-tailed non-negative volume of
test_winograd_layers_on_a_heavy_tailed_nonnegative_volume[0] at a ragged shape."""
import numpy as np
import pytest
import torch

from conftest import rel_l1
from oracle import oracle as orc
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER_ATOL = 2e-4   # x max|want|, as test_cfg2_every_layer_matches_oracle


@pytest.fixture(scope="module")
def state():
    sd = synthetic.random_costreg_state(seed=0)
    return sd, _lib.pack_weights(sd).to(DEV)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run_conv0(x, blob):
    return _lib.from_c8(_lib.conv_layer(0, _lib.to_c8(cu(x)), None, blob)).cpu().numpy()


# (D, H, W): tiles z x y x x = nb against 256 CUs
@pytest.mark.parametrize("shape", [
    (4, 12, 40),     # 1 x 2 x 2 = 4 tiles, ragged y and x, one z tile
    (8, 20, 200),    # 2 x 3 x 7 = 42, the DTU eval width
    (48, 12, 40),    # 12 x 2 x 2 = 48
    (48, 20, 200),   # 12 x 3 x 7 = 252: one tile per block
    (48, 64, 200),   # 12 x 8 x 7 = 672: XCD-banded order, 2-3 tiles per block
    (48, 144, 200),  # 12 x 18 x 7 = 1512: plain order, 5-6 tiles per block
])
def test_conv0_tile_edges_match_oracle(state, shape):
    sd, blob = state
    D, H, W = shape
    g = np.random.default_rng(D * 1000 + H * 10 + W)
    x = np.abs(g.standard_normal((32, D, H, W))).astype(np.float32)   # non-negative, as a variance volume
    want = orc.conv3d(x, sd["conv0.conv.weight"], bn=orc._bn(sd, "conv0.bn"))
    got = run_conv0(x, blob)
    np.testing.assert_allclose(got, want, rtol=0, atol=LAYER_ATOL * max(float(np.abs(want).max()), 1.0))
    assert rel_l1(got, want) < 2e-6, rel_l1(got, want)


def test_conv0_heavy_tailed_volume_at_a_ragged_shape(state):
    sd, blob = state
    g = np.random.default_rng(78)
    x = np.exp(3.0 * g.standard_normal((32, 48, 20, 200))).astype(np.float32)
    assert x.max() / np.median(x) > 1e4
    want = orc.conv3d(x, sd["conv0.conv.weight"], bn=orc._bn(sd, "conv0.bn"))
    got = run_conv0(x, blob)
    m = torch.from_numpy(x.max(axis=0))[None, None]
    m = torch.nn.functional.max_pool3d(m, kernel_size=(9, 3, 3), stride=1, padding=(4, 1, 1))[0, 0].numpy()
    gamma, beta, mean, var_ = orc._bn(sd, "conv0.bn")
    wmass = np.abs(sd["conv0.conv.weight"]).reshape(want.shape[0], -1).sum(1) * np.abs(gamma) / np.sqrt(var_ + 1e-5)
    worst = float((np.abs(got - want) / (2.5e-7 * wmass[:, None, None, None] * m[None] + 1e-6)).max())
    assert worst <= 1.0, worst
    assert rel_l1(got, want) < 5e-6
