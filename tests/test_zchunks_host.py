"""The restated launch-geometry searches of tests/zchunks.py on known values, and the reach of their case categories
(no GPU needed; tests/test_gpu_zchunks.py runs the cases)."""
import pytest

import zchunks

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
