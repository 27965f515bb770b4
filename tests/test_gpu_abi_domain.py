"""The smallest volumes include/mvs_abi.h admits, through the entry points themselves, against the fp64 references and
bounds that exist (softargmin_ref, warp_ref, featnet_ref; no new tolerance except the depth regression's fmaf chain).
These are the zero-trip loops and all-padding tiles: D below the soft-argmin's depth slices, one pixel, a last block
with one live lane, 2 x 2 maps, images smaller than one MFMA tile.  Every launch runs inside a guarded arena under the
three poisons (tests/guarded.py): an overrun lands in a guard band, an element nobody wrote shows as a difference.
Default kernel-selection environment; the conv layers' smallest volumes run in probe_check.py's children."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import featnet_ref as F  # noqa: E402
import guarded as G  # noqa: E402
import softargmin_ref as R  # noqa: E402
import warp_ref as W  # noqa: E402
from conftest import load_weights  # noqa: E402
from featnet_check import as_format, from_c8, to_c8  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def arena():
    return G.Arena(48 << 20, DEV)


def f32(raw, shape):
    return raw.view(torch.float32).numpy().reshape(shape)


# ---- mvs_softargmin_conf ---------------------------------------------------------------------------------------------
SOFTARGMIN = [(D, (1, hw)) for D in (1, 2, 3, 4, 5) for hw in (1, 15, 16, 17)] + \
             [(D, hw) for D in (1, 3, 7, 9) for hw in ((128, 128), (127, 129))] + [(1, (1, 129 * 127 + 2))]


def test_softargmin_shapes_sit_on_both_sides_of_the_dispatch():
    forms = {R.launch_form(D, h * w)[0] for D, (h, w) in SOFTARGMIN}
    assert forms == {"<8,16,16>", "<16,32,8>"}
    assert R.launch_form(9, 128 * 128)[1] == 32 and R.launch_form(9, 127 * 129)[1] == 16     # 16384 / 16383 pixels
    assert R.launch_form(1, 16385)[1] == 32 and 16385 % 32 == 1                              # one live lane in the last block


@pytest.mark.parametrize("D", sorted({D for D, _ in SOFTARGMIN}))
def test_softargmin_below_its_depth_slices(arena, D):
    worst = dict(depth=0.0, conf=0.0)
    for k, (_, (h, w)) in enumerate(c for c in SOFTARGMIN if c[0] == D):
        cost = R.logits("iid2", D, h * w, seed=10 * D + k)
        dv = synthetic.depth_values(D)

        def run(A):
            c, d = A.put(cu(cost).view(D, h, w), "in", "cost"), A.put(cu(dv), "in", "depth_values")
            with A.intercept(_lib):
                return _lib.softargmin_conf(c, d)
        (depth, conf), _ = G.same_under_all_poisons(arena, run)
        depth, conf = f32(depth, h * w), f32(conf, h * w)
        if D == 1:      # softmax of one logit is 1: the expectation is the depth value itself
            assert np.array_equal(depth, np.full(h * w, dv[0], np.float32)) and np.array_equal(conf, np.ones(h * w, np.float32))
        rd, rc, problems = R.check_forward(depth, conf, R.reference(cost, dv))
        print("softargmin D=%d %dx%d form %s: depth %.4f conf %.4f" % (D, h, w, R.launch_form(D, h * w)[0], rd, rc))
        assert not problems, problems
        worst = dict(depth=max(worst["depth"], rd), conf=max(worst["conf"], rc))
    print("WORST mvs_softargmin_conf D=%d: depth %.4f conf %.4f" % (D, worst["depth"], worst["conf"]))


# ---- mvs_depth_regression --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
def test_depth_regression_within_the_fmaf_chain_bound(arena, D):
    """depth = D fmafs from 0: any order of D fused multiply-adds errs by at most (D + 1) u sum |p dv| (assert_within of
    test_gpu_train_conv.py)."""
    worst = 0.0
    for hw in (1, 255, 256, 257):
        rng = np.random.default_rng(100 * D + hw)
        p = rng.random((D, hw), dtype=np.float32)
        dv = synthetic.depth_values(D)

        def run(A):
            pt, d = A.put(cu(p).view(D, 1, hw), "in", "p"), A.put(cu(dv), "in", "depth_values")
            out = A.carve((1, hw), torch.float32, "out", "depth")
            _lib.check(_lib.load().mvs_depth_regression(pt.data_ptr(), d.data_ptr(), out.data_ptr(), D, 1, hw,
                                                        _lib._stream(DEV)))
            return out
        (depth,), _ = G.same_under_all_poisons(arena, run)
        ref = (p.astype(np.float64) * dv.astype(np.float64)[:, None]).sum(0)
        bound = (D + 1) * U * np.abs(p.astype(np.float64) * dv.astype(np.float64)[:, None]).sum(0)
        r = float((np.abs(f32(depth, hw) - ref) / bound).max())
        print("depth_regression D=%d hw=%d: error / bound %.4f" % (D, hw, r))
        assert r <= 1.0
        worst = max(worst, r)
    print("WORST mvs_depth_regression D=%d: %.4f" % (D, worst))


# ---- mvs_relative_proj and mvs_homo_warp -----------------------------------------------------------------------------
def test_relative_proj_of_one_view_enqueues_nothing(arena):
    arena.reset()
    proj = arena.put(cu(synthetic.cameras(1, 8, 8)), "in", "proj")
    rt = arena.put(torch.full((1, 12), 123.25, device=DEV), "in", "rt_out")
    assert _lib.load().mvs_relative_proj(proj.data_ptr(), rt.data_ptr(), 1, _lib._stream(DEV)) == 0
    assert arena.check() == []


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (3, 2, 2, 5), (2, 3, 5, 2)])
def test_homo_warp_on_the_smallest_maps(arena, shape):
    Cn, D, h, w = shape
    fea = synthetic.random_features(1, Cn, h, w, seed=41)[0]
    proj = W.rig(h, w, [(np.eye(3), np.array([-30.0, 5.0, 0.0]))])
    dv = synthetic.depth_values(D)

    def run(A):
        f, p, d = A.put(cu(fea), "in", "src_fea"), A.put(cu(proj), "in", "proj"), A.put(cu(dv), "in", "depth_values")
        out = A.carve((Cn, D, h, w), torch.float32, "out", "warped")
        with A.intercept(_lib):
            rt = _lib.relative_proj(p)
        _lib.check(_lib.load().mvs_homo_warp(f.data_ptr(), rt.data_ptr(), d.data_ptr(), out.data_ptr(), Cn, D, h, w,
                                             _lib._stream(DEV)))
        return rt, out
    (rt, out), _ = G.same_under_all_poisons(arena, run)
    rt = f32(rt, (1, 12))
    want, bnd = W.relative_proj64(proj), W.relative_proj_bound(proj)
    with np.errstate(invalid="ignore", divide="ignore"):      # an entry whose bound is 0 is an exact zero
        rp = float(np.where(bnd > 0, np.abs(rt.astype(np.float64) - want) / bnd, np.where(rt == want, 0.0, np.inf)).max())
    wv, e, lo, na = W.warp_bound(fea, rt[0], dv)
    ratio, problems = W.compare(f32(out, shape), dict(var=wv, bound=e, loose=lo, nan=na))
    print("WORST mvs_homo_warp %s: %.4f (relative_proj N=2: %.4f; %.0f %% of the voxels bounded, %d nonzero)"
          % (shape, ratio, rp, 100 * (1 - (lo | na).mean()), int((wv != 0).sum())))
    assert rp <= 1.0 and not problems, (rp, problems)
    assert not (lo | na).any() and (wv != 0).any()      # the case checks values, not only zeros outside the image


# ---- mvs_feature_layer and mvs_feature_net_fmt -----------------------------------------------------------------------
IMAGES = [(N, H, Wd) for N in (1, 2) for H, Wd in ((4, 4), (4, 7), (7, 4), (5, 5))]


@pytest.fixture(scope="module")
def featnet():
    st = F.fstate(load_weights())
    return st, _lib.pack_feature_weights(st).to(DEV)


@pytest.mark.parametrize("layer", range(8))
def test_feature_layer_on_images_smaller_than_a_tile(arena, featnet, layer):
    st, fb = featnet
    worst = 0.0
    for k, (N, H, Wd) in enumerate(IMAGES):
        assert Wd < F.tile(layer)[1]                 # one ragged tile column; one or two tile rows
        x = F.make_input(layer, "normal", N, H, Wd, seed=300 + 10 * layer + k)

        def run(A):
            xt = A.put(cu(x) if layer == 0 else to_c8(cu(x)), "in", "x")
            b = A.put(fb, "in", "feature_blob")
            with A.intercept(_lib):
                return _lib.feature_layer(layer, xt, b)
        ci, co, _, s = F.LAYERS[layer]
        oshape = (co // 8, N, F.out_size(H, s), F.out_size(Wd, s), 8)
        (y,), _ = G.same_under_all_poisons(arena, run)
        got = from_c8(torch.from_numpy(f32(y, oshape))).numpy()
        ref, bound = F.dense_ref_bound(st, layer, x)
        r = F.ratio(got, ref, bound)
        print("feature layer %d N=%d %dx%d: error / bound %.4f" % (layer, N, H, Wd, r))
        assert r <= 1.0
        worst = max(worst, r)
    print("WORST mvs_feature_layer %d: %.4f" % (layer, worst))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_feature_net_on_images_smaller_than_a_tile(arena, featnet, fmt):
    st, fb = featnet
    worst = 0.0
    for k, (N, H, Wd) in enumerate(IMAGES):
        u8 = F.make_input(F.FUSED, "u8", N, H, Wd, seed=400 + k)
        img = as_format(u8, fmt)

        def run(A):
            i, b = A.put(cu(img), "in", "imgs"), A.put(fb, "in", "feature_blob")
            with A.intercept(_lib):
                return _lib.feature_net(i, b)
        h4, w4 = F.out_size(F.out_size(H, 2), 2), F.out_size(F.out_size(Wd, 2), 2)
        (y,), _ = G.same_under_all_poisons(arena, run)
        ref, E = F.chain_ref_bound(st, F.u8_to_f32(u8), consts={0: F.FUSED_C0})
        r = F.ratio(f32(y, (N, 32, h4, w4)), ref, E)
        print("feature_net %s N=%d %dx%d -> %dx%d: error / bound %.3e" % (fmt, N, H, Wd, h4, w4, r))
        assert r <= 1.0
        worst = max(worst, r)
    print("WORST mvs_feature_net_fmt %s: %.3e" % (fmt, worst))
