"""tests/featnet_ref.py checked without a GPU: the fp64 chain reproduces the reference (captured fixtures and the C oracle)
within the chained bound, the probes are what they claim to be, an fp32 numpy restatement of the kernels' MFMA order
lies within the dense bound, and every mutation of that restatement is CAUGHT by the probe family that exists for it
(the library itself is never built or run in a broken form):
    one dropped tap            -> lattice probes              swapped channel halves (g & 1) * 4 -> lattice probes
    ReLU(shift0) in the fused kernel's padding ring           -> crafted probe, variant "shift"
    a residue in the padded panel slots                       -> padded-tap probe
    the tap with the least weight mass dropped                -> dense bound, standard-normal input
Also the C-ABI refusals of mvs_feature_conv01_fmt (tests/refusals.py makes the calls in a child that sees no device).

Worst |reference fp32 - fp64 chain| / chained bound over the fixtures and the ragged oracle case: 5.5e-8 (printed by
test_fp64_chain_reproduces_the_reference; recorded as featnet_ref.REFERENCE_WORST).
"""
import os
import re
import sys

import numpy as np
import pytest

import featnet_ref as R
import probes
import refusals
from conftest import REPO, load_fixture, load_weights
from oracle import oracle as orc
from refusals import BAD_DTYPE, BAD_SHAPE, NULL
from scene_3dreconstruction_mvsnet_amd import _lib

ST = R.fstate(load_weights())


def test_constants_match_the_library_and_the_conv_probes():
    assert R.LAYERS == tuple(_lib.FEATURE_LAYERS)
    assert R.PROBE_ULPS == probes.PROBE_ULPS and R.DENSE_C <= min(R.analytic_k(l) for l in range(8))
    assert [R.analytic_k(l) for l in range(8)] == [80, 80, 208, 160, 160, 416, 320, 320]
    src = open(os.path.join(REPO, "scene_3dreconstruction_mvsnet_amd", "csrc", "featnet.hip")).read()
    inst = re.findall(r"case (\d): return run_fconv<(\d+), (\d+), (\d), (\d), (\d), (\d), (true|false), (true|false)>", src)
    seen = {}
    for l, ci, co, k, s, by, bx, relu, _ in inst:
        seen[int(l)] = ((int(ci), int(co), int(k), int(s)), (int(by), int(bx)), relu == "true")
    seen[3] = seen[4]                      # `case 3:` falls through to case 4
    assert sorted(seen) == list(range(8))
    for l in range(8):
        assert seen[l] == (R.LAYERS[l], R.BLOCK[l], l != 7), l
    assert "using G = FConv<8, 8, 3, 1, 4, 4>;" in src and R.tile(R.FUSED) == (8, 32)
    assert R.receptive_field() == (41, 4)


def test_fp64_chain_reproduces_the_reference():
    """the chained bound applied to the REFERENCE's own fp32 output: it must be wide enough for a correct fp32 net"""
    worst = 0.0
    for name in ("tiny", "small", "n5yaw", "b2"):
        fx = load_fixture(name)
        for b in range(fx["imgs"].shape[0]):
            ref, E = R.chain_ref_bound(ST, fx["imgs"][b])
            worst = max(worst, R.ratio(fx["features"][b], ref, E))
            # and plainly: the fp64 chain is the reference's function (fp32 noise of eight layers)
            np.testing.assert_allclose(fx["features"][b], ref, rtol=1e-4, atol=3e-6)
    imgs = np.random.default_rng(5).random((2, 3, 50, 70), dtype=np.float32)
    ref, E = R.chain_ref_bound(ST, imgs)
    want = np.stack([orc.feature_net(imgs[n], load_weights()) for n in range(2)])
    assert want.shape == ref.shape == (2, 32, 13, 18)
    worst = max(worst, R.ratio(want, ref, E))
    print("reference fp32 / chained bound: worst ratio %.3e" % worst)
    assert worst < 1.0
    assert R.REFERENCE_WORST is not None and worst <= 2 * R.REFERENCE_WORST


@pytest.mark.parametrize("layer", range(8))
def test_single_layer_oracle_lies_within_the_dense_bound(layer):
    """the C oracle's fp32 layer (unfolded BatchNorm, its own summation order) against the dense bound"""
    N, H, W = R.PROBE_SHAPE[layer]
    for fam in R.families(layer):
        x = R.make_input(layer, fam, 1, H, W, seed=layer)
        x = R.u8_to_f32(x) if fam == "u8" else x
        w, bn, bias = R.raw(ST, layer)
        got = orc.conv2d(x[0], w, bias=bias, bn=bn, stride=R.LAYERS[layer][3], relu=layer != 7)[None]
        ref, bound = R.dense_ref_bound(ST, layer, x)
        assert R.ratio(got, ref, bound) <= 1.0, (layer, fam)


def test_cases_walk_every_tile_edge_and_every_workgroup_residue():
    for kern, cases in R.CASES.items():
        s = 1 if kern == R.FUSED else R.LAYERS[kern][3]
        th, tw = R.tile(kern)
        tots = [R.workgroups(kern, *c) for c in cases]
        assert {t % 8 for t in tots if t >= 8} == set(range(8)) and any(t < 8 for t in tots), kern
        assert {c[0] for c in cases} == {1, 2, 5}
        for dim, t in ((1, th), (2, tw)):
            ins = {c[dim] for c in cases}
            outs = {R.out_size(v, s) for v in ins}
            assert min(ins) == 4 and {max(t - 1, R.out_size(4, s)), t, t + 1, 2 * t + 3} <= outs, (kern, dim, outs)
            if s == 2:
                assert {v % 2 for v in ins} == {0, 1}
        assert all(c[1] >= 4 and c[2] >= 4 for c in cases)


@pytest.mark.parametrize("layer", range(8))
def test_lattice_phases_are_single_product_and_cover_everything(layer):
    N, H, W = shape = R.PROBE_SHAPE[layer]
    ci_n, co_n, k, s = R.LAYERS[layer]
    rng = np.random.default_rng(layer)
    wf = fold32 = R.fold32(ST, layer)[0]
    assert (wf != 0).all()
    touched = np.zeros((N, H, W), bool)
    pairs = np.zeros((ci_n, k * k), bool)
    p = k // 2
    Ho, Wo = R.out_size(H, s), R.out_size(W, s)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for ph in R.phases(layer):
        x = R.lattice(layer, shape, ph, rng)
        nz = (x != 0).astype(np.float64)
        count = R.conv64(nz, np.ones_like(fold32, np.float64), s)     # nonzero products per output, in integers
        assert count.max() == 1.0 and (nz.sum(1) <= 1).all()
        touched |= nz.any(1)
        for tap in range(k * k):          # pixel (y, x) meets tap (ky, kx) in output ((y + p - ky) / s, (x + p - kx) / s)
            ky, kx = divmod(tap, k)
            oy, ox = ys + p - ky, xs + p - kx
            hit = (oy % s == 0) & (oy >= 0) & (oy // s < Ho) & (ox % s == 0) & (ox >= 0) & (ox // s < Wo)
            pairs[:, tap] |= (nz.astype(bool) & hit[None, None]).any((0, 2, 3))
    assert touched.all() and pairs.all()


def test_crafted_conv0_is_a_bit_exact_copy():
    rng = np.random.default_rng(3)
    u8 = R.crafted_image(R.PROBE_SHAPE[R.FUSED], rng)
    img = R.u8_to_f32(u8)
    assert (u8 > 0).all() and np.array_equal(img, (u8.astype(np.float64) / 255).astype(np.float32))
    for variant in ("copy", "shift"):
        st, conv0_exact = R.crafted_state(ST, 4, variant, rng)
        w0, s0, _ = R.fold32(st, 0)
        assert (w0 != 0).sum() == 8 and set(np.unique(w0)) == {0.0, 1.0}
        assert (s0 == (R.CRAFTED_SHIFT0 if variant == "shift" else 0)).all()
        c0 = conv0_exact(img)
        got = R.emulate_layer(st, 0, img)                     # the MFMA-order kernel of MVS_FEAT_SPLIT01
        assert np.array_equal(got, c0)
        if variant == "copy":
            assert np.array_equal(c0, img[:, [0, 1, 2, 0, 1, 2, 0, 1]])
        w1 = R.fold32(st, 1)[0]
        assert ((w1 != 0).reshape(8, -1).sum(1) == 1).all() and (w1 >= 0).all()
    seen = set()
    for run in range(R.CRAFTED_RUNS):
        w1 = R.fold32(R.crafted_state(ST, run, "copy", rng)[0], 1)[0]
        seen |= {(int(c), int(ky) * 3 + int(kx)) for _, c, ky, kx in zip(*np.nonzero(w1))}
    assert len(seen) == 72


def _probe_ratio(layer, st, x, mutation=None):
    want, bound = R.probe_want_bound(st, layer, x)
    return R.ratio(R.emulate_layer(st, layer, x, mutation), want, bound)


@pytest.mark.parametrize("layer", range(8))
def test_emulation_passes_probes_and_dense_bound_and_mutations_are_caught(layer):
    shape = R.PROBE_SHAPE[layer]
    ci_n, co_n, k, s = R.LAYERS[layer]
    rng = np.random.default_rng(100 + layer)
    taps = k * k
    drop = ("drop_tap", int(rng.integers(0, taps)))
    ok, dropped, swapped = 0.0, 0.0, 0.0
    for i, ph in enumerate(R.phases(layer)):
        x = R.lattice(layer, shape, ph, rng)
        ok = max(ok, _probe_ratio(layer, ST, x))
        if i % 4:                                              # every phase meets every tap and both halves: a few suffice
            continue
        dropped = max(dropped, _probe_ratio(layer, ST, x, drop))
        if layer:                                              # conv0's only chunk has no second half to swap with
            swapped = max(swapped, _probe_ratio(layer, ST, x, ("swap_halves",)))
    assert ok <= 1.0
    assert dropped > 1.0 and (swapped > 1.0 or layer == 0)
    # padded tap: magnitudes 2^100 x 2^-100; a residue of one fp32 denormal-sized weight in the padded slots shows
    stp = R.padded_tap_state(ST, layer, rng)
    x = R.lattice(layer, shape, (1, 2), rng, magnitude=100)
    assert _probe_ratio(layer, stp, x) <= 1.0
    assert _probe_ratio(layer, stp, x, ("residue", np.float32(2.0 ** -120))) > 1.0
    # dense: every family within the bound; the tap with the least weight mass dropped is not (standard normal)
    wf = R.fold32(ST, layer)[0]
    least = ("drop_tap", int(np.abs(wf).reshape(co_n, ci_n, taps).sum((0, 1)).argmin()))
    for fam in R.families(layer):
        x = R.make_input(layer, fam, *shape, seed=layer)
        x = R.u8_to_f32(x) if fam == "u8" else x
        ref, bound = R.dense_ref_bound(ST, layer, x)
        r = R.ratio(R.emulate_layer(ST, layer, x), ref, bound)
        assert r <= 1.0, (fam, r)
        if fam == "normal":
            assert R.ratio(R.emulate_layer(ST, layer, x, least), ref, bound) > 1.0


def test_fused_emulation_passes_and_the_relu_shift_ring_is_caught():
    shape = R.PROBE_SHAPE[R.FUSED]
    rng = np.random.default_rng(9)
    img = R.u8_to_f32(R.crafted_image(shape, rng))
    for variant in ("copy", "shift"):
        for run in (0, 4, 8):
            st, conv0_exact = R.crafted_state(ST, run, variant, rng)
            want, bound = R.crafted_want_bound(st, img, conv0_exact)
            assert R.ratio(R.emulate_fused(st, img), want, bound) <= 1.0
            ring = R.ratio(R.emulate_fused(st, img, ("ring",)), want, bound)
            # with shift0 = 0 the ring mutation is invisible: that is why the "shift" variant exists
            assert (ring > 1.0) == (variant == "shift"), (variant, run, ring)
    for fam in R.families(R.FUSED):
        x = R.make_input(R.FUSED, fam, *shape, seed=11)
        x = R.u8_to_f32(x) if fam == "u8" else x
        ref, E = R.fused_ref_bound(ST, x)
        assert R.ratio(R.emulate_fused(ST, x), ref, E) <= 1.0, fam
        if fam == "unit":       # the seed-0 shift0 is positive in some channel: the ring mutation breaks the dense bound too
            assert R.ratio(R.emulate_fused(ST, x, ("ring",)), ref, E) > 1.0


# ---- the C ABI refuses bad arguments and enqueues nothing ------------------------------------------------------------
# every refusal of mvs_feature_conv01_fmt, run by tests/refusals.py in a child that sees no device; the tests look their
# record up
NULLS = dict(imgs="imgs", y="y", blob="feature_blob")
FORMATS = [-1, 3]
BAD_SHAPES = [dict(H=3), dict(W=3), dict(N=0), dict(N=65536, H=4, W=4), dict(N=1, H=16384, W=16384), dict(N=52, H=2048, W=2560),
              dict(N=2, H=16384, W=8192)]
REFUSALS = {"mvs_feature_conv01_fmt": dict(
    good=dict(N=2, H=32, W=32, image_format=0),
    cases=refusals.cases(*[({p: None}, NULL, "NULL") for p in NULLS.values()],
                         *[(dict(image_format=f), BAD_DTYPE, "") for f in FORMATS], *[(bad, BAD_SHAPE, "") for bad in BAD_SHAPES]))}


def _refused(**ov):
    return refusals.expect(sys.modules[__name__], "mvs_feature_conv01_fmt", ov)


@pytest.mark.parametrize("null", list(NULLS))
def test_conv01_refuses_null(null):
    assert _refused(**{NULLS[null]: None}) == NULL


@pytest.mark.parametrize("fmt", FORMATS)
def test_conv01_refuses_unknown_format(fmt):
    assert _refused(image_format=fmt) == BAD_DTYPE


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_conv01_refuses_bad_shape(shape):
    assert _refused(**shape) == BAD_SHAPE
    assert "mvs_feature_conv01_fmt" in _lib.SYMBOLS
