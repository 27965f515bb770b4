"""CPU side of the non-finite contract of FeatureNet and the training kernels (tests/nonfinite_train_ref.py,
tests/nonfinite_train_check.py, tests/test_gpu_nonfinite_train.py): the checker passes the fp32 emulations of the
kernels on every case, reports each named defect, the derived spread sets are the fp64 references' own non-finite sets,
and every kernel-level case holds at least half of its outputs bit-equal (the coverage condition)."""
import numpy as np
import pytest
import torch

import bn3d_ref as BR
import featnet_ref as FR
import nonfinite_train_ref as T
import softargmin_ref as SR
from conftest import load_weights

ST = FR.fstate(load_weights())


def emulate_feat(kernel, x, mutation=None):
    with np.errstate(all="ignore"):
        return FR.emulate_fused(ST, x, mutation) if kernel == FR.FUSED else FR.emulate_layer(ST, kernel, x, mutation)


def feat_failures(kernel, rot, mutation=None):
    c = T.feat_case(ST, kernel, rot)
    return T.check_case(c, {"y": emulate_feat(kernel, c["x"], mutation)}, {"y": emulate_feat(kernel, c["base"])})


# ---------------------------------------------------------------------------------------------------------------
# FeatureNet
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", FR.KERNELS)
def test_featnet_emulation_meets_the_contract(kernel):
    for rot in range(T.ROTATIONS):
        assert not feat_failures(kernel, rot), (kernel, rot)


@pytest.mark.parametrize("kernel", FR.KERNELS)
def test_relu_that_drops_nan_is_reported(kernel):
    """fmaxf(NaN, 0) = 0: the parent commit's FeatureNet.  The last layer has no ReLU and nothing to report."""
    fails = [f for rot in range(T.ROTATIONS) for f in feat_failures(kernel, rot, ("relu_drops_nan",))]
    if kernel == 7:
        assert not fails
    else:
        assert any("R1 a finite value hides" in f for f in fails), fails[:3]


@pytest.mark.parametrize("kernel", range(8))
def test_halo_masked_by_multiplication_is_reported(kernel):
    """the first pixel of the view is non-finite in every case: times 0 it is NaN in the whole out-of-image halo, and
    every border output leaves the spread set"""
    fails = feat_failures(kernel, 0, ("mask_by_multiply",))
    assert any("R2'" in f for f in fails), fails[:3]


def test_every_position_holds_every_value_once():
    for kernel in FR.KERNELS:
        seen = {}
        for rot in range(T.ROTATIONS):
            c = T.feat_case(ST, kernel, rot)
            for name, (y, x) in T.feat_positions(kernel):
                v = c["x"][0, :, y, x]
                bad = v[~np.isfinite(v)]
                assert bad.size == 1
                seen.setdefault(name, set()).add("nan" if np.isnan(bad[0]) else "+inf" if bad[0] > 0 else "-inf")
            assert np.isfinite(c["x"][1]).all() and not c["spread"]["y"][1].any()      # view 1: clean, held whole
        assert all(v == {"nan", "+inf", "-inf"} for v in seen.values()), (kernel, seen)
        # both sides of a block-tile edge where the output has two block tiles, else of the 2 x 8 MFMA tile
        yb, xb = T.feat_boundaries(kernel)
        s = 1 if kernel == FR.FUSED else FR.LAYERS[kernel][3]
        assert yb % (2 * s) == 0 and xb % (8 * s) == 0 and 0 < yb < T.FEAT_SHAPE[1] and 0 < xb < T.FEAT_SHAPE[2]
        # the padded tap is walked: some injected pixel lies under the last tap (k - 1, k - 1) of an in-range output
        k = 3 if kernel == FR.FUSED else FR.LAYERS[kernel][2]
        assert any((y - k // 2) % s == 0 and (x - k // 2) % s == 0 and y >= k // 2 and x >= k // 2
                   for _, (y, x) in T.feat_positions(kernel)), kernel
    th, tw = FR.tile(FR.FUSED)
    assert T.FEAT_SHAPE[1] > 2 * th and T.FEAT_SHAPE[2] > tw        # at least two 8 x 32 tiles per axis, ragged
    for kernel in FR.KERNELS:
        s = 1 if kernel == FR.FUSED else FR.LAYERS[kernel][3]
        th, tw = FR.tile(kernel)
        # ragged in x for every block tile; in y for the 8-row tiles and the stride-2 layers (10 rows of 4-row tiles):
        # the 4-row tiles of the stride-1 layers 3, 4, 6, 7 divide the 20 rows
        assert FR.out_size(T.FEAT_SHAPE[2], s) % tw
        assert bool(FR.out_size(T.FEAT_SHAPE[1], s) % th) == (kernel not in (3, 4, 6, 7)), kernel


def test_whole_net_sets():
    """one corner pixel reaches at most 6 x 6 of the 24 x 32 features (receptive field 41, stride 4: feature f reads
    pixels 4 f - 20 .. 4 f + 20, which hold pixel 0 for f <= 5), and the fp64 chain makes exactly those NaN; a NaN
    weight or BatchNorm statistic makes every feature NaN"""
    rf, stride = FR.receptive_field()
    assert (rf, stride) == (41, 4)
    c = T.net_image_case(ST)
    sp = c["spread"]["y"]
    assert sp.shape == (2, 32, 24, 32) and sp[0, 0].sum() == 36 and sp[0, 0, :6, :6].all() and not sp[1].any()
    assert np.array_equal(np.isnan(c["ref"]["y"]), sp)
    assert T.coverage(c)["y"] >= T.MIN_OUTSIDE
    img = FR.make_input(0, "unit", 1, 32, 32, seed=1)
    for which in T.NET_WEIGHT_CASES:
        with np.errstate(all="ignore"):
            assert np.isnan(FR.chain64(T.nan_state(ST, which), img)).all(), which


def test_whole_net_with_a_relu_that_drops_nan_hides_a_nan_weight():
    """what the parent commit did: the NaN channel of conv3 (conv5) is 0 after fmaxf, and every feature is finite"""
    img = FR.make_input(0, "unit", 1, 32, 32, seed=1)
    for which in T.NET_WEIGHT_CASES:
        st = T.nan_state(ST, which)
        for mutation, hidden in ((("relu_drops_nan",), True), (None, False)):
            with np.errstate(all="ignore"):
                y = FR.emulate_fused(st, img, mutation)
                for l in range(2, 8):
                    y = FR.emulate_layer(st, l, y, mutation)
            assert np.isfinite(y).all() == hidden and np.isnan(y).all() != hidden, (which, mutation)


# ---------------------------------------------------------------------------------------------------------------
# training convolutions: no emulation; the derived sets against the fp64 reference, and the coverage condition
# ---------------------------------------------------------------------------------------------------------------
def test_conv_cases_are_those_of_the_gpu_test():
    assert len(T.CONV_CASES) == 11 + 6 and [c[0] for c in T.CONV_CASES[:11]] == ["layer%d" % l for l in range(11)]


@pytest.mark.parametrize("case", T.CONV_CASES, ids=lambda c: c[0])
def test_conv_spread_sets_are_the_references_own_and_half_is_held(case):
    for i, op in enumerate(T.CONV_OPS):
        c = T.conv_case(case, op, i % 3)
        for key, ref in c["ref"].items():
            # the derivation confirmed: fp64 conv3d / autograd on the CPU is non-finite on exactly the derived set
            assert np.array_equal(~np.isfinite(ref), c["spread"][key]), (c["name"], key)
        cov = T.coverage(c)
        held = min(v for k, v in cov.items() if k != "gb" or op == "wgrad_gy")
        if (case[0], op) in T.CONV_COVERAGE_EXEMPT:
            assert held < T.MIN_OUTSIDE, (c["name"], cov)       # exempt for a reason, not by default
        else:
            assert held >= T.MIN_OUTSIDE, (c["name"], cov)
        vals = c["inj"]["x" if op in ("forward", "wgrad_x") else "g"]
        bad = vals[~torch.isfinite(vals)]
        assert bad.numel() == len(c["positions"]) >= 1
        if len(c["positions"]) >= 3:
            assert bool(bad.isnan().any()) and bool((bad == np.inf).any()) and bool((bad == -np.inf).any())


def test_conv_positions_walk_the_tile_edges():
    """x = 15 | 16 of the 16-voxel tile and the last row of an MT y-group, in input coordinates of the forward"""
    pos = T.conv_positions((16, 26, 42), T.mt_of(16), 2)      # layer 1: stride 2, MT = 8
    assert (8, 14, 31) in pos and (8, 14, 32) in pos and (8, 15, 22) in pos and (8, 16, 22) in pos
    pos = T.conv_positions((12, 13, 41), T.mt_of(64), 1)      # NT = 4: MT = 4
    assert (6, 7, 15) in pos and (6, 7, 16) in pos and (6, 3, 21) in pos and (6, 4, 21) in pos
    assert pos[0] == (0, 0, 0) and pos[1] == (11, 12, 40)


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------
def bn_all():
    for C, M in T.BN_CASES:
        for i, row in enumerate(T.bn_rows(C, M)):
            for relu in (True, False):
                for skip in (True, False):
                    yield C, M, row, relu, skip, i % 3


def bn_failures(c, defects=()):
    got = T.bn_emulate(c["inj"]["y"], c["inj"]["p"], c["relu"], c["skip"], defects)
    clean = T.bn_emulate(c["clean"]["y"], c["clean"]["p"], c["relu"], c["skip"])
    return T.check_case(c, got, clean)


def test_bn_cases():
    assert set(BR.CASES) - {(16, 70001)} <= set(T.BN_CASES)
    assert any(M > BR.geometry(C, M)["RPB"] for C, M in T.BN_CASES)      # a boundary between two blocks is walked
    for C, M in T.BN_CASES:
        rows = T.bn_rows(C, M)
        assert rows["first"] == 0 and rows["last"] == M - 1
        geo = BR.geometry(C, M)
        if M > geo["RPB"]:
            assert geo["RPB"] - 1 in rows.values() and geo["RPB"] in rows.values()
        ch = T.bn_channels(C)
        assert len({ch["nan"], ch["pinf"], ch["ninf"], ch["go"]}) == 4 and max(ch.values()) < C


def test_bn_emulation_meets_the_contract_and_half_the_channels_are_held():
    n = 0
    for C, M, row, relu, skip, rot in bn_all():
        c = T.bn_case(C, M, row, relu, skip, rot)
        assert not bn_failures(c), c["name"]
        assert c["clean_channels"] >= T.MIN_OUTSIDE and min(T.coverage(c).values()) >= T.MIN_OUTSIDE, c["name"]
        n += 1
    assert n == 4 * sum(len(T.bn_rows(C, M)) for C, M in T.BN_CASES)


def test_bn_merge_that_mixes_channel_groups_is_reported():
    for C, M in T.BN_CASES:
        c = T.bn_case(C, M, "first", True, True)
        fails = bn_failures(c, ("nan_channel_leaks",))
        assert any("R2'" in f for f in fails), (C, M, fails[:3])


def test_bn_reference_mask_is_torchs_select():
    """a non-finite grad_out behind a closed ReLU is no gradient, and a NaN pre-activation passes it:
    F.relu's backward on the CPU says the same; bn3d_ref.reference multiplies by the mask"""
    y = np.array([[-1.0], [1.0], [2.0], [-2.0]], np.float32)
    p = dict(gamma=np.ones(1, np.float32), beta=np.zeros(1, np.float32), skip=None, rm=np.zeros(1, np.float32),
             rv=np.ones(1, np.float32), go=np.array([[np.nan], [1.0], [1.0], [np.inf]], np.float32))
    ref = T.bn_reference(y, p, True, False)
    assert ref["grad_beta"][0] == 2.0 and np.isfinite(ref["grad_y"]).all()
    with np.errstate(all="ignore"):
        old = BR.reference(y.astype(np.float64), np.ones(1), np.zeros(1), go=p["go"].astype(np.float64))
    assert np.isnan(old["grad_beta"][0])
    x = torch.tensor([np.nan, -1.0, 2.0], requires_grad=True)
    torch.relu(x).backward(torch.tensor([3.0, np.nan, 5.0]))
    assert x.grad.tolist() == [3.0, 0.0, 5.0]
    yn = y.copy()
    yn[0, 0] = np.nan                       # the channel is lost: every pre-activation is NaN, every grad_out passes
    pn = dict(p, go=np.array([[1.0], [2.0], [3.0], [4.0]], np.float32))
    assert T.bn_reference(yn, pn, True, False)["grad_beta"][0] == 10.0


def test_bn_mask_that_closes_on_nan_is_reported():
    """the kernels' mask before these tests, `pre > 0`: grad_beta of a lost channel is 0 where the reference sums a
    non-finite grad_out"""
    c = T.bn_case(8, 1001, "first", True, True)
    ch = T.bn_channels(8)
    inj = dict(c["inj"]["p"])
    inj["go"] = inj["go"].copy()
    inj["go"][5, ch["nan"]] = np.nan
    c["ref"] = T.bn_reference(c["inj"]["y"], inj, True, True)
    got = T.bn_emulate(c["inj"]["y"], inj, True, True)
    assert np.isnan(got["grad_beta"][ch["nan"]]) and np.isnan(c["ref"]["grad_beta"][ch["nan"]])
    closed = dict(got, grad_beta=np.where(np.isnan(got["mean"]), np.float32(0), got["grad_beta"]))
    clean = T.bn_emulate(c["clean"]["y"], c["clean"]["p"], True, True)
    assert not T.check_case(c, got, clean)
    assert any("hides" in f for f in T.check_case(c, closed, clean))


# ---------------------------------------------------------------------------------------------------------------
# soft-argmin backward
# ---------------------------------------------------------------------------------------------------------------
def sa_failures(c, defect=None):
    got = SR.emulate_backward(c["inj"]["cost"], c["inj"]["dv"], c["inj"]["gd"], defect=defect)
    clean = SR.emulate_backward(c["clean"]["cost"], c["clean"]["dv"], c["clean"]["gd"])
    return T.check_case(c, {"gc": got}, {"gc": clean})


@pytest.mark.parametrize("D", T.SOFTARGMIN_D)
def test_softargmin_backward_emulation_meets_the_contract(D):
    for P_ in T.SOFTARGMIN_P:
        kinds = set()
        for rot in range(len(T.SOFTARGMIN_KINDS)):
            c = T.softargmin_case(D, P_, rot)
            assert not sa_failures(c), c["name"]
            # P = 1 has no second pixel to hold: exempt from the coverage condition, and the only such case
            assert (T.coverage(c)["gc"] >= T.MIN_OUTSIDE) == (P_ > 1), c["name"]
            ref = c["ref"]["gc"]
            for q in T.softargmin_pixels(P_):
                assert q in c["single"] or np.isnan(ref[:, q]).all() or not np.isfinite(ref[:, q]).any(), (c["name"], q)
            for q in c["single"]:
                assert np.isfinite(ref[:, q]).all() and (ref[np.isneginf(c["inj"]["cost"][:, q]), q] == 0).all()
            kinds |= {T.SOFTARGMIN_KINDS[(k + rot) % 7] for k in range(len(T.softargmin_pixels(P_)))}
        assert kinds == set(T.SOFTARGMIN_KINDS)
    assert {127, 128} <= set(T.softargmin_pixels(129)) and {127, 128, 255, 256, 0, 299} <= set(T.softargmin_pixels(300))


def test_minus_inf_term_that_becomes_nan_is_reported():
    hits = 0
    for D in (2, 9, 48):
        for rot in range(len(T.SOFTARGMIN_KINDS)):
            c = T.softargmin_case(D, 300, rot)
            first = [q for q in c["single"] if np.isneginf(c["inj"]["cost"][0, q])]
            fails = sa_failures(c, "minus_inf_term_nan")
            assert bool(first) == any("keeps the value finite" in f for f in fails), (c["name"], fails[:2])
            hits += bool(first)
    assert hits >= 6


# ---------------------------------------------------------------------------------------------------------------
# the checker itself
# ---------------------------------------------------------------------------------------------------------------
def test_checker_rules_one_by_one():
    clean = np.arange(8, dtype=np.float32)
    ref = clean.astype(np.float64).copy()
    ref[2] = np.nan
    spread = np.zeros(8, bool)
    spread[2:4] = True
    got = clean.copy()
    got[2] = np.nan
    assert not T.check("t", got, clean, ref, spread)
    assert "hides" in T.check("t", clean, clean, ref, spread)[0]
    g = got.copy()
    g[2] = np.inf
    assert "infinity" in T.check("t", g, clean, ref, spread)[0]
    g = got.copy()
    g[5] = np.nextafter(g[5], np.float32(9))
    assert "R2'" in T.check("t", g, clean, ref, spread)[0]           # one ulp outside the spread set
    g = got.copy()
    g[3] = np.nan
    assert not T.check("t", g, clean, ref, spread)                   # inside it: allowed
    assert "keeps the value finite" in T.check("t", g, clean, ref, spread, finite=spread)[0]
    g[3] = 3.5
    assert "not the clean launch's bytes" in T.check("t", g, clean, ref, spread)[0]
    assert not T.check("t", g, clean, ref, spread, bound=np.full(8, 0.5))
    assert "beyond the fp64 bound" in T.check("t", g, clean, ref, spread, bound=np.full(8, 0.25))[0]
    r = ref.copy()
    r[6] = np.inf
    assert "outside the derived spread set" in T.check("t", got, clean, r, spread)[0]
    z = got.copy()
    z[0] = -0.0
    assert "R2'" in T.check("t", z, clean, ref, spread)[0]           # a signed zero: bytes, not values
