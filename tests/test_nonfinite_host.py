"""CPU side of the non-finite contract (tests/nonfinite_ref.py, tests/nonfinite_check.py, test_gpu_nonfinite.py): the
references keep NaN, the C oracle meets R1 - R3 with zero extents on every pattern, the finite-share conditions of the
chain hold for the oracle alone and for the derived extents, every kernel form has an extent -- and the checker reports
each of a list of plausible defects, emulated in numpy."""
import numpy as np
import pytest

import nonfinite_ref as N
import probes as P
import softargmin_ref as sar
from oracle import oracle as orc
from probe_check import CASES, INSTANTIATIONS, KERNELS
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic
from test_conv_probes_host import parse_conv_sources

SD = synthetic.random_costreg_state(seed=13)


# ---------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------
def test_reference_relu_keeps_nan_like_torch():
    assert N.ref64_keeps_nan()


def _oracle_layer(layer, x, skip):
    """One layer by the C oracle (fp32, its own loops), BN folded as the blob holds it."""
    wf, sh = P.folded(SD, layer)
    if layer == 10:
        return orc.conv3d(x, wf, bias=sh, bn=None, relu=False)
    if P.GEOM[layer][3]:
        wt = np.ascontiguousarray(wf.transpose(1, 0, 2, 3, 4))
        y = orc.deconv3d(x, wt, bn=None, relu=False) + sh[:, None, None, None]
        return skip + np.maximum(y, 0.0)
    return orc.conv3d(x, wf, bias=sh, bn=None, stride=P.GEOM[layer][2], relu=True)


@pytest.mark.parametrize("layer", range(11))
def test_oracle_meets_the_contract_with_zero_extents(layer):
    wf, sh = P.folded(SD, layer)
    chk = N.Checker()
    pats = N.layer_patterns(layer, np.random.default_rng(29))
    names = {p[0] for p in pats}
    assert {"nan@corner", "nan@interior", "+inf@interior", "-inf@interior"} <= names
    assert all(any(n.startswith("nan@%s" % ax) for n in names) for ax in "zyx")
    assert (layer in (7, 8, 9)) == ("skip nan@interior" in names)
    for name, x, skip in pats:
        with np.errstate(all="ignore"):
            got = _oracle_layer(layer, x, skip)
        ref, bound, touched = N.layer_reference(layer, x, skip, wf, sh)
        assert touched.any() and not touched.all(), name
        if name.startswith("-inf@") and layer != 10:   # after the ReLU the reference holds exact zeros inside the touched set
            assert (np.isfinite(ref) & touched[None]).any(), name
        chk.check(str(layer), name, got, ref, bound, touched, (0, 0, 0))
    assert not chk.failures, chk.failures[:5]
    assert chk.spreads[str(layer)] == (0, 0, 0)
    print(layer, "worst R2 ratio", chk.ratios)


def test_tail_reference_meets_the_contract_with_itself():
    w9, sh9 = P.folded(SD, 9)
    chk = N.Checker()
    for name, x, skip in N.tail_patterns(np.random.default_rng(29)):
        ref, bound, touched = N.tail_reference(x, skip, w9, sh9, SD["prob.weight"], SD["prob.bias"])
        with np.errstate(all="ignore"):
            d11 = _oracle_layer(9, x, skip)
            got = orc.conv3d(d11, SD["prob.weight"], bias=SD["prob.bias"], bn=None, relu=False)[0]
        chk.check("tail", name, got, ref, bound, touched, (0, 0, 0))
    assert not chk.failures, chk.failures[:5]


def test_stride_two_edge_pairs_hold_both_parities():
    for layer in (1, 3, 5):
        for n in P.GEOM[layer][4]:
            assert all((a % 2, b % 2) == (1, 0) for a, b in N.edge_pairs(n))
    assert N.edge_pairs(41) == [(7, 8), (15, 16), (31, 32)] and N.edge_pairs(7, True) == [(3, 4)]


# ---------------------------------------------------------------------------------------------------------------
# the chain's finite share: the oracle alone, and what the extents guarantee
# ---------------------------------------------------------------------------------------------------------------
def test_chain_finite_share_of_the_oracle_and_of_the_extents():
    var = N.chain_voxel_volume()
    assert np.isnan(var).sum() == 1
    cost = orc.costreg_forward(var, SD)
    depth, conf, _ = orc.softargmin_conf(cost, synthetic.depth_values(N.CHAIN_SHAPE[0]))
    nan_pix = np.isnan(cost).any(0)
    assert (np.isnan(cost).all(0) == nan_pix).all()              # every depth of such a pixel
    assert (np.isnan(depth) == nan_pix).all() and (np.isnan(conf) == nan_pix).all()
    assert 1 - nan_pix.mean() >= N.MIN_FINITE_REF_VOXEL, nan_pix.mean()
    rig = N.chain_rig()
    vol = orc.variance_volume(rig["feats"], rig["proj"], rig["dv"])
    cols = np.nonzero(np.isnan(vol).any((0, 1, 2)))[0]
    assert list(cols) == [0, 8, 24], cols                        # the warp's own NaN columns (Z == 0)
    d_rig, c_rig = orc.depth_infer(rig["feats"], rig["proj"], rig["dv"], SD)
    assert np.isfinite(d_rig).mean() >= N.MIN_FINITE_REF_RIG, np.isfinite(d_rig).mean()
    for storage in ("f32", "bf16"):
        for volume, d in ((var, depth), (vol, d_rig)):
            allowed = N.chain_allowed(~np.isfinite(volume).all(0), storage)
            assert not (~np.isfinite(d) & ~allowed).any()        # the carried set holds the oracle's
            assert 1 - allowed.mean() >= N.MIN_FINITE_GOT, (storage, allowed.mean())


# ---------------------------------------------------------------------------------------------------------------
# every kernel form has an extent
# ---------------------------------------------------------------------------------------------------------------
def test_every_conv_instantiation_and_kernel_has_an_extent():
    inst, kern = parse_conv_sources()
    assert inst and kern
    missing = []
    for name in sorted(inst | kern | set(INSTANTIATIONS) | set(KERNELS)):
        try:
            e = N.extent_of(name)
            assert len(e) == 3 and all(isinstance(v, int) and 0 <= v <= 3 for v in e), (name, e)
        except KeyError:
            missing.append(name)
    assert not missing, f"kernel forms without a spread extent: {missing}"
    assert not set(N.EXTENTS) - kern, f"stale entries: {sorted(set(N.EXTENTS) - kern)}"
    assert set(N.LAUNCHER_KERNEL.values()) <= set(N.EXTENTS)
    # the GPU child looks every (case, layer) up; the chain takes the largest extent per layer
    for case, c in CASES.items():
        assert set(c["layers"]) == set(N.CASE_KERNELS[case]), case
        for layer in c["layers"]:
            assert set(N.CASE_KERNELS[case][layer]) <= set(N.EXTENTS)
            N.case_extent(case, layer)
    reached = {k for c in N.CASE_KERNELS.values() for ks in c.values() for k in ks}
    assert reached == set(KERNELS), sorted(set(KERNELS) ^ reached)
    for table in N.CHAIN_KERNELS.values():
        assert set(table) == set(range(9)) | {"tail"}


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: emulated defects of one layer
# ---------------------------------------------------------------------------------------------------------------
SENS_LAYER = 2


def _hand_bf16(a):
    """A hand-rolled RNE to bf16 that forgets NaN: a NaN whose payload sits in the low 16 bits rounds to infinity."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def emulate_layer(x, wf, sh, defect=None, storage="f32"):
    """conv2 in numpy float32 (the fp64 sum rounded once) with a switchable defect."""
    with np.errstate(all="ignore"):
        pre = (P._conv64(SENS_LAYER, x, wf) + sh[:, None, None, None].astype(np.float64)).astype(np.float32)
        y = np.fmax(pre, np.float32(0)) if defect == "relu_fmax" else np.maximum(pre, np.float32(0))
        if defect == "nan_flood" and not np.isfinite(x).all():
            y = np.full_like(y, np.nan)
        if defect == "saturating_store":
            y = np.where(np.isinf(y), np.sign(y) * np.finfo(np.float32).max, y)
        if storage == "bf16":
            if defect == "bf16_nan_to_inf":     # the kernel's NaN with a low payload, then the hand-rolled rounding
                y = np.where(np.isnan(y), np.uint32(0x7F800001).view(np.float32), y)
                y = _hand_bf16(y)
            else:
                y = orc.round_storage(y, "bf16")
    return y.astype(np.float64)


LAYER_DEFECTS = {"exact": None, "relu_fmax": "R1 a finite value hides", "nan_flood": "R3", "saturating_store": "R1 a finite",
                 "bf16_nan_to_inf": "R1 NaN came back as an infinity"}


@pytest.mark.parametrize("defect", list(LAYER_DEFECTS))
def test_checker_reports_emulated_layer_defects(defect):
    storage = "bf16" if defect == "bf16_nan_to_inf" else "f32"
    wf, sh = P.folded(SD, SENS_LAYER)
    chk = N.Checker()
    for name, x, skip in N.layer_patterns(SENS_LAYER, np.random.default_rng(5), storage):
        xq = orc.round_storage(x, storage)
        got = emulate_layer(xq, wf if storage == "f32" else orc.round_storage(wf, storage), sh,
                            None if defect == "exact" else defect, storage)
        ref, bound, touched = N.layer_reference(SENS_LAYER, x, skip, wf, sh, storage)
        chk.check("2", name, got, ref, bound, touched, (0, 0, 0))
    print(defect, chk.failures[:3])
    if defect == "exact":
        assert not chk.failures, chk.failures[:3]
    else:
        assert any(LAYER_DEFECTS[defect] in f for f in chk.failures), chk.failures[:3]
        assert "at (" in chk.failures[0]             # the first offending index is named


# ---------------------------------------------------------------------------------------------------------------
# soft-argmin: the patterns, the fp32 emulation of the kernels, emulated defects
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_form():
    return N.softargmin_case("<8,16,16>")


def test_softargmin_patterns_give_nan_exactly_where_expected(small_form):
    want = np.zeros(small_form["cost"].shape[1], bool)
    for name in N.NAN_PATTERNS:
        want[small_form["pixels"][name]] = True
    assert (N.softmax_nan64(small_form["cost"]) == want).all()
    for form in sar.FORMS:          # every form-forcing shape takes the patterns on distinct pixels
        D, (h, w) = sar.FORM_SHAPES[form]
        assert sar.launch_form(D, h * w)[0] == form


@pytest.mark.parametrize("form", ["<8,16,16>", "<16,16,16>", "loop"])
def test_softargmin_emulation_meets_the_contract(form):
    c = N.softargmin_case(form)
    depth, conf = sar.emulate_forward(c["cost"], c["dv"])
    pix = np.concatenate(list(c["pixels"].values()))
    rd, rc, problems = N.check_softargmin(depth, conf, c["cost"], c["dv"], pix)
    assert not problems and rd <= 1 and rc <= 1, problems
    # the kernels before this contract: a slice that holds -inf logits only turned the pixel into NaN
    depth, conf = sar.emulate_forward(c["cost"], c["dv"], defect="minus_inf_term_nan")
    _, _, problems = N.check_softargmin(depth, conf, c["cost"], c["dv"], pix)
    assert any("NaN set differs" in p and "reference is finite" in p for p in problems), problems


def _softargmin_numpy(cost, dv, defect):
    """softmax, expectation and confidence in numpy float32 with a switchable defect."""
    c = np.asarray(cost, np.float32)
    D, P_ = c.shape
    with np.errstate(all="ignore"):
        if defect == "max_and_sum_skip_nan":
            M = np.nanmax(np.where(np.isnan(c).all(0), -np.inf, c), axis=0)
            e = np.exp(c - M)
            S = np.nansum(e, 0)
            p = np.nan_to_num(e, nan=0.0) / S
        else:
            e = np.exp(c - c.max(0))
            p = e / e.sum(0)
        depth = (p * np.asarray(dv, np.float32)[:, None]).sum(0)
        E = (p * np.arange(D, dtype=np.float32)[:, None]).sum(0)
        idx = np.clip(np.trunc(np.nan_to_num(E, nan=0.0)).astype(np.int64), 0, D - 1)
        conf = sar.window(p.astype(np.float64), idx)
        if defect == "conf_at_garbage_index":      # trunc(NaN) used unclamped: the tap lands in another pixel's logits
            bad = np.isnan(E)
            conf = np.where(bad, np.roll(np.nan_to_num(conf, nan=0.25), 1), conf)
    return depth, conf


@pytest.mark.parametrize("defect", [None, "max_and_sum_skip_nan", "conf_at_garbage_index"])
def test_checker_reports_emulated_softargmin_defects(defect, small_form):
    c = small_form
    depth, conf = _softargmin_numpy(c["cost"], c["dv"], defect)
    pix = np.concatenate(list(c["pixels"].values()))
    _, _, problems = N.check_softargmin(depth, conf, c["cost"], c["dv"], pix)
    print(defect, problems[:2])
    if defect is None:
        assert not problems, problems
    else:
        assert any("NaN set differs" in p and "reference is NaN" in p for p in problems), problems
        assert any(p.startswith("conf") for p in problems)
