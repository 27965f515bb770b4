"""CPU side of the conv probes (tests/probes.py, tests/probe_check.py, test_gpu_conv_probes.py): the lattice and the
crafted weights give every output at most one product, the crafted values split as designed under an exactly
identity BN, the Winograd matrices are the ones the bound is derived from, every kernel instantiation has a probe
case -- and the bounds catch plausible split-operand defects, emulated in numpy, while an exact emulation of the
six-term split with fp32 accumulation passes them."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import probes as P
import probe_check as PC
from oracle import oracle as orc
from probe_check import CASES, INSTANTIATIONS, INSTANTIATIONS16, KERNELS, UNREACHABLE16
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scene_3dreconstruction_mvsnet_amd",
                    "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------
# one product per output
# ---------------------------------------------------------------------------------------------------------------
def _count_products(layer, nz):
    """number of nonzero products each output receives from the 0/1 occupancy nz [D,H,W] (all weights nonzero)."""
    X = torch.from_numpy(nz.astype(np.float64))[None, None]
    ones = torch.ones((1, 1, 3, 3, 3), dtype=torch.float64)
    if P.GEOM[layer][3]:
        return F.conv_transpose3d(X, ones, stride=2, padding=1, output_padding=1)[0, 0].numpy()
    return F.conv3d(X, ones, stride=P.GEOM[layer][2], padding=1)[0, 0].numpy()


FORMS = [(layer, None) for layer in range(11)] + [(0, "F43"), (2, "F23"), (4, "F23")]


@pytest.mark.parametrize("layer,wino", FORMS)
def test_lattice_gives_every_output_one_product_at_most(layer, wino):
    ci, _, _, _, shape = P.GEOM[layer]
    sp = P.spacing(layer, wino)
    seen = np.zeros((ci,) + shape, np.int64)
    rng = np.random.default_rng(0)
    for ph in P.phases(sp):
        x = P.lattice(ci, shape, sp, ph, rng)
        nz = x != 0
        assert (nz.sum(0) <= 1).all()                      # one channel per voxel
        assert _count_products(layer, nz.any(0)).max() <= 1
        if wino:   # every tile's m + 2 input planes (any z offset) hold one lattice plane at most
            planes = nz.any(axis=(0, 2, 3)).astype(int)
            win = P.wino_tile(wino)[1]
            assert max(planes[z:z + win].sum() for z in range(shape[0])) <= 1
        seen += nz
    assert (seen.sum(0) >= 1).all(), "the phases together probe every voxel"


@pytest.mark.parametrize("layer", range(11))
def test_crafted_weights_give_every_output_one_product_and_sweep_all_taps(layer):
    ci, co = P.GEOM[layer][:2]
    base = synthetic.random_costreg_state(seed=1)
    runs = 27 if layer == 10 else P.crafted_runs(layer)
    taps = set()
    for r in range(runs):
        wf, sh = P.folded(P.crafted_state(base, r, np.random.default_rng(r)), layer)
        assert (sh == 0).all()
        nzw = wf != 0
        assert (nzw.reshape(co, -1).sum(1) == 1).all()        # one (ci, tap) per output channel
        taps |= {int(t) for t in np.nonzero(nzw.reshape(co, ci, 27))[2]}
    assert taps == set(range(27))


def test_crafted_values_split_as_designed():
    v = P.crafted((4096,), np.random.default_rng(3)).astype(np.float32)
    p1, p2, p3 = P.split3(v)
    v64, e = v.astype(np.float64), np.floor(np.log2(v.astype(np.float64)))
    assert ((p1.astype(np.float64) + p2 + p3) == v64).all()    # exact three-piece split
    np.testing.assert_array_equal(p2, (2.0 ** -8 - 2.0 ** -15) * 2.0 ** e)
    np.testing.assert_array_equal(p3, (2.0 ** -17 - 2.0 ** -23) * 2.0 ** e)
    # the cross terms a split kernel must keep: a2 b2 and a1 b3 (= a3 b1 by symmetry) are >= 16 ulp of a b
    ab = v64 * v64[::-1]
    for term in (p2.astype(np.float64) * p2[::-1], p1.astype(np.float64) * p3[::-1]):
        assert (term >= 16 * P.ulp32(ab)).all()


def test_identity_bn_packs_the_crafted_weights_unscaled():
    """The packer's folded weights equal the crafted weights bit for bit (scale exactly 1.0, shift 0): the split
    panels (pack_split_panels) and every other panel are packed from this section."""
    v1 = P.identity_var()
    assert np.float32(1.0) / np.sqrt(np.float32(v1) + np.float32(1e-5)) == np.float32(1.0)
    sd = P.crafted_state(synthetic.random_costreg_state(seed=2), 0, np.random.default_rng(0))
    blob = _lib.pack_weights(sd).numpy().view(np.float32)
    off = 0
    for l in range(11):
        ci, co = _lib._LAYER_CH[l]
        wf, sh = P.folded(sd, l)
        want = wf.reshape(co, ci, 27).transpose(2, 1, 0)
        np.testing.assert_array_equal(blob[off:off + 27 * ci * co].reshape(27, ci, co), want)
        off = (off + 27 * ci * co + 63) // 64 * 64
        np.testing.assert_array_equal(blob[off:off + co], sh)
        off = (off + co + 63) // 64 * 64
        if l < 10:
            raw = np.asarray(sd[_lib.CONV_WEIGHT_KEYS[l]], np.float32)
            raw = raw.transpose(1, 0, 2, 3, 4) if P.GEOM[l][3] else raw
            np.testing.assert_array_equal(wf, raw)
            nz = wf[wf != 0]
            p1, p2, p3 = P.split3(nz)
            assert ((p1.astype(np.float64) + p2 + p3) == nz).all() and (p2 > 0).all() and (p3 > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# the Winograd matrices of the bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F43", "F23"])
def test_winograd_matrices_compute_the_z_correlation(name):
    A, G, B = P.WINO[name]
    m, n = P.wino_tile(name)
    rng = np.random.default_rng(5)
    for _ in range(20):
        d, g = rng.standard_normal(n), rng.standard_normal(3)
        y = A @ ((G @ g) * (B @ d))
        np.testing.assert_allclose(y, [d[i:i + 3] @ g for i in range(m)], rtol=1e-12, atol=1e-12)
    assert 1.0 < P.wino_gain(name) < 200.0


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: emulated split-operand kernels against the probe and dense bounds
# ---------------------------------------------------------------------------------------------------------------
TERMS = ("a1b1", "a1b2", "a2b1", "a2b2", "a1b3", "a3b1")
SENS_LAYER, SENS_SHAPE = 2, (6, 7, 10)   # conv2's geometry (16 -> 16, stride 1) on a small ragged volume


def emulate_split(x, wf, sh, drop=(), halo_col=None, tap_shift=None, chan_swap=False):
    """A split-operand stride-1 conv in numpy: every product a b as the six bf16 cross terms (exact in fp32),
    accumulated in fp32 tap by tap, then relu(acc + shift) in fp32.  Defects: `drop` leaves out cross terms;
    `halo_col` stages the input column x == halo_col with its first piece only; `tap_shift` = tap index whose input
    is read one voxel off in x; `chan_swap` stages input channels 0 and 1 swapped."""
    ci, D, H, W = x.shape
    xs = x.copy()
    if chan_swap:
        xs[[0, 1]] = xs[[1, 0]]
    a = list(P.split3(xs))
    if halo_col is not None:
        for p in (1, 2):
            a[p] = a[p].copy()
            a[p][..., halo_col] = 0
    ap = [np.pad(t, ((0, 0), (1, 1), (1, 1), (1, 2))) for t in a]
    b = P.split3(wf)
    acc = np.zeros((wf.shape[0], D, H, W), np.float32)
    for tap in range(27):
        kz, ky, kx = np.unravel_index(tap, (3, 3, 3))
        dx = kx + (1 if tap == tap_shift else 0)
        for term in TERMS:
            if term in drop:
                continue
            ia, ib = int(term[1]) - 1, int(term[3]) - 1
            xa = ap[ia][:, kz:kz + D, ky:ky + H, dx:dx + W]
            prod = np.einsum("oc,czyx->oczyx", b[ib][:, :, kz, ky, kx], xa).astype(np.float32)   # exact
            for c in range(ci):
                acc = (acc + prod[:, c]).astype(np.float32)
    return np.maximum((acc + sh[:, None, None, None]).astype(np.float32), 0).astype(np.float64)


# defect -> (emulation arguments, caught by the dense bound too).  A dropped cross term errs by 2^-18 |a b| per
# product with random sign: at random-normal data that sits inside fp32 summation noise, only the probes pin it.
DEFECTS = {
    "exact": ({}, True),
    "halo column keeps piece 1 only": (dict(halo_col=SENS_SHAPE[2] - 1), True),
    "a2b2 dropped": (dict(drop=("a2b2",)), False),
    "a1b3 + a3b1 dropped": (dict(drop=("a1b3", "a3b1")), False),
    "tap shifted by one voxel": (dict(tap_shift=22), True),
    "staged channels 0 / 1 swapped": (dict(chan_swap=True), True),
}


def _sens_inputs():
    ci, co = P.GEOM[SENS_LAYER][:2]
    rng = np.random.default_rng(11)
    base = synthetic.random_costreg_state(seed=4)
    wf, sh = P.folded(base, SENS_LAYER)
    probes = [(P.lattice(ci, SENS_SHAPE, (3, 3, 3), ph, rng), wf, sh) for ph in P.phases((3, 3, 3))]
    for r in range(P.crafted_runs(SENS_LAYER)):
        wfc, shc = P.folded(P.crafted_state(base, r, rng), SENS_LAYER)
        probes.append((P.crafted((ci,) + SENS_SHAPE, rng), wfc, shc))
    # dense: random normal and heavy-tailed non-negative (as a variance volume)
    dense = [(rng.standard_normal((ci,) + SENS_SHAPE).astype(np.float32), wf, sh),
             (np.exp(3.0 * rng.standard_normal((ci,) + SENS_SHAPE)).astype(np.float32), wf, sh)]
    return probes, dense


@pytest.fixture(scope="module")
def sens_inputs():
    return _sens_inputs()


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_probe_and_dense_bounds_catch_emulated_split_defects(defect, sens_inputs):
    probes, dense = sens_inputs
    kw, dense_catches = DEFECTS[defect]
    worst_probe = worst_dense = 0.0
    for x, wf, sh in probes:
        want, bound = P.probe_want_bound(SENS_LAYER, x, None, wf, sh)
        got = emulate_split(x, wf, sh, **kw)
        worst_probe = max(worst_probe, float((np.abs(got - want) / bound).max()))
    for x, wf, sh in dense:
        ref, bound = P.dense_ref_bound(SENS_LAYER, x, None, wf, sh)
        got = emulate_split(x, wf, sh, **kw)
        worst_dense = max(worst_dense, float((np.abs(got - ref) / bound).max()))
    print(f"{defect}: probe {worst_probe:.3g} x bound, dense {worst_dense:.3g} x bound")
    if defect == "exact":
        assert worst_probe <= 1.0 and worst_dense <= 1.0, (worst_probe, worst_dense)
    else:
        assert worst_probe > 1.0, worst_probe
        if dense_catches:
            assert worst_dense > 1.0, worst_dense


# ---------------------------------------------------------------------------------------------------------------
# every kernel form has a probe case
# ---------------------------------------------------------------------------------------------------------------
CONV_SOURCES = ("conv3d_direct.hip", "conv3d_mfma.hip", "conv3d_mfma16.hip", "conv3d_small.hip",
                "conv_winograd.hip", "conv0_split.hip", "conv11_prob.hip")


def parse_conv_sources():
    """-> (launcher instantiations `run_x<...>`, kernel names) found in the conv sources (shared with
    test_nonfinite_host.py)."""
    inst, kern = set(), set()
    for name in CONV_SOURCES:
        src = _read(name)
        for m in re.finditer(r"\b(run_\w+)\s*<((?:[^<>;(]|<[^<>;(]*>)*)>\s*\(", src):
            args = re.sub(r"\s+", "", m.group(2))
            if re.search(r"\b(CIN|COUT|S|BZ|BY|BX|KW|CPT|STRIDE|DECONV|RELU|SKIP)\b", args):
                continue   # a launcher forwarding its own template parameters, not an instantiation
            inst.add(f"{m.group(1)}<{args}>")
        kern |= set(re.findall(r"\b(\w+_kernel)\s*(?:<[^<>;]*>)?\s*<<<", src))
    return inst, kern


def test_every_conv_instantiation_and_kernel_has_a_probe_case():
    inst, kern = parse_conv_sources()
    assert inst, "no run_*<...> instantiation found: the parser no longer matches the sources"
    assert not inst - set(INSTANTIATIONS), f"instantiations without a probe case: {sorted(inst - set(INSTANTIATIONS))}"
    assert not kern - set(KERNELS), f"kernels without a probe case: {sorted(kern - set(KERNELS))}"
    assert not set(INSTANTIATIONS) - inst, f"stale entries: {sorted(set(INSTANTIATIONS) - inst)}"
    assert not set(KERNELS) - kern, f"stale entries: {sorted(set(KERNELS) - kern)}"
    assert set(INSTANTIATIONS.values()) | set(KERNELS.values()) <= set(CASES)


def _function_body(src, signature):
    """the text of the function whose definition starts with `signature`, up to its closing brace in column 0"""
    i = src.index(signature)
    return src[i:src.index("\n}\n", i)]


def test_every_storage_templated_launcher_has_a_16bit_case():
    """A launcher templated on the storage type DT compiles other loads, stores and casts for F16 / BF16 (St<DT>):
    its F32 probe case does not cover them.  Reachability is read from the dispatch: plan_layer (launch_plan.h) sends
    16-bit storage to conv3d_mfma16.hip's forms unless MVS_MFMA16=0, and every `dtype`-taking launcher that
    launch_conv_layer calls for a form planned past that gate goes through MVS_DISPATCH_DTYPE, which instantiates all three storage types."""
    inst, _ = parse_conv_sources()
    templated = {k for k in inst if re.search(r"\bDT\b", k)}
    assert templated and templated == set(INSTANTIATIONS16), sorted(templated ^ set(INSTANTIATIONS16))
    for key, case in INSTANTIATIONS16.items():
        assert CASES[case]["storages"] == ("f16", "bf16"), (key, case)
    # the gate (csrc/launch_plan.h plans the form, launch_conv_layer switches over it), and what lies behind it
    header = _read("launch_plan.h")
    planner = _function_body(header, "inline Plan plan_layer(")
    gate = "if (opt.mfma16 && (dtype == MVS_F16 || dtype == MVS_BF16) && layer <= 9) return plan_layer16("
    assert gate in planner
    behind = planner[planner.index(gate) + len(gate):]
    assert "return plan_conv1(" in behind
    all_forms = set(re.findall(r"^\s+(k\w+)(?: = 0)?,", re.search(r"enum Form \{(.*?)\n\};", header, re.S).group(1), re.M))
    forms = set(re.findall(r"\bk[A-Z]\w+", behind + _function_body(header, "inline Plan plan_conv1("))) & all_forms
    f32_forms = {"kConv0WinoSplit", "kConvGSplit", "kDeconvGSplit"}      # each behind a dtype == MVS_F32 test
    assert f32_forms < forms
    call = behind[:behind.index("kConv0WinoSplit")]
    assert "dtype == MVS_F32" in call[call.rindex("if ("):]
    split_block = behind[behind.index("if (opt.split_layers && dtype == MVS_F32) {"):]
    split_block = split_block[:split_block.index("\n    }\n")]
    assert all(behind.count(f) == split_block.count(f) > 0 for f in ("kConvGSplit", "kDeconvGSplit"))
    body = _function_body(_read("conv3d_direct.hip"), "int launch_conv_layer(")
    launcher_of = {}
    for labels, arm in re.findall(r"((?:case plan::k\w+:\s*)+)(.*?)(?=case plan::|default:)", body, re.S):
        for form in re.findall(r"plan::(k\w+)", labels):
            launcher_of[form] = set(re.findall(r"return (launch_\w+)\(", arm))
    assert forms - {"kProbLds"} <= set(launcher_of) and set(launcher_of) | {"kProbLds", "kNone"} <= all_forms
    called = set().union(*(launcher_of[f] for f in forms - {"kProbLds"}))
    f32_only = {"launch_layer_split", "launch_conv0_wino43_split"}
    assert set().union(*(launcher_of[f] for f in f32_forms)) == f32_only
    assert len(called - f32_only) >= 7
    macro = _read("storage.h")
    assert all(f"case {t}: {{ constexpr int DT = {t};" in macro for t in ("MVS_F32", "MVS_F16", "MVS_BF16"))
    srcs = {n: _read(n) for n in CONV_SOURCES}
    for name in called - f32_only:
        fn = [_function_body(t, f"int {name}(") for t in srcs.values() if f"\nint {name}(" in t]
        assert len(fn) == 1 and "MVS_DISPATCH_DTYPE(dtype" in fn[0], name
    # every templated launcher of the fp32-arithmetic files is named by a function that such a dispatch reaches
    for key in templated:
        if "Op16" in key or key.startswith("run_convz16"):
            continue            # conv3d_mfma16.hip: launch_layer_mfma16, taken at the gate itself
        assert CASES[INSTANTIATIONS16[key]]["env"].get("MVS_MFMA16") == "0", key
    for what, (fname, line) in UNREACHABLE16.items():
        assert line in _read(fname), (what, fname)


def test_probe_cases_set_only_switches_options_reads():
    names = set(re.findall(r'"(MVS_\w+)"', _read("mvs_host.hip")))
    for name, case in CASES.items():
        assert set(case["env"]) <= names, (name, case["env"])
        assert case["storages"] in (("f32",), ("f16", "bf16"))
        assert case.get("arith", "mfma16") == ("fp32" if case["env"].get("MVS_MFMA16") == "0" else "mfma16")
        assert case["storages"] != ("f32",) or "arith" not in case


# ---------------------------------------------------------------------------------------------------------------
# 16-bit storage: the rounding helpers, the generators' conditions, and that the checker bites
# ---------------------------------------------------------------------------------------------------------------
B16 = ("f16", "bf16")


def test_rne_st_and_ulp_st_are_the_storage_types():
    rng = np.random.default_rng(23)
    v = np.concatenate([rng.standard_normal(200000) * 10.0 ** rng.integers(-9, 5, 200000),
                        [65519.99, 65520.0, 65504.0, -65520.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 0.0, 1e-8]])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(P.rne_st(v, "f16"), v.astype(np.float16).astype(np.float64))
    v32 = v.astype(np.float32)
    np.testing.assert_array_equal(P.rne_st(v32.astype(np.float64), "bf16"), orc.round_storage(v32, "bf16"))
    with np.errstate(over="ignore"):
        a = np.abs(v.astype(np.float16))
    a = a[a < 65504]        # np.spacing of the largest finite value is inf
    np.testing.assert_array_equal(P.ulp_st(a.astype(np.float64), "f16"), np.spacing(a).astype(np.float64))
    assert P.ulp_st(0.0, "f16") == 2.0 ** -24 and P.ulp_st(1e-6, "bf16") == 2.0 ** -27
    assert P.ulp_st(2.0 ** -100 * 1.5, "bf16") == 2.0 ** -107
    assert P.OVERFLOW_ST["f16"] == 65520.0 and P.FMAX_ST["f16"] == 65504.0


def test_err_st_around_the_largest_finite_value():
    ref = np.array([65519.0, 65519.0, 65521.0, 65521.0, 65519.0, 65519.0, 100.0, -65530.0, -65530.0])
    emax = np.array([0.5, 0.5, 0.5, 0.5, 2.0, 2.0, 0.5, 1.0, 1.0])
    got = np.array([65504.0, np.inf, np.inf, 65504.0, 65504.0, np.inf, np.inf, -np.inf, -65504.0])
    err, bound = P.err_st(got, ref, emax, "f16")
    np.testing.assert_array_equal(err <= bound, [True, False, True, False, True, True, False, True, False])


@pytest.mark.parametrize("storage", B16)
@pytest.mark.parametrize("layer", range(10))
def test_boundary_probes_sit_on_and_beside_the_midpoints(layer, storage):
    """Conditions on the INPUTS of the rounding-boundary probes: per layer and type at least a quarter of the outputs
    are exact midpoints, a quarter lie on each near side, and among the midpoints the storage value below has an even
    last bit in a third at least and an odd one in a third at least."""
    ci, co, _, tr, shape = P.GEOM[layer]
    base = synthetic.random_costreg_state(seed=1)
    rng = np.random.default_rng(41 + layer)
    stats = []
    taps = set()
    for r in range(P.boundary_runs(layer)):
        wf, sh = P.folded(P.boundary_state(base, r, storage), layer)
        assert (sh == 0).all() and ((wf != 0).reshape(co, -1).sum(1) == 1).all()
        taps |= {int(t) for t in np.nonzero((wf != 0).reshape(co, ci, 27))[2]}
        w = np.unique(wf[wf != 0])
        assert w.size == 1 and orc.round_storage(w, storage) == w and int(round((w[0] - 1) * 2 ** P.FRAC_ST[storage])) % 2
        for exps in P.BOUNDARY_EXPS[storage]:
            x = P.boundary_inputs((ci,) + shape, storage, exps, rng)
            np.testing.assert_array_equal(orc.round_storage(x, storage), x)
            p = P._conv64(layer, x, wf)
            assert ((p * 2.0 ** 40).astype(np.float32) == p * 2.0 ** 40).all()      # an exact fp32 number
            p = p[p > 0]    # the outputs that got their product (not the padded rim, 1 in 8 of a transposed layer's)
            assert p.size >= x[0].size // 2
            mid, lo, hi, bit = P.classify_boundary(p, storage)
            assert (mid | lo | hi).all()
            stats.append((mid.sum(), lo.sum(), hi.sum(), (mid & (bit == 0)).sum(), (mid & (bit == 1)).sum(), p.size))
    assert taps == set(range(27))
    m, lo, hi, even, odd, n = np.sum(stats, axis=0)
    assert min(m, lo, hi) >= n / 4, (m, lo, hi, n)
    assert min(even, odd) >= m / 3, (even, odd, m)


def test_range_end_probes_cover_the_ends_of_fp16():
    base = synthetic.random_costreg_state(seed=1)
    sd = P.ends_state(base)
    for layer in range(10):
        ci, co, _, tr, shape = P.GEOM[layer]
        wf, sh = P.folded(sd, layer)
        x = P.ends_inputs(ci, shape, np.random.default_rng(41 + layer))
        p = P._conv64(layer, x, wf)
        want = P.rne_st(p, "f16")
        assert ((wf != 0).reshape(co, -1).sum(1) == 1).all()
        assert ((p > 0) & (p < 2.0 ** -14)).sum() >= 64                         # subnormal outputs
        sub = p[(p > 0) & (p < 2.0 ** -14)]
        assert (np.abs(sub - P.rne_st(sub, "f16")) == 2.0 ** -25).sum() >= 8     # midpoints between subnormals
        assert (p == 2.0 ** -25).any() and (want[p == 2.0 ** -25] == 0).all()
        up = p == 2.0 ** -25 * (1 + 2.0 ** -10)
        assert up.any() and (want[up] == 2.0 ** -24).all()
        for v, w in ((65519.875, 65504.0), (65520.03125, np.inf), (65520.0, np.inf), (65488.0625, 65504.0),
                     (65487.96875, 65472.0)):
            assert (p == v).sum() >= 4 and (want[p == v] == w).all(), (layer, v)
        xs, ws = x[(x != 0) & (np.abs(x) < 2.0 ** -14)], wf[(wf != 0) & (np.abs(wf) < 2.0 ** -14)]
        assert xs.size and ws.size                                              # subnormal inputs, subnormal weights
        # ... whose products are normal fp16 numbers: a flush of the operand is the only way to lose them
        assert (P._conv64(layer, np.where(np.abs(x) < 2.0 ** -14, x, 0), wf).max() >= 2.0 ** -14)
        assert (P._conv64(layer, x, np.where(np.abs(wf) < 2.0 ** -14, wf, 0)).max() >= 2.0 ** -14)


@pytest.mark.parametrize("arith", ["mfma16", "fp32"])
def test_fp16_heavy_volume_sits_in_the_largest_octave_that_stays_finite(arith):
    sd = synthetic.random_costreg_state(seed=13)
    for layer in range(10):
        wf, sh = P.folded(sd, layer)
        x16, skip = P.heavy_launch(layer, "f16", wf, sh, arith)
        xb, _ = P.heavy_launch(layer, "bf16", wf, sh, arith)
        k = np.log2(x16.astype(np.float64).max() / xb.astype(np.float64).max())
        assert k == round(k) and (x16 == (xb.astype(np.float64) * 2.0 ** k).astype(np.float32)).all()
        assert P.f16_top(layer, x16, skip, wf, sh, arith, 0) < 65504.0
        assert not P.f16_top(layer, x16, skip, wf, sh, arith, 1) < 65504.0
        assert (np.abs(orc.round_storage(x16, "f16")) < 2.0 ** -14).mean() > 1e-4     # and reaches the subnormals


def old_bound16(layer, x, skip, wf, sh, storage, dense):
    """The 16-bit bounds as they were: the reference rounded to storage, one storage ulp with its floor at 2^-14 for
    both types (+ DENSE_C 2^-24 S)."""
    q = lambda t: orc.round_storage(np.asarray(t, np.float32), storage)  # noqa: E731
    qs = None if skip is None else q(skip)
    want = q(P.ref64(layer, q(x), q(wf), sh, qs)).astype(np.float64)
    return want, P.ulp16(want, storage) + (P.DENSE_C * P.U * P.scale64(layer, q(x), q(wf), sh, qs) if dense else 0.0)


@pytest.mark.parametrize("storage", B16)
def test_new_16bit_dense_bound_against_the_old_one(storage):
    """bound_st against the old `ulp16 + e_max` on the heavy-tailed references: strictly tighter wherever the result's
    spacing is at least the spacing at the old floor, and not wider anywhere -- but for ONE corner, which the derivation
    forces: where |ref64| is below e_max (a cancelled sum, every ReLU-clamped zero) the kernel's fp32 value may
    lie e_max away from the reference, and half a storage ulp THERE is more than the old bound's whole ulp at the
    reference.  The excess is at most 2^-11 (fp16) / 2^-8 (bf16) of e_max, which the old bound never accounted for."""
    sd = synthetic.random_costreg_state(seed=13)
    f = P.FRAC_ST[storage]
    for layer in range(10):
        wf, sh = P.folded(sd, layer)
        x, skip = P.heavy_launch(layer, storage, wf, sh)
        want_old, old = old_bound16(layer, x, skip, wf, sh, storage, True)
        ref, emax = P.ref_emax(layer, x, skip, wf, sh, storage, dense=True)
        _, new = P.dense_ref_bound(layer, x, skip, wf, sh, storage)
        corner = P.ulp_st(np.abs(ref) + emax, storage) > 2 * P.ulp16(want_old, storage)
        assert (new[~corner] <= old[~corner]).all(), (layer, float((new / old)[~corner].max()))
        assert (np.abs(ref[corner]) < emax[corner]).all()
        assert (new[corner] <= old[corner] + 2.0 ** -f * emax[corner]).all()
        # strictly tighter from the old floor's spacing up (equal only where |ref64| + e_max reaches the next binade)
        at_floor = (P.ulp_st(ref, storage) >= P.ulp16(2.0 ** -14, storage)) & ~corner
        same_binade = P.ulp_st(np.abs(ref) + emax, storage) <= P.ulp16(want_old, storage)
        assert (at_floor & same_binade).mean() > 0.25 and (new < old)[at_floor & same_binade].all()


# --- mutations of the cast -------------------------------------------------------------------------------------
MUT_LAYERS = {2: (6, 7, 10), 3: (6, 8, 10), 8: (3, 4, 5)}      # stride 1, stride 2, transposed; small ragged volumes


def _cast(v, storage, how):
    """fp32 values (as fp64) -> storage, correctly ("rne") or in one of the wrong ways"""
    q = P.ulp_st(v, storage)
    a, sg = np.abs(v), np.sign(v)
    other = "bf16" if storage == "f16" else "f16"
    with np.errstate(over="ignore", invalid="ignore"):
        r = {"rne": lambda: P.rne_st(v, storage),
             "truncation": lambda: sg * np.floor(a / q) * q,
             "round-half-away": lambda: sg * np.floor(a / q + 0.5) * q,
             "round-half-toward-zero": lambda: sg * np.ceil(a / q - 0.5) * q,
             "double rounding": lambda: P.rne_st(P.rne_st(v, other), storage),
             "subnormal results flushed": lambda: np.where(np.abs(P.rne_st(v, storage)) < 2.0 ** -14, 0.0,
                                                           P.rne_st(v, storage)),
             "saturation": lambda: np.clip(P.rne_st(v, storage), -65504.0, 65504.0),
             "inf one value early": lambda: np.where(np.abs(P.rne_st(v, storage)) == 65504.0, np.copysign(np.inf, v),
                                                     P.rne_st(v, storage))}[how]()
    if how in ("truncation", "round-half-away", "round-half-toward-zero"):
        r = np.where(np.abs(r) > P.FMAX_ST[storage], np.copysign(np.inf, v), r)
    return r


def emulate16(layer, x, skip, wf, sh, storage, how="rne", flush_operands=False):
    """A 16-bit-storage layer in numpy: narrowed operands, fp32 accumulator (the fp64 sum rounded once), fp32 shift, ReLU
    and skip, then the cast `how`."""
    xq, sq, wq = P.operands_st(x, skip, wf, storage, "mfma16", layer)
    if flush_operands:
        xq, wq = np.where(np.abs(xq) < 2.0 ** -14, 0, xq), np.where(np.abs(wq) < 2.0 ** -14, 0, wq)
    with np.errstate(over="ignore"):
        acc = P._conv64(layer, xq, wq).astype(np.float32)
        v = np.maximum(acc + np.asarray(sh, np.float32)[:, None, None, None], np.float32(0))
        if sq is not None:
            v = v + sq
    return _cast(v.astype(np.float64), storage, how)


FP16_ONLY = ("subnormal results flushed", "subnormal operands flushed", "saturation", "inf one value early")
MUTATIONS = ("truncation", "round-half-away", "round-half-toward-zero", "double rounding") + FP16_ONLY


def _launches(layer, storage):
    """(kind, x, skip, wf, sh) of lattice, boundary (+ ends) and dense launches at MUT_LAYERS' shape"""
    ci, co, s, tr, _ = P.GEOM[layer]
    shape = MUT_LAYERS[layer]
    oshape = (co,) + tuple(2 * n if tr else (n - 1) // s + 1 for n in shape)
    base = synthetic.random_costreg_state(seed=13)
    rng = np.random.default_rng(7 + layer)
    wf, sh = P.folded(base, layer)
    out = []
    for ph in P.phases(P.spacing(layer)):
        skip = rng.standard_normal(oshape).astype(np.float32) if tr else None
        out.append(("lattice", P.lattice(ci, shape, P.spacing(layer), ph, rng), skip, wf, sh))
    zero = np.zeros(oshape, np.float32) if tr else None
    for r in range(P.boundary_runs(layer)):
        wfb, shb = P.folded(P.boundary_state(base, r, storage), layer)
        for exps in P.BOUNDARY_EXPS[storage]:
            out.append(("boundary", P.boundary_inputs((ci,) + shape, storage, exps, rng), zero, wfb, shb))
    if storage == "f16":
        wfe, she = P.folded(P.ends_state(base), layer)
        out.append(("boundary", P.ends_inputs(ci, shape, rng), zero, wfe, she))
    skip = rng.standard_normal(oshape).astype(np.float32) if tr else None
    out.append(("dense", rng.standard_normal((ci,) + shape).astype(np.float32), skip, wf, sh))
    xh = P.heavy(ci, shape, rng)
    if storage == "f16":
        xh = (xh.astype(np.float64) * 2.0 ** P.f16_scale(layer, xh, skip, wf, sh)).astype(np.float32)
    out.append(("dense", xh, skip, wf, sh))
    return out


@pytest.mark.parametrize("storage", B16)
@pytest.mark.parametrize("layer", list(MUT_LAYERS))
def test_16bit_checks_reject_wrong_casts_that_the_old_bounds_let_through(layer, storage):
    """probe_check's own checks (check_single with its inexact16 rule, check_exact, check_dense) on emulated outputs: the
    correct cast passes all of them; every wrong one fails the boundary probes; truncation also fails the LATTICE
    through the inexact16 rule.  A wrong TIE rule cannot fail that rule on the lattice: it differs from RNE only where
    the kernel's fp32 value is itself a midpoint, the reference is then within e_max of that midpoint, and that is the
    case the rule must allow -- the boundary probes, whose product is exact, are what tells the tie rules apart.  The
    old bounds (old_bound16, on the old inputs: lattice and standard-normal dense) pass every rounding defect and both
    defects at 65504; the flushes they did catch, through the few lattice outputs that happen to be subnormal."""
    launches = _launches(layer, storage)
    result = {}
    for how in ("rne",) + MUTATIONS:
        if how in FP16_ONLY and storage == "bf16":
            continue        # bf16's subnormals and its largest value are fp32's: out of scope (probes.ulp_st)
        chk, old_ok = PC.Checker("host"), True
        fails = {"lattice": 0, "boundary": 0, "dense": 0}
        for kind, x, skip, wf, sh in launches:
            if how == "subnormal operands flushed":
                got = emulate16(layer, x, skip, wf, sh, storage, "rne", flush_operands=True)
            else:
                got = emulate16(layer, x, skip, wf, sh, storage, how)
            before = len(chk.failures)
            check = {"lattice": PC.check_single, "boundary": PC.check_exact, "dense": PC.check_dense}[kind]
            args = (chk, f"{layer}:{kind}:{storage}", layer, got, x, skip, wf, sh, storage, None)
            check(*args, "mfma16") if kind != "lattice" else check(*args)
            fails[kind] += len(chk.failures) - before
            if kind == "lattice" or (kind == "dense" and np.abs(x).max() < 8):
                want, bound = old_bound16(layer, x, skip, wf, sh, storage, kind == "dense")
                with np.errstate(invalid="ignore"):
                    old_ok &= bool((np.abs(got - want) <= bound).all())
        result[how] = (fails, old_ok, dict(chk.unexplained))
        print(layer, storage, how, fails, "old bounds pass" if old_ok else "old bounds fail")
    assert sum(result["rne"][0].values()) == 0 and result["rne"][1], result["rne"]
    for how, (fails, old_ok, unexplained) in result.items():
        if how == "rne":
            continue
        assert fails["boundary"] > 0, how
        if how == "truncation":
            assert unexplained.get(f"{layer}:lattice:{storage}", 0) > 0, how
        # (fp16 through bf16 loses three bits, which any bound sees; bf16 through fp16 is the subtle one)
        if how in ("truncation", "round-half-away", "round-half-toward-zero", "saturation", "inf one value early") \
                or (how == "double rounding" and storage == "bf16"):
            assert old_ok, how
