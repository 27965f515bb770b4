"""CPU side of the cost-volume backward's fp64 yardstick (tests/cost_volume_grad_ref.py): the left-out cap holds from
fp64 alone on every case (the training shape included), the case table provably contains waves on every path of
warp_variance_bwd_kernel, the fp64 adjoint agrees with float64 autograd of the reference formula, an fp32 emulation of
the kernel (wave layout, window paths, fallbacks, flush, NaN lanes) stays inside the bound on every case, clean and
with v_rcp_f32 at +-1 ulp, and each of the eight defects switched on in that emulation is caught by a named case."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cost_volume_grad_ref as G  # noqa: E402
import warp_ref as W  # noqa: E402
from training_ref import WAVE_WINDOW_TEXELS, torch_variance, wave_window_areas  # noqa: E402

CASES = G.cases()
_adj = {}


def adjoint(name):
    if name not in _adj:
        c = CASES[name]()
        rt = W.rt32(c["proj"]) if c["feats"].shape[0] > 1 else np.zeros((0, 12), np.float32)
        _adj[name] = (c, rt, G.Adjoint(c["feats"], rt, c["dv"]))
    return _adj[name]


@pytest.mark.parametrize("name", list(CASES))
def test_left_out_cap_from_fp64_alone(name):
    c, rt, adj = adjoint(name)
    frac = adj.left_out_fraction()
    print("%s: left out %.3f %% of the gradient entries, %d loose and %d non-finite samples"
          % (name, 100 * frac, int(adj.loose.sum()), int(adj.nan.sum())))
    if name not in ("behind", "behind_rot"):
        assert frac <= W.MAX_LEFT_OUT
    else:
        assert frac < 1.0
    if name == "behind":
        assert adj.nan.any()


@pytest.mark.parametrize("name", ["dtu_n3", "roll", "borders", "zoom", "dtu_n1"])
def test_adjoint_is_float64_autograd_of_the_reference_formula(name):
    c, rt, adj = adjoint(name)
    D, h, w = len(c["dv"]), adj.h, adj.w
    g = G.dense_g(D, h, w, 3)
    f = torch.from_numpy(c["feats"]).double().requires_grad_(True)
    torch_variance(f, torch.from_numpy(rt).double(), torch.from_numpy(c["dv"]).double()).backward(
        torch.from_numpy(g).double())
    res = adj.grad(g)
    want = f.grad.numpy()
    keep = ~np.broadcast_to(adj.left_out[:, None], want.shape)
    err = np.abs(res["grad"] - want)[keep].max()
    assert err <= 1e-9 * np.abs(want).max(), err
    # and the bound is a bound on something: no entry with contributions has a zero bound
    assert (res["bound"][keep & (want != 0)] > 0).all()


def test_nan_pattern_against_float64_autograd():
    """behind: the NaN entries the kernel's rule requires (nan_must: NaN weights on the clamped taps of a non-finite
    coordinate, NaN mean at the sample's reference pixel and at its taps in the other views), which the emulation
    reproduces exactly, against torch CPU autograd in float64.  DESIGN.md section 11.2 records the outcome."""
    c, rt, adj = adjoint("behind")
    D = len(c["dv"])
    g = G.dense_g(D, adj.h, adj.w, 3)
    f = torch.from_numpy(c["feats"]).double().requires_grad_(True)
    torch_variance(f, torch.from_numpy(rt).double(), torch.from_numpy(c["dv"]).double()).backward(
        torch.from_numpy(g).double())
    tn = torch.isnan(f.grad).numpy()
    assert (tn == tn[:, :1]).all()                               # all channels alike
    tn = tn[:, 0]
    em = np.isnan(G.emulate(c["feats"], rt, c["dv"], g))
    assert (em == em[:, :1]).all() and np.array_equal(em[:, 0], adj.nan_must)    # the kernel's rule, entry for entry
    assert np.array_equal(tn[0], adj.nan_must[0])                # reference view: autograd and the kernel agree exactly
    assert not (tn & ~adj.nan_reach).any()                       # autograd's NaNs lie inside what the reference leaves out
    for v in range(1, adj.N):
        both, only_t, only_k = (tn[v] & adj.nan_must[v]).sum(), (tn[v] & ~adj.nan_must[v]).sum(), \
            (~tn[v] & adj.nan_must[v]).sum()
        print("source view %d: NaN texels in both %d, autograd only %d, kernel only %d" % (v, both, only_t, only_k))
    NAN_SETS["autograd"], NAN_SETS["kernel"] = tn, adj.nan_must


NAN_SETS = {}


def test_every_wave_path_is_present():
    paths = {}
    for name in CASES:
        c, rt, adj = adjoint(name)
        paths[name] = G.wave_paths(rt, c["dv"], adj.h, adj.w)
    # (a) strictly increasing cell offsets on every step: plain read-add-write
    assert any(p["plain"] == G.SLAB and p["shared"] == 0 for p in paths["dtu_n2"])
    # (b) reversed (roll) and shared (zoom) cells: ds_add_f32
    assert any(p["shared"] > 0 for p in paths["roll"]) and sum(p["shared"] for p in paths["zoom"]) >= G.SLAB
    c, rt, adj = adjoint("zoom")
    V = adj.views[0]
    assert (np.diff(V["x0"][0, 3]) == 0).mean() > 0.5            # most neighbours of a row share their cell
    # (c) windows above and below 512 texels in one launch
    a = np.array([p["area"] for p in paths["overflow"]])
    c, rt, adj = adjoint("overflow")
    old = wave_window_areas(c["proj"], c["dv"], adj.h, adj.w)   # the bookkeeping test_gpu_training.py uses: same windows
    assert G.WINDOW == WAVE_WINDOW_TEXELS and np.array_equal(np.sort(a[a > 0]), np.sort(old.astype(np.int64)))
    assert (a > G.WINDOW).mean() > 0.2 and ((a > 0) & (a <= G.WINDOW)).mean() > 0.2, a
    # (d) no in-image tap at all
    assert any(p["area"] == 0 for p in paths["borders"]) and any(p["area"] == 0 for p in paths["corners"])
    # (e) a non-finite lane
    assert any(p["nan"] for p in paths["behind"])
    # (f) w % 32 != 0: a ragged tile whose wave has active and inactive lanes
    for name in ("dtu_n2", "dtu_n3", "zoom"):
        assert adjoint(name)[2].w % 32 and any(p["ragged"] and p["area"] > 0 for p in paths[name]), name
    # (g) N = 1, 2, 7
    assert {adjoint(n)[2].N for n in ("dtu_n1", "dtu_n2", "dtu_n7")} == {1, 2, 7}
    assert adjoint("overflow")[2].w % 32 == 0


def test_onehot_sweep_uses_every_wave_position_once():
    D, h, w = 16, 8, 40
    seen = np.zeros((G.C, D, h, w), np.int64)
    per_channel = np.zeros((D, h, w), np.int64)
    for s in range(G.ONEHOT_SWEEP):
        g = G.onehot_g(D, h, w, s)
        nz = g != 0
        for c in range(G.C):                     # one entry per wave footprint and channel
            assert nz[c].reshape(D // 8, 8, h // 2, 2, w).sum(axis=(1, 3)).reshape(D // 8, h // 2, w)[..., :32].sum(-1).max() <= 1
        per_channel += nz.sum(0)
        seen += nz
    assert (per_channel == 1).all()              # every (depth, pixel) position exactly once over sweep x channels


def test_left_out_cap_at_the_training_shape():
    t = G.TRAINING_SHAPE
    c = G.training_shape_case()
    depths = [sl * G.SLAB + j for sl in t["slabs"] for j in range(G.SLAB)]
    adj = G.Adjoint(c["feats"], W.rt32(c["proj"]), c["dv"], depths=depths)
    print("training shape: left out %.3f %%" % (100 * adj.left_out_fraction()))
    assert adj.left_out_fraction() <= W.MAX_LEFT_OUT


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_kernel_stays_inside_the_bound(name):
    """the kernel's own fp32 arithmetic, clean and with the reciprocal at +-1 ulp, dense and one-hot gradients"""
    c, rt, adj = adjoint(name)
    D = len(c["dv"])
    worst = 0.0
    for kind, g in (("dense", G.dense_g(D, adj.h, adj.w, 5)), ("onehot", G.onehot_g(D, adj.h, adj.w, 3))):
        res = adj.grad(g)
        for ulps in ((0, 1, -1) if kind == "dense" else (0,)):
            ratio, problems = G.compare(G.emulate(c["feats"], rt, c["dv"], g, rcp_ulps=ulps), res, adj)
            assert not problems, (kind, ulps, problems)
            worst = max(worst, ratio)
    print("%s: emulation worst error / bound = %.4f" % (name, worst))
    assert worst <= 1.0


# defect -> (case, gradient input) that must catch it, in the fp32 emulation of the kernel
CAUGHT_BY = {
    "o01_o10_swapped": ("corners", "onehot"),
    "m_without_reference_view": ("dtu_n2", "dense"),
    "two_over_n_minus_1": ("dtu_n7", "dense"),
    "duplicates_overwritten": ("zoom", "dense"),
    "oob_weight_kept": ("borders", "dense"),
    "last_window_row_not_flushed": ("dtu_n3", "onehot"),
    "nan_weights_to_zero": ("behind", "dense"),
    "inactive_lanes_write": ("ragged_z0", "dense"),
}


def _input(adj, D, kind):
    return G.dense_g(D, adj.h, adj.w, 5) if kind == "dense" else G.onehot_g(D, adj.h, adj.w, 3)


@pytest.mark.parametrize("defect", G.DEFECTS)
def test_every_defect_in_the_emulated_kernel_is_caught_by_a_named_case(defect):
    assert set(CAUGHT_BY) == set(G.DEFECTS) and len(G.DEFECTS) == 8
    name, kind = CAUGHT_BY[defect]
    c, rt, adj = adjoint(name)
    g = _input(adj, len(c["dv"]), kind)
    res = adj.grad(g)
    clean, problems = G.compare(G.emulate(c["feats"], rt, c["dv"], g), res, adj)
    assert clean <= 1.0 and not problems
    ratio, problems = G.compare(G.emulate(c["feats"], rt, c["dv"], g, defect=defect), res, adj)
    print("%s on %s/%s: error / bound = %.3g %s" % (defect, name, kind, ratio, problems[:1]))
    assert ratio > 1.0 or problems


def test_ragged_z0_puts_a_non_finite_coordinate_on_an_inactive_lane_only():
    c, rt, adj = adjoint("ragged_z0")
    assert adj.w % 32 and not adj.nan.any() and adj.left_out_fraction() <= W.MAX_LEFT_OUT
    wts, _, _ = G._samp32(rt[0], c["dv"], adj.h, adj.w, 32, 0, False)
    bad = np.isnan(wts[0])
    assert bad[:, :, adj.w:].any() and not bad[:, :, :adj.w].any()


@pytest.mark.parametrize("defect", G.ADJOINT_DEFECTS)
def test_every_defect_leaves_the_bound_on_a_named_case(defect):
    name, kind = CAUGHT_BY[defect]
    c, rt, adj = adjoint(name)
    g = _input(adj, len(c["dv"]), kind)
    res = adj.grad(g)
    clean, problems = G.compare(res["grad"], res, adj)
    assert clean == 0.0 and not problems
    ratio, _ = G.compare(adj.grad(g, defect=defect, bound=False)["grad"], res, adj)
    print("%s in the fp64 adjoint on %s/%s: error / bound = %.3g" % (defect, name, kind, ratio))
    assert ratio > 1.0
