"""The checks of tests/train_autograd_ref.py reject what they are for (CPU only).

The assertion helpers that tests/test_gpu_train_autograd.py applies to training.py's autograd functions run here on
torch-CPU fp32 restatements of the wrappers' loops (numpy fp32 emulations of the kernels for the cost volume and the
soft-argmin).  Run clean, the restatements pass every helper; with one of train_autograd_ref.DEFECTS switched on, the
helper meant to catch it fails, by the factor each test prints.  No helper skips an element (left_out == 0, bounds
finite and positive).  The last test is the CPU pre-check of the whole-CostRegNet recipe: torch fp32 against torch fp64
on the CPU stays below train_autograd_ref.PRECHECK in relative L2 on every tensor, so ReLU flips and BatchNorm over
M = 4 values do not blur the GPU comparison.
"""
import numpy as np
import pytest
import torch

import bn3d_ref as BR
import cost_volume_grad_ref as G
import softargmin_ref as SR
import train_autograd_ref as A
import warp_ref as W

CONV_CASES = A.conv_cases()
IDS = lambda c: "%s-B%d" % (c[0][0], c[1])  # noqa: E731


def conv_setup(case, B, seed=3):
    x, w, b, gy = A.conv_inputs(case, B, seed)
    _, kind, _, _, s, _ = case
    return kind, s, x, w, b, gy, A.conv_reference(kind, x, w, b, s, gy), A.conv_bounds(kind, x, w, b, s, gy)


# ---------------------------------------------------------------- 1. convolutions
@pytest.mark.parametrize("case,B", CONV_CASES, ids=[IDS(c) for c in CONV_CASES])
def test_clean_conv_restatement_passes_and_no_element_is_skipped(case, B):
    kind, s, x, w, b, gy, ref, bnd = conv_setup(case, B)
    for key, bound in bnd.items():
        if bound is not None:
            assert A.left_out(bound) == 0.0 and bool(torch.isfinite(bound).all()) and bool((bound > 0).all()), key
    got = A.restate_conv(kind, x, w, b, s, gy)
    ratios = A.check_conv(got, ref, bnd, case[0])
    assert set(ratios) == {"out", "gx", "gw"} | ({"gb"} if b is not None else set())
    assert max(ratios.values()) <= 1.0, ratios
    for i in range(B):   # an item of the batched call is the B = 1 call on that item
        one = A.restate_conv(kind, x[i:i + 1], w, b, s, gy[i:i + 1])
        assert A.same_bits(one["out"][0], got["out"][i]) and A.same_bits(one["gx"][0], got["gx"][i])


def test_the_layer_table_holds_every_tiny_shape_of_the_kernel_suite():
    import test_gpu_train_conv as TC
    table = {(cin, cout, s, shape) for kind, cin, cout, s, shape in A.LAYERS.values() if kind == "conv"}
    for _, cin, cout, s, shape in TC.TINY:
        assert (cin, cout, s, shape) in table, (cin, cout, s, shape)
    assert len(A.LAYERS) == 11 and {l for l in A.RAGGED} | set(A.BATCH3) <= set(A.LAYERS)


def caught(case, B, defect, key, gy=None):
    kind, s, x, w, b, g0, _, _ = conv_setup(case, B)
    gy = g0 if gy is None else gy
    ref, bnd = A.conv_reference(kind, x, w, b, s, gy), A.conv_bounds(kind, x, w, b, s, gy)
    clean = A.check_conv(A.restate_conv(kind, x, w, b, s, gy), ref, bnd, case[0] + " clean")
    bad = A.check_conv(A.restate_conv(kind, x, w, b, s, gy, defect=defect), ref, bnd, case[0] + " " + defect)
    print("%s on %s: %s exceeds its bound by a factor of %.3g (clean: %.3g)" % (defect, case[0], key, bad[key], clean[key]))
    assert max(clean.values()) <= 1.0 < bad[key], (clean, bad)
    return bad


@pytest.mark.parametrize("layer,B", [(2, 2), (5, 2), (8, 2), (4, 3)])
def test_the_weight_gradient_of_the_last_item_only_is_caught(layer, B):
    bad = caught(A.conv_case(layer), B, "last_item_weight", "gw")
    assert bad["out"] <= 1.0 and bad["gx"] <= 1.0   # nothing else moves


def test_a_bias_gradient_not_summed_over_the_items_is_caught():
    caught(A.conv_case(10), 2, "bias_not_summed", "gb")


@pytest.mark.parametrize("layer", [7, 8, 9])
def test_x_and_gy_exchanged_in_the_transposed_weight_gradient_is_caught(layer):
    caught(A.conv_case(layer), 2, "transposed_x_gy_exchanged", "gw")


@pytest.mark.parametrize("layer", [2, 9])
def test_an_expanded_gradient_read_with_its_strides_ignored_is_caught(layer):
    """y.sum().backward() hands over an all-ones gradient of stride 0, which reads the same with or without its
    strides; the per-(item, channel) gradient of y.sum((2, 3, 4)) has stride 0 along D, H, W only and does not."""
    case = A.conv_case(layer)
    kind, s, x, w, b, g0, _, _ = conv_setup(case, 2)
    v = A.heavy(g0.shape[:2], torch.Generator().manual_seed(9))
    gy = v[:, :, None, None, None].expand(g0.shape)
    assert gy.stride()[2:] == (0, 0, 0)
    bad = caught(case, 2, "expanded_strides_ignored", "gx", gy=gy)
    assert bad["gw"] > 1.0
    clean = A.restate_conv(kind, x, w, b, s, gy.contiguous())
    wrong = A.restate_conv(kind, x, w, b, s, gy, defect="expanded_strides_ignored")
    assert A.same_bits(A.restate_conv(kind, x, w, b, s, gy)["gx"], clean["gx"])
    assert not A.same_bits(wrong["gx"], clean["gx"])   # the GPU suite's bit-equality sees it too


def test_two_consumer_chain_passes_clean_and_catches_a_dropped_branch():
    import torch.nn.functional as F
    x, w1, w2, wT, go = A.two_consumer_inputs()
    ref, bnd = A.two_consumer_reference(x, w1, w2, wT, go)
    for key, bound in bnd.items():
        assert A.left_out(bound) == 0.0, key

    def run(drop_skip):
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, w2, wT)]
        conv = lambda a, w, s: F.conv3d(a, w, stride=s, padding=1)  # noqa: E731
        dec = lambda a, w: F.conv_transpose3d(a, w, stride=2, padding=1, output_padding=1)  # noqa: E731
        y = conv(leaves[0], leaves[1], 1)
        ys = y.detach() if drop_skip else y      # the skip's gradient dropped: y keeps one consumer only
        out = dec(conv(y, leaves[2], 2), leaves[3]) + ys
        out.backward(go)
        return dict(out=out, gx=leaves[0].grad, gw1=leaves[1].grad, gw2=leaves[2].grad, gwT=leaves[3].grad)

    clean = {k: A.worst(v, ref[k], bnd[k]) for k, v in run(False).items()}
    bad = {k: A.worst(v, ref[k], bnd[k]) for k, v in run(True).items()}
    print("two consumers clean", clean, "\nskip gradient dropped", bad)
    assert max(clean.values()) <= 1.0, clean
    assert bad["gx"] > 1.0 and bad["gw1"] > 1.0 and bad["out"] <= 1.0


# ---------------------------------------------------------------- 2. cost volume and soft-argmin, two different items
@pytest.mark.parametrize("D", A.CV_DEPTHS)
def test_cost_volume_items_pass_clean_and_the_other_items_rig_or_depths_are_caught(D):
    items, gs = A.cv_items(D), A.cv_grads(D)
    rts = [W.rt32(c["proj"])[:c["feats"].shape[0] - 1] for c in items]
    adjs = [G.Adjoint(c["feats"], rt, c["dv"]) for c, rt in zip(items, rts)]
    for adj, g in zip(adjs, gs):
        assert adj.left_out_fraction() <= W.MAX_LEFT_OUT
        res = adj.grad(g)
        kept = ~np.broadcast_to(adj.left_out[:, None], res["bound"].shape)
        # a texel no sample reaches has gradient 0 and bound 0: compare() holds it to exactly 0, it is not skipped
        assert np.isfinite(res["bound"][kept]).all() and (res["bound"][kept] > 0)[res["grad"][kept] != 0].all()
    clean = [G.emulate(c["feats"], rt, c["dv"], g) for c, rt, g in zip(items, rts, gs)]
    r, problems = A.check_cv(clean, adjs, gs, "D=%d clean" % D)
    assert r <= 1.0 and not problems, problems
    # the wrapper's defects in the fp32 restatement: item 0's rt (dv) for every item
    for defect, pick in (("rt_of_item_0", lambda b: (rts[0], items[b]["dv"])),
                         ("dv_of_item_0", lambda b: (rts[b], items[0]["dv"]))):
        bad = [G.emulate(c["feats"], *pick(b), g) for b, (c, g) in enumerate(zip(items, gs))]
        rb, pb = A.check_cv(bad, adjs, gs, "D=%d %s" % (D, defect))
        print("%s: item 1 exceeds its bound by a factor of %.3g" % (defect, rb))
        assert rb > 1.0 and pb and all(p.startswith("item 1") for p in pb)
    # and from the fp64 reference alone, both ways round: the other item's rt or dv lies outside this item's bound
    for b in range(2):
        o = 1 - b
        for what, adj_wrong in (("rt", G.Adjoint(items[b]["feats"], rts[o], items[b]["dv"])),
                                ("dv", G.Adjoint(items[b]["feats"], rts[b], items[o]["dv"]))):
            wrong = adj_wrong.grad(gs[b], bound=False)["grad"]
            ratio, _ = G.compare(np.where(np.isfinite(wrong), wrong, 0.0), adjs[b].grad(gs[b]), adjs[b])
            print("D=%d item %d with the other item's %s: error / bound %.3g" % (D, b, what, ratio))
            assert ratio > 1.0


@pytest.mark.parametrize("D", [48, 192])
def test_soft_argmin_items_pass_clean_and_item_0s_depth_values_are_caught(D):
    items = A.sa_items(D)
    for c in items:
        ref = SR.reference(c["cost"], c["dv"], c["gd"])
        for key in ("d_depth", "grad_bound"):
            assert np.isfinite(ref[key]).all() and (ref[key] > 0).all(), key

    def run(dv_of):
        fwd = [SR.emulate_forward(c["cost"], dv_of(b)) for b, c in enumerate(items)]
        grad = [SR.emulate_backward(c["cost"], dv_of(b), c["gd"]) for b, c in enumerate(items)]
        return [f[0] for f in fwd], [f[1] for f in fwd], grad

    r, problems = A.check_sa(*run(lambda b: items[b]["dv"]), items, "D=%d clean" % D)
    assert max(r.values()) <= 1.0 and not problems, problems
    rb, pb = A.check_sa(*run(lambda b: items[0]["dv"]), items, "D=%d dv_of_item_0" % D)
    print("dv_of_item_0: depth exceeds its bound by a factor of %.3g, grad_cost by %.3g" % (rb["depth"], rb["grad"]))
    assert rb["depth"] > 1.0 and rb["grad"] > 1.0 and rb["conf"] <= 1.0   # the confidence does not read the depths
    assert pb and all(p.startswith("item 1") for p in pb)


# ---------------------------------------------------------------- 4. batch_norm_relu
def fresh_bn(C, p, **kw):
    bn = torch.nn.BatchNorm3d(C, **kw).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(p["gamma"]))
        bn.bias.copy_(torch.from_numpy(p["beta"]))
        if bn.running_mean is not None:
            bn.running_mean.copy_(torch.from_numpy(p["rm"]))
            bn.running_var.copy_(torch.from_numpy(p["rv"]))
    return bn


@pytest.mark.parametrize("C", A.BN_CHANNELS)
@pytest.mark.parametrize("relu,skip", [(True, True), (False, True), (False, False)])
def test_clean_batch_norm_restatement_passes(C, relu, skip):
    y, p = A.bn_inputs(C, seed=C)
    ref, bnd = A.bn_reference(y, p, relu=relu, skip=skip, rm=p["rm"], rv=p["rv"])
    for key in ("out", "grad_y", "grad_gamma", "grad_beta", "rm", "rv"):
        assert np.isfinite(bnd[key]).all() and (bnd[key] > 0).all(), key
    got = A.restate_bn(y, p, fresh_bn(C, p), relu=relu, skip=skip)
    ratios = A.check_bn(got, ref, bnd, "C=%d relu=%s skip=%s" % (C, relu, skip))
    assert len(ratios) == 6 and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("C", A.BN_CHANNELS)
def test_momentum_none_follows_the_cumulative_average_and_0_1_is_caught(C):
    _, p = A.bn_inputs(C, seed=C)
    for defect in (None, "momentum_none_as_0.1"):
        bn = fresh_bn(C, p, momentum=None)
        for call in range(3):
            y = BR.field(("normal", "heavy", "offset")[call], C, int(np.prod(A.BN_DIMS)), 50 + call)
            rm, rv = bn.running_mean.numpy().astype(np.float64), bn.running_var.numpy().astype(np.float64)
            ref, bnd = A.bn_reference(y, p, rm=rm, rv=rv, momentum=1.0 / (call + 1))
            got = A.restate_bn(y, p, bn, defect=defect)
            ratios = A.check_bn({k: got[k] for k in ("rm", "rv")}, ref, bnd, "C=%d call %d %s" % (C, call, defect))
            assert int(bn.num_batches_tracked) == call + 1
            if defect is None:
                assert max(ratios.values()) <= 1.0, ratios
            else:
                print("%s, call %d: rm, rv exceed their bounds by %.3g, %.3g" % (defect, call, ratios["rm"], ratios["rv"]))
                assert min(ratios.values()) > 1.0, ratios


@pytest.mark.parametrize("C", A.BN_CHANNELS)
def test_a_running_variance_updated_with_the_biased_form_is_caught(C):
    y, p = A.bn_inputs(C, seed=C)
    ref, bnd = A.bn_reference(y, p, rm=p["rm"], rv=p["rv"])
    got = A.restate_bn(y, p, fresh_bn(C, p), defect="biased_running_var")
    ratios = A.check_bn(got, ref, bnd, "C=%d biased_running_var" % C)
    print("biased_running_var: rv exceeds its bound by a factor of %.3g" % ratios["rv"])
    assert ratios["rv"] > 1.0 and max(v for k, v in ratios.items() if k != "rv") <= 1.0


@pytest.mark.parametrize("defect", [None, "skip_grad_dropped", "skip_grad_doubled"])
def test_the_skips_gradient_with_a_second_consumer(defect):
    C = 8
    y, p = A.bn_inputs(C, seed=C)
    q = BR.params(C, y.shape[0], 91)
    other = q["go"].astype(np.float64) * q["skip"].astype(np.float64)      # the second consumer: (skip * c).backward(go2)
    got = A.restate_bn(y, p, fresh_bn(C, p), defect=defect)["skip_grad"]
    got = (got.astype(np.float32) + (q["go"] * q["skip"])).astype(np.float64)     # autograd's accumulation in fp32
    want, bound = p["go"].astype(np.float64) + other, A.skip_grad_bound(p["go"], other)
    assert np.isfinite(bound).all() and (bound > 0).all()
    ratio = BR.worst(got, want, bound)
    print("%s: skip.grad error / bound %.3g" % (defect, ratio))
    assert (ratio <= 1.0) if defect is None else (ratio > 1.0)


# ---------------------------------------------------------------- 3. the recipe of the whole-CostRegNet comparison
@pytest.mark.parametrize("dims", A.COSTREG_SHAPES)
def test_cpu_precheck_fp32_against_fp64_on_the_costreg_recipe(dims):
    cr32 = A.costreg_module()
    cr64 = A.fp64_copy(cr32)
    worst = 0.0
    for step in range(2):
        x, g = A.costreg_inputs(dims, step)
        got, ref = A.costreg_step(cr32, x, g), A.costreg_step(cr64, x.double(), g.double())
        assert set(got) == set(ref) and len(got) == 2 + 32 + 30
        for key in sorted(ref):
            if key.endswith("num_batches_tracked"):
                assert int(got[key]) == int(ref[key]) == step + 1
                continue
            e = A.rel_l2(got[key], ref[key])
            worst = max(worst, e)
            assert float(ref[key].double().norm()) > 0, key
            assert e <= A.PRECHECK, (key, step, e)
    print("costreg recipe %s: worst fp32 / fp64 relative L2 over all tensors and both steps %.3g" % (dims, worst))
