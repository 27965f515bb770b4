"""NaN and infinity through FeatureNet (csrc/featnet.hip) and the training kernels (csrc/train_conv3d.hip,
csrc/train_bn3d.hip, softargmin_bwd_kernel of csrc/train_backward.hip): the contract, the injection patterns, the
per-kernel spread sets with their derivations, the checker and the references.  Shared by
tests/test_nonfinite_train_host.py (CPU), tests/nonfinite_train_check.py (the GPU child) and
tests/test_gpu_nonfinite_train.py.  Nothing here touches the GPU or the library.

Contract.  R1 and R3 are those of tests/nonfinite_ref.py; R2 is sharpened, because every kernel in scope is
bit-reproducible (the suite asserts that elsewhere).  For a kernel output `got`, the output `clean` of the SAME launch
on the clean input (the same tensors with every injected value replaced by the finite value that stood there) and the
NaN-propagating fp64 reference `ref` of the injected input:
  R1   never hide     wherever ref is non-finite got is non-finite; where ref is NaN got is NaN (NaN for +-inf is
                      accepted: a padded tap turns inf into inf * 0, a Chan merge an infinite mean into inf - inf).
  R2'  nothing moves  outside the spread set the bytes of got equal the bytes of clean.  No tolerance.
  R3   bounded spread got may differ from clean only inside the spread set, which is derived per kernel from its operand
                      geometry below and is a superset of ref's non-finite set (the checker asserts that too).  Inside
                      it, where ref and got are both finite (a -inf that the ReLU turns into an exact 0, a single -inf
                      logit, a gradient that does not depend on the damaged operand), got is held to the kernel's fp64
                      bound of the clean input against ref; where no bound is given, to the bytes of clean.

Spread sets (each next to the function that builds it):
  fconv_mfma_kernel      K holds (tap, channel) pairs of ONE output pixel (an MFMA row is one pixel, and a row's sum
                         never meets another row's operands); the padded tap re-reads the pixel under the last tap of
                         that same output against a packed 0; out-of-image halo pieces are selected to 0, not multiplied;
                         the upper half of a half-empty N-tile is never stored.  Extent (0, 0): exactly the k x k
                         footprint of the reference, every output channel of it.          feat_spread()
  fconv01_fused_kernel   conv0 on conv1's halo (a select puts the 0 ring around the image), then conv1: the composition
                         of two 3 x 3 footprints, 5 x 5 clipped to the image, and nothing more.    feat_spread()
  the whole net          the eight footprints composed: receptive_field() = 41 image pixels per feature pixel.  net_spread()
  conv_kernel            (kFwd1, kFwd2, kDgrad2, flip) an MFMA row is one output voxel; invalid lanes, rows and taps
                         are selected to 0 or skipped; padded columns are not stored: the reference's footprint,
                         every output channel.                                        conv_spread_fwd / conv_spread_dgrad
  wgrad_kernel + reduce  M = gy channels, N = x channels, K = output voxels.  A non-finite x[ci] at voxel v is a
                         non-finite B entry of column ci for the taps whose in-range output reads v: gw[:, ci, those
                         taps].  A non-finite gy[co] at an output is a non-finite A entry of row co: it meets every
                         column, also the taps that are out of range there and hold a selected 0 (NaN * 0): all of
                         gw[co, :, :], and gbias[co].                                                wgrad_spread()
  BatchNorm forward      a thread owns one channel group of its rows; the block tree and bn_stats_final_kernel merge
                         per channel.  A non-finite y[:, c] takes out[:, c], save_mean[c], save_invstd[c],
                         running_mean[c] and running_var[c]; a non-finite skip element its own output element only.
  BatchNorm backward     a non-finite grad_out[:, c] or y[:, c] (through the saved statistics too) takes grad_y[:, c],
                         grad_gamma[c] and grad_beta[c].                                              bn_case()
  softargmin_bwd_kernel  a thread owns a pixel: a non-finite logit or grad_depth at pixel p takes grad_cost[:, p].
                         A single -inf logit leaves the pixel finite (a term of exactly 0): it stays in the spread set,
                         since the clean launch has another softmax there, and is held to softargmin_ref's backward
                         bound.                                                                 softargmin_case()
The relayouts (mvs_volume_relayout, c8_to_nchw_kernel) move bits: the GPU tests compare them as int32, no set needed.

The backward's ReLU mask is a select that lets a NaN pre-activation pass, `!(pre <= 0) ? grad_out : 0`, as torch's
threshold_backward and as the forward's own `!(t <= 0) ? t : 0`: bn_reference().  A non-finite grad_out behind a closed
ReLU is no gradient; in a channel whose statistics are NaN every element passes, so that grad_beta is the plain sum of
grad_out there and is non-finite exactly when torch's is.  (The kernels' mask was `pre > 0` until these tests: a
channel lost in the forward then had grad_beta = 0, and a training step whose loss was NaN reported finite gradients
for the BatchNorm biases where torch reports NaN.)  bn3d_ref.reference() multiplies by the mask instead, which would
turn a masked non-finite grad_out into NaN where neither torch nor the kernel does.
"""
import numpy as np
import torch
import torch.nn.functional as F

import bn3d_ref as BR
import featnet_ref as FR
import probes as P
import softargmin_ref as SR

VALUES = (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))
F32 = np.float32
MIN_OUTSIDE = 0.5           # coverage condition: at least this share of the outputs (BatchNorm: of the channels) is held
                            # bit-equal, so that a case cannot pass on R1 / R3 alone


# ---------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def check(what, got, clean, ref, spread, bound=None, finite=None):
    """-> list of violations (empty: the contract holds).  got, clean: fp32 arrays of one output; ref: fp64 of the
    injected input; spread: bool, broadcastable; bound: fp64 array or None; finite: bool or None, the part of the
    spread set where the contract promises a finite value wherever ref is finite (a single -inf logit)."""
    got, clean, ref = np.asarray(got, F32), np.asarray(clean, F32), np.asarray(ref, np.float64)
    if not (got.shape == clean.shape == ref.shape):
        return ["%s: shapes differ: got %s clean %s reference %s" % (what, got.shape, clean.shape, ref.shape)]
    spread = np.broadcast_to(np.asarray(spread, bool), ref.shape)
    out = []

    def fail(rule, mask):
        if mask.any():
            i = tuple(int(v) for v in np.argwhere(mask)[0])
            out.append("%s: %s at %s: got %r, clean %r, reference %r (%d elements)"
                       % (what, rule, i, float(got[i]), float(clean[i]), float(ref[i]), int(mask.sum())))

    nf_ref, nf_got = ~np.isfinite(ref), ~np.isfinite(got)
    fail("the clean launch is not finite", ~np.isfinite(clean))
    fail("the reference is non-finite outside the derived spread set", nf_ref & ~spread)
    fail("R1 a finite value hides a non-finite one", nf_ref & ~nf_got)
    fail("R1 NaN came back as an infinity", np.isnan(ref) & nf_got & ~np.isnan(got))
    fail("R2' bytes differ from the clean launch outside the spread set", ~spread & (bits(got) != bits(clean)))
    if finite is not None:
        fail("R3 non-finite where the contract keeps the value finite", np.broadcast_to(finite, ref.shape) & nf_got & ~nf_ref)
    inside = spread & ~nf_ref & ~nf_got
    if bound is None:
        fail("R3 finite inside the spread set, but not the clean launch's bytes", inside & (bits(got) != bits(clean)))
    else:
        with np.errstate(all="ignore"):
            off = inside & ~(np.abs(got.astype(np.float64) - ref) <= np.broadcast_to(bound, ref.shape))
        fail("R3 finite inside the spread set, but beyond the fp64 bound", off)
    return out


def inf_fate(got, ref):
    """-> (infinite reference values, of them the same infinity in got, of them NaN in got): what a run reports"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf = np.isinf(ref)
    return int(inf.sum()), int((inf & (got == ref)).sum()), int((inf & np.isnan(got)).sum())


def outside_share(spread, shape=None):
    s = np.broadcast_to(np.asarray(spread, bool), shape) if shape is not None else np.asarray(spread, bool)
    return 1.0 - float(s.mean())


def check_case(case, got, clean):
    """case: dict(ref, spread, bound) keyed by output name; got, clean: dicts of arrays -> violations."""
    out = []
    for key in case["ref"]:
        out += check("%s/%s" % (case["name"], key), got[key], clean[key], case["ref"][key], case["spread"][key],
                     case["bound"].get(key), case.get("finite", {}).get(key))
    return out


def coverage(case):
    """output name -> share of its elements outside the spread set"""
    return {k: outside_share(case["spread"][k], np.shape(case["ref"][k])) for k in case["ref"]}


def channel_of(C, vi):
    """channel of injected value vi (0 NaN, 1 +inf, 2 -inf): one channel per value, a third of the channels apart
    (C < 3: as far apart as C allows)"""
    return min(vi * max(C // 3, 1), C - 1)


# ---------------------------------------------------------------------------------------------------------------
# FeatureNet
# ---------------------------------------------------------------------------------------------------------------
FEAT_SHAPE = (2, 20, 44)        # ragged in x for every block tile of featnet_ref.BLOCK, in y for all but the 4-row
                                # tiles of the stride-1 layers 3, 4, 6, 7; 3 x 2 tiles of the 8 x 32 tile
NET_SHAPE = (2, 96, 128)
ROTATIONS = 3                   # over the three rotations every position holds every value once


def feat_boundaries(kernel):
    """(y, x) input coordinate of the first pixel behind a tile edge: the block tile's where the output has more than
    one block tile along that axis, else the 2 x 8 MFMA tile's"""
    s = 1 if kernel == FR.FUSED else FR.LAYERS[kernel][3]
    _, H, W = FEAT_SHAPE
    th, tw = FR.tile(kernel)
    Ho, Wo = FR.out_size(H, s), FR.out_size(W, s)
    return s * (th if th < Ho else 2), s * (tw if tw < Wo else 8)


def feat_positions(kernel):
    """name -> (y, x) in view 0: the first and the last pixel, both sides of a tile edge in y and in x, one interior
    (both coordinates even: at stride 2 as well it lies under the LAST tap of an in-range output, whose padded twin
    multiplies it by the packed 0)"""
    _, H, W = FEAT_SHAPE
    yb, xb = feat_boundaries(kernel)
    my, mx = H // 2 + 3, W // 2 + 3
    pos = [("first", (0, 0)), ("last", (H - 1, W - 1)), ("y%d" % (yb - 1), (yb - 1, mx)), ("y%d" % yb, (yb, mx)),
           ("x%d" % (xb - 1), (my, xb - 1)), ("x%d" % xb, (my, xb)), ("interior", (H // 2 + 4, W // 4 + 1))]
    assert len({p for _, p in pos}) == len(pos)
    return pos


def feat_spread(kernel, mask):
    """mask [N,H,W] of injected pixels (any channel) -> [N,Ho,Wo]: the outputs whose k x k window (the fused kernel:
    whose two composed 3 x 3 windows) holds an injected pixel.  Every output channel reads every input channel."""
    m = np.asarray(mask, np.float64)[:, None]
    for l in ((0, 1) if kernel == FR.FUSED else (kernel,)):
        _, _, k, s = FR.LAYERS[l]
        m = (FR.conv64(m, np.ones((1, 1, k, k)), s) != 0).astype(np.float64)
    return m[:, 0] != 0


def net_spread(mask):
    m = np.asarray(mask, np.float64)[:, None]
    for _, _, k, s in FR.LAYERS:
        m = (FR.conv64(m, np.ones((1, 1, k, k)), s) != 0).astype(np.float64)
    return m[:, 0] != 0


def feat_case(st, kernel, rot):
    """One launch of a layer (0..7, through mvs_feature_layer) or of the fused kernel at FEAT_SHAPE: view 0 holds the
    seven positions with NaN, +inf, -inf in turn (rotated by `rot`), each value in channels of its own; view 1 is clean
    and lies outside the spread set whole."""
    N, H, W = FEAT_SHAPE
    ci = 3 if kernel == FR.FUSED else FR.LAYERS[kernel][0]
    idx = 8 if kernel == FR.FUSED else kernel
    base = FR.make_input(kernel, "unit" if kernel in (0, FR.FUSED) else "normal", N, H, W, seed=4000 + idx)
    x, mask = base.copy(), np.zeros((N, H, W), bool)
    for k, (_, (py, px)) in enumerate(feat_positions(kernel)):
        vi = (k + rot) % 3
        x[0, channel_of(ci, vi), py, px] = VALUES[vi][1]
        mask[0, py, px] = True
    with np.errstate(all="ignore"):
        if kernel == FR.FUSED:
            ref, bound = FR.chain64(st, x, 0, 1), FR.fused_ref_bound(st, base)[1]
        else:
            ref, bound = FR.block64(st, kernel, x), FR.dense_ref_bound(st, kernel, base)[1]
    spread = np.broadcast_to(feat_spread(kernel, mask)[:, None], ref.shape)
    return dict(name="feat/%s/rot%d" % (kernel, rot), x=x, base=base, ref={"y": ref}, spread={"y": spread},
                bound={"y": bound})


def net_image_case(st):
    """The whole net at NET_SHAPE, one NaN pixel in the corner (0, 0) of view 0 (green channel)."""
    N, H, W = NET_SHAPE
    base = FR.make_input(0, "unit", N, H, W, seed=4100)
    x, mask = base.copy(), np.zeros((N, H, W), bool)
    x[0, 1, 0, 0] = np.nan
    mask[0, 0, 0] = True
    with np.errstate(all="ignore"):
        ref = FR.chain64(st, x)
    return dict(name="net/nan_corner", x=x, base=base, ref={"y": ref},
                spread={"y": np.broadcast_to(net_spread(mask)[:, None], ref.shape)}, bound={})


NET_WEIGHT_CASES = {"nan_weight_conv3": ("conv3.conv.weight", (5, 2, 1, 1)), "nan_var_conv5": ("conv5.bn.running_var", (7,))}


def nan_state(st, which):
    """copy of the FeatureNet state with one NaN parameter: a diverged run, a damaged checkpoint"""
    key, idx = NET_WEIGHT_CASES[which]
    st = dict(st)
    a = np.array(st[key], np.float32, copy=True)
    a[idx] = np.nan
    st[key] = a
    return st


# ---------------------------------------------------------------------------------------------------------------
# training convolutions: tensors are torch, [C,D,H,W] on the CPU, as in test_gpu_train_conv.py
# ---------------------------------------------------------------------------------------------------------------
def conv_cases():
    """test_gpu_train_conv.CASES + TINY restated (the GPU test asserts they are equal): (name, Cin, Cout, stride, dims)
    as a CONVOLUTION; a transposed layer is the adjoint of the stride-2 conv with its channels exchanged."""
    out = []
    for l, (cin, cout, stride, transposed, shape) in P.GEOM.items():
        out.append(("layer%d" % l, cout, cin, 2, tuple(2 * s for s in shape)) if transposed else
                   ("layer%d" % l, cin, cout, stride, shape))
    return out + [("conv6_tiny", 64, 64, 1, (2, 2, 3)), ("conv4_tiny", 32, 32, 1, (4, 4, 6)),
                  ("conv5_tiny", 32, 64, 2, (4, 4, 6)), ("conv3_tiny", 16, 32, 2, (8, 8, 12)),
                  ("conv2_tiny", 16, 16, 1, (8, 8, 12)), ("prob_tiny", 8, 1, 1, (2, 2, 3))]


CONV_CASES = conv_cases()
CONV_OPS = ("forward", "dgrad", "wgrad_x", "wgrad_gy")


def ref_fwd(x, w, b, s):
    return F.conv3d(x.double()[None], w.double(), None if b is None else b.double(), stride=s, padding=1)[0]


def ref_dgrad(g, w, s):
    return F.conv_transpose3d(g.double()[None], w.double(), stride=s, padding=1, output_padding=s - 1)[0]


def ref_wgrad(x, g, s, cout, cin):
    w = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double()[None], w, stride=s, padding=1)[0]
    return torch.autograd.grad(y, w, g.double())[0]


def mt_of(nc):
    """ConvCfg::MT of csrc/train_conv3d.hip: the tile rows (consecutive y) of one wave"""
    return 8 if (nc + 15) // 16 <= 2 else 4


def conv_positions(dims, mt, scale):
    """(z, y, x) in a tensor of `dims` whose tile space is 1 / scale of it: the first and the last voxel, both sides of
    the 16-voxel tile edge in x (x = 15 | 16 in tile space) and of the last row of an MT y-group (y = MT - 1 | MT), and
    an interior voxel; where the axis is too short for the edge, its middle.  z has no tile (a wave owns one z)."""
    D, H, W = dims
    xb = 16 * scale if 16 * scale < W else max(W // 2, 1)
    yb = mt * scale if mt * scale < H else max(H // 2, 1)
    zc, yc, xc = D // 2, min(H // 2 + 1, H - 1), min(W // 2 + 1, W - 1)
    pos = [(0, 0, 0), (D - 1, H - 1, W - 1), (zc, yc, xb - 1), (zc, yc, xb), (zc, yb - 1, xc), (zc, yb, xc),
           (max(zc - 1, 0), H // 3, W // 3)]
    return list(dict.fromkeys(pos))


def inject(t, positions, rot):
    """t [C,D,H,W] torch -> (injected copy, mask [C,D,H,W] bool)"""
    x, mask = t.clone(), torch.zeros(t.shape, dtype=torch.bool)
    for k, (z, y, xx) in enumerate(positions):
        vi = (k + rot) % 3
        c = channel_of(t.shape[0], vi)
        x[c, z, y, xx] = float(VALUES[vi][1])
        mask[c, z, y, xx] = True
    return x, mask


def conv_spread_fwd(mask, s):
    """voxel mask [D,H,W] -> outputs whose 3 x 3 x 3 window at stride s holds a marked voxel"""
    return F.conv3d(mask.double()[None, None], torch.ones((1, 1, 3, 3, 3), dtype=torch.float64), stride=s, padding=1)[0, 0] != 0


def conv_spread_dgrad(mask, s):
    """output-voxel mask -> input voxels whose forward window holds a marked output: the adjoint footprint"""
    return F.conv_transpose3d(mask.double()[None, None], torch.ones((1, 1, 3, 3, 3), dtype=torch.float64), stride=s,
                              padding=1, output_padding=s - 1)[0, 0] != 0


def wgrad_spread(xmask, gmask, s, cout, cin, odims):
    """-> (gw spread [cout,cin,3,3,3], gbias spread [cout]) of the module docstring"""
    gw, gb = torch.zeros((cout, cin, 27), dtype=torch.bool), torch.zeros(cout, dtype=torch.bool)
    for c, z, y, x in (xmask.nonzero().tolist() if xmask is not None else []):
        for tap in range(27):
            t = (tap // 9, tap // 3 % 3, tap % 3)
            o = [(v - k + 1) for v, k in zip((z, y, x), t)]          # s o = v - k + 1 per axis
            if all(a % s == 0 and 0 <= a // s < n for a, n in zip(o, odims)):
                gw[:, c, tap] = True
    for c in (gmask.nonzero()[:, 0].tolist() if gmask is not None else []):
        gw[c] = True
        gb[c] = True
    return gw.reshape(cout, cin, 3, 3, 3), gb


def conv_inputs(case, seed=51):
    _, cin, cout, s, dims = case
    odims = tuple(d // s for d in dims)
    gen = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn((cin,) + dims, generator=gen), g=torch.randn((cout,) + odims, generator=gen),
                w=torch.randn((cout, cin, 3, 3, 3), generator=gen) * 0.1, b=torch.randn((cout,), generator=gen))


def _conv_spread(op, mask, s, cout, cin, odims):
    if op == "forward":
        return {"y": conv_spread_fwd(mask.any(0), s).numpy()[None]}
    if op == "dgrad":
        return {"gx": conv_spread_dgrad(mask.any(0), s).numpy()[None]}
    gw, gb = wgrad_spread(mask if op == "wgrad_x" else None, mask if op == "wgrad_gy" else None, s, cout, cin, odims)
    return {"gw": gw.numpy(), "gb": gb.numpy()}


def conv_case(case, op, rot):
    """op in CONV_OPS -> dict(name, inj, clean: the operands; ref, spread, bound).  The non-finite values sit in the
    operand the A side reads (forward: x; dgrad: gy; wgrad_x: x only; wgrad_gy: gy only).  Of conv_positions, in its
    order, as many as leave MIN_OUTSIDE of every output outside the spread set (the tiny volumes hold fewer than
    seven), and always the first."""
    name, cin, cout, s, dims = case
    odims = tuple(d // s for d in dims)
    t = conv_inputs(case)
    clean, inj = dict(t), dict(t)
    key, pos = ("x", conv_positions(dims, mt_of(cout), s)) if op in ("forward", "wgrad_x") else \
        ("g", conv_positions(odims, mt_of(cin), 1))      # dgrad: tile space = gy's dims, in kFwd1-flip and kDgrad2 alike
    keep = pos[:1]
    for q in pos[1:]:
        sp = _conv_spread(op, inject(t[key], keep + [q], rot)[1], s, cout, cin, odims)
        if all(outside_share(v) >= MIN_OUTSIDE for k, v in sp.items() if k != "gb"):
            keep.append(q)
    inj[key], mask = inject(t[key], keep, rot)
    spread = _conv_spread(op, mask, s, cout, cin, odims)
    with np.errstate(all="ignore"):
        if op == "forward":
            ref = {"y": ref_fwd(inj["x"], t["w"], t["b"], s).numpy()}
        elif op == "dgrad":
            ref = {"gx": ref_dgrad(inj["g"], t["w"], s).numpy()}
        else:
            ref = {"gw": ref_wgrad(inj["x"], inj["g"], s, cout, cin).numpy(),
                   "gb": inj["g"].double().sum((1, 2, 3)).numpy()}
    spread = {k: np.broadcast_to(v, ref[k].shape) for k, v in spread.items()}
    return dict(name="conv/%s/%s/rot%d" % (name, op, rot), inj=inj, clean=clean, ref=ref, spread=spread, bound={},
                stride=s, positions=keep)


# the cases that cannot meet the coverage condition and are exempt from it (they run all the same):
#   * a 2 x 2 x 3 volume: the 3 x 3 x 3 window of its first voxel alone holds 8 of its 12 voxels;
#   * wgrad_gy with one output channel: the only row of gw is the whole gradient.
CONV_COVERAGE_EXEMPT = {("conv6_tiny", "forward"), ("conv6_tiny", "dgrad"), ("prob_tiny", "forward"),
                        ("prob_tiny", "dgrad"), ("prob_tiny", "wgrad_gy"), ("layer10", "wgrad_gy")}


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------
# bn3d_ref.CASES without the 70001-row one; none of those has a second block (rows_per_block is 128 .. 1024), so two
# cases with a block boundary inside are added: (64, 130) and (8, 1030)
BN_CASES = [(64, 2), (64, 12), (8, 1001), (32, 2 * 4 * 4 * 6), (64, 130), (8, 1030)]


def bn_rows(C, M):
    """name -> row: the first row, the last valid row of the last block, and both sides of the boundary between two
    blocks (rows_per_block); where M has one block only, of the boundary between a thread's rows j and j + 1 (row R)"""
    geo = BR.geometry(C, M)
    rows = {"first": 0, "last": M - 1}
    edge = geo["RPB"] if M > geo["RPB"] else geo["R"] if M > geo["R"] else None
    if edge is not None:
        rows["row%d" % (edge - 1)], rows["row%d" % edge] = edge - 1, edge
    return rows


def bn_channels(C):
    """channels of the NaN, +inf, -inf in y and of the non-finite skip and grad_out elements (these two share a
    channel: the skip reaches `out` only, grad_out the gradients only): four of C >= 8, in different channel groups
    where C allows; the other channels, at least half, stay clean in every output"""
    step, off = C // 8, (1 if C > 8 else 0)
    return dict(nan=0, pinf=2 * step + off, ninf=4 * step + 2 * off, skip=7 * step + 3 * off, go=7 * step + 3 * off)


def bn_reference(y, p, relu, skip):
    """fp64 reference with the backward's mask as torch's select (module docstring) -> dict of fp64 arrays"""
    f = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    with np.errstate(all="ignore"):
        ref = BR.reference(f(y), f(p["gamma"]), f(p["beta"]), f(p["skip"]) if skip else None, f(p["rm"]), f(p["rv"]),
                           relu=relu)
        M = ref["M"]
        g = np.where(ref["pre"] <= 0, 0.0, f(p["go"])) if relu else f(p["go"])
        gb, gg = g.sum(0), (g * ref["xhat"]).sum(0)
        gy = f(p["gamma"]) * ref["invstd"] * (g - gb / M - ref["xhat"] * (gg / M))
    return dict(out=ref["out"], mean=ref["mean"], invstd=ref["invstd"], rm=ref["rm"], rv=ref["rv"], grad_y=gy,
                grad_gamma=gg, grad_beta=gb)


def bn_case(C, M, row_name, relu, skip, rot=0, seed=7):
    """One forward + backward: y holds NaN, +inf and -inf at one row in three channels (rotated by `rot`), the skip one
    non-finite element in a fourth, grad_out one there too and a NaN in the channel of y's first value.  -> dict(inj, clean: y, p; ref, spread, bound)."""
    row = bn_rows(C, M)[row_name]
    y = BR.field("normal", C, M, seed + C + M)
    p = BR.params(C, M, seed + C + M, skip=True, running=True)
    ch = bn_channels(C)
    yi, pi = y.copy(), {k: (None if v is None else v.copy()) for k, v in p.items()}
    vals = [VALUES[(k + rot) % 3][1] for k in range(3)]
    yi[row, ch["nan"]], yi[row, ch["pinf"]], yi[row, ch["ninf"]] = vals
    pi["skip"][row, ch["skip"]] = vals[1]
    pi["go"][row, ch["go"]] = vals[2]
    pi["go"][(row + 1) % M, ch["nan"]] = np.nan       # passes the ReLU of the lost channel: grad_beta there is NaN
    ref = bn_reference(yi, pi, relu, skip)
    dead_f = np.zeros(C, bool)
    dead_f[[ch["nan"], ch["pinf"], ch["ninf"]]] = True
    dead_b = dead_f.copy()
    dead_b[ch["go"]] = True
    out_spread = np.broadcast_to(dead_f[None], (M, C)).copy()
    if skip:
        out_spread[row, ch["skip"]] = True
    spread = dict(out=out_spread, mean=dead_f, invstd=dead_f, rm=dead_f, rv=dead_f,
                  grad_y=np.broadcast_to(dead_b[None], (M, C)), grad_gamma=dead_b, grad_beta=dead_b)
    f = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    sk = f(p["skip"]) if skip else None
    cref = BR.reference(f(y), f(p["gamma"]), f(p["beta"]), sk, f(p["rm"]), f(p["rv"]), relu=relu, go=f(p["go"]))
    b = BR.bounds(cref, f(y), f(p["gamma"]), f(p["beta"]), sk, f(p["rm"]), f(p["rv"]), go=f(p["go"]))
    # a channel lost in the forward passes every grad_out: its grad_beta is the sum the relu = 0 backward forms, and
    # takes that backward's bound where it is the larger one
    open_ = BR.bounds(BR.reference(f(y), f(p["gamma"]), f(p["beta"]), sk, relu=False, go=f(p["go"])), f(y), f(p["gamma"]),
                      f(p["beta"]), sk, go=f(p["go"]))
    bound = dict(out=b["out"], mean=b["mean"], invstd=b["rho_is"] * cref["invstd"], rm=b["rm"], rv=b["rv"],
                 grad_y=b["grad_y"], grad_gamma=b["grad_gamma"], grad_beta=np.maximum(b["grad_beta"], open_["grad_beta"]))
    return dict(name="bn/C%d_M%d/%s/relu%d_skip%d" % (C, M, row_name, relu, skip), inj=dict(y=yi, p=pi),
                clean=dict(y=y, p=p), ref=ref, spread=spread, bound=bound, relu=relu, skip=skip,
                clean_channels=1.0 - float((dead_b | (np.arange(C) == ch["skip"])).mean()))


def bn_emulate(y, p, relu, skip, defects=()):
    """bn3d_ref's fp32 emulation of the forward, then of the backward fed with that forward's statistics"""
    with np.errstate(all="ignore"):
        fw = BR.emulate_forward(y, p["gamma"], p["beta"], p["skip"] if skip else None, p["rm"], p["rv"], relu=relu,
                                defects=defects)
        bw = BR.emulate_backward(y, p["go"], p["gamma"], p["beta"], fw["mean"], fw["invstd"], relu=relu)
    return dict(out=fw["out"], mean=fw["mean"], invstd=fw["invstd"], rm=fw["rm"], rv=fw["rv"], grad_y=bw["grad_y"],
                grad_gamma=bw["grad_gamma"], grad_beta=bw["grad_beta"])


# ---------------------------------------------------------------------------------------------------------------
# soft-argmin backward
# ---------------------------------------------------------------------------------------------------------------
SOFTARGMIN_D = (1, 2, 9, 48)
SOFTARGMIN_P = (1, 127, 128, 129, 300)          # the 128-thread block boundary
SOFTARGMIN_KINDS = ("nan_logit", "+inf_logit", "-inf_all", "nan_gd", "+inf_gd", "-inf_gd", "-inf_single")


def softargmin_pixels(P_):
    """the first and the last pixel, both sides of every 128-thread block boundary, one interior"""
    pix = [0, P_ - 1] + [q for b in range(128, P_, 128) for q in (b - 1, b)] + [P_ // 2 + 1]
    return [q for q in dict.fromkeys(pix) if 0 <= q < P_]


def softargmin_case(D, P_, rot):
    """-> dict(inj, clean: cost [D,P], dv [D], gd [P]; ref, spread, bound for "gc" [D,P]).  Pixel k of
    softargmin_pixels holds kind (k + rot) % 7."""
    cost = SR.logits("gain3", D, P_, 7000 + 13 * D + P_)
    dv = SR.depth_axis("dtu", D)
    gd = np.random.default_rng(D * 1000 + P_).standard_normal(P_).astype(F32)
    ci, gi = cost.copy(), gd.copy()
    spread = np.zeros(P_, bool)
    single = []
    for k, q in enumerate(softargmin_pixels(P_)):
        kind = SOFTARGMIN_KINDS[(k + rot) % len(SOFTARGMIN_KINDS)]
        spread[q] = True
        d = 0 if k % 2 == 0 else (3 * k + 1) % D       # every other pixel: the first logit a loop meets
        if kind == "nan_logit":
            ci[d, q] = np.nan
        elif kind == "+inf_logit":
            ci[d, q] = np.inf
        elif kind == "-inf_all":
            ci[:, q] = -np.inf
        elif kind == "-inf_single":
            ci[d, q] = -np.inf
            if D > 1:
                single.append(q)
        else:
            gi[q] = dict(nan_gd=np.nan)[kind] if kind == "nan_gd" else (np.inf if kind == "+inf_gd" else -np.inf)
    with np.errstate(all="ignore"):
        c = ci.astype(np.float64)
        e = np.exp(c - c.max(0))
        p = e / e.sum(0)
        depth = (p * dv.astype(np.float64)[:, None]).sum(0)
        ref = gi.astype(np.float64)[None] * p * (dv.astype(np.float64)[:, None] - depth[None])
    bound = np.zeros((D, P_))       # non-zero only where a bound is needed: the single -inf pixels
    if single:
        cs = np.where(np.isneginf(ci[:, single]), F32(-1e5), ci[:, single])     # a term of exactly 0 in fp64 as well
        bound[:, single] = SR.reference(cs, dv, gi[single])["grad_bound"]
    return dict(name="softargmin_bwd/D%d_P%d/rot%d" % (D, P_, rot), inj=dict(cost=ci, dv=dv, gd=gi),
                clean=dict(cost=cost, dv=dv, gd=gd), ref={"gc": ref}, spread={"gc": np.broadcast_to(spread[None], (D, P_))},
                bound={"gc": bound}, finite={"gc": np.broadcast_to(np.isin(np.arange(P_), single)[None], (D, P_))},
                single=single)
