"""fp64 reference, single-product probes, derived bounds and the shape list for FeatureNet's kernels (csrc/featnet.hip).

Shared by tests/test_featnet_ref_host.py (CPU), tests/featnet_check.py (the GPU child) and the size-guard test.
Pure numpy; nothing here touches the GPU or the library.

Reference: one block in the reference's own form -- conv (fp64 sums of the fp32 inputs and fp32 weights), eval BatchNorm
with the fp32 parameters `(y - mean) / sqrt(var + eps) * gamma + beta` evaluated in fp64, ReLU; the last layer is
conv + bias -- and the chain of the eight blocks.

Dense bound.  The library folds BatchNorm on the host in fp32 (mvs_pack_feature_weights, restated in `fold32`):
    scale = fl(g / fl(sqrt(fl(v + eps))))   w_fold = fl(w scale)   shift = fl(b - fl(m scale))
and the kernels add K = 8 ceil(Cin/8) * 2 ceil(k k/2) products serially in fp32 on the MFMA (`analytic_k`: 80 in conv0 /
conv1, 208 conv2, 160 conv3 / conv4, 416 conv5, 320 conv6 / feature), then the shift.  With u = 2^-24 and
    S  = conv(|x|, |w_fold|) + |shift|,       SF = conv(|x|, |w_fold|) + |b| + |m scale|   (>= S)
the bound on |got - ref64| is
    dense_c u S  +  FOLD_C u SF.
First term: the kernel against the exact value of its own folded operands; worst case K u S, `dense_c` below.
Second term, the fold against the unfolded fp64 form: v + eps, the square root and the division round once each
(the rounded sum enters the root, which halves its relative error, and float(1e-5) is within u of 1e-5), so scale is off
by at most (1/2 + 1/2 + 1 + 1) u = 3 u relatively; w scale rounds once more -> every folded weight within 4 u, every
product within 4 u |x w_fold|; m scale within 4 u |m scale|, and the subtraction rounds once: u |shift| <= u (|b| +
|m scale|).  Together <= 5 u SF, FOLD_C = 5 (second-order terms are below 1e-6 of that).  ReLU is 1-Lipschitz.

Chained bound (the fused conv0 + conv1 kernel, the whole net): E_0 = 0 on the image,
    E_{l+1} = conv(E_l, |w_fold_{l+1}|) + c_{l+1} u S_{l+1} + FOLD_C u SF_{l+1},
with S and SF taken on |x_ref| + E_l, so that the scale of what the kernel really read is covered.  c = dense_c for the
MFMA kernels; the fused kernel's conv0 half runs on the VALU: 27 FMAs from the shift, one rounding each, so
|a_27 - exact| <= 27 u S rigorously (gamma_27), FUSED_C0 = 27 -- derived from that chain, not taken from the MFMA layers.
Every propagation multiplies E by the next layer's weight mass (about 2.5, 4.4, 7, 6, 6, 10, 8.4, 8.5 for the seed-0
weights), a worst case no real input meets: after one layer (the fused kernel) the bound is still sharp enough to see a
wrong tile edge, after eight it is about 1e7 times the error observed (REFERENCE_WORST).  The whole net is therefore
ALSO held bit-equal to the composition of the separately bounded launches (fused kernel, then mvs_feature_layer 2..7):
it is the same kernels on the same buffers, so nothing but bit equality is right.

Probes (every output one product at most, so no summation-order tolerance: PROBE_ULPS ulp32 of |x w| + |shift|, from
tests/probes.py, against the exact value of the FOLDED operands):
  lattice    -- one nonzero pixel per lattice cell in one pseudo-random channel, dense folded weights; spacing 3 for
                the k3 layers, 5 for the k5 stride-2 layers (an output reads 5 consecutive inputs per dimension).  All
                phases together put a nonzero into every pixel and pair every (ci, tap) with every co.  Exists for:
                a dropped or misplaced tap, a wrong (ci, tap, co) route in the panel packing, the swapped channel halves
                `(g & 1) * 4`, a wrong chunk rotation, a wrong epilogue scatter, halo / tile-edge errors.
  crafted    -- the fused kernel: a dense positive image, conv0 an exact copy of R, G or B (identity BatchNorm, one
                centre-tap weight 1.0), conv1 one nonzero weight (ci, tap) per output channel.  Variant "shift" gives
                conv0 a positive shift: a padding ring holding ReLU(shift0) instead of 0 then shows at the border.
  padded tap -- one lattice phase with |x| ~ 2^100 and |w_fold| ~ 2^-100: the kernels' last k-step multiplies the voxel
                under the last tap a second time (tap 25 of the k5 layers, tap 9 of the k3 layers) and relies on a
                packed weight of exactly 0, as do the channels >= Cin of conv0's only chunk; any residue shows.
The dense bound exists for what no probe sees: accumulation precision and anything value-dependent.
"""
import itertools

import numpy as np

U = 2.0 ** -24
PROBE_ULPS = 2          # as tests/probes.py (test_featnet_ref_host.py asserts they are equal)
FOLD_C = 5              # derived above
FUSED_C0 = 27           # derived above
# Dense constant of the MFMA layers.  Starts from DENSE_C = 64 of tests/probes.py (below every layer's analytic K); rule:
# kept while the worst measured |got - ref64| / (u S) on the GPU over all CASES x families is under half of it, otherwise
# twice the measured worst, never above analytic_k(layer).  Measured worst ratio against the whole bound (MI355X), per
# kernel: see MEASURED below.
DENSE_C = 64
BN_EPS = 1e-5

# (cin, cout, k, stride) of conv0..conv6 and `feature`; (BY, BX) block tile in MFMA tiles of 2 x 8 output pixels
# (launch_feature_layer in csrc/featnet.hip).  test_featnet_ref_host.py asserts LAYERS against _lib.FEATURE_LAYERS and
# the tiles against the source text.
LAYERS = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1),
          (32, 32, 3, 1))
BLOCK = ((4, 4), (4, 4), (2, 4), (2, 4), (2, 4), (2, 2), (2, 2), (2, 2))
FUSED = "fused"         # kernel key of fconv01_fused_kernel: image -> conv1's output, block tile 8 x 32
KERNELS = tuple(range(8)) + (FUSED,)
FORMATS = ("f32_chw", "u8_chw", "u8_hwc")

# worst |got - ref64| / bound measured on the MI355X over every CASES shape x input family (featnet_check.py prints
# them); the reference's own fp32 output against the chained bound is REFERENCE_WORST (test_featnet_ref_host.py).
MEASURED = {}           # NOT MEASURED YET: no MI355X run of featnet_check.py has been recorded; DENSE_C is the rule's start value
REFERENCE_WORST = 5.5e-8     # tiny fixture; small, n5yaw 4.4e-8, b2 3.4e-8, ragged oracle case below those


def tile(kernel):
    """output pixels (rows, columns) of one workgroup"""
    by, bx = (4, 4) if kernel == FUSED else BLOCK[kernel]
    return 2 * by, 8 * bx


def analytic_k(layer):
    ci, _, k, _ = LAYERS[layer]
    return 8 * ((ci + 7) // 8) * 2 * ((k * k + 1) // 2)


def out_size(n, stride):
    return (n - 1) // stride + 1


def receptive_field():
    """image pixels per feature pixel and dimension, and the feature stride, from LAYERS"""
    r, j = 1, 1
    for _, _, k, s in reversed(LAYERS):
        r = (r - 1) * s + k
        j *= s
    return r, j


# ---- parameters ------------------------------------------------------------------------------------------------------
def fstate(weights):
    """state dict of the whole model -> names relative to `feature.`"""
    return {k[len("feature."):]: np.asarray(v) for k, v in weights.items() if k.startswith("feature.")}


def raw(st, layer):
    """(w, (g, b, m, v) or None, bias or None) of layer 0..7, fp32"""
    if layer == 7:
        return np.asarray(st["feature.weight"], np.float32), None, np.asarray(st["feature.bias"], np.float32)
    bn = tuple(np.asarray(st[f"conv{layer}.bn.{q}"], np.float32) for q in ("weight", "bias", "running_mean", "running_var"))
    return np.asarray(st[f"conv{layer}.conv.weight"], np.float32), bn, None


def fold32(st, layer):
    """(w_fold, shift, fold_abs) as mvs_pack_feature_weights computes them in fp32; fold_abs = |b| + |m scale|"""
    w, bn, bias = raw(st, layer)
    if bn is None:
        return w, bias, np.abs(bias).astype(np.float64)
    g, b, m, v = bn
    scale = (g / np.sqrt((v + np.float32(BN_EPS)).astype(np.float32)).astype(np.float32)).astype(np.float32)
    ms = (m * scale).astype(np.float32)
    shift = (b - ms).astype(np.float32)
    return (w * scale[:, None, None, None]).astype(np.float32), shift, np.abs(b).astype(np.float64) + np.abs(ms)


def identity_var():
    """running_var with float32(var) + float32(1e-5) == 1.0: the packer's scale is then exactly gamma"""
    v = np.float32(1.0 - 1e-5)
    for _ in range(64):
        s = np.float32(v) + np.float32(BN_EPS)
        if s == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0) if s < 1 else np.float32(0.0), dtype=np.float32)
    raise AssertionError("no running_var gives scale 1.0")


def with_folded(st, layer, wf, shift):
    """copy of `st` whose layer folds EXACTLY to (wf, shift): identity BatchNorm (gamma 1, mean 0, identity_var), beta =
    shift; layer 7 takes them as weight and bias"""
    st = dict(st)
    wf, shift = np.asarray(wf, np.float32), np.asarray(shift, np.float32)
    if layer == 7:
        st["feature.weight"], st["feature.bias"] = wf, shift
        return st
    co = wf.shape[0]
    st[f"conv{layer}.conv.weight"] = wf
    st[f"conv{layer}.bn.weight"] = np.ones(co, np.float32)
    st[f"conv{layer}.bn.bias"] = shift
    st[f"conv{layer}.bn.running_mean"] = np.zeros(co, np.float32)
    st[f"conv{layer}.bn.running_var"] = np.full(co, identity_var(), np.float32)
    return st


# ---- fp64 reference --------------------------------------------------------------------------------------------------
def conv64(x, w, stride):
    """x [N,C,H,W], w [Co,Ci,k,k] -> [N,Co,Ho,Wo] in fp64, zero padding k // 2: one matrix product per tap"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    N, C, H, W = x.shape
    co, ci, k, _ = w.shape
    assert ci == C
    p = k // 2
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = np.zeros((C, N, H + 2 * p, W + 2 * p))
    xp[:, :, p:p + H, p:p + W] = x.transpose(1, 0, 2, 3)
    y = np.zeros((co, N * Ho * Wo))
    for ky in range(k):
        for kx in range(k):
            patch = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            y += w[:, :, ky, kx] @ patch.reshape(C, -1)
    return y.reshape(co, N, Ho, Wo).transpose(1, 0, 2, 3)


def _c(v):
    return np.asarray(v, np.float64)[None, :, None, None]


def block64(st, layer, x):
    """one block in the reference's form, fp64 of the fp32 parameters"""
    w, bn, bias = raw(st, layer)
    y = conv64(x, w, LAYERS[layer][3])
    if bn is None:
        return y + _c(bias)
    g, b, m, v = bn
    return np.maximum((y - _c(m)) / np.sqrt(_c(v) + BN_EPS) * _c(g) + _c(b), 0.0)


def chain64(st, x, first=0, last=7):
    for l in range(first, last + 1):
        x = block64(st, l, x)
    return x


def folded64(st, layer, x):
    """the layer on the library's folded operands, exact: relu(conv(x, w_fold) + shift) (layer 7: no ReLU)"""
    wf, sh, _ = fold32(st, layer)
    y = conv64(x, wf, LAYERS[layer][3]) + _c(sh)
    return y if layer == 7 else np.maximum(y, 0.0)


def scale64(st, layer, x_abs):
    """(S, SF) of the module docstring for |x| = x_abs (fp64, >= 0)"""
    wf, sh, fa = fold32(st, layer)
    a = conv64(x_abs, np.abs(wf), LAYERS[layer][3])
    return a + _c(np.abs(sh)), a + _c(fa)


def dense_ref_bound(st, layer, x, c=None):
    """(ref64, bound) of one layer on fp32 input x"""
    S, SF = scale64(st, layer, np.abs(np.asarray(x, np.float64)))
    return block64(st, layer, x), (DENSE_C if c is None else c) * U * S + FOLD_C * U * SF


def chain_ref_bound(st, x, first=0, last=7, consts=None):
    """(ref64, E) of layers first..last on fp32 input x (exact: E_0 = 0); consts[l] overrides DENSE_C for layer l"""
    ref = np.asarray(x, np.float64)
    E = np.zeros_like(ref)
    for l in range(first, last + 1):
        wf = np.abs(fold32(st, l)[0])
        N = ref.shape[0]
        both = conv64(np.concatenate([np.abs(ref) + E, E]), wf, LAYERS[l][3])
        _, sh, fa = fold32(st, l)
        c = DENSE_C if consts is None or l not in consts else consts[l]
        E = both[N:] + c * U * (both[:N] + _c(np.abs(sh))) + FOLD_C * U * (both[:N] + _c(fa))
        ref = block64(st, l, ref)
    return ref, E


def fused_ref_bound(st, img):
    """(ref64, E) of the fused conv0 + conv1 kernel on an fp32 image"""
    return chain_ref_bound(st, img, 0, 1, consts={0: FUSED_C0})


def ulp32(s):
    return np.spacing(np.maximum(np.abs(s), 2.0 ** -126).astype(np.float32)).astype(np.float64)


def probe_want_bound(st, layer, x):
    """(want, bound) of a probe launch of one layer: the exact value of the folded operands, PROBE_ULPS ulp32(S)"""
    return folded64(st, layer, x), PROBE_ULPS * ulp32(scale64(st, layer, np.abs(np.asarray(x, np.float64)))[0])


def ratio(got, ref, bound):
    """worst |got - ref| / bound; inf where got is not finite or the bound is 0 and the values differ"""
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape:
        return float("inf")
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- inputs ----------------------------------------------------------------------------------------------------------
def families(kernel):
    return ("normal", "heavy", "unit", "u8") if kernel in (0, FUSED) else ("normal", "heavy")


def make_input(kernel, family, N, H, W, seed):
    """fp32 [N,Cin,H,W] (family "u8": uint8 [N,3,H,W]; its fp32 value is `u8_to_f32`)"""
    rng = np.random.default_rng(seed)
    ci = 3 if kernel == FUSED else LAYERS[kernel][0]
    shape = (N, ci, H, W)
    if family == "normal":
        return rng.standard_normal(shape).astype(np.float32)
    if family == "heavy":      # exp(3 N(0,1)) with a random sign, as tests/test_gpu_fullsize.py uses for volumes
        return (np.exp(3.0 * rng.standard_normal(shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if family == "unit":
        return rng.random(shape, dtype=np.float32)
    if family == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    raise ValueError(family)


def u8_to_f32(u8):
    """the loader's `np.array(img, dtype=np.float32) / 255.` (one IEEE division in fp32)"""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)


# ---- probes ----------------------------------------------------------------------------------------------------------
# per-layer probe shape (N, H, W): several block tiles in y and x, ragged at both ends, odd sizes for the stride-2 layers
PROBE_SHAPE = {0: (2, 19, 70), 1: (2, 19, 70), 2: (2, 21, 131), 3: (2, 11, 70), 4: (2, 11, 70), 5: (2, 21, 67),
               6: (2, 11, 37), 7: (2, 11, 37), FUSED: (2, 19, 70)}


def spacing(layer):
    return LAYERS[layer][2]        # 3 for k3 stride 1; 5 for k5 stride 2: the inputs one output reads per dimension


def phases(layer):
    return list(itertools.product(range(spacing(layer)), repeat=2))


def lattice(layer, shape, phase, rng, magnitude=None):
    """one nonzero pixel per lattice cell in one pseudo-random channel; standard normal, or +-2^magnitude (1 + r)"""
    N, H, W = shape
    sp = spacing(layer)
    x = np.zeros((N, LAYERS[layer][0], H, W), np.float32)
    ys, xs = np.arange(phase[0], H, sp), np.arange(phase[1], W, sp)
    n, Y, X = np.meshgrid(np.arange(N), ys, xs, indexing="ij")
    ch = rng.integers(0, LAYERS[layer][0], n.shape)
    if magnitude is None:
        v = rng.standard_normal(n.shape)
    else:
        v = (1 + rng.random(n.shape)) * 2.0 ** magnitude * rng.choice([-1.0, 1.0], n.shape)
    x[n, ch, Y, X] = v
    return x


def padded_tap_state(st, layer, rng):
    """folded weights of magnitude 2^-100 (random sign and mantissa), shift 0"""
    co, ci, k, _ = (LAYERS[layer][1], LAYERS[layer][0], LAYERS[layer][2], 0)
    w = ((1 + rng.random((co, ci, k, k))) * 2.0 ** -100 * rng.choice([-1.0, 1.0], (co, ci, k, k))).astype(np.float32)
    return with_folded(st, layer, w, np.zeros(co, np.float32))


def crafted_image(shape, rng):
    """dense positive uint8 [N,3,H,W] in 1..255"""
    N, H, W = shape
    return rng.integers(1, 256, (N, 3, H, W), dtype=np.uint8)


CRAFTED_RUNS = 9            # 8 output channels x 9 runs = the 72 (ci, tap) pairs of conv1
CRAFTED_SHIFT0 = np.float32(0.25)


def crafted_state(st, run, variant, rng):
    """conv0: identity BatchNorm, centre-tap weight 1.0 from input channel co % 3 -> output channel co; shift0 = 0
    ("copy") or CRAFTED_SHIFT0 ("shift").  conv1: identity BatchNorm, shift 0, ONE nonzero weight per output channel at
    (ci, tap) = divmod((co + 8 run) % 72, 9).  Returns (state, conv0's exact output as a function of the fp32 image)."""
    w0 = np.zeros((8, 3, 3, 3), np.float32)
    for co in range(8):
        w0[co, co % 3, 1, 1] = 1.0
    s0 = np.full(8, CRAFTED_SHIFT0 if variant == "shift" else 0.0, np.float32)
    w1 = np.zeros((8, 8, 3, 3), np.float32)
    for co in range(8):
        ci, tap = divmod((co + 8 * run) % 72, 9)
        w1[co, ci, tap // 3, tap % 3] = np.float32(1 + rng.random())      # positive: the ReLU passes the product
    st = with_folded(with_folded(st, 0, w0, s0), 1, w1, np.zeros(8, np.float32))

    def conv0_exact(img32):     # fma(x, 1.0, shift0) rounds once: fl(x + shift0); x > 0 so the ReLU is the identity
        return (img32[:, [co % 3 for co in range(8)]] + s0[None, :, None, None]).astype(np.float32)
    return st, conv0_exact


def crafted_want_bound(st, img32, conv0_exact):
    """every conv1 output of the crafted probe is one exact product of conv0's exact copy (zero outside the image)"""
    return probe_want_bound(st, 1, conv0_exact(img32))


# ---- the MFMA order restated in numpy (fp32, serial): the CPU suite's stand-in for the kernels, and its mutations -------
def pack_panels(wf):
    """pack_fconv_weights: w [co][ci][k][k] -> bp [NCH][NT][KS][64 lanes][4]; lane = 16 g + n: tap = 2 ks + (g >> 1),
    ci = 8 c + 4 (g & 1) + j4, co = 16 t + n; 0 where tap, ci or co is past the end"""
    co_n, ci_n, k, _ = wf.shape
    taps = k * k
    nch, nt, ksn = (ci_n + 7) // 8, (co_n + 15) // 16, (taps + 1) // 2
    w = np.asarray(wf, np.float32).reshape(co_n, ci_n, taps)
    bp = np.zeros((nch, nt, ksn, 64, 4), np.float32)
    for c, t, ks, lane, j4 in itertools.product(range(nch), range(nt), range(ksn), range(64), range(4)):
        g, n = lane >> 4, lane & 15
        tap, ci, co = 2 * ks + (g >> 1), 8 * c + 4 * (g & 1) + j4, 16 * t + n
        if tap < taps and ci < ci_n and co < co_n:
            bp[c, t, ks, lane, j4] = w[co, ci, tap]
    return bp


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_layer(st, layer, x, mutation=None, prepadded=False):
    """fconv_mfma_kernel in fp32 numpy: acc += a b serially over (chunk, k-step, j4, lane group g), the padded tap read
    from the clamped LDS offset, then + shift (and ReLU).  `prepadded`: x already carries conv's zero ring (the fused
    kernel's conv1 half).  mutation: ("drop_tap", tap) zeroes that tap's packed weights, "swap_halves" reads the other
    channel half, ("residue", v) leaves v in the padded panel slots.  Two more show on non-finite input only
    (tests/test_nonfinite_train_host.py): ("relu_drops_nan",) is the ReLU as fmaxf(v, 0), whose NaN is 0;
    ("mask_by_multiply",) fills the out-of-image halo with the clamped load of the view's first pixel times 0 instead
    of a selected 0."""
    ci_n, co_n, k, s = LAYERS[layer]
    wf, sh, _ = fold32(st, layer)
    bp = pack_panels(wf)
    nch, nt, ksn = bp.shape[:3]
    taps, p = k * k, k // 2
    if mutation and mutation[0] == "drop_tap":
        for ks, g in itertools.product(range(ksn), range(4)):
            if 2 * ks + (g >> 1) == mutation[1]:
                bp[:, :, ks, 16 * g:16 * g + 16, :] = 0
    if mutation and mutation[0] == "residue":
        for ks, g in itertools.product(range(ksn), range(4)):
            if 2 * ks + (g >> 1) >= taps:
                bp[:, :, ks, 16 * g:16 * g + 16, :] = mutation[1]
    x = np.asarray(x, np.float32)
    N = x.shape[0]
    if prepadded:
        H, W = x.shape[2] - 2 * p, x.shape[3] - 2 * p
        xp = np.zeros((N, 8 * nch) + x.shape[2:], np.float32)
        xp[:, :ci_n] = x
    else:
        H, W = x.shape[2:]
        xp = np.zeros((N, 8 * nch, H + 2 * p, W + 2 * p), np.float32)
        if mutation == ("mask_by_multiply",):
            with np.errstate(invalid="ignore"):
                xp[:, :ci_n] = x[:, :, :1, :1] * np.float32(0)
        xp[:, :ci_n, p:p + H, p:p + W] = x
    Ho, Wo = out_size(H, s), out_size(W, s)
    acc = np.zeros((N, 16 * nt, Ho, Wo), np.float32)
    for c, ks, j4, g in itertools.product(range(nch), range(ksn), range(4), range(4)):
        tap = min(2 * ks + (g >> 1), taps - 1)
        half = (g & 1) ^ 1 if mutation and mutation[0] == "swap_halves" else g & 1
        ky, kx = divmod(tap, k)
        a = xp[:, 8 * c + 4 * half + j4, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
        b = bp[c, :, ks, 16 * g:16 * g + 16, j4].reshape(-1)
        acc = _fma32(a[:, None], b[None, :, None, None], acc)
    y = (acc[:, :co_n] + sh[None, :, None, None]).astype(np.float32)
    return y if layer == 7 else (np.fmax if mutation == ("relu_drops_nan",) else np.maximum)(y, np.float32(0))


def emulate_fused(st, img32, mutation=None):
    """fconv01_fused_kernel: conv0 as 27 serial fp32 FMAs from the shift on conv1's halo (the image grown by one pixel),
    ReLU, the halo pixels outside the image set to 0 -- mutation "ring": left as computed, i.e. ReLU(shift0) -- then
    conv1 in the MFMA order.  ("relu_drops_nan",): both ReLUs as fmaxf(v, 0)."""
    w0, s0, _ = fold32(st, 0)
    img32 = np.asarray(img32, np.float32)
    N, _, H, W = img32.shape
    ip = np.zeros((N, 3, H + 4, W + 4), np.float32)
    ip[:, :, 2:2 + H, 2:2 + W] = img32
    a = np.broadcast_to(s0[None, :, None, None], (N, 8, H + 2, W + 2)).astype(np.float32)
    for c, ky, kx in itertools.product(range(3), range(3), range(3)):
        a = _fma32(ip[:, c, None, ky:ky + H + 2, kx:kx + W + 2], w0[None, :, c, ky, kx, None, None], a)
    a = (np.fmax if mutation == ("relu_drops_nan",) else np.maximum)(a, np.float32(0))
    if mutation != ("ring",):
        inside = np.zeros((H + 2, W + 2), bool)
        inside[1:1 + H, 1:1 + W] = True
        a = np.where(inside[None, None], a, np.float32(0))
    return emulate_layer(st, 1, a, mutation=mutation if mutation == ("relu_drops_nan",) else None, prepadded=True)


# ---- shapes ----------------------------------------------------------------------------------------------------------
def _sizes(t, stride):
    """input sizes whose OUTPUT size is the minimum, tile - 1, tile, tile + 1 and 2 tiles + an odd remainder; for a
    stride-2 layer odd and even input sizes alternate (and both for the tile itself)"""
    outs = [t - 1, t, t + 1, 2 * t + 3]
    if stride == 1:
        return sorted({4, *(max(4, o) for o in outs)})      # check_image_dims refuses H or W < 4
    return sorted({4, 5, 2 * outs[0] - 1, 2 * outs[1], 2 * outs[1] - 1, 2 * outs[2], 2 * outs[3] - 1})


def workgroups(kernel, N, H, W):
    s = 1 if kernel == FUSED else LAYERS[kernel][3]
    th, tw = tile(kernel)
    return N * (-(-out_size(H, s) // th)) * (-(-out_size(W, s) // tw))


def _build_cases():
    """kernel -> [(N, H, W)] (input sizes).  Every H and every W of _sizes once (H list against the rotated W list, N
    cycling through 1, 2, 5), then the smallest further (N, H, W), taller images included, that adds a missing residue of the workgroup count
    tot % 8 among tot >= 8, and one tot < 8: the XCD re-deal `b = k q + min(k, rem) + (lin >> 3)` has a different shape
    for every residue."""
    cases = {}
    for kern in KERNELS:
        s = 1 if kern == FUSED else LAYERS[kern][3]
        th, tw = tile(kern)
        hs, ws = _sizes(th, s), _sizes(tw, s)
        n = max(len(hs), len(ws))
        got = [((1, 2, 5)[i % 3], hs[i % len(hs)], ws[(i + 2) % len(ws)]) for i in range(n)]
        more = [s * (m * th + 1) - (s - 1) * (m % 2) for m in range(3, 11)]     # 4..11 tile rows: residues 3 and 5 need a 7 or 11
        cand = sorted(((N, h, w) for N in (1, 2, 5) for h in hs + more for w in ws), key=lambda c: (workgroups(kern, *c), c))
        need = set(range(8)) - {workgroups(kern, *c) % 8 for c in got if workgroups(kern, *c) >= 8}
        for c in cand:
            t = workgroups(kern, *c)
            if t >= 8 and t % 8 in need and c not in got:
                got.append(c)
                need.discard(t % 8)
        if not any(workgroups(kern, *c) < 8 for c in got):
            got.append(cand[0])
        assert not need, (kern, need)
        cases[kern] = got
    return cases


CASES = _build_cases()

# whole-net shapes (N, H, W): ragged, a multiple of 32, and the benchmark's 5 x 512 x 640
NET_SHAPES = {"ragged": (2, 50, 70), "mult32": (2, 64, 96), "cfg2": (5, 512, 640)}
