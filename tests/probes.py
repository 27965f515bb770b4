"""Single-product probes and the dense fp64 bound for the CostRegNet conv kernels.

Shared by tests/probe_check.py (the GPU child) and tests/test_conv_probes_host.py (CPU).

Single-product probe: a sparse input in which every output receives at most ONE nonzero product, so the exact result
is known (fp64 of fp32 operands) and no summation-order tolerance is needed.  Two sets:
  lattice -- one nonzero voxel per lattice cell (one pseudo-random input channel), dense folded weights; the lattice
             spacing keeps two nonzero voxels out of every receptive field, all phases together probe every voxel;
  crafted -- every voxel nonzero and positive, one nonzero folded weight (ci, tap) per output channel, under an
             exact identity BN (scale 1.0, shift 0); every value has its 2nd and 3rd bf16 pieces near their largest
             magnitude, so a split-operand kernel that drops a2b2, a1b3 or a3b1 is off by >= 16 ulp in one direction.
Dense bound: |got - ref64| <= c 2^-24 S with S = conv(|x|, |w_fold|) + |shift| (+ |skip|), all in fp64.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as orc
from scene_3dreconstruction_mvsnet_amd import _lib

U = 2.0 ** -24          # unit roundoff of fp32
PROBE_ULPS = 2          # direct, MFMA and split forms: |got - want| <= 2 ulp32(S)
TAIL_ULPS = 4           # fused conv11 + prob: two chained single products
# direct, MFMA and split forms: |got - ref64| <= 64 * 2^-24 * S.  Not 16: an output of conv4 / conv6 sums 864 / 1,728
# products in fp32 (x 6 cross terms in the split forms), serially in the direct and fp32-MFMA kernels; on the
# heavy-tailed volume that measured 39 x 2^-24 S (convg conv4) and 44 x (direct conv6) on the GPU, 29 x in the exact
# numpy emulation of the split (test_conv_probes_host.py).
DENSE_C = 64
WINO_C = 4              # Winograd probes: |got - want| <= 4 * 2^-24 * (K |x| max|w_co| + |shift|)
WINO_DENSE_C = 4.2      # Winograd dense: 4.2 * 2^-24 (= 2.5e-7, test_gpu_conv0_tile) * local max|x| * weight mass

# layer -> (Cin, Cout, stride, transposed, probe input shape (D, H, W)).  Every shape is ragged in y and x for every
# tile of every form (odd output rows / columns, not a multiple of 8) and has several tiles in z; conv0 keeps D % 4 == 0
# (the Winograd F(4,3) forms), the stride-2 convolutions even input dims.
GEOM = {
    0: (32, 8, 1, False, (16, 13, 41)),
    1: (8, 16, 2, False, (16, 26, 42)),
    2: (16, 16, 1, False, (12, 13, 41)),
    3: (16, 32, 2, False, (16, 14, 42)),
    4: (32, 32, 1, False, (12, 13, 41)),
    5: (32, 64, 2, False, (8, 14, 26)),
    6: (64, 64, 1, False, (8, 7, 21)),
    7: (64, 32, 2, True, (4, 7, 13)),
    8: (32, 16, 2, True, (6, 7, 21)),
    9: (16, 8, 2, True, (8, 7, 21)),
    10: (8, 1, 1, False, (16, 13, 41)),
}
TAIL_SHAPE = (8, 7, 21)   # conv11_prob input (16 channels); skip and logits at twice the size

# Winograd along z.  F(4,3) (conv_winograd.hip header): U = B d, G g, m_t = U_t G_t, y = A m
F43_B = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                  [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
F43_G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                  [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
F43_A = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
# F(2,3): G = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2), y0 = m0 + m1 + m2, y1 = m1 - m2 - m3
F23_B = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
F23_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
F23_A = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
WINO = {"F43": (F43_A, F43_G, F43_B), "F23": (F23_A, F23_G, F23_B)}


def wino_gain(name):
    """K = max over output plane i and input plane l of sum_t |A_it| (sum_j |G_tj|) |B_tl|.

    Every transformed operand, product and partial sum of output i that carries the one nonzero voxel d_l (times one
    z column g of weights) is bounded by K |d_l| max|g|, and each of the O(1) fp32 roundings on the way errs by at most
    2^-24 of such a value; the transformed weights themselves are rounded once to fp32.  Hence the probe bound
    WINO_C 2^-24 (K |x| max|w_co| + |shift|)."""
    A, G, B = WINO[name]
    return float(max((np.abs(A[i]) * np.abs(G).sum(1) * np.abs(B[:, l])).sum()
                     for i in range(A.shape[0]) for l in range(B.shape[1])))


def wino_tile(name):
    """(output planes per tile m, input planes per tile m + 2)."""
    m = WINO[name][0].shape[0]
    return m, m + 2


def spacing(layer, wino=None):
    """Lattice spacing (z, y, x): 3 for the convolutions (a stride-2 output reads 3 consecutive inputs per dim too),
    2 for the transposed ones (an output reads at most 2 consecutive inputs per dim), the tile's z halo (m + 2 input
    planes) for a Winograd-along-z form: every transformed plane of a tile then carries at most one lattice plane."""
    if wino:
        return (wino_tile(wino)[1], 3, 3)
    return (2, 2, 2) if GEOM[layer][3] else (3, 3, 3)


def phases(sp):
    return list(itertools.product(*(range(s) for s in sp)))


def lattice(cin, shape, sp, phase, rng, values=None):
    """One nonzero voxel per lattice cell, in one pseudo-random channel; `values(n)` draws them (standard normal)."""
    x = np.zeros((cin,) + tuple(shape), np.float32)
    axes = [np.arange(p, n, s) for p, n, s in zip(phase, shape, sp)]
    Z, Y, X = np.meshgrid(*axes, indexing="ij")
    ch = rng.integers(0, cin, Z.shape)
    v = rng.standard_normal(Z.shape) if values is None else values(Z.shape)
    x[ch, Z, Y, X] = v
    return x


def crafted(shape, rng):
    """Positive fp32 values p1 + p2 + p3 with p1 = (1 + k/128) 2^e (bf16), p2 = 2^e (2^-8 - 2^-15) and
    p3 = 2^e (2^-17 - 2^-23): the 2nd and 3rd bf16 pieces just below half an ulp of the previous piece, i.e. near
    their largest magnitude (exact in fp32; the split is checked by test_crafted_values_split_as_designed)."""
    k = rng.integers(0, 128, shape).astype(np.float64)
    e = rng.integers(-2, 3, shape).astype(np.float64)
    v = (1 + k / 128 + 2.0 ** -8 - 2.0 ** -15 + 2.0 ** -17 - 2.0 ** -23) * 2.0 ** e
    out = v.astype(np.float32)
    assert (out.astype(np.float64) == v).all()
    return out


def split3(a):
    """The three bf16 pieces of fp32 values (RNE, as pack_split_panels and the kernels' staging)."""
    a = np.asarray(a, np.float32)
    p1 = orc.round_storage(a, "bf16")
    r = (a - p1).astype(np.float32)
    p2 = orc.round_storage(r, "bf16")
    p3 = orc.round_storage((r - p2).astype(np.float32), "bf16")
    return p1, p2, p3


def identity_var():
    """running_var with float32(var) + float32(1e-5) == 1.0: the packer's scale g / sqrt(var + eps) is exactly g."""
    v = np.float32(1.0 - 1e-5)
    for _ in range(64):
        s = np.float32(v) + np.float32(1e-5)
        if s == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0) if s < 1 else np.float32(0.0), dtype=np.float32)
    raise AssertionError("no running_var gives scale 1.0")


def crafted_runs(layer):
    """Runs needed to sweep all 27 taps: output channel co takes tap (co + r Cout) % 27 in run r."""
    return -(-27 // GEOM[layer][1])


def crafted_state(base, run, rng):
    """`base` with identity BN (gamma 1, beta 0, mean 0, identity_var) and, per layer and output channel, ONE nonzero
    weight (ci, tap) = ((5 co + run) % Cin, (co + run Cout) % 27) of crafted value; prob.weight has one nonzero entry
    (channel run % 8, tap run % 27) and prob.bias is 0."""
    sd = {k: np.array(v, np.float32, copy=True) for k, v in base.items()}
    v1 = identity_var()
    for l in range(10):
        ci_n, co_n, _, tr, _ = GEOM[l]
        key = _lib.CONV_WEIGHT_KEYS[l]
        w = np.zeros_like(sd[key])
        for co in range(co_n):
            ci, tap = (5 * co + run) % ci_n, (co + run * co_n) % 27
            idx = (ci, co) if tr else (co, ci)
            w[idx + np.unravel_index(tap, (3, 3, 3))] = crafted((), rng)
        sd[key] = w
        pre = _lib.BN_PREFIXES[l]
        sd[pre + ".weight"] = np.ones(co_n, np.float32)
        sd[pre + ".bias"] = np.zeros(co_n, np.float32)
        sd[pre + ".running_mean"] = np.zeros(co_n, np.float32)
        sd[pre + ".running_var"] = np.full(co_n, v1, np.float32)
    sd["prob.weight"] = single_prob_weight(run % 8, run % 27, crafted((), rng))
    sd["prob.bias"] = np.zeros(1, np.float32)
    return sd


def single_prob_weight(c, tap, value):
    w = np.zeros((1, 8, 3, 3, 3), np.float32)
    w[(0, c) + np.unravel_index(tap, (3, 3, 3))] = value
    return w


def folded(sd, layer):
    """(w_fold [Cout,Cin,3,3,3], shift [Cout]) fp32 as the blob holds them (orc._fold; layer 10: prob, no BN)."""
    if layer == 10:
        return np.asarray(sd["prob.weight"], np.float32), np.asarray(sd["prob.bias"], np.float32)
    return orc._fold(sd, _lib.CONV_WEIGHT_KEYS[layer], _lib.BN_PREFIXES[layer], transposed=GEOM[layer][3])


def _conv64(layer, x, w):
    X = torch.from_numpy(np.asarray(x, np.float64))[None]
    W = torch.from_numpy(np.asarray(w, np.float64))
    if GEOM[layer][3]:
        return F.conv_transpose3d(X, W.transpose(0, 1), stride=2, padding=1, output_padding=1)[0].numpy()
    return F.conv3d(X, W, stride=GEOM[layer][2], padding=1)[0].numpy()


def ref64(layer, x, wf, shift, skip=None):
    """fp64 layer of fp32 operands: relu(conv(x, wf) + shift) (+ skip); layer 10 without the ReLU."""
    y = _conv64(layer, x, wf) + np.asarray(shift, np.float64)[:, None, None, None]
    if layer != 10:
        y = np.maximum(y, 0.0)
    if skip is not None:
        y = y + skip
    return y


def scale64(layer, x, wf, shift, skip=None):
    """S = conv(|x|, |wf|) + |shift| (+ |skip|) in fp64."""
    s = _conv64(layer, np.abs(x), np.abs(wf)) + np.abs(np.asarray(shift, np.float64))[:, None, None, None]
    return s if skip is None else s + np.abs(skip)


def tail64(x, skip, w9, sh9, pw, pb):
    """conv11_prob in fp64: prob(relu(deconv(x, w9) + sh9) + skip) -> logits, and its scale S."""
    d11 = ref64(9, x, w9, sh9, skip)
    s11 = scale64(9, x, w9, sh9, skip)
    return ref64(10, d11, pw, pb)[0], scale64(10, s11, pw, pb)[0]


def ulp32(s):
    return np.spacing(np.maximum(np.abs(s), 2.0 ** -126).astype(np.float32)).astype(np.float64)


def ulp16(v, storage):
    a = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - (10 if storage == "f16" else 7))


def local_max(x, mz):
    """max over channels of |x| in the (mz, 3, 3) window around every voxel (same dims as x[0])."""
    m = torch.from_numpy(np.abs(x).max(axis=0).astype(np.float32))[None, None]
    return F.max_pool3d(m, kernel_size=(mz, 3, 3), stride=1, padding=(mz // 2, 1, 1))[0, 0].numpy().astype(np.float64)


def probe_want_bound(layer, x, skip, wf, sh, storage="f32", wino=None):
    """(want, bound) of one probe launch of layer 0..10 (every output one product at most).
    fp32: the fp64 value of the fp32 operands; bound PROBE_ULPS ulp32(S), or for a Winograd form
    WINO_C 2^-24 (K |x|_local max|w_co| + |shift|).  16-bit layers 0..9: round16 of the exact value of round16
    operands, within one storage ulp.  16-bit layer 10: 16-bit input, fp32 weights and logits."""
    q = lambda t: orc.round_storage(np.asarray(t, np.float32), storage)  # noqa: E731
    if storage == "f32":
        want = ref64(layer, x, wf, sh, skip)
        if wino:
            m = wino_tile(wino)[0]
            wmax = np.abs(wf).reshape(wf.shape[0], -1).max(1)[:, None, None, None]
            return want, WINO_C * U * (wino_gain(wino) * local_max(x, 2 * m + 1)[None] * wmax
                                       + np.abs(sh)[:, None, None, None])
        return want, PROBE_ULPS * ulp32(scale64(layer, x, wf, sh, skip))
    if layer == 10:
        return ref64(10, q(x), wf, sh), PROBE_ULPS * ulp32(scale64(10, q(x), wf, sh))
    want = q(ref64(layer, q(x), q(wf), sh, None if skip is None else q(skip))).astype(np.float64)
    return want, ulp16(want, storage)


def dense_ref_bound(layer, x, skip, wf, sh, storage="f32", wino=None):
    """(ref, bound) of a dense launch: |got - ref64| <= DENSE_C 2^-24 S (Winograd forms: WINO_DENSE_C 2^-24
    (|x|_local weight mass + |shift|)); 16-bit layers 0..9 additionally one storage ulp of the matched value."""
    q = lambda t: orc.round_storage(np.asarray(t, np.float32), storage)  # noqa: E731
    if storage == "f32":
        ref = ref64(layer, x, wf, sh, skip)
        if wino:
            m = wino_tile(wino)[0]
            wmass = np.abs(wf).reshape(wf.shape[0], -1).sum(1)[:, None, None, None]
            return ref, WINO_DENSE_C * U * (local_max(x, 2 * m + 1)[None] * wmass + np.abs(sh)[:, None, None, None])
        return ref, DENSE_C * U * scale64(layer, x, wf, sh, skip)
    if layer == 10:
        return ref64(10, q(x), wf, sh), DENSE_C * U * scale64(10, q(x), wf, sh)
    qs = None if skip is None else q(skip)
    ref = q(ref64(layer, q(x), q(wf), sh, qs)).astype(np.float64)
    return ref, ulp16(ref, storage) + DENSE_C * U * scale64(layer, q(x), q(wf), sh, qs)
