"""fp64 reference of the soft-argmin (softmax over depth, depth regression, photometric confidence) and of its backward,
derived per-pixel / per-element error bounds for the fp32 kernels, exact probes, the dense cases, and an fp32 numpy
emulation of the kernels' arithmetic with switchable defects.  Shared by tests/test_softargmin_ref_host.py (CPU) and
tests/test_gpu_softargmin_ref.py (GPU).

Written from models/mvsnet.py:192-218 and models/module.py:144-147, not from the kernels and without oracle/.  Plain
numpy, float64.  Per pixel:
    p = softmax(c)   depth = sum_d p_d dv_d   E = sum_d p_d d   idx = clip(trunc(E), 0, D-1)
    conf = sum_{k=-1..2} p_{idx+k} (zero outside [0, D))        grad_cost_d = gd p_d (dv_d - depth)

The bound, with u = 2^-24 (one fp32 rounding); every magnitude is the float64 reference's own value.  EXP_ULPS = 2 is
an ASSUMPTION, not a measurement: no copy of HIP's math-accuracy table is installed with the toolchain, so expf is
taken to be within 2 ulp = 4u relative.  1 / S is charged 1 ulp = 2u, like v_rcp_f32 in warp_ref.py (an IEEE division
is inside that).

Forward (csrc/softargmin.hip).  D is cut into NS slices of per = ceil(D / NS) depths; the launcher picks (PIX, NS) =
(32, 8) or (16, 16), and for D > 256 the looping form (NS = 16, online rescale).  One bound serves all seven launch
forms, so each term below is the larger of the two layouts, and the loop form's extra operations are counted from the
logits (R_d, exact: the number of times the running maximum of d's slice rises after d).
  term d of slice k reaches the merged sums as  expf(c_d - m_k) * expf(m_k - M)  (loop form: the same product built
  from R_d + 1 rescales, whose arguments telescope to m_k - c_d).  Each subtraction rounds once, and through exp a
  rounding u |x| of the argument is a relative error u |x| of the value:
      tau_c(d) = u (|c_d - m_k| + |m_k - M|) + 2 u EXP_ULPS (2 + R_d)            common to S, SD (depth) and SI (E)
  the sums: per fma / add roundings inside the slice, NS fmas in the merge, R_d rescale multiplies, each <= u times
  a partial sum of non-negative terms (K terms in any order: (K - 1) u Sigma):
      tau_s(d) = u (Ksum + R_d),   Ksum = max over layouts of (per + NS)         separate for S, SD, SI
  Sharper for peaked pixels: an add or fma into an accumulator errs by at most u |result| AND by at most its smaller
  operand (the larger operand is itself a candidate result), so the in-slice step of term t_i errs by <= min(u T, |t_i|)
  with T = sum |t|, and the merge step of a slice by <= min(u T, |slice sum|) <= sum over the slice of the same.  For a
  normalised sum of terms p_d x_d the roundings of both levels together are therefore
      A(x) = min( Ksum u T, 2 sum_d min(u T, p_d |x_d|) ),   T = sum_d p_d |x_d|
  and "sum p tau_s (|x| + |mean|)" below stands for  A(x) + |mean| A(1) + u sum_d p_d R_d (|x_d| + |mean|).
  a term below 2^-126 may be flushed: phi = 2^-126 (D + NS) / S absolute on every normalised sum (S >= 1).
      dS / S = sigma = sum_d p_d (tau_c + tau_s) + phi
  depth = SD * (1 / S): the common errors cancel against the mean, the separate ones do not; 1 / S 2u, the product u:
      d(depth) = 2 [ sum p tau_c |dv - depth| + sum p tau_s (|dv| + |depth|) + 3u |depth| + phi (max|dv| + |depth|) ]
      dE       = the same with d in place of dv_d ((float)d is exact)
  conf for a fixed idx: c4 = sum over the window of expf(c_d - M) (M the merged maximum, one subtraction, one expf),
  <= 3 adds inside the slices and one across them (4u), times inv (sigma + 2u) with one rounding (u):
      d(conf | idx) = 2 [ sum_win p_d (u |c_d - M| + 2 u EXP_ULPS) + conf (sigma + 7u) + 4 * 2^-126 / S ]
  Each first-order bound is doubled once for the second-order terms.

Truncation.  A pixel is ambiguous iff [E - dE, E + dE] holds an integer j, 1 <= j <= D - 1; there the kernel's
confidence must lie within d(conf | idx) of the window sum for idx = j or idx = j - 1; everywhere else for the single
idx = clip(trunc(E)).  At most MAX_AMBIGUOUS of a case's pixels may be ambiguous (asserted from fp64 alone).

Backward (softargmin_bwd_kernel): thread = pixel, M over all D, e_d = expf(c_d - M) (rho_e = u |c_d - M| +
2 u EXP_ULPS, the same value in all passes), S by D - 1 adds, SD by D fmas, inv = 1 / S, depth = SD * inv,
gi = gd * inv, grad = (e * gi) * (dv - depth):
      sigma_b = sum p rho_e + A_D(1) + 2^-126 D / S
      d1(depth) = sum p rho_e |dv - depth| + A_D(dv) + |depth| A_D(1) + 3u |depth| + 2^-126 D / S (max|dv| + |depth|)
                  (A_D: one level of D roundings, min(D u T, sum_d min(u T, p_d |x_d|)); sigma_b uses A_D(1) likewise)
      rho_d = rho_e(d) + sigma_b + 2u (1 / S) + 3u (gi, e * gi, the final product)
      |d grad_d| <= 2 |gd| p_d [ rho_d |dv_d - depth| + d1(depth) + u |dv_d| + u |dv_d - depth| ]
                    + 2 * 2^-126 (1 + (1 + |gd|) |dv_d - depth|)

Exact probes: background logit -200, K in {1, 2, 4} spikes at logit 0, integer dv, power-of-two gd.  expf(-200) = 0 and
expf(0) = 1 exactly, 1 / K is a power of two, every sum is a sum of small integers: depth, trunc(E), confidence and
grad_cost are known exactly and compared bit for bit.
"""
import numpy as np

from scene_3dreconstruction_mvsnet_amd import synthetic

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_ULPS = 2               # assumption (module docstring)
MAX_AMBIGUOUS = 0.01
LAYOUTS = ((32, 8), (16, 16))      # (PIX, NS) of softargmin_conf_kernel


def launch_form(D, hw):
    """launch_softargmin's choice -> (name, PIX, NS, MAXPER or None for the looping form)."""
    if hw >= 32 * 512 and D <= 256:
        per = (D + 7) // 8
        mp = 16 if per <= 16 else 24 if per <= 24 else 32
        return ("<%d,32,8>" % mp, 32, 8, mp)
    per = (D + 15) // 16
    if per <= 8:
        return ("<8,16,16>", 16, 16, 8)
    if per <= 16:
        return ("<16,16,16>", 16, 16, 16)
    return ("loop/hw>=16384" if hw >= 32 * 512 else "loop", 16, 16, None)


FORMS = ("<8,16,16>", "<16,16,16>", "loop", "<16,32,8>", "<24,32,8>", "<32,32,8>", "loop/hw>=16384")


# ---------------------------------------------------------------------------------------------------------------
# the reference and its bounds
# ---------------------------------------------------------------------------------------------------------------
def window(p, idx):
    """sum of p [D,P] over [idx - 1, idx + 2], zero outside [0, D)."""
    D = p.shape[0]
    out = np.zeros(idx.shape, np.float64)
    for k in (-1, 0, 1, 2):
        j = idx + k
        ok = (j >= 0) & (j < D)
        out += np.where(ok, np.take_along_axis(p, np.clip(j, 0, D - 1)[None], 0)[0], 0.0)
    return out


def _slice_max(c, NS):
    D, P = c.shape
    per = -(-D // NS)
    pad = np.full((NS * per, P), -np.inf)
    pad[:D] = c
    mk = pad.reshape(NS, per, P).max(1)
    return np.repeat(mk, per, axis=0)[:D], per


def _rescales(c):
    """R_d of the looping form (NS = 16): rises of the slice's running maximum after d."""
    D, P = c.shape
    per = -(-D // 16)
    R = np.zeros((D, P))
    for d0 in range(0, D, per):
        s = c[d0:min(d0 + per, D)]
        run = np.maximum.accumulate(s, axis=0)
        rise = np.zeros(s.shape)
        rise[1:] = run[1:] > run[:-1]
        R[d0:d0 + s.shape[0]] = rise.sum(0)[None] - np.cumsum(rise, axis=0)
    return R


def reference(cost, dv, gd=None):
    """cost [D,P] fp32, dv [D] fp32, gd [P] fp32 or None -> dict of float64 arrays: the reference values, the bounds
    d_depth, dE [P], the backward's grad [D,P] and grad_bound, and what conf_ref() needs."""
    c = np.asarray(cost, np.float64)
    dvv = np.asarray(dv, np.float64)[:, None]
    D, P = c.shape
    dd = np.arange(D, dtype=np.float64)[:, None]
    M = c.max(0)
    e = np.exp(c - M)
    S = e.sum(0)
    p = e / S
    depth = (p * dvv).sum(0)
    E = (p * dd).sum(0)
    idx = np.clip(np.trunc(E).astype(np.int64), 0, D - 1)

    sub, Ksum = np.zeros((D, P)), 0
    for _, NS in LAYOUTS:
        mk, per = _slice_max(c, NS)
        sub = np.maximum(sub, np.abs(c - mk) + np.abs(mk - M))
        Ksum = max(Ksum, per + NS)
    R = _rescales(c) if D > 256 else 0.0
    tau_c = U * sub + 2 * U * EXP_ULPS * (2 + R)
    phi = TINY * (D + 16) / S

    def A(x, K, levels):
        T = (p * np.abs(x)).sum(0)
        return np.minimum(K * U * T, levels * np.minimum(U * T, p * np.abs(x)).sum(0))

    one = np.ones((D, 1))
    sigma = (p * (tau_c + U * R)).sum(0) + A(one, Ksum, 2) + phi

    def mean_bound(x):
        m = (p * x).sum(0)
        sep = A(x, Ksum, 2) + np.abs(m) * A(one, Ksum, 2) + (p * U * R * (np.abs(x) + np.abs(m))).sum(0)
        return 2 * ((p * tau_c * np.abs(x - m)).sum(0) + sep + 3 * U * np.abs(m) + phi * (np.abs(x).max() + np.abs(m)))

    out = dict(p=p, depth=depth, E=E, idx=idx, d_depth=mean_bound(dvv), dE=mean_bound(dd), sigma=sigma, S=S,
               tap=p * (U * np.abs(c - M) + 2 * U * EXP_ULPS))
    if gd is not None:
        g = np.asarray(gd, np.float64)[None]
        rho_e = U * np.abs(c - M) + 2 * U * EXP_ULPS
        fl = TINY * D / S
        sigma_b = (p * rho_e).sum(0) + A(one, D, 1) + fl
        dev = np.abs(dvv - depth)
        d1 = ((p * rho_e * dev).sum(0) + A(dvv, D, 1) + np.abs(depth) * A(one, D, 1) + 3 * U * np.abs(depth)
              + fl * (np.abs(dvv).max() + np.abs(depth)))
        rho = rho_e + sigma_b + 5 * U
        out["grad"] = g * p * (dvv - depth)
        out["grad_bound"] = (2 * np.abs(g) * p * (rho * dev + d1 + U * np.abs(dvv) + U * dev)
                             + 2 * TINY * (1 + (1 + np.abs(g)) * dev))
    return out


def conf_ref(ref, idx):
    """-> (window sum for idx, its bound d(conf | idx)), [P] each."""
    conf = window(ref["p"], idx)
    return conf, 2 * (window(ref["tap"], idx) + conf * (ref["sigma"] + 7 * U) + 4 * TINY / ref["S"])


def ambiguous(ref):
    """-> (mask [P], j [P]): pixels whose [E - dE, E + dE] holds an integer j with 1 <= j <= D - 1."""
    D = ref["p"].shape[0]
    j = np.rint(ref["E"]).astype(np.int64)
    return (np.abs(ref["E"] - j) <= ref["dE"]) & (j >= 1) & (j <= D - 1), j


def check_forward(depth, conf, ref):
    """-> (worst depth ratio, worst conf ratio, problems)."""
    depth, conf = np.asarray(depth, np.float64).ravel(), np.asarray(conf, np.float64).ravel()
    D = ref["p"].shape[0]
    problems = []
    rd = np.abs(depth - ref["depth"]) / ref["d_depth"]
    rd = np.where(np.isfinite(rd), rd, np.inf)
    amb, j = ambiguous(ref)
    c0, b0 = conf_ref(ref, ref["idx"])
    rc = np.abs(conf - c0) / b0
    if amb.any():
        jj = np.clip(j, 1, D - 1)
        ca, ba = conf_ref(ref, jj)
        cb, bb = conf_ref(ref, jj - 1)
        rc = np.where(amb, np.minimum(np.abs(conf - ca) / ba, np.abs(conf - cb) / bb), rc)
    rc = np.where(np.isfinite(rc), rc, np.inf)
    for what, r, got, want in (("depth", rd, depth, ref["depth"]), ("conf", rc, conf, c0)):
        if r.max() > 1.0:
            i = int(r.argmax())
            problems.append("%s error / bound = %.3g at pixel %d: got %.9g want %.9g E %.6f (%d pixels over)"
                            % (what, r.max(), i, got[i], want[i], ref["E"][i], int((r > 1).sum())))
    return float(rd.max()), float(rc.max()), problems


def check_backward(grad, ref):
    grad = np.asarray(grad, np.float64).reshape(ref["grad"].shape)
    r = np.abs(grad - ref["grad"]) / ref["grad_bound"]
    r = np.where(np.isfinite(r), r, np.inf)
    problems = []
    if r.max() > 1.0:
        i = np.unravel_index(int(r.argmax()), r.shape)
        problems.append("grad error / bound = %.3g at (d, pixel) %s: got %.9g want %.9g (%d elements over)"
                        % (r.max(), i, grad[i], ref["grad"][i], int((r > 1).sum())))
    return float(r.max()), problems


# ---------------------------------------------------------------------------------------------------------------
# dense cases
# ---------------------------------------------------------------------------------------------------------------
SMALL_HW, LARGE_HW = (47, 83), (127, 131)      # 3901 and 16637 pixels: neither a multiple of 16 nor of 32
FORM_SHAPES = {"<8,16,16>": (48, SMALL_HW), "<16,16,16>": (192, SMALL_HW), "loop": (300, SMALL_HW),
               "<16,32,8>": (128, LARGE_HW), "<24,32,8>": (192, LARGE_HW), "<32,32,8>": (256, LARGE_HW),
               "loop/hw>=16384": (264, LARGE_HW)}
LOGITS = ("gain1", "gain3", "gain10", "gain30", "gain80", "ridges", "iid80")
UNCAPPED = ("iid80",)
DVS = ("dtu", "inverse", "descending")


def depth_axis(kind, D):
    if kind == "dtu":
        return synthetic.depth_values(D)
    if kind == "inverse":
        return (1.0 / np.linspace(1 / 400.0, 1 / 2500.0, D)).astype(np.float32)
    assert kind == "descending", kind
    return synthetic.depth_values(D)[::-1].copy()


def logits(kind, D, P, seed):
    """gainG: G times a unit-variance random field that is smooth along depth (white noise under a Gaussian of sigma = 8
    depths), as a regularised cost volume is: the winning depth has neighbours of comparable logit at every gain, so E
    is spread over the reals and not pinned to the integers as it is for independent logits at gain >= 10, where fp32
    cannot tell trunc(d - 1e-9) from trunc(d + 1e-9) on most pixels.  ridges: two ridges that move across every slice
    boundary from pixel to pixel.  iidG: G times independent noise, the near-one-hot regime with winners at d = 0 and
    D - 1 too; exempt from the ambiguity cap (UNCAPPED): depth and grad_cost do not depend on trunc and are held to the
    bound on every element, the confidence is allowed either window wherever E is within dE of an integer."""
    rng = np.random.default_rng(seed)
    if kind.startswith("iid"):
        return (float(kind[3:]) * rng.standard_normal((D, P))).astype(np.float32)
    if kind.startswith("gain"):
        t = np.arange(-24, 25, dtype=np.float64)
        k = np.exp(-t * t / 128.0)
        k /= np.sqrt((k * k).sum())
        x = rng.standard_normal((D + 48, P))
        z = np.zeros((D, P))
        for i, wk in enumerate(k):
            z += wk * x[i:i + D]
        # winners stay off the two end depths (there E = D - 1 - 1e-9 is undecidable in fp32 however the logits are
        # drawn; the probes pin d = 0, 1, D - 2, D - 1 exactly): two standard deviations taken off towards the ends
        z -= 2.0 * (2.0 * np.arange(D)[:, None] / max(D - 1, 1) - 1.0) ** 8
        return (float(kind[4:]) * z).astype(np.float32)
    assert kind == "ridges", kind
    d = np.arange(D, dtype=np.float64)[:, None]
    px = np.arange(P, dtype=np.float64)[None]
    r1, r2 = (0.37 * px) % D, (D - 1 - 0.23 * px) % D
    c = 12 * np.exp(-(d - r1) ** 2 / 8) + 11 * np.exp(-(d - r2) ** 2 / 18) + 0.5 * rng.standard_normal((D, P))
    return c.astype(np.float32)


def dense_cases():
    """name -> builder of dict(cost [D,P], dv [D], gd [P], h, w): every launch form x every logit kind; the depth axes
    rotate so that each form and each logit kind meets all three."""
    out = {}
    for fi, form in enumerate(FORMS):
        D, (h, w) = FORM_SHAPES[form]
        assert launch_form(D, h * w)[0] == form, (form, launch_form(D, h * w))
        for li, kind in enumerate(LOGITS):
            dvk = DVS[(fi + li) % 3]

            def build(D=D, h=h, w=w, kind=kind, dvk=dvk, seed=100 * fi + li):
                gd = (np.random.default_rng(seed + 7).standard_normal(h * w) ** 3).astype(np.float32)
                return dict(cost=logits(kind, D, h * w, seed), dv=depth_axis(dvk, D), gd=gd, h=h, w=w)
            out["%s/%s/%s" % (form, kind, dvk)] = build
    return out


# ---------------------------------------------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------------------------------------------
BACKGROUND = -200.0
PROBE_SHAPES = [(D, SMALL_HW) for D in (1, 3, 17, 128, 129, 256, 257)] + \
               [(D, LARGE_HW) for D in (128, 129, 192, 193, 256)]
K2_OFFSETS = ((0, 1), (0, 3), (0, 4), (0, 5))
K4_OFFSETS = ((0, 1, 2, 3), (0, 1, 2, 9), (0, 4, 5, 7), (0, 2, 3, 7), (0, 1, 5, 6), (0, 8, 9, 11), (0, 3, 4, 5),
              (0, 20, 40, 60))


def slice_boundaries(D):
    out = set()
    for _, NS in LAYOUTS:
        per = -(-D // NS)
        out |= {k * per for k in range(1, NS) if k * per < D}
    return sorted(out)


def probe_list(D):
    """spike position tuples: at the ends of [0, D), on both sides of every slice boundary of both layouts, and the
    K = 2 / K = 4 patterns anchored so that their windows straddle those boundaries."""
    anchors = {0, 1, D - 2, D - 1, D // 2}
    for b in slice_boundaries(D):
        anchors |= {b - 4, b - 2, b - 1, b}
    anchors = sorted(a for a in anchors if 0 <= a < D)
    out = []
    for a in anchors:
        out.append((a,))
        for offs in K2_OFFSETS + K4_OFFSETS:
            for base in (a, a - offs[-1]):               # the pattern starting and ending at the anchor
                pos = tuple(base + o for o in offs)
                if pos[0] >= 0 and pos[-1] < D:
                    out.append(pos)
    seen, uniq = set(), []
    for pos in out:
        if pos not in seen:
            seen.add(pos)
            uniq.append(pos)
    return uniq


def probe_case(D, h, w):
    """-> dict(cost, dv, gd, spikes [list per pixel]) and the exact expectations depth, idx, conf [P], grad [D,P] as
    float32, computed in integer / rational arithmetic."""
    P = h * w
    probes = probe_list(D)
    dv = (425 + 3 * np.arange(D)).astype(np.float32)
    cost = np.full((D, P), BACKGROUND, np.float32)
    gd = np.empty(P, np.float32)
    depth, conf, idx = np.empty(P, np.float64), np.empty(P, np.float64), np.empty(P, np.int64)
    grad = np.zeros((D, P), np.float64)
    spikes = []
    for px in range(P):
        pos = probes[px % len(probes)]
        K = len(pos)
        spikes.append(pos)
        cost[list(pos), px] = 0.0
        gd[px] = (-1.0) ** px * 2.0 ** (px % 7 - 3)
        depth[px] = sum(425 + 3 * d for d in pos) / K
        idx[px] = min(max(sum(pos) // K, 0), D - 1)
        conf[px] = sum(1 for d in pos if idx[px] - 1 <= d <= idx[px] + 2) / K
        for d in pos:
            grad[d, px] = float(gd[px]) / K * ((425 + 3 * d) - depth[px])
    return dict(cost=cost, dv=dv, gd=gd, spikes=spikes, depth=depth, idx=idx, conf=conf, grad=grad, h=h, w=w)


def same_bits(a, b, zero_sign=True):
    """bit for bit.  zero_sign=False is for grad_cost only: its background entries are 0 * gd * (dv - depth), whose
    sign follows gd and dv - depth, and the sign of such a zero is not compared."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    if not zero_sign:
        a, b = np.where(a == 0, np.float32(0), a), np.where(b == 0, np.float32(0), b)
    return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels, one numpy float32 operation per device operation
# ---------------------------------------------------------------------------------------------------------------
FWD_DEFECTS = ("merge_without_rescale", "window_idx_plus_1", "window_not_clipped", "round_not_trunc",
               "ragged_shadow_write", "empty_slice_exp0")
BWD_DEFECTS = ("bwd_dv_minus_dv_idx",)
f32 = np.float32


def _fma(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _step(x, ulps):
    for _ in range(abs(ulps)):
        x = np.nextafter(x, f32(np.inf if ulps > 0 else -np.inf)).astype(f32)
    return x


def _expf(x, ulps=0):
    with np.errstate(all="ignore"):
        y = np.exp(np.asarray(x, np.float64)).astype(f32)
    return np.maximum(_step(y, ulps), f32(0)) if ulps else y


def _rcp(x, ulps=0):
    with np.errstate(all="ignore"):
        return _step((f32(1.0) / x).astype(f32), ulps)


def emulate_forward(cost, dv, hw_form=None, exp_ulps=0, rcp_ulps=0, defect=None):
    """cost [D,P] fp32 -> (depth, conf) [P] fp32 as launch_softargmin's form for (D, P) computes them; hw_form
    overrides P in the form choice (a small P standing in for a large map).  A -inf logit is a term of exactly 0, as
    in the kernels; defect "minus_inf_term_nan" (not in FWD_DEFECTS: it shows on non-finite logits only,
    test_nonfinite_host.py) computes expf(-inf - m) instead, NaN while the slice's maximum is still -inf."""
    c = np.asarray(cost, f32)
    dv = np.asarray(dv, f32)
    D, P = c.shape
    _, PIX, NS, maxper = launch_form(D, hw_form or P)
    per = -(-D // NS)
    zero = np.zeros(P, f32)
    ex = lambda x: _expf(x, exp_ulps)  # noqa: E731
    with np.errstate(all="ignore"):
        ms, ss, sds, sis = [], [], [], []
        for k in range(NS):
            d0, d1 = k * per, min(k * per + per, D)
            if d0 >= d1:
                if defect == "empty_slice_exp0":      # the clamped load of depth D - 1 taken for an element
                    ms.append(c[D - 1].copy()), ss.append(zero + f32(1)), sds.append(zero + dv[D - 1])
                    sis.append(zero + f32(D - 1))
                else:
                    ms.append(zero - f32(np.inf)), ss.append(zero), sds.append(zero), sis.append(zero)
                continue
            s, sd, si = zero, zero, zero
            if maxper is not None:
                m = c[d0:d1].max(0)
                for d in range(d0, d1):
                    e = ex(c[d] - m) if defect == "minus_inf_term_nan" else np.where(c[d] == -np.inf, f32(0), ex(c[d] - m))
                    s = s + e
                    sd = _fma(e, dv[d], sd)
                    si = _fma(e, f32(d), si)
            else:
                m = zero - f32(np.inf)
                for d in range(d0, d1):
                    up = c[d] > m
                    r = np.where(up, ex(m - c[d]), f32(1))
                    s, sd, si = np.where(up, s * r, s), np.where(up, sd * r, sd), np.where(up, si * r, si)
                    m = np.where(up, c[d], m)
                    e = ex(c[d] - m) if defect == "minus_inf_term_nan" else np.where(c[d] == -np.inf, f32(0), ex(c[d] - m))
                    s = s + e
                    sd = _fma(e, dv[d], sd)
                    si = _fma(e, f32(d), si)
            ms.append(m), ss.append(s), sds.append(sd), sis.append(si)
        M = ms[0]
        for k in range(1, NS):
            M = np.maximum(M, ms[k])
        S, SD, SI = zero, zero, zero
        for k in range(NS):
            r = np.where(ms[k] == -np.inf, f32(0), ex(ms[k] - M))
            if defect == "merge_without_rescale":
                r = np.where(ms[k] == -np.inf, f32(0), f32(1))
            S, SD, SI = _fma(ss[k], r, S), _fma(sds[k], r, SD), _fma(sis[k], r, SI)
        inv = _rcp(S, rcp_ulps)
        depth = SD * inv
        t = SI * inv
        idx = (np.rint(t) if defect == "round_not_trunc" else np.trunc(t)).astype(np.int64)
        idx = np.clip(idx, 0, D - 1)
        lo, hi = idx - 1, idx + (1 if defect == "window_idx_plus_1" else 2)
        if maxper is not None:
            c4 = zero
            for k in range(NS):
                part = zero
                for d in range(k * per, min(k * per + per, D)):
                    part = np.where((d >= lo) & (d <= hi), part + ex(c[d] - M), part)
                c4 = c4 + part
        else:
            c4 = zero
            for kk in range(-1, hi[0] - idx[0] + 1):
                j = idx + kk
                ok = (j >= 0) & (j < D)
                tapv = ex(np.take_along_axis(c, np.clip(j, 0, D - 1)[None], 0)[0] - M)
                c4 = np.where(ok, c4 + tapv, c4)
        if defect == "window_not_clipped":            # taps beyond D - 1 read the clamped depth D - 1 again
            for j in (D, D + 1):
                c4 = np.where(j <= hi, c4 + ex(c[D - 1] - M), c4)
        conf = c4 * inv
    if defect == "ragged_shadow_write" and P % PIX:
        first = (P // PIX) * PIX                      # a lane of the last block writes its value to the shadow pixel
        depth, conf = depth.copy(), conf.copy()
        depth[P - 1], conf[P - 1] = depth[first], conf[first]
    return depth.astype(f32), conf.astype(f32)


def emulate_backward(cost, dv, gd, exp_ulps=0, rcp_ulps=0, defect=None):
    """softargmin_bwd_kernel in fp32 numpy.  Defect "minus_inf_term_nan" (not in BWD_DEFECTS: it shows on non-finite
    logits only, tests/test_nonfinite_train_host.py): the maximum is found on the way, as the forward's loop form does,
    and a -inf logit met while the running maximum is still -inf is expf(-inf - -inf), NaN, instead of a term of 0."""
    c, dv, gd = np.asarray(cost, f32), np.asarray(dv, f32), np.asarray(gd, f32)
    D, P = c.shape
    with np.errstate(all="ignore"):
        M = c.max(0)
        S, SD, SI = np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, f32)
        e = _expf(c - M[None], exp_ulps)
        if defect == "minus_inf_term_nan":
            e = np.where(np.isnan(_expf(c - np.maximum.accumulate(c, 0))), f32(np.nan), e)
        for d in range(D):
            S = S + e[d]
            SD = _fma(e[d], dv[d], SD)
            SI = _fma(e[d], f32(d), SI)
        inv = _rcp(S, rcp_ulps)
        depth = SD * inv
        if defect == "bwd_dv_minus_dv_idx":
            depth = dv[np.clip(np.trunc(SI * inv).astype(np.int64), 0, D - 1)]
        gi = gd * inv
        return ((e * gi[None]) * (dv[:, None] - depth[None])).astype(f32)
