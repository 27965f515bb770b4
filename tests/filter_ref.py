"""Scenes, path census, comparison rules and named defects for the depth-map filter / fusion kernel
(csrc/filter_depth.hip + mvs_filter_compose; oracle/filter_oracle.py; fixture tests/golden/fx_filter.npz written by
tests/golden/gen_filter_golden.py from the reference's own reproject_with_depth / check_geometric_consistency /
depth2pts_np).  Host-only numpy; the GPU suite (tests/test_gpu_filter_ref.py) and the host suite
(tests/test_filter_ref_host.py) both state their criteria through the two rules below and nowhere else.

Rule (a) -- kernel against oracle: every output bit-equal (`rule_a`).  The oracle fixes one operation order and the
kernel + mvs_filter_compose follow it, so nothing is left to a tolerance.

Rule (b) -- oracle (CPU) and kernel (GPU) against the fixture (`rule_b`).  The reference forms inv(K), inv(E),
inv(R) and E_a inv(E_b) in float32 through whatever LAPACK / BLAS numpy links, so its float32 matrix entries may
differ from the oracle's in the last bits, and its float64 matrix-vector products may be summed in another order.
Derivation of the bands and bounds (u = 2^-24, float32 unit roundoff; all of it evaluated per pixel from the scene
inputs and the reference's recorded fields in the fixture, never from the code under test):

  1. Matrix entries.  A backward-stable float32 inverse X of an n x n matrix A (LU with partial pivoting, any
     variant) satisfies, to first order, |X - inv(A)| <= c u |inv(A)| |A| |inv(A)| + u |inv(A)| entrywise (Higham,
     Accuracy and Stability, sec. 14.3; the last term is the final rounding); a float32 product of a float32 matrix A
     with such an X, summed in any order with or without fused multiply-adds, adds c u |A| |X| + u |A X|  (`_inv_err`,
     `_mm_err`).  Two evaluations (the reference's and the oracle's) differ by at most twice that.  The bound scales
     with |A||B|, not with the entry: the translation column of E_src inv(E_ref) is a cancelling sum, where "one ulp of
     the entry" would be too small.  The worst-case constants are c = 2n and c = 4; with them the bands alone would
     leave out 3-5 % of the decisions of 30-50 px scenes, and the oracle sits a factor 12 inside.  c = 1 is used (one
     rounding of the size of the largest partial sum per entry -- the "one-ulp disagreement" model), which the CPU
     suite then has to justify by measurement: see MEASURED_MAX_RATIO below.
  2. Forward chain (eval.py:525-532), float64: the entry errors propagate linearly, e(p_ref) = e(Kri)|pix|,
     e(p_src) = e(T)|[p_ref;1]| + |T| e(p_ref), e(q) = |K_src| e(p_src), e(x_src) = (e(q0) + |x_src| e(q2)) / |q2|;
     the float32 casts at eval.py:538-539 add one float32 ulp, 2^-23 |x_src|, to the disagreement.  float64 rounding
     (2^-53 per operation, about 20 operations) is 9 orders below and is covered by the factor (1 + 1e-6).
  3. Tie band.  remap quantises 32 x_src with round-half-even.  A decision is LEFT OUT when the reference's recorded
     32 x_src or 32 y_src lies within 32 (2 e(x_src) + 2^-23 |x_src|) of a half-integer: there the two evaluations may
     sample with different weights (0.26 px in x_reprojected was measured at such pixels next to the zero border).
     Everywhere else both sample the same taps with the same weights, and the sample is bit-identical.
  4. Backward chain (eval.py:545-555): the same propagation with e(inv(K_src)), e(T2), and the input error
     2 e(x_src) |sample| of xy_src * sample; casts at eval.py:551-555 add 2^-23 |value|.  This gives per decision
     D(d_rep), D(x_rep), D(y_rep), the largest possible disagreement of depth_reprojected / x- / y_reprojected.
  5. Threshold bands.  |dist_a - dist_b| <= D(x_rep) + D(y_rep); |rel_a - rel_b| <= D(d_rep)/|d_ref| + 2^-22 rel
     (one float32 subtraction and one division each side).  A decision whose recorded dist (rel) is within that of
     condmask_pixel (float32(condmask_depth)) is left out.  A pixel is left out if any of its decisions is.  A decision
     whose d_ref is 0 or non-finite is never left out: its rel is inf or NaN whatever is sampled, so it is rejected.
  6. Values on the kept pixels: |depth_reprojected| to D(d_rep) where the mask holds; depth_avg to
     (sum of D(d_rep) over agreeing views + 2 (S+1) u |sum|) / (geo+1)  (the float32 `sum()` of eval.py:699); xyz_world
     by propagating e(Kri), e(inv(R)) and D(depth_avg) through eval.py:256-264.
  `rule_b` returns the largest observed / bound ratio; it must be <= 1.  The CPU suite measures the oracle at
  ratio <= MEASURED_MAX_RATIO (DESIGN.md f3 records the figures), i.e. the bounds carry a margin of at least
  1 / MEASURED_MAX_RATIO over the largest oracle-vs-fixture disagreement; the kernel is held to the same bounds and
  was not consulted for them.
  The left-out share may not exceed LEFT_OUT_CAP of a scene's decisions (`left_out_share`, from the fixture alone);
  `ties` is exempt: it is built to sit on the ties and is judged by rule (a) and by hand-computed expectations.

Defects (`chain(..., defects=...)`): a test-side restatement of the oracle's per-pixel chain in the kernel's calling
convention (ref_idx [R], src_idx [R][S] with -1 = no view) with one named mistake switched on.  With no defect it is
bit-identical to the oracle (asserted by the host suite).  DEFECTS maps each name to the scene that must catch it.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import filter_oracle as fo
from synthetic_scene import make_scene

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
INT_MIN = -2147483648
C_INV, C_MM = 1.0, 1.0      # see step 1 of the derivation
LEFT_OUT_CAP = 0.01
MEASURED_MAX_RATIO = 0.25     # asserted upper limit of observed/bound for the oracle on the CPU: a margin of >= 4x
DEFAULTS = dict(n_view_filter=10, photomask=0.8, geomask=3, condmask_pixel=1.0, condmask_depth=0.01)


# ------------------------------------------------------------------------------------------------ scenes
def _scene(name, depths, confs, Ks, Es, pairs, fixture=True, **kw):
    th = dict(DEFAULTS)
    th.update(kw)
    return dict(name=name, depths=np.ascontiguousarray(depths, F32), confs=np.ascontiguousarray(confs, F32),
                Ks=np.ascontiguousarray(Ks, F32), Es=np.ascontiguousarray(Es, F32),
                pairs=[(int(r), [int(s) for s in ss]) for r, ss in pairs], th=th, fixture=fixture)


def _rel_threshold_plants(n=4):
    """(d_ref, sample) float32 pairs with float32(|sample - d_ref| / d_ref) == float32(0.01) exactly: the relative-depth
    test `<` must reject them, and a comparison carried out in float64 (0.01 > float32(0.01)) would accept them."""
    c = F32(0.01)
    out = []
    d = F32(500.0)
    while len(out) < n:
        d = np.nextafter(d, F32(np.inf))
        base = F32(d + d * c)
        for k in range(-4, 5):
            s = base
            for _ in range(abs(k)):
                s = np.nextafter(s, F32(np.inf if k > 0 else -np.inf))
            if F32(np.abs(F32(s - d)) / d) == c:
                out.append((d, s))
                break
    return out


def _fronto(h, w, cx, cy, shifts, ramp=True):
    """Fronto-parallel views with K = [[64,0,cx],[0,64,cy],[0,0,1]] and pure x/y translations: at depth 512 view v sees
    the reference pixel (x, y) at exactly (x + sx, y + sy) for shifts in multiples of 1/64 px -- every operation of the
    forward chain is exact in float64 (powers of two, small integers)."""
    V = len(shifts) + 1
    K = np.array([[64, 0, cx], [0, 64, cy], [0, 0, 1]], F32)
    Es = np.tile(np.eye(4, dtype=F32), (V, 1, 1))
    ys, xs = np.mgrid[0:h, 0:w]
    depths = np.full((V, h, w), 512, F32)
    for v, (sx, sy) in enumerate(shifts, 1):
        Es[v, 0, 3], Es[v, 1, 3] = 8.0 * sx, 8.0 * sy            # shift = f t / d = t / 8
        if ramp:
            depths[v] = (512 + ((xs + 2 * ys) % 8) * 0.5).astype(F32)
    confs = (0.5 + 0.5 * np.sin(xs * 0.37) * np.cos(ys * 0.23))[None].repeat(V, 0).astype(F32)
    return depths, confs, np.tile(K, (V, 1, 1)), Es


TIES_SHIFTS = ((1 / 64, 0.0), (-3 - 1 / 64, 3 / 64), (5 + 3 / 64, -2 - 1 / 64), (2.0, -1.0), (0.0, 0.0))


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "distinctK":
        d, c, K, E, _ = make_scene(V=4, h=28, w=36, seed=21, k_spread=0.04, skew=1.5)
        c[0, 0, :6] = F32(0.8)                                   # confidence == photomask exactly: `>` rejects
        return _scene(name, d, c, K, E, [(0, [1, 2, 3]), (2, [3, 0, 1])], geomask=2)
    if name == "exact":
        d, c, K, E, p = make_scene(V=4, h=28, w=36, seed=22, noise=0, k_spread=0.03, skew=1.0)
        return _scene(name, d, c, K, E, p, fixture=False, geomask=2)
    if name == "wide":
        # loose thresholds: a sample that lost taps to the zero border is 1/2 or 1/4 of the depth and must still be
        # able to pass, or nothing the border does could reach an output
        d, c, K, E, _ = make_scene(V=4, h=32, w=40, seed=40, rot=0.12, baseline=2.0, k_spread=0.02, skew=0.5)
        return _scene(name, d, c, K, E, [(1, [0, 2, 3]), (2, [3, 0, 1])], geomask=2, condmask_pixel=60.0,
                      condmask_depth=0.9)
    if name == "holes":
        d, c, K, E, _ = make_scene(V=4, h=28, w=36, seed=24, roll=0.02)
        for v in range(4):
            o = 3 * v
            d[v, 2:6, 3 + o:9 + o] = 0
            d[(v + 1) % 4, 9:13, 20 - o:26 - o] = -300
            d[(v + 2) % 4, 16:20, 5 + o:11 + o] = np.inf
            d[(v + 3) % 4, 22:26, 24 - o:30 - o] = np.nan
        return _scene(name, d, c, K, E, [(0, [1, 2, 3]), (3, [0, 1, 2])], geomask=2)
    if name == "ties":
        h, w = 16, 24
        d, c, K, E = _fronto(h, w, 12, 8, TIES_SHIFTS)
        d[5] = 512                                               # view 5 = view 0's camera
        for i, (dr, s) in enumerate(_rel_threshold_plants()):
            d[0, h - 1, 2 + i], d[5, h - 1, 2 + i] = dr, s
        return _scene(name, d, c, K, E, [(0, [1, 2, 3, 4, 5]), (1, [0, 2]), (5, [0, 3])])
    if name.startswith("ragged_"):
        h, w = (int(t) for t in name[7:].split("x"))
        if min(h, w) == 1:     # one pixel high / wide: shifts along the long side only, so that samples still pass
            a, b = (2.3, -1.7) if max(h, w) > 1 else (0.0, 0.3)
            d, c, K, E = _fronto(h, w, w // 2, h // 2, ((a, 0.0), (b, 0.0)) if h == 1 else ((0.0, a), (0.0, b)))
            return _scene(name, d, c, K, E, [(0, [1, 2])], geomask=1)
        d, c, K, E, _ = make_scene(V=3, h=h, w=w, seed=25 + h, k_spread=0.03, skew=0.5)
        return _scene(name, d, c, K, E, [(0, [1, 2])], geomask=1)
    if name in ("limit_row", "limit_col"):
        # x_src = x +- 40000: past +-32768 px on part of the row, where the 16-bit clip of the integer coordinate
        # engages with a finite coordinate (a wrapping 16-bit store would land back inside the image)
        n = 32767
        if name == "limit_row":
            d, c, K, E = _fronto(1, n, 16384, 0, ((40000.0, 0.0), (-40000.0, 0.0), (3 + 1 / 64, 0.0)))
        else:
            d, c, K, E = _fronto(n, 1, 0, 16384, ((0.0, 40000.0), (0.0, -40000.0), (0.0, 3 + 1 / 64)))
        return _scene(name, d, c, K, E, [(0, [1, 2, 3])], fixture=False, geomask=1)
    raise KeyError(name)


SCENES = ("distinctK", "exact", "wide", "holes", "ties", "ragged_37x53", "ragged_1x300", "ragged_300x1", "ragged_1x1",
          "limit_row", "limit_col")
FIXTURE_SCENES = tuple(n for n in SCENES if n not in ("exact", "limit_row", "limit_col"))


def same_K_scene():
    """Today's make_scene defaults (every view shares one K): the scene on which the K-swap defects are invisible."""
    d, c, K, E, p = make_scene(V=4, h=28, w=36, seed=21)
    return _scene("sameK", d, c, K, E, p, fixture=False)


def abi_rows(sc):
    """(ref_idx [R], src_idx [R][S]) as fusion._pad_pairs lays a pair list out."""
    nvf = sc["th"]["n_view_filter"]
    S = max(1, max(len(s[:nvf]) for _, s in sc["pairs"]))
    ref = np.array([r for r, _ in sc["pairs"]], np.int32)
    src = np.full((len(ref), S), -1, np.int32)
    for i, (_, s) in enumerate(sc["pairs"]):
        src[i, :len(s[:nvf])] = s[:nvf]
    return ref, src


# direct-ABI cases on the distinct-K scene that fusion._pad_pairs cannot produce: name -> (ref_idx, src_idx)
ABI_CASES = {
    # -1 in the middle of a row; a row of only -1; the same ref in two rows; src == ref (row 3)
    "mixed": ([0, 1, 0, 2], [[1, -1, 2], [-1, -1, -1], [3, 2, 1], [2, 0, -1]]),
    "S1": ([0, 3], [[1], [0]]),
    "S10": ([0, 1], [[1, 2, 3, 1, 2, 3, 1, 2, 3, 1], [0, -1, 2, 3, 0, 2, -1, 3, 0, 2]]),
}


def abi_case(name):
    ref, src = ABI_CASES[name]
    return np.array(ref, np.int32), np.array(src, np.int32)


def oracle_rows(sc, ref_idx=None, src_idx=None, n_view_filter=None):
    """oracle/filter_oracle.py on a scene; with (ref_idx, src_idx) the -1 entries are dropped, which is what "no view"
    means."""
    th = dict(sc["th"])
    if n_view_filter is not None:
        th["n_view_filter"] = n_view_filter
    pairs = sc["pairs"]
    if ref_idx is not None:
        pairs = [(int(r), [int(s) for s in row if s >= 0]) for r, row in zip(ref_idx, src_idx)]
        th["n_view_filter"] = 1 << 30
    return fo.filter_views(sc["depths"], sc["confs"], sc["Ks"], sc["Es"], pairs, **th)


# ------------------------------------------------------------------------------------------------ rule (a)
OUTPUTS = ("geo_sum", "photo", "geo", "final", "depth_avg", "xyz_world")


def rule_a(got, want):
    """Bit-equality of every output, row by row (NaN == NaN at the same positions)."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in OUTPUTS:
            a, b = np.asarray(g[k]), np.asarray(w[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
            np.testing.assert_array_equal(a, b, err_msg=k)


def fails(rule, *a, **kw):
    try:
        rule(*a, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ census
def _remap_paths(x_src, y_src, h, w):
    with np.errstate(all="ignore"):
        vx, vy = x_src * F32(32), y_src * F32(32)
    sx, sy = fo._cv_round(vx), fo._cv_round(vy)
    qx, qy = sx >> 5, sy >> 5
    ix, iy = np.clip(qx, -32768, 32767), np.clip(qy, -32768, 32767)
    x0, x1, y0, y1 = (ix >= 0) & (ix < w), (ix + 1 >= 0) & (ix + 1 < w), (iy >= 0) & (iy < h), (iy + 1 >= 0) & (iy + 1 < h)
    gone = (ix >= w) | (ix + 1 < 0) | (iy >= h) | (iy + 1 < 0)
    live = ~gone
    c = {}
    c["taps4"] = live & x0 & x1 & y0 & y1
    c["side_left"] = live & ~x0 & x1 & y0 & y1
    c["side_right"] = live & x0 & ~x1 & y0 & y1
    c["side_top"] = live & x0 & x1 & ~y0 & y1
    c["side_bottom"] = live & x0 & x1 & y0 & ~y1
    c["corner_tl"] = live & ~x0 & x1 & ~y0 & y1
    c["corner_tr"] = live & x0 & ~x1 & ~y0 & y1
    c["corner_bl"] = live & ~x0 & x1 & y0 & ~y1
    c["corner_br"] = live & x0 & ~x1 & y0 & ~y1
    c["out_right"], c["out_left"], c["out_bottom"], c["out_top"] = ix >= w, ix + 1 < 0, iy >= h, iy + 1 < 0
    c["int_min"] = (sx == INT_MIN) | (sy == INT_MIN)
    c["clip_finite"] = ((sx != INT_MIN) & (qx != ix)) | ((sy != INT_MIN) & (qy != iy))
    c["neg_frac"] = ((sx != INT_MIN) & (sx < 0) & ((sx & 31) != 0)) | ((sy != INT_MIN) & (sy < 0) & ((sy & 31) != 0))
    with np.errstate(all="ignore"):
        for v in (vx, vy):
            tie = np.isfinite(v) & (np.abs(v) < 2.0 ** 22) & (np.abs(v - np.floor(v) - F32(0.5)) == 0)
            r = np.rint(v)
            c["tie_down"] = c.get("tie_down", False) | (tie & (r < v))
            c["tie_up"] = c.get("tie_up", False) | (tie & (r > v))
            c["tie_negative"] = c.get("tie_negative", False) | (tie & (v < 0))
    return c


def census(sc):
    """Number of (ref, src, pixel) triples on each remap and decision path, and of (ref, pixel) on each per-pixel path,
    from the oracle's intermediates."""
    th, d, K, E = sc["th"], sc["depths"], sc["Ks"], sc["Es"]
    h, w = d.shape[1:]
    cnt = {}

    def add(k, m):
        cnt[k] = cnt.get(k, 0) + int(np.count_nonzero(m))

    S = 0
    for ref, srcs in sc["pairs"]:
        srcs = srcs[:th["n_view_filter"]]
        S = max(S, len(srcs))
        geo = np.zeros((h, w), np.int64)
        for s in srcs:
            _, _, _, x_src, y_src = fo.reproject(d[ref], K[ref], E[ref], d[s], K[s], E[s])
            for k, m in _remap_paths(x_src, y_src, h, w).items():
                add(k, m)
            mask, _, dist, rel = fo.geometric_consistency(d[ref], K[ref], E[ref], d[s], K[s], E[s],
                                                          th["condmask_pixel"], th["condmask_depth"])
            with np.errstate(all="ignore"):
                okd, okr = dist < th["condmask_pixel"], rel < F32(th["condmask_depth"])
            add("pass", okd & okr)
            add("fail_dist_only", ~okd & okr)
            add("fail_depth_only", okd & ~okr)
            add("fail_both", ~okd & ~okr)
            add("nan_rel", np.isnan(rel))
            add("rel_eq_threshold", rel == F32(th["condmask_depth"]))
            assert np.array_equal(mask, okd & okr)
            geo += mask
        for g in range(len(srcs) + 1):
            add(f"geo_{g}_of_{len(srcs)}", geo == g)
        add("geo_eq_geomask", geo == th["geomask"])
        add("geo_eq_geomask_minus_1", geo == th["geomask"] - 1)
        add("conf_eq_photomask", sc["confs"][ref] == F32(th["photomask"]))
    return cnt


# counter -> the scene that owns it (the host suite asserts census(scene(owner))[counter] > 0)
CENSUS_OWNERS = {
    "taps4": "distinctK", "side_left": "wide", "side_right": "wide", "side_top": "wide", "side_bottom": "wide",
    "corner_tl": "wide", "corner_tr": "wide", "corner_bl": "wide", "corner_br": "wide",
    "out_right": "wide", "out_left": "wide", "out_bottom": "wide", "out_top": "wide",
    "int_min": "holes", "clip_finite": "limit_row", "neg_frac": "wide",
    "tie_down": "ties", "tie_up": "ties", "tie_negative": "ties",
    "pass": "distinctK", "fail_dist_only": "holes", "fail_depth_only": "distinctK", "fail_both": "distinctK",
    "nan_rel": "holes", "rel_eq_threshold": "ties", "conf_eq_photomask": "distinctK",
    "geo_0_of_3": "distinctK", "geo_1_of_3": "distinctK", "geo_2_of_3": "distinctK", "geo_3_of_3": "distinctK",
    "geo_eq_geomask": "distinctK", "geo_eq_geomask_minus_1": "distinctK",
}
CENSUS_ALSO = (("clip_finite", "limit_col"), ("geo_5_of_5", "ties"), ("side_bottom", "limit_row"), ("side_right", "limit_col"))


# ------------------------------------------------------------------------------------------------ rule (b)
def fixture_scene(fx, name):
    """The scene as the fixture holds it (inputs and thresholds), so the GPU machine needs no generator."""
    g = lambda k: fx[f"{name}/{k}"]   # noqa: E731
    pr, ps = g("pair_ref"), g("pair_src")
    pairs = [(int(r), [int(s) for s in row if s >= 0]) for r, row in zip(pr, ps)]
    th = dict(n_view_filter=int(g("n_view_filter")), photomask=float(g("photomask")), geomask=int(g("geomask")),
              condmask_pixel=float(g("condmask_pixel")), condmask_depth=float(g("condmask_depth")))
    return _scene(name, g("depths"), g("confs"), g("Ks"), g("Es"), pairs, **th)


def _inv_err(A):
    A = np.asarray(A, F64)
    X = np.linalg.inv(A)
    return X, C_INV * U * (np.abs(X) @ np.abs(A) @ np.abs(X)) + U * np.abs(X)


def _mm_err(A, X, eX):
    A = np.asarray(A, F64)
    return A @ X, np.abs(A) @ eX + C_MM * U * (np.abs(A) @ np.abs(X)) + U * np.abs(A @ X)


def _proj(k, ek):
    with np.errstate(all="ignore"):
        x, y = k[0] / k[2], k[1] / k[2]
        return x, y, (ek[0] + np.abs(x) * ek[2]) / np.abs(k[2]), (ek[1] + np.abs(y) * ek[2]) / np.abs(k[2])


def _near(v, target, band):
    """|v - target| <= band, False where anything is NaN."""
    with np.errstate(all="ignore"):
        return np.abs(v - target) <= band


def pair_bounds(sc, fx, ref, j, s):
    """Per pixel for decision (ref, j-th source s): left_out, D(d_rep), and the recorded dist / rel (steps 2-5)."""
    name, d, K, E, th = sc["name"], sc["depths"], sc["Ks"], sc["Es"], sc["th"]
    h, w = d.shape[1:]
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.reshape(-1).astype(F64), ys.reshape(-1).astype(F64)
    g = lambda k: fx[f"{name}/{ref}_{j}/{k}"]   # noqa: E731
    x_src, y_src = g("x_src"), g("y_src")
    dr = d[ref].reshape(-1).astype(F64)
    with np.errstate(all="ignore"):
        pix = np.stack([xs * dr, ys * dr, dr])
        Kri, eKri = _inv_err(K[ref])
        Eri, eEri = _inv_err(E[ref])
        Esi, eEsi = _inv_err(E[s])
        Ksi, eKsi = _inv_err(K[s])
        T, eT = _mm_err(E[s], Eri, eEri)
        T2, eT2 = _mm_err(E[ref], Esi, eEsi)
        Ks, Kr = K[s].astype(F64), K[ref].astype(F64)
        p_ref, e_pref = Kri @ pix, eKri @ np.abs(pix)
        p_src = T[:3, :3] @ p_ref + T[:3, 3:4]
        e_psrc = eT[:3, :3] @ np.abs(p_ref) + eT[:3, 3:4] + np.abs(T[:3, :3]) @ e_pref
        xs_, ys_, e_x, e_y = _proj(Ks @ p_src, np.abs(Ks) @ e_psrc)
        Dx = (2 * e_x + 2 * U * np.abs(xs_)) * (1 + 1e-6)
        Dy = (2 * e_y + 2 * U * np.abs(ys_)) * (1 + 1e-6)
        vx, vy = x_src.reshape(-1).astype(F64) * 32, y_src.reshape(-1).astype(F64) * 32
        tie = _near(vx - np.floor(vx), 0.5, 32 * Dx) | _near(vy - np.floor(vy), 0.5, 32 * Dy)
        # the sample both evaluations take away from the ties (the reference's cv2.remap is the oracle's restatement)
        sm = fo.remap_linear(d[s], x_src, y_src).reshape(-1).astype(F64)
        b_in = np.stack([xs_ * sm, ys_ * sm, sm])
        e_bin = np.stack([Dx * np.abs(sm), Dy * np.abs(sm), np.zeros_like(sm)]) / 2
        back, e_back = Ksi @ b_in, eKsi @ np.abs(b_in) + np.abs(Ksi) @ e_bin
        p_rep = T2[:3, :3] @ back + T2[:3, 3:4]
        e_prep = eT2[:3, :3] @ np.abs(back) + eT2[:3, 3:4] + np.abs(T2[:3, :3]) @ e_back
        xr, yr, e_xr, e_yr = _proj(Kr @ p_rep, np.abs(Kr) @ e_prep)
        D_d = (2 * e_prep[2] + 2 * U * np.abs(p_rep[2])) * (1 + 1e-6)
        D_xr = (2 * e_xr + 2 * U * np.abs(xr)) * (1 + 1e-6)
        D_yr = (2 * e_yr + 2 * U * np.abs(yr)) * (1 + 1e-6)
        # eval.py:572-576 on the RECORDED fields
        x_rep, y_rep, d_rep = g("x_reprojected"), g("y_reprojected"), g("depth_reprojected")
        X, Y = np.meshgrid(np.arange(w), np.arange(h))
        dist = np.sqrt((x_rep - X) ** 2 + (y_rep - Y) ** 2).reshape(-1)
        rel = (np.abs(d_rep - d[ref]) / d[ref]).reshape(-1)
        near_d = _near(dist, th["condmask_pixel"], D_xr + D_yr)
        near_r = _near(rel.astype(F64), F64(F32(th["condmask_depth"])), D_d / np.abs(dr) + 4 * U * np.abs(rel.astype(F64)))
    near_r &= np.isfinite(rel)          # d_ref = 0: rel is inf or NaN on both sides, the decision is not in doubt
    # d_ref zero or non-finite: rel is inf or NaN whatever is sampled, the decision (reject) is owed on both sides
    doubt = (tie | near_d | near_r) & np.isfinite(dr) & (dr != 0)
    return dict(left_out=doubt.reshape(h, w), D_d=D_d.reshape(h, w), dist=dist, rel=rel,
                tie=tie, near_d=near_d, near_r=near_r, Dx=Dx)


def left_out_share(sc, fx):
    """Share of a scene's decisions that rule (b) leaves out; from the fixture alone."""
    n = k = 0
    for ref, srcs in sc["pairs"]:
        for j, s in enumerate(srcs[:sc["th"]["n_view_filter"]]):
            lo = pair_bounds(sc, fx, ref, j, s)["left_out"]
            n, k = n + lo.size, k + int(lo.sum())
    return k / n


def _ratio(got, want, bound, keep):
    """max |got - want| / bound over `keep`, NaN positions coinciding everywhere; 0 where both are equal."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    with np.errstate(all="ignore"):
        diff = np.abs(got - want)
        diff = np.where((got == want) | np.isnan(want), 0.0, diff)       # inf == inf included
        r = np.where(diff == 0, 0.0, diff / bound)
    r = r[keep]
    assert not np.isnan(r).any()
    return float(r.max()) if r.size else 0.0


def rule_b(sc, fx, rows, pair_rows=None):
    """`rows` (one dict per reference view: geo_sum, photo, geo, final, depth_avg, xyz_world) against the fixture;
    `pair_rows[i][j] = (mask, depth_reprojected)` as well where the caller has them (the oracle).  Returns the largest
    observed / bound ratio after asserting it is <= 1 and that every integer output is identical on the kept pixels."""
    name, d, K, E, th = sc["name"], sc["depths"], sc["Ks"], sc["Es"], sc["th"]
    h, w = d.shape[1:]
    worst = 0.0
    for i, (ref, srcs) in enumerate(sc["pairs"]):
        srcs = srcs[:th["n_view_filter"]]
        keep = np.ones((h, w), bool)
        sumD = np.zeros((h, w))
        for j, s in enumerate(srcs):
            b = pair_bounds(sc, fx, ref, j, s)
            keep &= ~b["left_out"]
            m = fx[f"{name}/{ref}_{j}/mask"]
            sumD += np.where(m, b["D_d"], 0.0)
            if pair_rows is not None:
                gm, gd = pair_rows[i][j]
                np.testing.assert_array_equal(gm[~b["left_out"]], m[~b["left_out"]])
                worst = max(worst, _ratio(gd, fx[f"{name}/{ref}_{j}/depth_reprojected"], b["D_d"], ~b["left_out"] & m))
        g = lambda k: fx[f"{name}/{ref}/{k}"]   # noqa: E731
        r = rows[i]
        for k, fk in (("geo_sum", "geo_mask_sum"), ("photo", "photo_mask"), ("geo", "geo_mask"), ("final", "final_mask")):
            np.testing.assert_array_equal(np.asarray(r[k])[keep], g(fk)[keep], err_msg=f"{name} ref {ref} {k}")
        avg = g("depth_est_averaged")
        geo = g("geo_mask_sum").astype(F64)
        with np.errstate(all="ignore"):
            D_avg = (sumD + 2 * (len(srcs) + 1) * U * np.abs(avg) * (geo + 1)) / (geo + 1)
            worst = max(worst, _ratio(r["depth_avg"], avg, D_avg, keep))
            # eval.py:256-264
            ys, xs = np.mgrid[0:h, 0:w]
            G = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5, np.ones(h * w)])
            Kri, eKri = _inv_err(K[ref])
            Ri, eRi = _inv_err(E[ref][:3, :3])
            uv, a = Kri @ G, avg.reshape(-1)
            cam = uv * a - E[ref][:3, 3:4].astype(F64)
            D_cam = 2 * (eKri @ G) * np.abs(a) + np.abs(uv) * D_avg.reshape(-1)
            D_w = (2 * eRi @ np.abs(cam) + np.abs(Ri) @ D_cam) * np.array([[1.0531], [1.0531], [1.0]]) * (1 + 1e-6)
            D_w = D_w + 8 * 2.0 ** -53 * np.abs(g("xyz_world").T)
        worst = max(worst, _ratio(r["xyz_world"], g("xyz_world"), D_w.T, np.repeat(keep.reshape(-1, 1), 3, 1)))
    assert worst <= 1.0, (name, worst)
    return worst


def oracle_pair_rows(sc):
    th, d, K, E = sc["th"], sc["depths"], sc["Ks"], sc["Es"]
    out = []
    for ref, srcs in sc["pairs"]:
        row = []
        for s in srcs[:th["n_view_filter"]]:
            m = fo.geometric_consistency(d[ref], K[ref], E[ref], d[s], K[s], E[s], th["condmask_pixel"],
                                         th["condmask_depth"])[0]
            row.append((m, fo.reproject(d[ref], K[ref], E[ref], d[s], K[s], E[s])[0]))
        out.append(row)
    return out


# ------------------------------------------------------------------------------------------------ defects
# name -> the scene that must catch it ("abi:<case>" = a direct-ABI case on the distinct-K scene)
DEFECTS = {
    "Kref_for_Ksrc_forward": "distinctK", "invKref_for_invKsrc_back": "distinctK", "T_for_T2": "distinctK",
    "no_translation_column": "distinctK", "no_skew": "distinctK", "round_truncates": "ties",
    "c_division_by_32": "ties", "replicate_border": "wide",
    "outside_left_off_by_one": "wide", "outside_right_off_by_one": "wide", "outside_top_off_by_one": "wide",
    "outside_bottom_off_by_one": "wide",
    # removing the clip outright changes nothing while the size guard holds w, h <= 32767 (the clipped and the
    # unclipped coordinate are both outside); what the clip protects against is the 16-bit store wrapping
    "short_wraps_instead_of_clipping": "limit_row",
    "dot3_in_f32": "distinctK", "sum_includes_failing_views": "distinctK", "average_over_geo": "distinctK",
    "photo_ge": "distinctK", "geo_gt": "distinctK", "condmask_depth_in_f64": "ties", "no_half_pixel": "distinctK",
    "factor_on_z": "distinctK", "R_for_invR": "distinctK", "plus_t": "distinctK",
    "minus1_is_view0": "abi:mixed", "minus1_breaks": "abi:mixed",
}


def _remap_d(src, mx, my, D):
    H, W = src.shape
    with np.errstate(all="ignore"):
        vx, vy = mx * F32(32), my * F32(32)
    if "round_truncates" in D:
        def rnd(v):
            r = np.trunc(v)
            ok = np.isfinite(r) & (r >= -2147483648.0) & (r < 2147483648.0)
            o = np.full(v.shape, INT_MIN, np.int64)
            o[ok] = r[ok].astype(np.int64)
            return o
    else:
        rnd = fo._cv_round
    sx, sy = rnd(vx), rnd(vy)
    fx = (sx & 31).astype(F32) / F32(32)
    fy = (sy & 31).astype(F32) / F32(32)
    if "c_division_by_32" in D:
        qx, qy = np.trunc(sx / 32).astype(np.int64), np.trunc(sy / 32).astype(np.int64)
    else:
        qx, qy = sx >> 5, sy >> 5
    if "short_wraps_instead_of_clipping" in D:
        ix, iy = ((qx + 32768) & 0xFFFF) - 32768, ((qy + 32768) & 0xFFFF) - 32768
    else:
        ix, iy = np.clip(qx, -32768, 32767), np.clip(qy, -32768, 32767)
    one = F32(1)
    wts = [(one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return v if "replicate_border" in D else np.where(ok, v, F32(0))

    with np.errstate(invalid="ignore", over="ignore"):
        out = tap(iy, ix) * wts[0]
        out = out + tap(iy, ix + 1) * wts[1]
        out = out + tap(iy + 1, ix) * wts[2]
        out = out + tap(iy + 1, ix + 1) * wts[3]
    gone = (ix >= W - ("outside_right_off_by_one" in D)) | (ix + 1 < ("outside_left_off_by_one" in D)) \
        | (iy >= H - ("outside_bottom_off_by_one" in D)) | (iy + 1 < ("outside_top_off_by_one" in D))
    return np.where(gone, F32(0), out).astype(F32)


def chain(sc, ref_idx=None, src_idx=None, defects=()):
    """The oracle's per-pixel chain in the kernel's calling convention, with the named defects switched on."""
    D = set(defects)
    assert D <= set(DEFECTS), D - set(DEFECTS)
    th, depth, conf, K, E = sc["th"], sc["depths"], sc["confs"], sc["Ks"], sc["Es"]
    if ref_idx is None:
        ref_idx, src_idx = abi_rows(sc)
    h, w = depth.shape[1:]
    xg, yg = fo._pix_rows(h, w)

    def dot3(m, a, b, c, skewless=False):
        if skewless:
            m = np.array([m[0], 0, m[2]])
        if "dot3_in_f32" in D:
            m = np.asarray(m, F32)
            return ((m[0] * a.astype(F32) + m[1] * b.astype(F32)) + m[2] * c.astype(F32)).astype(F64)
        m = np.asarray(m, F64)
        return (m[0] * a + m[1] * b) + m[2] * c

    def dot4(m, a, b, c):
        return dot3(m, a, b, c) + (F64(0) if "no_translation_column" in D else F64(m[3]))

    def mat3(M, a, b, c):
        return [dot3(M[i], a, b, c, skewless=("no_skew" in D and i == 0)) for i in range(3)]

    out = []
    for ref, row in zip(ref_idx, src_idx):
        ref = int(ref)
        d_ref, Kr, Er = depth[ref], K[ref], E[ref]
        Kri, Eri = fo._inv_f32(Kr), fo._inv_f32(Er)
        geo = np.zeros((h, w), np.int32)
        acc = np.zeros((h, w), F32)
        with np.errstate(all="ignore"):
            pix = np.stack([xg, yg, np.ones_like(xg)]) * d_ref.reshape(-1)
            p_ref = mat3(Kri, *pix)
            for s in row:
                s = int(s)
                if s < 0:
                    if "minus1_breaks" in D:
                        break
                    if "minus1_is_view0" not in D:
                        continue
                    s = 0
                Ks_, Es_ = K[s], E[s]
                Ksi, Esi = fo._inv_f32(Ks_), fo._inv_f32(Es_)
                T, T2 = fo._mm4_f32(Es_, Eri), fo._mm4_f32(Er, Esi)
                p_src = [dot4(T[i], *p_ref) for i in range(3)]
                q = mat3(Kr if "Kref_for_Ksrc_forward" in D else Ks_, *p_src)
                xs_, ys_ = q[0] / q[2], q[1] / q[2]
                x_src, y_src = xs_.reshape(h, w).astype(F32), ys_.reshape(h, w).astype(F32)
                sm = _remap_d(depth[s], x_src, y_src, D).reshape(-1).astype(F64)
                back = mat3(Kri if "invKref_for_invKsrc_back" in D else Ksi, xs_ * sm, ys_ * sm, sm)
                TT = T if "T_for_T2" in D else T2
                p_rep = [dot4(TT[i], *back) for i in range(3)]
                d_rep = p_rep[2].reshape(h, w).astype(F32)
                q2 = mat3(Kr, *p_rep)
                x_rep = (q2[0] / q2[2]).reshape(h, w).astype(F32)
                y_rep = (q2[1] / q2[2]).reshape(h, w).astype(F32)
                dx, dy = x_rep - xg.reshape(h, w), y_rep - yg.reshape(h, w)
                dist = np.sqrt(dx * dx + dy * dy)
                rel = np.abs(d_rep - d_ref) / d_ref
                if "condmask_depth_in_f64" in D:
                    okr = rel.astype(F64) < F64(th["condmask_depth"])
                else:
                    okr = rel < F32(th["condmask_depth"])
                ok = (dist < th["condmask_pixel"]) & okr
                geo = geo + ok.astype(np.int32)
                acc = acc + (d_rep if "sum_includes_failing_views" in D else np.where(ok, d_rep, F32(0)))
            avg = (acc + d_ref) / (geo if "average_over_geo" in D else geo + 1)
            pm = F32(th["photomask"])
            photo = conf[ref] >= pm if "photo_ge" in D else conf[ref] > pm
            gmask = geo > th["geomask"] if "geo_gt" in D else geo >= th["geomask"]
            half = 0.0 if "no_half_pixel" in D else 0.5
            gx, gy, one = xg + half, yg + half, np.ones(h * w)
            Ri = Er[:3, :3] if "R_for_invR" in D else fo._inv_f32(np.ascontiguousarray(Er[:3, :3]))
            a = avg.reshape(-1)
            sgn = -1.0 if "plus_t" in D else 1.0
            cam = [dot3(Kri[i], gx, gy, one, skewless=("no_skew" in D and i == 0)) * a - sgn * F64(Er[i, 3])
                   for i in range(3)]
            world = np.stack([dot3(Ri[i], *cam) for i in range(3)], axis=1)
            if "factor_on_z" in D:
                world = world * 1.0531
            else:
                world[:, :2] = world[:, :2] * 1.0531
        out.append(dict(geo_sum=geo, depth_avg=avg, photo=photo, geo=gmask, final=photo & gmask, xyz_world=world))
    return out


def defect_case(name):
    """(scene, ref_idx, src_idx) of the case that must catch defect `name`."""
    owner = DEFECTS[name]
    if owner.startswith("abi:"):
        return (scene("distinctK"),) + abi_case(owner[4:])
    sc = scene(owner)
    return (sc,) + abi_rows(sc)
