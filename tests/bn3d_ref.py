"""fp64 reference of the training batch-norm (+ ReLU, + skip) and of its backward, derived error bounds for the fp32
kernels of csrc/train_bn3d.hip, an fp32 numpy emulation of those kernels with switchable defects, and the cases.
Shared by tests/test_bn3d_ref_host.py (CPU) and tests/test_gpu_bn3d.py (GPU).

Written from the formulas of nn.BatchNorm3d in training mode (models/module.py:26-33, models/mvsnet.py:47-60, 66-70):
per channel, over the M rows of y [M, C],
    mean = sum y / M      var = sum (y - mean)^2 / M      invstd = 1 / sqrt(var + eps)      xhat = (y - mean) invstd
    pre = xhat gamma + beta      r = max(pre, 0) with relu      out = r + skip
    running <- (1 - momentum) running + momentum stat, the variance as var M / (M - 1)
    g = grad_out [pre > 0]      grad_beta = sum g      grad_gamma = sum g xhat
    grad_y = gamma invstd (g - grad_beta / M - xhat grad_gamma / M)
momentum and eps reach the kernels as fp32, so the reference rounds them to fp32 first: they are inputs, not errors.
reference() and bounds() use only operations numpy arrays and torch tensors share, so the largest case runs them on
the GPU in float64.

The kernels' structure (geometry()).  A block owns RPB = 8 R rows, R = 256 / (C / 4); thread (q, cg) owns the float4 of
channel group cg in the rows k = j R + q, j < 8.  Statistics: the thread's mean is a pairwise sum of <= 8 values divided
by their count, its M2 the pairwise sum of (v - mean)^2; a tree over q (log2 R levels) and then bn_stats_final_kernel
(slot s of S = 256 / C takes blocks s, s + S, ... one after another, then a tree over the slots) merge pairs by
    n = na + nb    wb = fl(nb) / fl(n)    wab = fl(na) wb    d = mb - ma    mean = ma + d wb    M2 = (qa + qb) + (d d) wab
so a value passes at most  Lm = log2 R + ceil(nblocks / S) + log2 S  merges.  The backward's two sums take the same
route with plain additions: at most  Ls = 3 + Lm  additions.  -ffp-contract=off: nothing is fused.

Bounds, u = 2^-24 (one fp32 rounding); every magnitude is the fp64 reference's own.  SQRT_U = DIV_U = 1 are
ASSUMPTIONS: sqrtf and the fp32 division are taken to be correctly rounded (<= u relative), which is what the compiler
emits by default for HIP; the first exact probe checks one value of each on the device.  First-order sums are doubled
once for the second-order terms.
  mean and var: a running error analysis, stat_bounds(), which walks the kernels' merge structure in fp64 and carries
    for every partial result its true mean m and M2 q and bounds dm, dq on the computed values' errors.
    thread (cnt <= 8 values): 3 additions and a division, dm = 4u sum |v| / cnt.  Its M2 is the sum of squares about
    its COMPUTED mean, q + cnt (mean error)^2 exactly (the cross term vanishes about the true mean); each term rounds
    3 times (sub, square), the sum 3 times: dq = 6u q + cnt dm^2.
    merge, d = mb - ma: d rounds once (u), wb carries two conversions and a division (3u), the product one (u), the
    addition u |m|; the inherited errors are averaged with the weights:
        dm = (1 - wb) dma + wb dmb + 5u |d| wb + u |m|
    the computed d is off by at most dma + dmb, so d^2 wab by wab (2 |d| (dma + dmb) + (dma + dmb)^2), its own
    roundings (d u twice, square u, wab 5u, product u, rounded up) 10u d^2 wab, the two additions 2u q:
        dq = dqa + dqb + wab (2 |d| (dma + dmb) + (dma + dmb)^2 + 10u d^2) + 2u q
    E_mean = 2 dm,  E_var = 2 (dq / M + 2u var)   (the division by fl(M) rounds twice).
    The mean enters dq only through dm ~ u |mean|, multiplied by |d| ~ std: the relative bound on var grows like
    u |mean| / std, never like u mean^2 / var, which is what E[y^2] - E[y]^2 loses.
  invstd: rho_is = E_var / (2 (var + eps)) + 2u (1 + SQRT_U + DIV_U)   relative.
  pre = ((y - mean) invstd) gamma + beta:  sub, mul, mul 3u; the last addition u |pre|:
        E_pre = |gamma| invstd [E_mean + |y - mean| (rho_is + 6u)] + 2u |pre|
    max(., 0) is 1-Lipschitz; the skip addition rounds once:  E_out = E_pre + 2u |out| [skip].
  running: keep = fl(1 - momentum) u, two products, one sum:
        E_run(stat) = momentum E_stat + 2u (2 |keep running| + |momentum stat| + |new|),
        E_unbiased = E_var M / (M - 1) + 4u var M / (M - 1)
  backward.  xhat: E_x = invstd E_mean + |xhat| (rho_is + 4u).  An element is AMBIGUOUS when |pre| <= E_pre: the
    kernel's mask (the sign of its own forward, bit for bit) may differ from the reference's there, which moves g by
    |grad_out|.
        E_gb = 2u Ls sum |g| + sum_amb |grad_out|
        E_gg = sum |g| (E_x + 2u |xhat|) + 2u Ls sum |g xhat| + sum_amb |grad_out| (|xhat| + E_x)
        mb = grad_beta / fl(M): E_mb = E_gb / M + 4u |mb|, mg likewise
        t = (g - mb) - xhat mg:  E_t = E_mb + 2u |g - mb| + E_x |mg| + |xhat| E_mg + 2u |xhat mg| + 2u |t|
        k = gamma invstd:  E_gy = |k| E_t + |k t| (rho_is + 4u) + |k| |grad_out| [ambiguous]
"""
import numpy as np

U = 2.0 ** -24
SQRT_U = 1     # assumption (module docstring)
DIV_U = 1      # assumption
BLOCK, ROWS = 256, 8
CHANNELS = (8, 16, 32, 64)

# (C, M): the smallest legal; the golden step's deepest level 2x2x3; ragged against any tile; many blocks, ragged;
# a B = 2 pooled batch
CASES = [(64, 2), (64, 12), (8, 1001), (16, 70001), (32, 2 * 4 * 4 * 6)]
FIELDS = ("normal", "heavy", "offset")
DEFECTS = ("naive_variance", "unbiased_norm", "biased_running", "skip_before_relu", "mask_from_out",
           "folded_backward", "no_mean_terms", "merge_weights")


def geometry(C, M):
    G = C // 4
    R = BLOCK // G
    RPB = ROWS * R
    nblocks = -(-M // RPB)
    S = BLOCK // C
    Lm = int(np.log2(R)) + -(-nblocks // S) + int(np.log2(S))
    return dict(G=G, R=R, RPB=RPB, nblocks=nblocks, S=S, Lm=Lm, Ls=3 + Lm)


def workspace_bytes(C, M):
    """Restatement of the library's formula: one (mean, M2) or (sum g, sum g xhat) pair of [C] floats per block."""
    return (geometry(C, M)["nblocks"] * 2 * C * 4 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def field(kind, C, M, seed):
    """y [M, C] fp32.  normal: unit normal times a per-channel scale; heavy: normal times exp(1.5 normal);
    offset: mean = 100 std, the case that separates a sound variance from E[y^2] - E[y]^2."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((M, C))
    scale = np.exp(rng.uniform(-1.0, 1.0, C))
    if kind == "heavy":
        y = y * np.exp(1.5 * rng.standard_normal((M, C)))
    if kind == "offset":
        y = y + 100.0 * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    assert kind in FIELDS
    return (y * scale).astype(np.float32)


def params(C, M, seed, skip=True, running=True):
    rng = np.random.default_rng(seed + 1000)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    p = dict(gamma=f(rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.25, -1.0, 1.0)),
             beta=f(rng.uniform(-0.5, 0.5, C)), go=f(rng.standard_normal((M, C))))
    p["skip"] = f(rng.standard_normal((M, C))) if skip else None
    p["rm"] = f(rng.standard_normal(C)) if running else None
    p["rv"] = f(rng.uniform(0.5, 2.0, C)) if running else None
    return p


def pm_one(C, M, seed):
    """y in {-1, +1}, in equal numbers within every aligned run of 256 rows (or of M rows, M < 256): every partial mean
    is then a ratio of small integers over a power of two and every merge is exact."""
    rng = np.random.default_rng(seed)
    run = min(M, 256)
    base = np.repeat(np.array([-1.0, 1.0], np.float32), run // 2)
    y = np.stack([np.concatenate([rng.permutation(base) for _ in range(M // run)]) for _ in range(C)], axis=1)
    return np.ascontiguousarray(y)


def edge_lattice(C, M, seed):
    """y on the integer lattice {-8 .. 7}, and beta chosen in fp64 so that the pre-activation of one lattice value per
    channel cancels: about 1/16 of the entries sit at the ReLU's edge, where the sign of pre is decided by the last
    rounding of the instruction sequence that computes it.  -> y, gamma, beta (fp32)."""
    rng = np.random.default_rng(seed)
    y = rng.integers(-8, 8, (M, C)).astype(np.float64)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64)
    v0 = rng.integers(-8, 8, C).astype(np.float64)
    mean = y.mean(0)
    invstd = (((y - mean) ** 2).mean(0)) ** -0.5      # eps = 0 in this probe
    beta = -(v0 - mean) * invstd * gamma
    return y.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32), v0.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the reference and its bounds (numpy float64 arrays or torch float64 tensors)
# ---------------------------------------------------------------------------------------------------------------
def _max0(a):
    return a.amax(0) if hasattr(a, "amax") else a.max(0)


def _min0(a):
    return a.amin(0) if hasattr(a, "amin") else a.min(0)


def reference(y, gamma, beta, skip=None, rm=None, rv=None, momentum=0.1, eps=1e-5, relu=True, go=None):
    M = y.shape[0]
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    mean = y.sum(0) / M
    yc = y - mean
    var = (yc * yc).sum(0) / M
    invstd = (var + eps) ** -0.5
    xhat = yc * invstd
    pre = xhat * gamma + beta
    r = pre.clip(min=0) if relu else pre
    out = r if skip is None else r + skip
    ref = dict(M=M, mom=mom, eps=eps, relu=relu, mean=mean, var=var, invstd=invstd, yc=yc, xhat=xhat, pre=pre, out=out)
    if rm is not None:
        ref["unbiased"] = var * (M / (M - 1.0))
        ref["rm"] = (1 - mom) * rm + mom * mean
        ref["rv"] = (1 - mom) * rv + mom * ref["unbiased"]
    if go is not None:
        g = go * (pre > 0) if relu else go
        gb = g.sum(0)
        gg = (g * xhat).sum(0)
        ref.update(g=g, grad_beta=gb, grad_gamma=gg, grad_y=gamma * invstd * (g - gb / M - xhat * (gg / M)))
    return ref


def bounds(ref, y, gamma, beta, skip=None, rm=None, rv=None, go=None):
    C, M = y.shape[1], ref["M"]
    geo = geometry(C, M)
    Lm, Ls = geo["Lm"], geo["Ls"]
    mom, var, invstd = ref["mom"], ref["var"], ref["invstd"]
    e_mean, e_var = stat_bounds(y)
    rho_is = e_var / (2 * (var + ref["eps"])) + 2 * U * (1 + SQRT_U + DIV_U)
    e_pre = abs(gamma) * invstd * (e_mean + abs(ref["yc"]) * (rho_is + 6 * U)) + 2 * U * abs(ref["pre"])
    e_out = e_pre if skip is None else e_pre + 2 * U * abs(ref["out"])
    b = dict(mean=e_mean, var=e_var, rho_is=rho_is, pre=e_pre, out=e_out)
    if rm is not None:
        e_unb = e_var * (M / (M - 1.0)) + 4 * U * ref["unbiased"]
        b["rm"] = mom * e_mean + 2 * U * (2 * abs((1 - mom) * rm) + abs(mom * ref["mean"]) + abs(ref["rm"]))
        b["rv"] = mom * e_unb + 2 * U * (2 * abs((1 - mom) * rv) + abs(mom * ref["unbiased"]) + abs(ref["rv"]))
    if go is not None:
        xhat, g = ref["xhat"], ref["g"]
        e_x = invstd * e_mean + abs(xhat) * (rho_is + 4 * U)
        flip = abs(go) * (abs(ref["pre"]) <= e_pre) if ref["relu"] else 0.0 * go
        e_gb = 2 * U * Ls * abs(g).sum(0) + flip.sum(0)
        e_gg = (abs(g) * (e_x + 2 * U * abs(xhat))).sum(0) + 2 * U * Ls * abs(g * xhat).sum(0) \
            + (flip * (abs(xhat) + e_x)).sum(0)
        mb, mg = ref["grad_beta"] / M, ref["grad_gamma"] / M
        e_mb, e_mg = e_gb / M + 4 * U * abs(mb), e_gg / M + 4 * U * abs(mg)
        t = g - mb - xhat * mg
        e_t = e_mb + 2 * U * abs(g - mb) + e_x * abs(mg) + abs(xhat) * e_mg + 2 * U * abs(xhat * mg) + 2 * U * abs(t)
        k = gamma * invstd
        b.update(grad_beta=e_gb, grad_gamma=e_gg, grad_y=abs(k) * e_t + abs(k * t) * (rho_is + 4 * U) + abs(k) * flip,
                 ambiguous=flip != 0)
    return b


def stat_bounds(y):
    """E_mean, E_var [C] of the module docstring for y [M, C] (numpy float64, or a torch tensor, whose device and dtype
    the result then takes)."""
    is_torch = not isinstance(y, np.ndarray)
    yn = y.detach().cpu().numpy() if is_torch else y
    M, C = yn.shape
    geo = geometry(C, M)
    nrows = _block_rows(geo, M)
    v = _tiles(yn, geo, np.float64)
    cnt = _cls(np.arange(geo["R"])[None, :, None], geo["R"], nrows[:, None, None])
    live = np.arange(ROWS)[None, :, None, None] < cnt[:, None]
    c1 = np.maximum(cnt, 1)
    m = v.sum(1) / c1
    q = np.where(live, (v - m[:, None]) ** 2, 0.0).sum(1)
    dm = 4 * U * np.abs(v).sum(1) / c1
    dq = 6 * U * q + cnt * dm * dm

    def merge(a, b, na, nb):
        (ma, qa, dma, dqa), (mb, qb, dmb, dqb) = a, b
        n = na + nb
        wb = nb / np.maximum(n, 1)
        wab = na * wb
        d, dd = mb - ma, dma + dmb
        mn = ma + d * wb
        qn = qa + qb + d * d * wab
        return (mn, qn, (1 - wb) * dma + wb * dmb + 5 * U * np.abs(d) * wb + U * np.abs(mn),
                dqa + dqb + wab * (2 * np.abs(d) * dd + dd * dd + 10 * U * d * d) + 2 * U * qn)

    parts = _tree_q((m, q, dm, dq), geo, nrows, merge)
    m, q, dm, dq = _final(parts, nrows, geo, merge)
    e_mean, e_var = 2 * dm, 2 * (dq / M + 2 * U * q / M)
    if is_torch:
        import torch
        e_mean, e_var = (torch.from_numpy(a).to(device=y.device, dtype=y.dtype) for a in (e_mean, e_var))
    return e_mean, e_var


def worst(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0): <= 1 means inside the bound."""
    err = abs(got - want)
    ratio = err / (bound + (bound == 0) * 1.0)
    ratio = ratio + ((err > 0) & (bound == 0)) * (err * 0 + 1e30)   # an error where the bound is 0 is outside it
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels: one numpy operation per device operation, with the block and merge structure
# ---------------------------------------------------------------------------------------------------------------
F = np.float32


def _cls(q, m, nrows):
    return np.where(q < nrows, (nrows - q - 1) // m + 1, 0)


def _tiles(a, geo, dtype=None):
    """[M, C] -> [nblocks, 8, R, C] (row k = j R + q of a block), zero-filled past M as the kernels' guarded loads."""
    M, C = a.shape
    p = np.zeros((geo["nblocks"] * geo["RPB"], C), dtype or F)
    p[:M] = a
    return p.reshape(geo["nblocks"], ROWS, geo["R"], C)


def _sum8(t):
    return ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7]))


def _merge(ma, qa, mb, qb, na, nb, equal_weights=False):
    n = na + nb
    wb = nb.astype(F) / np.maximum(n, 1).astype(F)
    if equal_weights:                                  # defect: every pair merged as if both sides counted alike
        wb = np.where(n > 0, F(0.5), F(0)) + F(0) * wb
    wab = na.astype(F) * wb
    d = mb - ma
    return ma + d * wb, (qa + qb) + (d * d) * wab


def _block_rows(geo, M):
    return np.minimum(geo["RPB"], M - np.arange(geo["nblocks"]) * geo["RPB"])


def _tree_q(vals, geo, nrows, merge):
    """the LDS tree over q; vals: tuple of [nblocks, R, C]; merge(a_vals, b_vals, na, nb) -> vals."""
    s = geo["R"] // 2
    while s >= 1:
        q = np.arange(s)[None, :, None]
        nr = nrows[:, None, None]
        na, nb = _cls(q, 2 * s, nr), _cls(q + s, 2 * s, nr)
        vals = merge(tuple(v[:, :s] for v in vals), tuple(v[:, s:2 * s] for v in vals), na, nb)
        s //= 2
    return tuple(v[:, 0] for v in vals)


def _final(parts, counts, geo, merge):
    """the one-block second kernel; parts: tuple of [nblocks, C], counts [nblocks] -> tuple of [C]."""
    S, nblocks = geo["S"], geo["nblocks"]
    C = parts[0].shape[1]
    rounds = -(-nblocks // S)
    pad = rounds * S - nblocks
    dt = parts[0].dtype
    parts = tuple(np.concatenate([p, np.zeros((pad, C), dt)]).reshape(rounds, S, C) for p in parts)
    cnt = np.concatenate([counts, np.zeros(pad, np.int64)]).reshape(rounds, S, 1)
    acc = tuple(np.zeros((S, C), dt) for _ in parts)
    n = np.zeros((S, 1), np.int64)
    for i in range(rounds):
        acc = merge(acc, tuple(p[i] for p in parts), n, cnt[i])
        n = n + cnt[i]
    s = S // 2
    while s >= 1:
        acc = merge(tuple(a[:s] for a in acc), tuple(a[s:2 * s] for a in acc), n[:s], n[s:2 * s])
        n = n[:s] + n[s:2 * s]
        s //= 2
    return tuple(a[0] for a in acc)


def emulate_forward(y, gamma, beta, skip=None, rm=None, rv=None, momentum=0.1, eps=1e-5, relu=True, defects=()):
    """-> dict(mean, invstd, var, out, pre, rm, rv) in fp32, computed as bn_stats_kernel, bn_stats_final_kernel and
    bn_apply_kernel compute them.  Defect "nan_channel_leaks" (not in DEFECTS: it shows on non-finite input only,
    tests/test_nonfinite_train_host.py): the last merge also reads the partial of the neighbouring channel group,
    behind a weight of 0."""
    M, C = y.shape
    geo = geometry(C, M)
    y, gamma, beta = y.astype(F), gamma.astype(F), beta.astype(F)
    mom, eps = F(momentum), F(eps)
    nrows = _block_rows(geo, M)
    v = _tiles(y, geo)
    q = np.arange(geo["R"])[None, :, None]
    cnt = _cls(q, geo["R"], nrows[:, None, None])                       # [nblocks, R, 1]
    mean_t = _sum8(v) / np.maximum(cnt, 1).astype(F)
    dev = v - mean_t[:, None]
    live = np.arange(ROWS)[None, :, None, None] < cnt[:, None]
    m2_t = _sum8(np.where(live, dev * dev, F(0)))
    eq = "merge_weights" in defects

    def merge(a, b, na, nb):
        return _merge(a[0], a[1], b[0], b[1], na, nb, equal_weights=eq)

    pm, pq = _tree_q((mean_t, m2_t), geo, nrows, merge)
    mean, m2 = _final((pm, pq), nrows, geo, merge)
    if "nan_channel_leaks" in defects:
        mean, m2 = mean + F(0) * np.roll(mean, 4), m2 + F(0) * np.roll(m2, 4)
    var = m2 / F(M)
    if "naive_variance" in defects:                                     # E[y^2] - E[y]^2 from fp32 sums
        mean = np.sum(y, 0, dtype=F) / F(M)
        var = np.sum(y * y, 0, dtype=F) / F(M) - mean * mean
        m2 = var * F(M)
    unbiased = m2 / F(M - 1)
    invstd = F(1) / np.sqrt((unbiased if "unbiased_norm" in defects else var) + eps)
    pre = ((y - mean) * invstd) * gamma + beta
    if skip is not None and "skip_before_relu" in defects:
        pre_s = pre + skip.astype(F)
        out = np.where(~(pre_s <= 0), pre_s, F(0)) if relu else pre_s
    else:
        out = np.where(~(pre <= 0), pre, F(0)) if relu else pre
        if skip is not None:
            out = out + skip.astype(F)
    res = dict(mean=mean, var=var, invstd=invstd, pre=pre, out=out)
    if rm is not None:
        keep = F(1) - mom
        res["rm"] = keep * rm.astype(F) + mom * mean
        res["rv"] = keep * rv.astype(F) + mom * (var if "biased_running" in defects else unbiased)
    assert all(a.dtype == F for a in res.values())
    return res


def emulate_mask(y, gamma, beta, mean, invstd, defects=(), out=None):
    """the backward's ReLU mask: closed where pre <= 0, so that a NaN pre-activation passes (as the forward's ReLU
    and torch's threshold_backward)."""
    if "mask_from_out" in defects:                  # defect: the stored output, which includes the skip
        return out > 0
    if "folded_backward" in defects:                # defect: pre recomputed as a y + b
        a = gamma * invstd
        return ~(a * y + (beta - mean * a) <= 0)
    return ~(((y - mean) * invstd) * gamma + beta <= 0)


def emulate_backward(y, go, gamma, beta, mean, invstd, relu=True, defects=(), out=None):
    """-> dict(grad_y, grad_gamma, grad_beta, mask) in fp32, as bn_bwd_sums_kernel, bn_bwd_final_kernel and
    bn_bwd_apply_kernel compute them from the forward's saved mean and invstd."""
    M, C = y.shape
    geo = geometry(C, M)
    y, go, gamma, beta = y.astype(F), go.astype(F), gamma.astype(F), beta.astype(F)
    mask = emulate_mask(y, gamma, beta, mean, invstd, defects, out) if relu else np.ones(y.shape, bool)
    g = np.where(mask, go, F(0))
    xhat = (y - mean) * invstd
    add = lambda a, b, na, nb: (a[0] + b[0], a[1] + b[1])  # noqa: E731
    nrows = _block_rows(geo, M)
    pa, pb = _tree_q((_sum8(_tiles(g, geo)), _sum8(_tiles(g * xhat, geo))), geo, nrows, add)
    gb, gg = _final((pa, pb), nrows, geo, add)
    k = gamma * invstd
    if "no_mean_terms" in defects:
        gy = k * g
    else:
        gy = k * ((g - gb / F(M)) - xhat * (gg / F(M)))
    res = dict(grad_y=gy, grad_gamma=gg, grad_beta=gb)
    assert all(a.dtype == F for a in res.values())
    res["mask"] = mask
    return res


def check_forward(got, ref, bnd, label="", report=print):
    """got: dict with mean, var (or invstd), out and, when the reference has them, rm, rv.  -> worst ratios."""
    ratios = {}
    for key in ("mean", "var", "out", "rm", "rv"):
        if key in got and key in ref:
            ratios[key] = worst(np.asarray(got[key], np.float64), ref[key], bnd[key])
    if "invstd" in got:
        ratios["invstd"] = worst(np.asarray(got["invstd"], np.float64), ref["invstd"], bnd["rho_is"] * ref["invstd"])
    report(f"{label} forward worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios


def check_backward(got, ref, bnd, label="", report=print):
    ratios = {k: worst(np.asarray(got[k], np.float64), ref[k], bnd[k]) for k in ("grad_beta", "grad_gamma", "grad_y")}
    report(f"{label} backward worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios
