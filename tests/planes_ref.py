"""The yardstick of mvs_cloud_planes: include/ext/mvs_planes_abi.h's definition in numpy float64, operation for operation,
the workspace formula, and the bounds its tests hold the device to.

    members     normals_ref.members_of: box_min <= p <= box_max on every axis, both ends inclusive; q = p - o
    key         SplitMix64 in numpy uint64, which wraps modulo 2^64 like the device's unsigned long long
    candidates  the header's a, b, n, nn, d0, thr: numpy's float64 products, sums and differences are IEEE operations, one
                at a time, so every candidate here has the device's bits
    counts      s = ((n0*q0 + n1*q1) + n2*q2) - d0, s*s <= thr, vectorised over candidates x active members: integers,
                with no square root and no division, so the device's counts are these exactly
    sums        exact_sums: math.fsum over the inliers, the correctly rounded exact sum; tree_sums: the header's tree
                (groups of 256, then of 256, an xor butterfly inside each), which gives the device's bytes
    fit         fit(): the header's mean, covariance, Jacobi sweeps and sign in Python floats, the same operations in the
                same order; fit_eigh(): the same plane through numpy.linalg.eigh, another road to the same eigenvector
    labels      fabs(((n0*x + n1*y) + n2*z) + d) <= t on p itself
    segment     the header's loop.  With planes= (the device's own planes_out) the final inliers of every round are taken
                from those, so that everything else -- active sets, candidates, counts, winners, stops, labels -- has to be
                equal exactly, round after round, however the last bits of the two fits differ.

The bounds (u = 2^-53):
    sum_bound   A pairwise sum over a tree of depth h differs from the exact sum by at most gamma_h * sum|x| (Higham,
                Accuracy and Stability, section 4.2); fsum adds one rounding: (h + 1) u / (1 - (h + 1) u) * sum|terms|,
                h = tree_depth(P).  The terms carry no error: q and q[a]*q[b] are the same operations on both sides.
    plane_bound mean[a] = S_a / m and C[a][b] = S_ab / m - mean[a] mean[b]: from the sums' errors dS entry by entry,
                    dmean = dS_a / m + u |mean|
                    dC_ab = dS_ab / m + u |S_ab / m| + dmean_a |mean_b| + |mean_a| dmean_b + 2 u |mean_a mean_b| + u |C_ab|
                The Jacobi sweeps apply 24 rotations, each within 8 u ||C||_F of an exact similarity (the allowance of
                register_ref for its 4 x 4 sweeps), and what they leave off the diagonal is measured: `residual`, the
                largest off-diagonal entry after the sweeps in fit().  LAPACK's eigh on the other side gets the same 24
                rotations' allowance.  So ||dC||_2 <= 3 max dC_ab + 2 * 24 * 8 u ||C||_F + 3 residual, and the unit
                eigenvector of the smallest eigenvalue moves by at most dn = ||dC|| / (gap - ||dC||), gap = lambda_1 -
                lambda_0 (Davis-Kahan); normalising adds 4 u.  d = -(n . c), c = mean + o:
                    dd = sqrt(3) (dn + 4 u) max|c| + sum(dmean + u |c|) + 4 u sum|c|
"""
import math

import numpy as np

import normals_ref
import register_ref as RR

CANDIDATES_MAX, PLANES_MAX, SUMS, TILE, GROUP, FANIN, JACOBI_SWEEPS, SCALARS = 8192, 64, 9, 1024, 256, 256, 8, 512
MAX_PLANES, NO_PLANE, EXHAUSTED = 1, 2, 3
U = 2.0 ** -53
KEY_CHECK = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)      # key(0, 0), key(0, 1), key(0, 2)


# ---------------------------------------------------------------- the workspace and the tree
def levels(P):
    """[L_0, L_1, ..., 1]; [] for P == 0."""
    if P <= 0:
        return []
    out = [-(-P // GROUP)]
    while out[-1] > 1:
        out.append(-(-out[-1] // FANIN))
    return out


def workspace_bytes(P, K):
    T, K64 = -(-P // TILE), 64 * -(-K // 64)
    return 24 * P + 8 * ((T + 2) // 2) + 68 * K64 + 8 * SUMS * sum(levels(P)) + SCALARS


def tree_depth(P):
    """Additions on the longest path of the header's tree over P points."""
    return 8 * len(levels(P))


def tree_sums(terms):
    """The header's sum of every column of terms [P, k], literally -> [k]."""
    a = np.asarray(terms, np.float64)
    if len(a) == 0:
        return np.zeros(a.shape[1])
    a = RR._fold(a, GROUP)
    while len(a) > 1:
        a = RR._fold(a, FANIN)
    return a[0]


def sum_bound(terms):
    a = np.asarray(terms, np.float64)
    h = tree_depth(len(a)) + 1
    return h * U / (1 - h * U) * RR.exact_sums(np.abs(a))


# ---------------------------------------------------------------- keys, candidates, counts
def key(seed, i):
    """key(seed, i) of the header for an integer or an array of integers i -> uint64."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def candidates(q, r, K, seed, t):
    """The K candidates of round r over the active members' q [M,3] -> dict(ranks [K,3], n [K,3], nn, d0, thr, void [K])."""
    M = len(q)
    c = np.arange(K, dtype=np.uint64)
    base = np.uint64(3) * (np.uint64(r) * np.uint64(K) + c)
    ranks = np.stack([(key(seed, base + np.uint64(j)) % np.uint64(M)).astype(np.int64) for j in range(3)], axis=1)
    q0, q1, q2 = q[ranks[:, 0]], q[ranks[:, 1]], q[ranks[:, 2]]
    a, b = q1 - q0, q2 - q0
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        d0 = (n[:, 0] * q0[:, 0] + n[:, 1] * q0[:, 1]) + n[:, 2] * q0[:, 2]
        thr = (np.float64(t) * np.float64(t)) * nn
    void = (ranks[:, 0] == ranks[:, 1]) | (ranks[:, 0] == ranks[:, 2]) | (ranks[:, 1] == ranks[:, 2]) | ~(nn > 0) \
        | ~np.isfinite(nn) | ~np.isfinite(thr)
    return dict(ranks=ranks, n=n, nn=nn, d0=d0, thr=thr, void=void, q0=q0)


def inliers_of(q, cand, c):
    """The mask over q [M,3] of candidate c's inliers."""
    n, d0, thr = cand["n"][c], cand["d0"][c], cand["thr"][c]
    if cand["void"][c]:
        return np.zeros(len(q), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((n[0] * q[:, 0] + n[1] * q[:, 1]) + n[2] * q[:, 2]) - d0
        return s * s <= thr


def counts_of(q, cand, chunk=64):
    """count[c] of every candidate, vectorised [chunk, M] at a time -> int64 [K]."""
    K = len(cand["void"])
    out = np.zeros(K, np.int64)
    n, d0, thr = cand["n"], cand["d0"], cand["thr"]
    q0, q1, q2 = q[:, 0][None], q[:, 1][None], q[:, 2][None]
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, K, chunk):
            e = slice(a, a + chunk)
            s = ((n[e, 0:1] * q0 + n[e, 1:2] * q1) + n[e, 2:3] * q2) - d0[e, None]
            out[e] = (s * s <= thr[e, None]).sum(axis=1)
    out[cand["void"]] = 0
    return out


# ---------------------------------------------------------------- the fit
def terms_of(q, inl):
    """[P, 9]: the header's nine terms of every point, +0.0 where inl is False."""
    q = np.where(inl[:, None], q, 0.0)
    cols = [q[:, 0], q[:, 1], q[:, 2]] + [q[:, a] * q[:, b] for a in range(3) for b in range(a, 3)]
    return np.where(inl[:, None], np.stack(cols, axis=1), 0.0)


def _rotate(A, V, p, q, r):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = A[p][p] - t * apq
    A[q][q] = A[q][q] + t * apq
    A[p][q] = A[q][p] = 0.0
    arp, arq = A[r][p], A[r][q]
    A[r][p] = A[p][r] = c * arp - s * arq
    A[r][q] = A[q][r] = s * arp + c * arq
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = c * vkp - s * vkq
        V[k][q] = s * vkp + c * vkq


def orient(n, c, toward):
    a = [abs(v) for v in n]
    big = n[0] if a[0] >= a[1] and a[0] >= a[2] else n[1] if a[1] >= a[2] else n[2]
    pl = [-v for v in n] if big < 0.0 else list(n)
    pl.append(-((pl[0] * c[0] + pl[1] * c[1]) + pl[2] * c[2]))
    if toward is not None and ((pl[0] * toward[0] + pl[1] * toward[1]) + pl[2] * toward[2]) + pl[3] < 0.0:
        pl = [-v for v in pl]
    return pl


def covariance(sums, m):
    sums = [float(v) for v in sums]
    mean = [sums[a] / m for a in range(3)]
    A = [[0.0] * 3 for _ in range(3)]
    k = 3
    for a in range(3):
        for b in range(a, 3):
            A[a][b] = A[b][a] = sums[k] / m - mean[a] * mean[b]
            k += 1
    return mean, A


def fit(sums, m, o, toward=None, cand=None):
    """The header's plane from the nine sums over m inliers -> (plane [4], fitted: bool, residual: the largest off-diagonal
    entry the sweeps left).  cand = (n [3], q^0 [3]) is the candidate the header falls back to."""
    with np.errstate(all="ignore"):
        try:
            mean, A = covariance(sums, float(m))
            ok = all(math.isfinite(v) for v in mean) and all(math.isfinite(v) for row in A for v in row)
        except (ZeroDivisionError, OverflowError):
            ok = False
        residual = 0.0
        if ok:
            V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
            for _ in range(JACOBI_SWEEPS):
                _rotate(A, V, 0, 1, 2)
                _rotate(A, V, 0, 2, 1)
                _rotate(A, V, 1, 2, 0)
            residual = max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2]))
            use1 = A[1][1] < A[0][0]
            l01 = A[1][1] if use1 else A[0][0]
            col = 2 if A[2][2] < l01 else 1 if use1 else 0
            v = [V[a][col] for a in range(3)]
            length = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if length > 0.0 and math.isfinite(length):
                pl = orient([x / length for x in v], [mean[a] + o[a] for a in range(3)], toward)
                if math.isfinite(pl[3]):
                    return np.array(pl), True, residual
        n, q0 = [float(v) for v in cand[0]], [float(v) for v in cand[1]]
        length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        return np.array(orient([x / length for x in n], [q0[a] + o[a] for a in range(3)], toward)), False, residual


def fit_eigh(sums, m, o, toward=None):
    """The same plane by numpy.linalg.eigh -> (plane [4], eigenvalues ascending)."""
    mean, A = covariance(sums, float(m))
    w, v = np.linalg.eigh(np.array(A))
    return np.array(orient(list(v[:, 0]), [mean[a] + o[a] for a in range(3)], toward)), w


def plane_bound(sums, dsums, m, o, residual):
    """|device plane - reference plane| entry by entry [4] for sums within dsums of each other; see the head of this file."""
    sums, dsums, o = np.asarray(sums, np.float64), np.asarray(dsums, np.float64), np.asarray(o, np.float64)
    mean, A = covariance(sums, float(m))
    mean, C = np.array(mean), np.array(A)
    dmean = dsums[:3] / m + U * np.abs(mean)
    dC = np.zeros((3, 3))
    k = 3
    for a in range(3):
        for b in range(a, 3):
            dC[a, b] = dC[b, a] = dsums[k] / m + U * abs(sums[k] / m) + dmean[a] * abs(mean[b]) + abs(mean[a]) * dmean[b] \
                + 2 * U * abs(mean[a] * mean[b]) + U * abs(C[a, b])
            k += 1
    w = np.linalg.eigvalsh(C)
    gap = w[1] - w[0]
    norm = 3 * dC.max() + 2 * 3 * JACOBI_SWEEPS * 8 * U * np.linalg.norm(C, "fro") + 3 * residual
    assert norm < 0.25 * gap, "the normal is too close to ambiguous for a bound"
    dn = norm / (gap - norm) + 4 * U
    c = np.abs(mean + o)
    dd = math.sqrt(3) * dn * c.max() + (dmean + U * c).sum() + 4 * U * c.sum()
    return np.array([dn, dn, dn, dd])


# ---------------------------------------------------------------- labels and the loop
def on_plane(p, plane, t):
    with np.errstate(over="ignore", invalid="ignore"):
        v = ((plane[0] * p[:, 0] + plane[1] * p[:, 1]) + plane[2] * p[:, 2]) + plane[3]
        return np.abs(v) <= t, v


def segment(xyz, box_min, box_max, t, K, max_planes=1, min_inliers=3, seed=0, toward=None, planes=None, tree=False):
    """The header's loop -> dict(planes [max_planes,4] (NaN where none), rounds [max_planes,4] (-1 where not known), counts
    [4], labels [P], cand_counts [max_planes,K] (-1), sums [max_planes,9] (NaN): fsum's, or the tree's with tree=True,
    winners: per round that reached the fit dict(inl: the winner's inliers over all P, cand, fitted, residual),
    margin: the smallest | |value| - t | of any active point against any round's plane).
    planes: take the final inliers of round r from planes[r] (the device's) instead of from this fit."""
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    P = len(p)
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    o = 0.5 * (lo + hi)
    member = normals_ref.members_of(p, lo, hi) if P else np.zeros(0, bool)
    labels = np.where(member, -1, -2).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        q_all = p - o
    out_planes, rounds = np.full((max_planes, 4), np.nan), np.full((max_planes, 4), -1, np.int64)
    cand_counts, sums_out = np.full((max_planes, K), -1, np.int32), np.full((max_planes, SUMS), np.nan)
    winners, margin, found, stop = [], np.inf, 0, MAX_PLANES
    for r in range(max_planes):
        act = np.flatnonzero(labels == -1)
        M = len(act)
        rounds[r, 0] = M
        if M < 3:
            stop = EXHAUSTED
            break
        q = q_all[act]
        cand = candidates(q, r, K, seed, t)
        cnt = counts_of(q, cand)
        cand_counts[r] = cnt
        c = int(np.argmax(cnt))                    # the first of the largest
        rounds[r, 1:3] = c, cnt[c]
        if cnt[c] < min_inliers:
            stop = NO_PLANE
            break
        inl = np.zeros(P, bool)
        inl[act] = inliers_of(q, cand, c)
        assert inl.sum() == cnt[c]
        terms = terms_of(q_all, inl)
        sums = tree_sums(terms) if tree else RR.exact_sums(terms)
        sums_out[r] = sums
        pl, fitted, residual = fit(sums, cnt[c], o, toward, (cand["n"][c], cand["q0"][c]))
        winners.append(dict(inl=inl, cand=c, fitted=fitted, residual=residual, terms=terms))
        out_planes[r] = pl
        use = pl if planes is None else np.asarray(planes[r], np.float64)
        on, v = on_plane(p[act], use, t)
        if M:
            margin = min(margin, float(np.abs(np.abs(v) - t).min()))
        labels[act[on]] = r
        rounds[r, 3] = on.sum()
        found = r + 1
    on_planes = int((labels >= 0).sum())
    return dict(planes=out_planes, rounds=rounds, counts=np.array([member.sum(), found, on_planes, stop], np.int64),
                labels=labels, cand_counts=cand_counts, sums=sums_out, winners=winners, margin=margin)


# ---------------------------------------------------------------- the planted scene of the issue
SCENE_BOX = ((-300.0, -200.0, 590.0), (300.0, 200.0, 830.0))


def planted_scene(P, sigma=0.5):
    """A bin of 570 x 370 x 220 lifted to z = 600, numpy.random.default_rng(7), stored as float32: 50 % of the points on
    the floor, 20 % on the wall x = -285, 15 % on the wall y = 185, each with Gaussian noise sigma, 15 % uniform inside
    -> (xyz float32 [P,3], truth [P]: 0 floor, 1, 2 walls, 3 inside)."""
    rng = np.random.default_rng(7)
    n = [int(P * 0.5), int(P * 0.2), int(P * 0.15)]
    n.append(P - sum(n))
    lo, hi = np.array([-285.0, -185.0, 0.0]), np.array([285.0, 185.0, 220.0])
    f = rng.uniform(lo, hi, (n[0], 3))
    f[:, 2] = 0
    w1 = rng.uniform(lo, hi, (n[1], 3))
    w1[:, 0] = -285
    w2 = rng.uniform(lo, hi, (n[2], 3))
    w2[:, 1] = 185
    b = rng.uniform(lo + 20, hi - 20, (n[3], 3))
    x = np.concatenate([f, w1, w2, b])
    x[: sum(n[:3])] += rng.normal(0, sigma, (sum(n[:3]), 3))
    truth = np.concatenate([np.full(k, i) for i, k in enumerate(n)])
    perm = rng.permutation(P)
    return (x[perm] + np.array([0, 0, 600.0])).astype(np.float32), truth[perm]
