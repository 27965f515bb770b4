"""The yardstick of mvs_cloud_register: include/ext/mvs_register_abi.h's definition in numpy float64, and the bounds its
tests hold the device to.

    members     normals_ref.members_of: box_min <= q <= box_max on every axis, both ends inclusive
    counted     a source whose three coordinates are finite
    image       s[a] = ((R[a][0]*p[0] + R[a][1]*p[1]) + R[a][2]*p[2]) + t[a]
    nearest     brute force: d2 = (dx*dx + dy*dy) + dz*dz with d = q[j] - s; np.argmin returns the first minimum and the
                members are taken in ascending j, which is the smallest (d2, j); kept iff d2 <= max_dist * max_dist
    terms       the header's 31 per source, in its operation order: numpy's float64 products, sums and differences are
                IEEE operations, one at a time, so a term computed here from the device's T_k has the device's bits
    sums        exact_sums: math.fsum over the sources, the correctly rounded exact sum; tree_sums: the header's tree
                (groups of 32, then of 256, an xor butterfly inside each), which gives the device's bytes
    step        point-to-plane: numpy.linalg.solve of A x = -b, then the header's Rz Ry Rx; point-to-point: Kabsch through
                numpy.linalg.svd with the determinant fix (the device takes Horn's quaternion instead: another road to the
                same rotation), cross-checked against scipy's Rotation.align_vectors in tests/test_cloud_register_host.py
    loop        the header's: evaluate, history, converged / max_iterations / degenerate, T_{k+1} = dT T_k

The bounds (u = 2^-53):
    sum_bound   A pairwise sum over a tree of depth h differs from the exact sum by at most gamma_h * sum|x|, gamma_h =
                h u / (1 - h u) (Higham, Accuracy and Stability, section 4.2); fsum adds one rounding of the result.  The
                terms themselves carry no error: both sides form them from the same T_k by the same operations.  So
                |device sum - fsum| <= (h + 1) u / (1 - (h + 1) u) * sum|terms|, h = tree_depth(N).
    plane_step_bound  x solves A x = -b.  The device's A and b are within sum_bound of the reference's; LDL^T without
                pivoting on a positive definite A has the backward error of Cholesky, |dA| <= gamma_{3n+1} |L||D||L^T|,
                whose 2-norm is at most n gamma_{3n+1} ||A||_2 (Higham, theorem 10.3 and (10.7)); numpy's LU is given the
                same allowance.  With dA the sum of the three and db likewise, ||dx|| <= ||A^-1|| (||db|| + ||dA|| ||x||) /
                (1 - ||A^-1|| ||dA||) (theorem 7.2).  Each entry of Rz Ry Rx has a gradient of norm <= sqrt(3) in the
                three angles, sin and cos are taken to 2 ulps and an entry is three products and a sum away: sqrt(3) ||dx||
                + 16 u for the rotation, ||dx|| for the translation.
    point_step_bound  S = Sxy - Sx Sy / n entry by entry from the sum bounds; Horn's N is sums of three entries of S, so
                ||dN||_2 <= 4 max|dN_ij| <= 4 (3 max|dS| + 9 u max|S|); the Jacobi sweeps apply 60 rotations, each within
                8 u ||N||_F of an exact similarity, and LAPACK's SVD on the other side is given the same allowance.  The
                unit eigenvector of the largest eigenvalue moves by at most dN / (gap - dN) with gap = lambda_1 - lambda_2
                (Davis-Kahan).  An entry of R is quadratic in the unit quaternion with a gradient of norm 2, so |dR_ij|
                <= 2 dq (1 + dq) + 16 u, and t = (mq + o) - R (ms + o) follows entry by entry.
    transform_bound   T_{k+1} = dT T_k in four products and three sums per entry: |dT_err| |T_k| + 8 u |dT| |T_k|.
    loop        With the same correspondences on both sides a point-to-point T_{k+1} minimises sum |T p - q|^2 over the
                rigid T and so does not depend on T_k at all, and a point-to-plane T_{k+1} depends on T_k through the
                linearisation only, with a factor of the order of the step's angle, below 1 for every step under a
                radian.  So the errors of the steps add at most: the loop's bound is the sum of the step bounds along
                the reference's own trajectory, as long as the correspondences agree, which the relative gap between the
                nearest and the second-nearest d2 guarantees (nearest_gap).
"""
import math

import numpy as np

import normals_ref

TERMS, HISTORY, GROUP, FANIN, SCALARS, ITERATIONS_MAX, JACOBI_SWEEPS = 31, 19, 32, 256, 512, 1000, 10
TERMS_POINT = 18
CONVERGED, MAX_ITERATIONS, DEGENERATE = 1, 2, 3
U = 2.0 ** -53


# ---------------------------------------------------------------- the workspace and the tree
def levels(N):
    """[L_0, L_1, ..., 1]; [] for N == 0."""
    if N <= 0:
        return []
    out = [-(-N // GROUP)]
    while out[-1] > 1:
        out.append(-(-out[-1] // FANIN))
    return out


def workspace_bytes(P, N, box_min, box_max, cell):
    return normals_ref.workspace_bytes(P, box_min, box_max, cell) + 8 * TERMS * sum(levels(N)) + SCALARS


def tree_depth(N):
    """Additions on the longest path of the header's tree over N sources."""
    return 5 * bool(levels(N)) + 8 * max(len(levels(N)) - 1, 0)


def _fold(a, width):
    """[n, k] -> [ceil(n / width), k]: each `width` consecutive rows summed by the xor butterfly, +0.0 past the end."""
    n = len(a)
    pad = -(-n // width) * width - n
    a = np.concatenate([a, np.zeros((pad,) + a.shape[1:])]).reshape(-1, width, *a.shape[1:])
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def tree_sums(terms):
    """The header's sum of every column of terms [N, k], literally -> [k]."""
    a = np.asarray(terms, np.float64)
    if len(a) == 0:
        return np.zeros(a.shape[1])
    a = _fold(a, GROUP)
    while len(a) > 1:
        a = _fold(a, FANIN)
    return a[0]


def exact_sums(terms):
    a = np.asarray(terms, np.float64)
    return np.array([math.fsum(a[:, k][a[:, k] != 0]) for k in range(a.shape[1])])      # zeros add nothing: most rows of a long cloud


def sum_bound(terms):
    """|tree sum - fsum| of every column, see the head of this file."""
    a = np.asarray(terms, np.float64)
    h = tree_depth(len(a)) + 1
    return h * U / (1 - h * U) * exact_sums(np.abs(a))


# ---------------------------------------------------------------- evaluate
def image(T, p):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def nearest(target, box_min, box_max, s, max_dist, chunk=256, second=False):
    """-> (idx int32 [n] (-1: none), d2 [n]) of the images s [n,3], all finite; with second=True also the smallest d2 of
    any OTHER member (inf for none), whatever max_dist is."""
    r = np.asarray(target).astype(np.float64).reshape(-1, 3)
    ids = np.flatnonzero(normals_ref.members_of(r, box_min, box_max))
    m = r[ids]
    n = len(s)
    idx, best, nxt = np.full(n, -1, np.int32), np.full(n, np.inf), np.full(n, np.inf)
    cap = np.float64(max_dist) * np.float64(max_dist)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, n if len(ids) else 0, chunk):
            d = m[None, :, :] - s[a:a + chunk, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d2 = np.where(np.isfinite(d2), d2, np.inf)
            j = np.argmin(d2, axis=1)
            rows = np.arange(len(j))
            b = d2[rows, j]
            if second and len(ids) > 1:
                d2[rows, j] = np.inf
                nxt[a:a + chunk] = d2.min(axis=1)
            ok = np.isfinite(b) & ~(b > cap)
            idx[a:a + chunk][ok] = ids[j[ok]]
            best[a:a + chunk] = np.where(ok, b, np.inf)
    return (idx, best, nxt) if second else (idx, best)


def evaluate(T, source, target, normals, box_min, box_max, max_dist, second=False):
    """Evaluate(T) -> dict(idx [N], terms [N, 31], counted, inlier, gap: the smallest relative gap (d2' - d2) / d2' between
    an inlier's nearest and second-nearest member, with second=True)."""
    p = np.asarray(source).astype(np.float64).reshape(-1, 3)
    q = np.asarray(target).astype(np.float64).reshape(-1, 3)
    N = len(p)
    counted = np.isfinite(p).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        s = image(T, np.where(counted[:, None], p, 0.0))
    searched = counted & np.isfinite(s).all(axis=1)
    idx, d2 = np.full(N, -1, np.int32), np.full(N, np.inf)
    got = nearest(q, box_min, box_max, s[searched], max_dist, second=second)
    idx[searched], d2[searched] = got[0], got[1]
    inlier = idx >= 0
    terms = np.zeros((N, TERMS))
    terms[:, 0] = counted
    terms[:, 1] = inlier
    terms[inlier, 2] = d2[inlier]
    si, qi = s[inlier], q[idx[inlier]]
    if normals is None:
        o = 0.5 * (np.asarray(box_min, np.float64) + np.asarray(box_max, np.float64))
        sp, qp = si - o, qi - o
        terms[inlier, 3:6], terms[inlier, 6:9] = sp, qp
        for a in range(3):
            for b in range(3):
                terms[inlier, 9 + 3 * a + b] = sp[:, a] * qp[:, b]
    else:
        n = np.asarray(normals).astype(np.float64).reshape(-1, 3)[idx[inlier]]
        ok = np.isfinite(n).all(axis=1)
        n = np.where(ok[:, None], n, 0.0)
        e = si - qi
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        J = np.stack([si[:, 1] * n[:, 2] - si[:, 2] * n[:, 1], si[:, 2] * n[:, 0] - si[:, 0] * n[:, 2],
                      si[:, 0] * n[:, 1] - si[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
        block = np.zeros((len(si), TERMS - 3))
        t = 0
        for a in range(6):
            for b in range(a, 6):
                block[:, t] = J[:, a] * J[:, b]
                t += 1
        for a in range(6):
            block[:, 21 + a] = J[:, a] * r
        block[:, 27] = r * r
        terms[inlier, 3:] = np.where(ok[:, None], block, 0.0)
    out = dict(idx=idx, terms=terms, counted=counted, inlier=inlier, d2=d2)
    if second:
        nxt = np.full(N, np.inf)
        nxt[searched] = got[2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gaps = np.where(inlier & np.isfinite(nxt) & (nxt > 0), (nxt - d2) / nxt, 1.0)
        out["gap"] = float(gaps[inlier].min()) if inlier.any() else 1.0
    return out


def fitness_rmse(sums):
    n_counted, n_inliers = sums[0], sums[1]
    return (n_inliers / n_counted if n_counted > 0 else 0.0), (math.sqrt(sums[2] / n_inliers) if n_inliers > 0 else 0.0)


# ---------------------------------------------------------------- the step
def vector6_to_matrix(x):
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    T = np.eye(4)
    T[0, :3] = [cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa]
    T[1, :3] = [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa]
    T[2, :3] = [-sb, cb * sa, cb * ca]
    T[:3, 3] = x[3:6]
    return T


def plane_system(sums):
    A = np.zeros((6, 6))
    t = 3
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[t]
            t += 1
    return A, np.asarray(sums[24:30], np.float64)


def ldlt_pivots(A):
    """The pivots d[j] of the header's LDL^T, in its operation order."""
    a = np.array(A, np.float64)
    d = []
    for j in range(6):
        v = a[j, j]
        for m in range(j):
            v = v - (a[j, m] * a[j, m]) * a[m, m]
        d.append(v)
        if not (v > 0 and math.isfinite(v)):
            break
        a[j, j] = v
        for i in range(j + 1, 6):
            w = a[j, i]
            for m in range(j):
                w = w - (a[i, m] * a[j, m]) * a[m, m]
            a[i, j] = w / v
    return d


def kabsch(S):
    """The proper rotation R maximising trace(R S) for S[a][b] = sum source[a] * target[b]: target ~ R source."""
    Uu, _, Vt = np.linalg.svd(S)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ Uu.T)) or 1.0])
    return Vt.T @ D @ Uu.T


def horn_matrix(S):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = np.asarray(S, np.float64)
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def covariance(sums):
    n = sums[1]
    return np.array([[sums[9 + 3 * a + b] - (sums[3 + a] * sums[6 + b]) / n for b in range(3)] for a in range(3)])


def step(sums, plane, origin):
    """dT [4,4] of the header's step from the reduced sums, or None where it is degenerate."""
    sums = np.asarray(sums, np.float64)
    used = TERMS if plane else TERMS_POINT
    if sums[1] < (6 if plane else 3) or not np.isfinite(sums[:used]).all():
        return None
    if plane:
        A, b = plane_system(sums)
        d = ldlt_pivots(A)
        if len(d) < 6 or not all(v > 0 and math.isfinite(v) for v in d):
            return None
        dT = vector6_to_matrix(np.linalg.solve(A, -b))
    else:
        n, o = sums[1], np.asarray(origin, np.float64)
        S = covariance(sums)
        if not np.isfinite(S).all():
            return None
        R = kabsch(S)
        dT = np.eye(4)
        dT[:3, :3] = R
        dT[:3, 3] = (sums[6:9] / n + o) - R @ (sums[3:6] / n + o)
    return dT if np.isfinite(dT).all() else None


def compose(A, B):
    C = np.eye(4)
    for i in range(3):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


# ---------------------------------------------------------------- the bounds of one step
def plane_step_bound(sums, dsums):
    """|dT_device - dT_reference| entry by entry [4,4] for sums within dsums of each other, see the head of this file."""
    A, b = plane_system(sums)
    dA, db = plane_system(dsums)
    x = np.linalg.solve(A, -b)
    inv = np.linalg.norm(np.linalg.inv(A), 2)
    g = 19 * U / (1 - 19 * U)
    nA = np.linalg.norm(dA, "fro") + 2 * 6 * g * np.linalg.norm(A, 2)
    nb = np.linalg.norm(db) + 2 * 6 * g * np.linalg.norm(b)
    assert inv * nA < 0.5, "the system is too close to singular for a bound"
    dx = inv * (nb + nA * np.linalg.norm(x)) / (1 - inv * nA)
    out = np.zeros((4, 4))
    out[:3, :3] = math.sqrt(3) * dx + 16 * U
    out[:3, 3] = dx
    return out


def point_step_bound(sums, dsums, origin):
    sums, dsums = np.asarray(sums, np.float64), np.asarray(dsums, np.float64)
    n, o = sums[1], np.abs(np.asarray(origin, np.float64))
    S = covariance(sums)
    dS = np.array([[dsums[9 + 3 * a + b] + (dsums[3 + a] * abs(sums[6 + b]) + abs(sums[3 + a]) * dsums[6 + b]
                                            + 3 * U * abs(sums[3 + a] * sums[6 + b])) / n + U * abs(S[a, b])
                    for b in range(3)] for a in range(3)])
    Nm = horn_matrix(S)
    lam = np.linalg.eigvalsh(Nm)
    gap = lam[-1] - lam[-2]
    dN = 4 * (3 * dS.max() + 9 * U * np.abs(S).max()) + 2 * 60 * 8 * U * np.linalg.norm(Nm, "fro")
    assert dN < 0.25 * gap, "the rotation is too close to ambiguous for a bound"
    dq = dN / (gap - dN)
    dR = 2 * dq * (1 + dq) + 16 * U
    cs, cq = np.abs(sums[3:6]) / n + o, np.abs(sums[6:9]) / n + o
    dcs, dcq = dsums[3:6] / n + 2 * U * cs, dsums[6:9] / n + 2 * U * cq
    out = np.zeros((4, 4))
    out[:3, :3] = dR
    out[:3, 3] = dcq + dR * cs.sum() + dcs.sum() + 8 * U * (cq + cs.sum())
    return out


def transform_bound(dT, ddT, T):
    return np.abs(ddT) @ np.abs(T) + 8 * U * (np.abs(dT) @ np.abs(T))


def step_bound(sums, dsums, plane, origin, T):
    """|T_{k+1, device} - T_{k+1, reference}| [4,4] when both start from the same T and the same correspondences."""
    dT = step(sums, plane, origin)
    ddT = plane_step_bound(sums, dsums) if plane else point_step_bound(sums, dsums, origin)
    return transform_bound(dT, ddT, T)


# ---------------------------------------------------------------- the loop
def icp(source, target, box_min, box_max, max_dist, normals=None, init=None, max_iterations=30, rel_fitness=1e-6,
        rel_rmse=1e-6, bounds=False):
    """The header's loop on the CPU, with exact sums -> dict(T, counts [4], stats [2], history [max_iterations + 1, 19], idx,
    and with bounds=True: bound [4,4], the sum of the step bounds; gap, the smallest nearest_gap of any evaluation;
    margin, how far the convergence test was from flipping at its closest, in units of its thresholds)."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    plane = normals is not None
    origin = 0.5 * (np.asarray(box_min, np.float64) + np.asarray(box_max, np.float64))
    history = np.full((max_iterations + 1, HISTORY), np.nan)
    total, gap, margin, prev = np.zeros((4, 4)), 1.0, np.inf, None
    for k in range(max_iterations + 1):
        ev = evaluate(T, source, target, normals, box_min, box_max, max_dist, second=bounds)
        sums = exact_sums(ev["terms"])
        fit, rmse = fitness_rmse(sums)
        history[k, :16], history[k, 16:] = T.reshape(-1), (fit, rmse, sums[1])
        if bounds:
            gap = min(gap, ev["gap"])
        stop = 0
        if k > 0:
            if rel_fitness > 0 and rel_rmse > 0:
                margin = min(margin, max(abs(abs(fit - prev[0]) / rel_fitness - 1), abs(abs(rmse - prev[1]) / rel_rmse - 1)))
            if abs(fit - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
                stop = CONVERGED
        if not stop and k == max_iterations:
            stop = MAX_ITERATIONS
        if not stop:
            dT = step(sums, plane, origin)
            if dT is None:
                stop = DEGENERATE
            else:
                if bounds:
                    total += step_bound(sums, sum_bound(ev["terms"]), plane, origin, T)
                T, prev = compose(dT, T), (fit, rmse)
        if stop:
            out = dict(T=T, counts=[int(sums[0]), int(sums[1]), k, stop], stats=np.array([fit, rmse]), history=history,
                       idx=ev["idx"])
            if bounds:
                out.update(bound=total, gap=gap, margin=margin)
            return out
