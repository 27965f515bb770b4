"""The yardstick of mvs_cloud_normals and mvs_cloud_downsample_normals: include/mvs_normals_abi.h's definitions in numpy
float64 (Open3D's estimate_normals restated, with the sign specified; neither Open3D nor scipy is needed).

    members     box_min <= p <= box_max on every axis, both ends inclusive, on the value as float64
    neighbours  the min(knn, M) members with the smallest (d2, index), d2 = (dx*dx + dy*dy) + dz*dz: brute force over all
                members in chunks, np.lexsort on (index, d2)
    covariance  mean = sum / m, C = sum (q - mean)(q - mean)^T / m, both summed in ascending (d2, index)
    normal      numpy.linalg.eigh's eigenvector of the smallest eigenvalue; (0, 0, 1) for m < 3 and for C == 0
    sign        towards centres[r] for view_starts[r] <= i < view_starts[r+1]; else the largest component positive

The angle bound (`angle_bound`, radians, per member).  The kernel and this file each compute a covariance and an
eigenvector of it in double.  Let s = the largest |q - mean|^2 of the neighbourhood and u = 2^-53.
  * an entry of C is a sum of m products of two differences, divided once: each product carries three roundings (two
    differences, one product) of relative size u, the running sum m more, the division one: at most (m + 4) u s per entry,
    and a mean that is itself off by e moves C by e e^T only (the deviations sum to zero), |e| <= (m + 1) u max|q|, which
    is second order and covered by doubling.  Over nine entries (Frobenius) and for BOTH sides:
        E_cov = 2 * 3 * 2 * (m + 4) * u * s
  * a symmetric eigen-solver (cyclic Jacobi there, LAPACK here) returns the exact eigenvectors of a matrix within
    p * u * |C|_F of its input; p = 64 covers 8 sweeps of 3 rotations with a few roundings each, and LAPACK's own
    modest constant.  For both sides:  E_eig = 2 * 64 * u * |C|_F
  * Davis-Kahan: the unit eigenvectors of the smallest eigenvalue of two symmetric matrices E apart enclose an angle
    theta with sin(theta) <= 2 E / (l1 - l0).
  * the output is rounded to float32: each component moves by at most 2^-25 (half an ulp below 1), the vector by
    sqrt(3) * 2^-25, its direction by at most that over its length; doubled for the arcsine: sqrt(3) * 2^-24.
        angle_bound = arcsin(min(1, 2 * (E_cov + E_eig) / (l1 - l0))) + sqrt(3) * 2^-24
The Rayleigh quotient needs no gap: n^T C n <= l0 + 2 E for the exact eigenvector of a matrix E away, and moving n by
d changes it by at most 2 |d| l2:   rayleigh_slack = 2 * (E_cov + E_eig) + sqrt(3) * 2^-23 * l2   (absolute).
"""
import numpy as np

U = 2.0 ** -53
KNN_MAX, TILE = 64, 1024


def grid_shape(box_min, box_max, cell):
    """n[a] = floor((box_max - box_min) / cell) + 1, as the header states it."""
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    return [int(x) for x in np.floor((hi - lo) / np.float64(cell)) + 1]


def workspace_bytes(P, box_min, box_max, cell):
    """The header's formula: 24 P + 8 ceil(P / 2) + 8 ceil(cells / 2) + 8 ceil((ceil(cells / TILE) + 1) / 2)."""
    n = grid_shape(box_min, box_max, cell)
    cells = n[0] * n[1] * n[2]
    return 24 * P + 8 * -(-P // 2) + 8 * -(-cells // 2) + 8 * -(-(-(-cells // TILE) + 1) // 2)


def members_of(xyz, box_min, box_max):
    p = np.asarray(xyz).astype(np.float64)
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    with np.errstate(invalid="ignore"):
        return np.all((lo <= p) & (p <= hi), axis=1)         # False for NaN


def neighbours(xyz, box_min, box_max, knn, chunk=256):
    """-> (member bool [P], nbr int32 [P, knn] in ascending (d2, index), -1 pads, last_d2 float64 [P] (nan for
    non-members): d2 of the last neighbour)."""
    p = np.asarray(xyz).astype(np.float64)
    P = len(p)
    member = members_of(p, box_min, box_max)
    ids = np.flatnonzero(member)
    q = p[ids]
    M = len(ids)
    m = min(knn, M)
    nbr = np.full((P, knn), -1, np.int32)
    last = np.full(P, np.nan)
    for a in range(0, M, chunk):
        d = q[None, :, :] - q[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.lexsort((np.broadcast_to(ids, d2.shape), d2), axis=1)[:, :m]
        rows = ids[a:a + chunk]
        nbr[rows, :m] = ids[order]
        last[rows] = np.take_along_axis(d2, order[:, m - 1:m], axis=1)[:, 0]
    return member, nbr, last


def estimate(xyz, box_min, box_max, knn, view_starts=None, centres=None):
    """The header's definition -> dict(member, nbr, normals float64 [P,3] (zeros for non-members), counts [3],
    eig float64 [P,3] ascending, cov [P,3,3], degenerate bool [P] (m < 3 or C == 0), angle_bound [P], rayleigh_slack [P],
    view int [P] (-1: in no view's range))."""
    assert 3 <= knn <= KNN_MAX
    p = np.asarray(xyz).astype(np.float64)
    P = len(p)
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    member, nbr, last = neighbours(p, lo, hi, knn)
    M = int(member.sum())
    m = min(knn, M)
    normals = np.zeros((P, 3))
    eig = np.zeros((P, 3))
    cov = np.zeros((P, 3, 3))
    degenerate = np.zeros(P, bool)
    angle = np.full(P, np.inf)
    slack = np.zeros(P)
    view = np.full(P, -1)
    if view_starts is not None:
        vs = np.asarray(view_starts, np.int64)
        r = np.searchsorted(vs, np.arange(P), side="right") - 1
        ok = (r >= 0) & (r < len(vs) - 1)
        ok[ok] = np.arange(P)[ok] < vs[r[ok] + 1]
        view = np.where(ok, r, -1)
    ids = np.flatnonzero(member)
    n = np.tile([0.0, 0.0, 1.0], (len(ids), 1))
    some = np.zeros(len(ids), bool)
    if m >= 3:
        mean = np.zeros((len(ids), 3))
        for j in range(m):                      # in ascending (d2, index), from 0
            mean = mean + p[nbr[ids, j]]
        mean = mean / m
        C = np.zeros((len(ids), 3, 3))
        s = np.zeros(len(ids))
        for j in range(m):
            d = p[nbr[ids, j]] - mean
            C = C + d[:, :, None] * d[:, None, :]
            s = np.maximum(s, (d * d).sum(axis=1))
        C = C / m
        cov[ids] = C
        some = (C != 0).any(axis=(1, 2))
        w, v = np.linalg.eigh(C[some])
        k = ids[some]
        eig[k] = w
        n[some] = v[:, :, 0] / np.linalg.norm(v[:, :, 0], axis=1, keepdims=True)
        E = 2 * 3 * 2 * (m + 4) * U * s[some] + 2 * 64 * U * np.linalg.norm(C[some], axis=(1, 2))
        gap = w[:, 1] - w[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            angle[k] = np.where(gap > 0, np.arcsin(np.minimum(1.0, 2 * E / gap)), np.pi / 2) + np.sqrt(3) * 2.0 ** -24
        slack[k] = 2 * E + np.sqrt(3) * 2.0 ** -23 * w[:, 2]
    degenerate[ids] = ~some
    c = np.zeros((len(ids), 3))
    seen = view[ids] >= 0
    if seen.any():
        c[seen] = np.asarray(centres, np.float64)[view[ids][seen]] - p[ids][seen]
    dot = (n[:, 0] * c[:, 0] + n[:, 1] * c[:, 1]) + n[:, 2] * c[:, 2]
    a = np.abs(n)
    big = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), n[:, 0], np.where(a[:, 1] >= a[:, 2], n[:, 1], n[:, 2]))
    flip = np.where(seen, dot < 0, big < 0)
    normals[ids] = np.where(flip[:, None], -n, n)
    with np.errstate(invalid="ignore"):
        f = np.minimum(p - lo, hi - p).min(axis=1)
        unsure = member & ((m < knn) | (last > f * f))
    counts = [M, M if M >= 3 else 0, int(unsure.sum())]
    return dict(member=member, nbr=nbr, normals=normals, counts=counts, eig=eig, cov=cov, degenerate=degenerate,
                angle_bound=angle, rayleigh_slack=slack, view=view, uncertified=unsure)


def angle_between(a, b):
    """Angle between the LINES of a and b (sign-blind), [..,3] each, accurate near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def voxel_mean_normals(xyz, normals, box_min, box_max, v):
    """mvs_cloud_downsample_normals' normals in fp64: the mean of clamp(n, -1, 1) (NaN as 0) over each occupied voxel, in
    ascending (iz, iy, ix) -> float64 [Q,3].  The grid is cloud_ref.downsample's (include/mvs_cloud_abi.h)."""
    p = np.asarray(xyz).astype(np.float64)
    n = np.asarray(normals).astype(np.float64)
    n = np.clip(np.where(np.isnan(n), 0.0, n), -1.0, 1.0)
    keep = members_of(p, box_min, box_max)
    p, n = p[keep], n[keep]
    if len(p) == 0:
        return np.zeros((0, 3))
    v = np.float64(v)
    idx = np.floor((p - (p.min(axis=0) - 0.5 * v)) / v).astype(np.int64)
    size = idx.max(axis=0) + 1
    lin = (idx[:, 2] * size[1] + idx[:, 1]) * size[0] + idx[:, 0]
    order = np.argsort(lin, kind="stable")
    lin, n = lin[order], n[order]
    first = np.flatnonzero(np.r_[True, lin[1:] != lin[:-1]])
    count = np.diff(np.r_[first, len(lin)])
    return np.add.reduceat(n, first, axis=0) / count[:, None]
