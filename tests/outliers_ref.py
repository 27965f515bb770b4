"""The yardstick of mvs_cloud_outliers: include/mvs_outliers_abi.h's definition in numpy float64 (Open3D's
RemoveStatisticalOutliers restated, with the tie order, the summation order and the cases of fewer than two valid points
specified; neither Open3D nor scipy is needed).

    members     normals_ref.members_of: box_min <= p <= box_max on every axis, both ends inclusive
    neighbours  normals_ref.neighbours: the min(nb, M) members with the smallest (d2, index), brute force
    dist        (sum of sqrt(d2) in ascending (d2, index), from 0.0) / m; -1.0 for a non-member
    valid       member and dist > 0
    S           tree_sum: pad with +0.0 to a power of two, then a[0::2] + a[1::2] until one value is left
    mean        S(x) / n_valid, x = dist where valid else +0.0, in point-index order
    std         sqrt(S((x - mean)^2 where valid else +0.0) / (n_valid - 1)); 0 for n_valid < 2
    threshold   mean + std_ratio * std; mean = std = threshold = 0 for n_valid == 0
    keep        valid and dist < threshold
numpy's sqrt, division, product and sum of float64 are IEEE operations, correctly rounded, one at a time.
"""
import numpy as np

import normals_ref

KNN_MAX, BLOCK, SCALARS = normals_ref.KNN_MAX, 1024, 64
NAN32, NAN64 = np.uint32(0x7FC00000), np.uint64(0x7FF8000000000000)


def partial_sums(P):
    """The header's L_1 + L_2 + ...: L_0 = P, L_{k+1} = ceil(L_k / BLOCK) down to the first L_k == 1."""
    total, L = 0, P
    while L > 1:
        L = -(-L // BLOCK)
        total += L
    return total


def workspace_bytes(P, box_min, box_max, cell):
    """The header's formula: the normals' workspace + 8 bytes per partial sum + the scalar block."""
    return normals_ref.workspace_bytes(P, box_min, box_max, cell) + 8 * partial_sums(P) + SCALARS


def tree_sum(x):
    """The balanced pairwise sum S(x) of the header, literally."""
    a = np.asarray(x, np.float64).reshape(-1)
    n = 1
    while n < len(a):
        n *= 2
    a = np.concatenate([a, np.zeros(n - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return np.float64(a[0])


def mean_distances(xyz, box_min, box_max, nb):
    """-> (member bool [P], dist float64 [P], -1.0 for non-members): brute force over the members only."""
    p = np.asarray(xyz).astype(np.float64)
    member, nbr, _ = normals_ref.neighbours(p, box_min, box_max, nb)
    ids = np.flatnonzero(member)
    m = min(nb, len(ids))
    dist = np.full(len(p), -1.0)
    total = np.zeros(len(ids))
    for j in range(m):                          # in ascending (d2, index), from 0.0
        d = p[nbr[ids, j]] - p[ids]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        total = total + np.sqrt(d2)
    if m:
        dist[ids] = total / np.float64(m)
    return member, dist


def statistics(dist, std_ratio):
    """dist [P] (-1.0 for non-members) -> (keep bool [P], counts [M, n_valid, kept], stats float64 [mean, std, threshold])."""
    dist = np.asarray(dist, np.float64)
    valid = dist > 0
    n_valid = int(valid.sum())
    x = np.where(valid, dist, 0.0)
    mean = std = threshold = np.float64(0.0)
    if n_valid > 0:
        mean = tree_sum(x) / np.float64(n_valid)
        if n_valid > 1:
            e = x - mean
            std = np.sqrt(tree_sum(np.where(valid, e * e, 0.0)) / np.float64(n_valid - 1))
        scaled = np.float64(std_ratio) * std
        threshold = mean + scaled
    keep = valid & (dist < threshold)
    return keep, [int((dist >= 0).sum()), n_valid, int(keep.sum())], np.array([mean, std, threshold], np.float64)


def masked_bits(xyz, keep):
    """xyz_masked_out as unsigned integers of xyz's width: the input's bits where kept, the canonical quiet NaN elsewhere."""
    xyz = np.ascontiguousarray(xyz)
    bits = xyz.view(np.uint32 if xyz.dtype == np.float32 else np.uint64).copy()
    bits[~np.asarray(keep, bool)] = NAN32 if xyz.dtype == np.float32 else NAN64
    return bits


def remove(xyz, box_min, box_max, nb, std_ratio):
    """The header's definition -> dict(member, dist, keep, counts [3], stats float64 [3], masked: bits as masked_bits)."""
    assert 2 <= nb <= KNN_MAX and np.isfinite(std_ratio) and std_ratio > 0
    member, dist = mean_distances(xyz, box_min, box_max, nb)
    keep, counts, stats = statistics(dist, std_ratio)
    assert counts[0] == int(member.sum())
    return dict(member=member, dist=dist, keep=keep, counts=counts, stats=stats, masked=masked_bits(np.asarray(xyz), keep))
