"""The yardstick of mvs_cloud_cluster: include/mvs_cluster_abi.h's definitions in numpy float64.

    members     normals_ref.members_of: box_min <= p <= box_max on every axis, both ends inclusive
    neighbours  d2 = (dx*dx + dy*dy) + dz*dz <= eps * eps (one product), d = p[j] - p[i].  scipy's cKDTree only proposes
                candidates, within a radius a little above eps; every pair is decided by that expression, here
    core        a member with at least min_points neighbours, itself counted
    parallel    cluster(): the header's rule -- the connected components of the core graph (scipy's csgraph), numbered in
                the order of their smallest core index; a border point takes the smallest number among its core
                neighbours; noise is -1, a non-member -2
    sequential  traverse(): the libraries' DBSCAN as a traversal in index order, a second and independent statement of the
                labels: an unlabelled core point starts the next cluster, which is expanded completely (a stack of points
                to visit; a point is labelled when it is first reached; only core points pass the visit on) before the
                visit goes on
    keep        label >= 0 and the size of that cluster, core and border counted, >= min_size
    counts      [members, core, border, noise, clusters, kept points, size of the largest cluster]
numpy's products and sums of float64 are IEEE operations, correctly rounded, one at a time.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import normals_ref

COUNTERS = 8      # MVS_CLUSTER_COUNTERS


def workspace_bytes(P, box_min, box_max, cell):
    """The header's formula: the normals' workspace + four words per point (8 ceil(P / 2) bytes each) + the root tiles
    8 ceil((ceil(P / 1024) + 1) / 2) + 8 COUNTERS."""
    tiles = -(-P // 1024)
    return normals_ref.workspace_bytes(P, box_min, box_max, cell) + 4 * 8 * -(-P // 2) + 8 * -(-(tiles + 1) // 2) + 8 * COUNTERS


def neighbour_pairs(xyz, box_min, box_max, eps):
    """-> (ids int64 [M]: the members' rows, a, b int64 [E]: the neighbour pairs as positions in `ids`, a < b, each once,
    d2 float64 [E])."""
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    eps = np.float64(eps)
    assert np.isfinite(eps) and eps >= 0
    ids = np.flatnonzero(normals_ref.members_of(p, box_min, box_max))
    m = p[ids]
    empty = np.zeros(0, np.int64)
    if len(ids) < 2:
        return ids, empty, empty, np.zeros(0)
    with np.errstate(over="ignore"):
        eps2 = eps * eps
        radius = eps * (1.0 + 1e-9) + 1e-300
        if np.isfinite(radius) and np.isfinite(eps2):
            cand = cKDTree(m).query_pairs(radius, output_type="ndarray").astype(np.int64)
        else:                                              # an overflowed bound: every pair is a candidate
            cand = np.column_stack(np.triu_indices(len(ids), 1)).astype(np.int64)
        a, b = cand[:, 0], cand[:, 1]
        d = m[b] - m[a]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    near = d2 <= eps2
    a, b, d2 = a[near], b[near], d2[near]
    swap = a > b
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    return ids, a, b, d2


def _graph(M, a, b):
    """Neighbour lists without the point itself, CSR: (start int64 [M + 1], nbr int64 [2E])."""
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.argsort(src, kind="stable")
    return np.searchsorted(src[order], np.arange(M + 1)), dst[order]


def _finish(P, ids, lab, core, min_size):
    labels = np.full(P, -2, np.int32)
    labels[ids] = lab
    clusters = int(lab.max()) + 1 if len(lab) and lab.max() >= 0 else 0
    sizes = np.bincount(lab[lab >= 0], minlength=clusters)
    keep = np.zeros(P, bool)
    keep[ids] = (lab >= 0) & (sizes[np.maximum(lab, 0)] >= min_size if clusters else False)
    counts = [len(ids), int(core.sum()), int(((lab >= 0) & ~core).sum()), int((lab < 0).sum()), clusters, int(keep.sum()),
              int(sizes.max()) if clusters else 0]
    return labels, keep, counts


def cluster(xyz, box_min, box_max, eps, min_points, min_size=1, pairs=None):
    """The header's parallel rule -> (labels int32 [P], keep bool [P], counts [7])."""
    assert min_points >= 1 and min_size >= 1
    P = len(np.asarray(xyz).reshape(-1, 3))
    ids, a, b, _ = neighbour_pairs(xyz, box_min, box_max, eps) if pairs is None else pairs
    M = len(ids)
    degree = np.bincount(a, minlength=M) + np.bincount(b, minlength=M) + 1       # itself counted
    core = degree >= min_points
    lab = np.full(M, -1, np.int64)
    if core.any():
        both = core[a] & core[b]
        n_comp, comp = connected_components(coo_matrix((np.ones(both.sum(), np.int8), (a[both], b[both])), shape=(M, M)),
                                            directed=False)
        # the smallest core position of every component that has a core member; positions ascend with the indices
        first = np.full(n_comp, M, np.int64)
        np.minimum.at(first, comp[core], np.flatnonzero(core))
        number = np.full(n_comp, -1, np.int64)
        with_core = np.flatnonzero(first < M)
        number[with_core[np.argsort(first[with_core])]] = np.arange(len(with_core))
        lab[core] = number[comp[core]]
        # border: the smallest number among the core neighbours, from both ends of every pair
        best = np.full(M, np.iinfo(np.int64).max, np.int64)
        for u, v in ((a, b), (b, a)):
            sel = ~core[u] & core[v]
            np.minimum.at(best, u[sel], lab[v[sel]])
        border = ~core & (best < np.iinfo(np.int64).max)
        lab[border] = best[border]
    return _finish(P, ids, lab, core, min_size)


def traverse(xyz, box_min, box_max, eps, min_points, min_size=1, pairs=None):
    """The sequential traversal in index order -> (labels, keep, counts) as cluster() gives them."""
    assert min_points >= 1 and min_size >= 1
    P = len(np.asarray(xyz).reshape(-1, 3))
    ids, a, b, _ = neighbour_pairs(xyz, box_min, box_max, eps) if pairs is None else pairs
    M = len(ids)
    start, nbr = _graph(M, a, b)
    core = (np.diff(start) + 1) >= min_points
    lab = np.full(M, -1, np.int64)
    current = 0
    for s in range(M):
        if lab[s] != -1 or not core[s]:
            continue
        stack = [s]
        while stack:
            x = stack.pop()
            if lab[x] != -1:
                continue
            lab[x] = current
            if core[x]:
                stack.extend(int(y) for y in nbr[start[x]:start[x + 1]] if lab[y] == -1)
        current += 1
    return _finish(P, ids, lab, core, min_size)
