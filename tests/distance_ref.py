"""The yardstick of mvs_cloud_distance: include/mvs_distance_abi.h's definition in numpy float64, brute force (neither
scipy nor a grid is needed).

    members     normals_ref.members_of: box_min <= r <= box_max on every axis, both ends inclusive
    counted     a query whose three coordinates are finite; every other query gets dist -1.0, idx -1
    d2          (dx*dx + dy*dy) + dz*dz with d = r[j] - q[i], the full [queries, members] matrix in chunks of queries
    nearest     the member with the smallest (d2, j) among the finite d2: np.argmin returns the first minimum, and the
                members are taken in ascending j
    cap         none, or d2 > max_dist * max_dist (one product) -> dist +inf, idx -1; else sqrt(d2), j, "within"
    counts      n_counted, n_within, then the within queries with dist < thresholds[t], strictly
    S           outliers_ref.tree_sum over x = dist where within else +0.0, in query-index order
    stats       S(x), S(x) / n_within (0 when n_within == 0)
numpy's sqrt, division, product and sum of float64 are IEEE operations, correctly rounded, one at a time.
"""
import numpy as np

import normals_ref
import outliers_ref

THRESHOLDS_MAX, SCALARS = 8, 64


def workspace_bytes(P, N, box_min, box_max, cell):
    """The header's formula: the normals' workspace over P + 8 bytes per partial sum over N + the scalar block."""
    return normals_ref.workspace_bytes(P, box_min, box_max, cell) + 8 * outliers_ref.partial_sums(N) + SCALARS


def distance(ref, query, box_min, box_max, max_dist=np.inf, thresholds=(), chunk=512):
    """The header's definition -> dict(member bool [P], dist float64 [N], idx int32 [N], counts [2 + T], stats float64 [2])."""
    r = np.asarray(ref).astype(np.float64).reshape(-1, 3)
    q = np.asarray(query).astype(np.float64).reshape(-1, 3)
    max_dist = np.float64(max_dist)
    assert max_dist >= 0 and len(thresholds) <= THRESHOLDS_MAX
    assert all(np.isfinite(t) and t >= 0 for t in thresholds)
    member = normals_ref.members_of(r, box_min, box_max)
    ids = np.flatnonzero(member)
    m = r[ids]
    counted = np.isfinite(q).all(axis=1)
    N = len(q)
    dist = np.full(N, -1.0)
    idx = np.full(N, -1, np.int32)
    dist[counted] = np.inf
    cap = max_dist * max_dist
    rows = np.flatnonzero(counted)
    with np.errstate(over="ignore"):
        for a in range(0, len(rows) if len(ids) else 0, chunk):
            i = rows[a:a + chunk]
            d = m[None, :, :] - q[i, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            j = np.argmin(d2, axis=1)                       # the first minimum: the smallest member index
            best = d2[np.arange(len(i)), j]
            within = np.isfinite(best) & ~(best > cap)
            dist[i[within]] = np.sqrt(best[within])
            idx[i[within]] = ids[j[within]]
    within = counted & np.isfinite(dist)
    counts = [int(counted.sum()), int(within.sum())] + [int((within & (dist < np.float64(t))).sum()) for t in thresholds]
    total = outliers_ref.tree_sum(np.where(within, dist, 0.0)) if N else np.float64(0.0)
    mean = total / np.float64(counts[1]) if counts[1] else np.float64(0.0)
    return dict(member=member, dist=dist, idx=idx, counts=counts, stats=np.array([total, mean], np.float64))


def lower_median(x):
    """The ((n + 1) // 2)-th smallest of x; NaN for none."""
    x = np.sort(np.asarray(x, np.float64))
    return float(x[(len(x) + 1) // 2 - 1]) if len(x) else float("nan")


def evaluate(pred, gt, max_dist=20.0, thresholds=(1.0, 2.0, 5.0), box=None):
    """fusion.evaluate_cloud's dict from the definition: both directions, each over the bounding box of its finite
    reference points unless a box is given."""
    def bbox(p):
        p = np.asarray(p).astype(np.float64).reshape(-1, 3)
        p = p[np.isfinite(p).all(axis=1)]
        return ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if len(p) == 0 else (p.min(axis=0), p.max(axis=0))

    out = {}
    for name, query, ref in (("accuracy", pred, gt), ("completeness", gt, pred)):
        lo, hi = bbox(ref) if box is None else box
        got = distance(ref, query, lo, hi, max_dist, thresholds)
        d = got["dist"]
        out[name] = dict(mean=float(got["stats"][1]), median=lower_median(d[np.isfinite(d) & (d >= 0)]),
                         n=got["counts"][0], n_within=got["counts"][1], below=got["counts"][2:])
    acc, comp = out["accuracy"], out["completeness"]
    out["overall"] = (acc["mean"] + comp["mean"]) / 2
    out["precision"] = [b / acc["n"] if acc["n"] else 0.0 for b in acc["below"]]
    out["recall"] = [b / comp["n"] if comp["n"] else 0.0 for b in comp["below"]]
    out["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    out["max_dist"], out["thresholds"] = float(max_dist), [float(t) for t in thresholds]
    return out
