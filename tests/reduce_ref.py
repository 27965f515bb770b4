"""The yardstick of mvs_cloud_reduce and mvs_cloud_select: include/mvs_reduce_abi.h's definitions in numpy float64 and
uint64, brute force (neither scipy nor a grid is needed).

    members     normals_ref.members_of: box_min <= p <= box_max on every axis, both ends inclusive
    keys        SplitMix64's (i+1)-th output from `seed`, in uint64 arithmetic that wraps; the order is (h(i), i)
    near        d2 = (dx*dx + dy*dy) + dz*dz <= min_dist * min_dist (one product), d = p[j] - p[i], the [members, members]
                matrix in chunks of rows (less the columns too far along x to be near, see earlier_near); of it only E(i)
                is kept: the near members with a smaller key
    sequential  reduce_sequential: the members in key order, one kept iff none of E(i) was kept -- the definition
    rounds      reduce_rounds: the header's synchronous rule; every round is computed from a copy of the state the round
                before left, so it reads only what earlier rounds decided
    select      MATLAB's round (half away from zero) of (p - origin) / res per axis, compared with the mask's shape as
                doubles; ((P0*x + P1*y) + P2*z) + P3 > 0
numpy's products, sums, quotients and floors of float64 are IEEE operations, correctly rounded, one at a time.
"""
import numpy as np

import distance_ref
import normals_ref

ROUNDS_MAX = 256
FIRST_KEYS_SEED0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)


def workspace_bytes(P, box_min, box_max, cell):
    """The header's formula: the normals' workspace + 8 ceil(P / 2) for the states + 8 (ROUNDS_MAX + 2) for the counters."""
    return normals_ref.workspace_bytes(P, box_min, box_max, cell) + 8 * -(-P // 2) + 8 * (ROUNDS_MAX + 2)


def keys(P, seed=0, rows=None):
    """h(i) for i = 0 .. P-1 -> uint64 [P]; with `rows` (int [P]) for i = rows[0] .. rows[P-1]: the points are rows of a
    larger cloud."""
    i = np.arange(P, dtype=np.uint64) if rows is None else np.asarray(rows).astype(np.uint64)
    assert len(i) == P
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def earlier_near(xyz, box_min, box_max, min_dist, seed=0, chunk=256, rows=None):
    """-> (ids int64 [M]: the members' rows, rank int64 [M]: each member's place in key order, src, dst int64 [E]: the
    pairs (a, b) of positions in `ids` with b in E(a): near a, with a smaller key).  `rows` (increasing): the index each
    point has in the cloud it was taken from, which is what its key hashes."""
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    min_dist = np.float64(min_dist)
    assert np.isfinite(min_dist) and min_dist >= 0
    ids = np.flatnonzero(normals_ref.members_of(p, box_min, box_max))
    m = p[ids]
    M = len(ids)
    h = keys(len(p), seed, rows)[ids]
    rank = np.empty(M, np.int64)
    rank[np.lexsort((ids, h))] = np.arange(M)
    md2 = min_dist * min_dist
    # The rows are taken in ascending x, and a chunk of rows meets only the columns whose x lies within `reach` of the
    # chunk's: a pair farther apart than that along x is not near (|dx| > reach gives dx*dx > md2, and the two sums only
    # add non-negative terms; rounding is monotone).  Everything inside the window is still the full matrix.
    reach = min_dist * (1.0 + 2.0 ** -40) + 1e-150 if np.isfinite(md2) else np.inf      # an overflowed bound holds every pair
    by_x = np.argsort(m[:, 0], kind="stable")
    ms, rs = m[by_x], rank[by_x]
    src, dst = [], []
    with np.errstate(over="ignore"):
        for a in range(0, M, chunk):
            b = min(a + chunk, M)
            c0 = np.searchsorted(ms[:, 0], ms[a, 0] - reach, "left")
            c1 = np.searchsorted(ms[:, 0], ms[b - 1, 0] + reach, "right")
            dx = ms[None, c0:c1, 0] - ms[a:b, None, 0]
            dy = ms[None, c0:c1, 1] - ms[a:b, None, 1]
            dz = ms[None, c0:c1, 2] - ms[a:b, None, 2]
            near = ((dx * dx + dy * dy) + dz * dz) <= md2
            near &= rs[None, c0:c1] < rs[a:b, None]                    # a smaller key; this also drops the member itself
            s, d = np.nonzero(near)
            src.append(by_x[s + a])
            dst.append(by_x[d + c0])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)      # noqa: E731
    return ids, rank, cat(src).astype(np.int64), cat(dst).astype(np.int64)


def _result(P, ids, kept, undecided, rounds):
    mask = np.zeros(P, bool)
    mask[ids[kept]] = True
    return mask, [len(ids), int(kept.sum()), int(undecided), int(rounds)]


def reduce_sequential(xyz, box_min, box_max, min_dist, seed=0):
    """The definition: the members in key order, one kept iff no member kept before it is near -> (mask bool [P], kept)."""
    ids, rank, src, dst = earlier_near(xyz, box_min, box_max, min_dist, seed)
    M = len(ids)
    order = np.argsort(src, kind="stable")
    dst = dst[order]
    start = np.searchsorted(src[order], np.arange(M + 1))
    kept = np.zeros(M, bool)
    for a in np.argsort(rank):
        kept[a] = not kept[dst[start[a]:start[a + 1]]].any()
    mask = np.zeros(len(np.asarray(xyz).reshape(-1, 3)), bool)
    mask[ids[kept]] = True
    return mask, int(kept.sum())


def reduce_rounds(xyz, box_min, box_max, min_dist, seed=0, max_rounds=64, rows=None):
    """The header's synchronous rule -> (mask bool [P], counts [members, kept, undecided, rounds])."""
    assert 1 <= max_rounds <= ROUNDS_MAX
    ids, _, src, dst = earlier_near(xyz, box_min, box_max, min_dist, seed, rows=rows)
    M = len(ids)
    decided, kept = np.zeros(M, bool), np.zeros(M, bool)
    rounds = 0
    while rounds < max_rounds and not decided.all():
        rounds += 1
        was_decided, was_kept = decided.copy(), kept.copy()           # what earlier rounds decided
        has_kept = np.bincount(src, weights=was_kept[dst], minlength=M) > 0
        has_open = np.bincount(src, weights=~was_decided[dst], minlength=M) > 0
        removed = ~was_decided & has_kept
        keep = ~was_decided & ~has_kept & ~has_open
        decided |= removed | keep
        kept |= keep
    return _result(len(np.asarray(xyz).reshape(-1, 3)), ids, kept, (~decided).sum(), rounds)


def depth(xyz, box_min, box_max, min_dist, seed=0):
    """The rounds the rule needs on this input."""
    return reduce_rounds(xyz, box_min, box_max, min_dist, seed, ROUNDS_MAX)[1][3]


def mround(x):
    """MATLAB's round: half away from zero."""
    x = np.asarray(x, np.float64)
    return np.where(x < 0, -np.floor(-x + 0.5), np.floor(x + 0.5))


def select(xyz, obs_mask=None, plane=None):
    """The header's two tests -> (keep bool [P], counts [finite, observed, kept]).  obs_mask = dict(mask [n0,n1,n2],
    origin (3,), res)."""
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    finite = np.isfinite(p).all(axis=1)
    observed = finite.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if obs_mask is not None:
            mask = np.asarray(obs_mask["mask"])
            origin, res = np.asarray(obs_mask["origin"], np.float64), np.float64(obs_mask["res"])
            g = mround((p - origin) / res)
            inside = finite & np.all((g >= 0.0) & (g < np.asarray(mask.shape, np.float64)), axis=1)
            gi = g[inside].astype(np.int64)
            observed = np.zeros(len(p), bool)
            observed[inside] = mask[gi[:, 0], gi[:, 1], gi[:, 2]] != 0
        keep = observed.copy()
        if plane is not None:
            P = np.asarray(plane, np.float64)
            keep &= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3]) > 0.0
    return keep, [int(finite.sum()), int(observed.sum()), int(keep.sum())]


def _bbox(p):
    p = np.asarray(p).astype(np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    return ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if len(p) == 0 else (p.min(axis=0), p.max(axis=0))


def _nan_rows(xyz, keep):
    out = np.array(xyz, copy=True)
    out[~keep] = np.nan
    return out


def evaluate(pred, gt, max_dist=20.0, thresholds=(1.0, 2.0, 5.0), box=None, reduce=None, obs_mask=None, plane=None):
    """fusion.evaluate_cloud's dict with the three options, on top of distance_ref.evaluate: the reconstruction reduced
    over its own bounding box (and the ground truth with reduce["gt"]), accuracy from its observed points to the whole
    ground truth, completeness from the ground truth above the plane to the whole reduced reconstruction."""
    if reduce is None and obs_mask is None and plane is None:
        return distance_ref.evaluate(pred, gt, max_dist, thresholds, box)
    pred, gt = np.asarray(pred), np.asarray(gt)
    reduction = {}
    if reduce is not None:
        opt = dict(dict(min_dist=0.2, seed=0, gt=False, max_rounds=64), **reduce)
        clouds = dict(pred=pred, gt=gt)
        for name in ("pred", "gt") if opt["gt"] else ("pred",):
            mask, counts = reduce_rounds(clouds[name], *_bbox(clouds[name]), opt["min_dist"], opt["seed"], opt["max_rounds"])
            assert counts[2] == 0
            reduction[name] = counts
            clouds[name] = _nan_rows(clouds[name], mask)
        pred, gt = clouds["pred"], clouds["gt"]
    keep_a, sel_a = select(pred, obs_mask=obs_mask)
    keep_c, sel_c = select(gt, plane=plane)
    out = dict(distance_ref.evaluate(_nan_rows(pred, keep_a), gt, max_dist, thresholds, box))
    out["completeness"] = distance_ref.evaluate(pred, _nan_rows(gt, keep_c), max_dist, thresholds, box)["completeness"]
    acc, comp = out["accuracy"], out["completeness"]
    out["overall"] = (acc["mean"] + comp["mean"]) / 2
    out["precision"] = [b / acc["n"] if acc["n"] else 0.0 for b in acc["below"]]
    out["recall"] = [b / comp["n"] if comp["n"] else 0.0 for b in comp["below"]]
    out["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    out["selection"] = dict(accuracy=sel_a, completeness=sel_c)
    out["reduction"] = reduction
    return out
