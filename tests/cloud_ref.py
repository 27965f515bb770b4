"""The yardstick of mvs_cloud_downsample: include/mvs_cloud_abi.h's definition in numpy float64 (Open3D's
crop + voxel_down_sample + scale, eval.py:831-840, restated from its documented behaviour; Open3D is not needed).

    crop      box_min <= p <= box_max on every axis, both ends inclusive, on the value as float64
    grid      vmin = min(kept) - 0.5 * v;  idx = floor((p - vmin) / v)   -- plain IEEE double, one operation at a time
    order     ascending (iz, iy, ix), a stable sort
    mean      sum of the voxel's float64 points / count, then * scale
    colour    (2 * sum + count) // (2 * count) per channel: the mean of the bytes rounded half up
"""
import numpy as np


def grid_shape(box_min, box_max, v):
    """n[a] = floor((box_max - box_min) / v + 0.5) + 2, as the header states it."""
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    return [int(x) for x in np.floor((hi - lo) / np.float64(v) + 0.5) + 2]


def workspace_bytes(P, box_min, box_max, v, chunk=1024, tile=1024, record=64):
    """The header's formula: 64 + record * cells + 32 * ceil(P / chunk) + 8 * ceil((ceil(cells / tile) + 1) / 2)."""
    n = grid_shape(box_min, box_max, v)
    cells = n[0] * n[1] * n[2]
    return 64 + record * cells + 32 * -(-P // chunk) + 8 * -(-(-(-cells // tile) + 1) // 2)


def downsample(xyz, rgb, box_min, box_max, v, scale=1.0):
    """-> dict(kept, voxels, idx int64 [Q,3] (ix, iy, iz), count int64 [Q], mean float64 [Q,3] (mean * scale, fp64),
    xyz float32 [Q,3], rgb uint8 [Q,3], bound float64 [Q,3]).

    bound is what a float32 output of the fixed-point scheme may differ from `mean` by:
        ulp32(mean) / 2 + |scale| * (v * 2^-33 + (count + 4) * 2^-53 * max|coordinate|)
    -- the float32 rounding of the result; the quantisation of one offset to 2^-32 of a voxel (half a step, and a mean of
    values each off by at most that is off by at most that); and the fp64 roundings: `count` of them in THIS function's
    sum, four more for the scheme's corner, quotient, product and final sum, each at most 2^-53 of the largest coordinate."""
    p = np.asarray(xyz).astype(np.float64)
    c = np.asarray(rgb)
    assert p.ndim == 2 and p.shape[1] == 3 and c.shape == p.shape and c.dtype == np.uint8
    lo, hi, v = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64), np.float64(v)
    with np.errstate(invalid="ignore"):
        keep = np.all((lo <= p) & (p <= hi), axis=1)         # False for NaN
    p, c = p[keep], c[keep].astype(np.int64)
    kept = int(keep.sum())
    empty = dict(kept=kept, voxels=0, idx=np.zeros((0, 3), np.int64), count=np.zeros(0, np.int64),
                 mean=np.zeros((0, 3)), xyz=np.zeros((0, 3), np.float32), rgb=np.zeros((0, 3), np.uint8),
                 bound=np.zeros((0, 3)))
    if kept == 0:
        return empty
    vmin = p.min(axis=0) - 0.5 * v
    idx = np.floor((p - vmin) / v).astype(np.int64)
    n = grid_shape(lo, hi, v)
    assert (idx >= 0).all() and (idx <= np.array(n) - 1).all(), "the header's bound on the indices"
    lin = (idx[:, 2] * n[1] + idx[:, 1]) * n[0] + idx[:, 0]
    order = np.argsort(lin, kind="stable")
    lin, p, c, idx = lin[order], p[order], c[order], idx[order]
    first = np.flatnonzero(np.r_[True, lin[1:] != lin[:-1]])
    count = np.diff(np.r_[first, len(lin)]).astype(np.int64)
    mean = np.add.reduceat(p, first, axis=0) / count[:, None] * np.float64(scale)
    csum = np.add.reduceat(c, first, axis=0)
    colour = ((2 * csum + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    big = np.abs(p).max()
    # ulp32 of the float64 value itself (not of its rounded float32, whose spacing doubles at a power of two)
    ulp32 = np.where(mean == 0, 2.0 ** -149, np.maximum(np.ldexp(1.0, np.frexp(mean)[1] - 24), 2.0 ** -149))
    bound = ulp32 / 2 + abs(float(scale)) * (v * 2.0 ** -33 + (count[:, None] + 4) * 2.0 ** -53 * big)
    return dict(kept=kept, voxels=len(first), idx=idx[first], count=count, mean=mean, xyz=mean.astype(np.float32),
                rgb=colour, bound=bound)
