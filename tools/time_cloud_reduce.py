#!/usr/bin/env python3
"""Time DTU's point reduction (mvs_cloud_reduce, fusion.reduce_cloud) and the evaluation that uses it, on the synthetic
49-view 640 x 512 scan of tools/time_cloud_distance.py with thresholds that keep every pixel (about a million points) and
its jittered ground truth.  min_dist is found by bisection on the device so that about half the points go; the share that
is kept is reported.

  reduce, per lane count   one _lib.cloud_reduce call on the resident cloud, device events around it, the two thread shapes
                           of the round kernel (1 lane per member, 16 lanes per member) in alternating runs; box = the
                           cloud's bounding box, cell = fusion.reduce_cell's.  `rounds` is the call's fourth count
  evaluate_cloud           fusion.evaluate_cloud end to end with and without reduce + obs_mask + plane (a synthetic mask of
                           MASK_RES-sized voxels over the cloud's box, three quarters of them set, and a plane through its
                           middle): host clock around a call that ends in its device-to-host copy
  host                     the same greedy thinning on the host, on a cloud already there: the same keys, the points
                           visited in key order, scipy.spatial.cKDTree.query_ball_point around every point that is kept;
                           and whether its mask is the device's (scipy forms its squared distance in another order, so a
                           pair on the bound can fall the other way: reported, not asserted)

Figures are median [min, max].  Before anything is reported the two thread shapes and three cell sizes must give the same
bytes, and undecided must be 0.

    python tools/time_cloud_reduce.py [--runs 20] [--warmup 3] [--out FILE]
Writes profiles/cloud_reduce_timing.json.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import normals_ref  # noqa: E402
import reduce_ref  # noqa: E402
from time_cloud_distance import THRESHOLDS, bounding_box, clouds, timed  # noqa: E402
from time_cloud_downsample import D, H, W, stats, wall  # noqa: E402
from time_scan_fusion import NVIEWS, V  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, fusion  # noqa: E402

LANES = (1, 16)
MASK_RES, MASK_SET, MASK_SEED = 10.0, 0.75, 11


def host_greedy(xyz, lo, hi, min_dist, seed):
    """-> (mask bool [P], seconds for the tree, seconds for the pass)."""
    from scipy.spatial import cKDTree
    p = xyz.astype(np.float64)
    ids = np.flatnonzero(normals_ref.members_of(p, lo, hi))
    order = np.lexsort((ids, reduce_ref.keys(len(p), seed)[ids]))
    t0 = time.perf_counter()
    tree = cKDTree(p[ids])
    t1 = time.perf_counter()
    removed = np.zeros(len(ids), bool)
    kept = np.zeros(len(ids), bool)
    m = p[ids]
    for a in order:
        if not removed[a]:
            kept[a] = True
            removed[tree.query_ball_point(m[a], min_dist)] = True
    t2 = time.perf_counter()
    mask = np.zeros(len(p), bool)
    mask[ids[kept]] = True
    return mask, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 10, "at least 10 timed runs"
    _lib.load()
    set_lanes = ctypes.CDLL(_lib.LIB_PATH).mvs_test_reduce_lanes
    default_lanes = set_lanes(0)
    dev = torch.device("cuda:0")
    pred_h, gt_h = clouds(dev, args.tmp)
    pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
    lo, hi = bounding_box(pred_h)
    P = len(pred_h)

    def call(min_dist, cell=None, out=None):
        cell = fusion.reduce_cell((lo, hi), P, min_dist) if cell is None else cell
        return _lib.cloud_reduce(pred, lo, hi, cell, min_dist, seed=args.seed, out=out)

    # ---- min_dist: about half the points go
    a, b = 0.0, float(np.max(hi - lo))
    for _ in range(24):
        mid = 0.5 * (a + b)
        c = call(mid)[1].tolist()
        a, b = (mid, b) if c[1] > c[0] // 2 else (a, mid)
        if abs(c[1] / max(c[0], 1) - 0.5) < 0.01:
            break
    min_dist = mid
    cell = fusion.reduce_cell((lo, hi), P, min_dist)
    # ---- the result first: both thread shapes, three cell sizes, the same bytes
    outs = {}
    for lanes in LANES:
        set_lanes(lanes)
        outs[lanes] = call(min_dist)
        for other in (2.0 * cell, 0.4 * cell):
            got = call(min_dist, cell=other)
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs[lanes], got)), (lanes, other)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs[1], outs[16]))
    counts = outs[1][1].tolist()
    assert counts[2] == 0, counts
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup,
           "shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D), "points": P, "min_dist": min_dist, "seed": args.seed, "cell": cell,
           "search_grid": normals_ref.grid_shape(lo, hi, cell), "counts": counts, "kept_share": counts[1] / max(counts[0], 1),
           "rounds": counts[3], "max_rounds": 64, "default_lanes": default_lanes,
           "workspace_bytes": _lib.query_reduce_workspace(P, lo, hi, cell),
           "identical_bytes_for": {"lanes": list(LANES), "cells": [cell, 2.0 * cell, 0.4 * cell]}}
    # ---- device calls, the two thread shapes alternating
    times = {lanes: [] for lanes in LANES}
    for it in range(args.warmup + args.runs):
        for lanes in LANES:
            set_lanes(lanes)
            t = timed(lambda: call(min_dist, out=outs[lanes]))
            if it >= args.warmup:
                times[lanes].append(t)
    set_lanes(default_lanes)
    res["reduce_ms"] = {f"lanes_{lanes}": stats(times[lanes], "ms") for lanes in LANES}
    # ---- the whole evaluation, with and without DTU's three steps
    n = np.floor((hi - lo) / MASK_RES + 0.5).astype(int) + 1
    rng = np.random.default_rng(MASK_SEED)
    obs = dict(mask=torch.from_numpy((rng.uniform(size=tuple(n)) < MASK_SET).astype(np.uint8)).to(dev), origin=lo, res=MASK_RES)
    plane = (0.0, 0.0, 1.0, -float(0.5 * (lo[2] + hi[2])))
    options = dict(reduce=dict(min_dist=min_dist, seed=args.seed), obs_mask=obs, plane=plane)
    for name, kw in (("evaluate_cloud", {}), ("evaluate_cloud_dtu", options)):
        walls = []
        for it in range(args.warmup + 10):
            dt, got = wall(lambda: fusion.evaluate_cloud(pred, gt, max_dist=20.0, thresholds=THRESHOLDS, **kw))
            if it >= args.warmup:
                walls.append(dt)
        res[name] = got
        res[name + "_wall_s"] = stats(walls, "s")
    res["obs_mask"] = dict(shape=[int(v) for v in n], res=MASK_RES, set=MASK_SET, seed=MASK_SEED)
    res["plane"] = list(plane)
    # ---- the host baseline
    device_mask = outs[1][0].cpu().numpy()
    parts = []
    for it in range(2):
        mask, tree_s, pass_s = host_greedy(pred_h, lo, hi, min_dist, args.seed)
        parts.append((tree_s, pass_s))
        print(f"host run {it}: tree {tree_s:.3f} s, pass {pass_s:.3f} s", flush=True)
    res["host"] = {"method": "keys as on the device; cKDTree(members); in key order, query_ball_point(p, min_dist) around each kept point",
                   "runs": len(parts), "tree_s": stats([x[0] for x in parts], "s"), "pass_s": stats([x[1] for x in parts], "s"),
                   "total_s": stats([sum(x) for x in parts], "s"), "mask_equal": bool(np.array_equal(mask, device_mask)),
                   "mask_differs_at": int((mask != device_mask).sum())}
    best = min(np.median(times[lanes]) for lanes in LANES)
    res["host_total_over_reduce"] = res["host"]["total_s"]["median_s"] * 1e3 / float(best)
    text = json.dumps(res, indent=1, default=lambda o: np.asarray(o).tolist())
    with open(os.path.join(REPO, "profiles", "cloud_reduce_timing.json"), "w") as f:
        f.write(text + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
