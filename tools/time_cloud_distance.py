#!/usr/bin/env python3
"""Time the scoring of a fused cloud against a ground-truth cloud (mvs_cloud_distance, fusion.evaluate_cloud) on the
synthetic 49-view 640 x 512 scan of tools/time_cloud_outliers.py, with thresholds that keep every pixel (about a million
points).  The ground truth is a jittered, differently sampled copy of the fused cloud of about the same size: GT_KEEP of
its finite points, drawn with a seed, each moved by Gaussian noise of GT_JITTER units per axis.

  accuracy, completeness   one _lib.cloud_distance call per direction on the resident clouds, alternating, device events
                           around each; box = the reference cloud's bounding box, cell = fusion.distance_cell's
  grid                     the same call with ONE query: the grid build over the reference cloud and nothing else to speak
                           of; search = the call's median minus this one's (the search, the counts and the sum tree)
  evaluate_cloud           fusion.evaluate_cloud end to end, both directions, boxes and medians included: host clock
                           around a call that ends in its device-to-host copy
  host                     the same distances on the host, on clouds already there: scipy.spatial.cKDTree(ref) and
                           .query(k=1, distance_upper_bound=max_dist, workers=16), per direction

Figures are median [min, max].  Before anything is reported the device result is checked against the host tree's: the
indices equal wherever the tree's two nearest are not within 1e-12 of one another, the distances to a few ulps, and the
same bytes for three cell sizes.

    python tools/time_cloud_distance.py [--runs 20] [--warmup 3] [--max_dist 20] [--out FILE] [--calls-only N]
Writes profiles/cloud_distance_timing.json.  --calls-only N builds the clouds, runs both directions N times and writes
nothing: the program to put under a kernel trace.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import normals_ref  # noqa: E402
from time_cloud_downsample import D, H, W, stats, wall  # noqa: E402
from time_scan_fusion import NVIEWS, V, write_scan  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, fusion, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.dataset_eval import EvalDataset  # noqa: E402

GT_KEEP, GT_JITTER, GT_SEED = 0.95, 0.5, 7
THRESHOLDS = (1.0, 2.0, 5.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def clouds(dev, tmp):
    """-> (pred float32 [P,3], gt float32 [Q,3]) as host arrays: the fused cloud of the synthetic scan and its jittered,
    resampled copy."""
    root = tempfile.mkdtemp(prefix="mvs_distance_", dir=tmp)
    try:
        data, listfile = write_scan(root, H, W)
        ds = EvalDataset(data, listfile, "test", NVIEWS, D, 1.06, img_res=(H, W), dataset_name="dtu")
        model = MVSNet(refine=False)
        synthetic.randomize_bn_(model, seed=0, prob_gain=30.0)
        model = model.to(dev).eval()
        pred, _ = fusion.reconstruct_scan(model, ds, "scan1", geomask=0, photomask=0.0, device=dev)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rng = np.random.default_rng(GT_SEED)
    finite = pred[np.isfinite(pred).all(axis=1)]
    rows = np.sort(rng.choice(len(finite), int(GT_KEEP * len(finite)), replace=False))
    gt = (finite[rows].astype(np.float64) + rng.normal(0.0, GT_JITTER, (len(rows), 3))).astype(np.float32)
    return pred, gt


def bounding_box(xyz):
    finite = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    return finite.min(axis=0), finite.max(axis=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max_dist", type=float, default=20.0)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 10 or args.calls_only, "at least 10 timed runs"
    _lib.load()
    dev = torch.device("cuda:0")
    pred_h, gt_h = clouds(dev, args.tmp)
    pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
    # direction -> (query, ref, their host copies, the reference's box, the rule's cell)
    sides = {}
    for name, q, r, qh, rh in (("accuracy", pred, gt, pred_h, gt_h), ("completeness", gt, pred, gt_h, pred_h)):
        lo, hi = bounding_box(rh)
        sides[name] = dict(q=q, r=r, qh=qh, rh=rh, lo=lo, hi=hi, cell=fusion.distance_cell((lo, hi), len(rh)))

    def call(s, cell=None, out=None, n=None):
        q = s["q"] if n is None else s["q"][:n]
        return _lib.cloud_distance(s["r"], q, s["lo"], s["hi"], s["cell"] if cell is None else cell, args.max_dist, THRESHOLDS,
                                   indices=True, out=out)
    outs = {k: call(s) for k, s in sides.items()}
    ones = {k: call(s, n=1) for k, s in sides.items()}
    if args.calls_only:
        for _ in range(args.calls_only):
            for k, s in sides.items():
                call(s, out=outs[k])
        torch.cuda.synchronize()
        print(f"{args.calls_only + 1} calls per direction on {len(pred_h)} / {len(gt_h)} points")
        return
    # ---- the result first
    from scipy.spatial import cKDTree
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup,
           "shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D), "pred_points": len(pred_h), "gt_points": len(gt_h),
           "gt": dict(keep=GT_KEEP, jitter=GT_JITTER, seed=GT_SEED), "max_dist": args.max_dist, "thresholds": list(THRESHOLDS),
           "mapping": "one wave per query, 8 queries per wave in turn, 4 waves per block", "directions": {}}
    for k, s in sides.items():
        dist, idx, counts, st = outs[k]
        cells = (s["cell"], 2.0 * s["cell"], 0.5 * s["cell"])
        for cell in cells[1:]:          # the same bytes for every cell size
            other = call(s, cell=cell)
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs[k], other)), (k, cell)
        rh = s["rh"].astype(np.float64)
        qh = s["qh"].astype(np.float64)
        member = normals_ref.members_of(rh, s["lo"], s["hi"])
        ids = np.flatnonzero(member)
        counted = np.isfinite(qh).all(axis=1)
        parts = []
        for it in range(3):
            t0 = time.perf_counter()
            tree = cKDTree(rh[ids])
            t1 = time.perf_counter()
            hd, hj = tree.query(qh[counted], k=1, distance_upper_bound=args.max_dist, workers=16)
            t2 = time.perf_counter()
            parts.append((t1 - t0, t2 - t1))
            print(f"{k} host run {it}: tree {t1 - t0:.3f} s, query {t2 - t1:.3f} s", flush=True)
        d_dist, d_idx = dist.cpu().numpy(), idx.cpu().numpy()
        found = np.isfinite(hd)
        assert (d_dist[~counted] == -1.0).all() and np.array_equal(np.isfinite(d_dist[counted]), found)
        assert np.allclose(d_dist[counted][found], hd[found], rtol=1e-13, atol=0)
        two, _ = tree.query(qh[counted][found], k=2, workers=16)
        clear = two[:, 1] - two[:, 0] > 1e-12 * two[:, 1]          # duplicates and near-ties: the tree picks as it likes
        assert np.array_equal(d_idx[counted][found][clear], ids[hj[found]][clear])
        assert counts.tolist()[:2] == [int(counted.sum()), int(found.sum())]
        res["directions"][k] = {
            "queries": len(qh), "reference_points": len(rh), "members": int(member.sum()), "cell": s["cell"],
            "search_grid": normals_ref.grid_shape(s["lo"], s["hi"], s["cell"]), "counts": counts.tolist(),
            "stats": st.cpu().numpy().tolist(), "identical_bytes_for_cells": list(cells),
            "workspace_bytes": _lib.query_distance_workspace(len(rh), len(qh), s["lo"], s["hi"], s["cell"]),
            "check": {"max_abs_dist_difference_from_the_k_d_tree": float(np.abs(d_dist[counted][found] - hd[found]).max()),
                      "queries_with_a_near_tie": int((~clear).sum())},
            "host": {"method": "scipy.spatial.cKDTree(members).query(k=1, distance_upper_bound=max_dist, workers=16)",
                     "runs": 3, "tree_s": stats([x[0] for x in parts], "s"), "query_s": stats([x[1] for x in parts], "s"),
                     "total_s": stats([sum(x) for x in parts], "s")}}
    # ---- device calls, alternating: the full call and the grid alone, both directions
    times = {(k, what): [] for k in sides for what in ("call", "grid")}
    for it in range(args.warmup + args.runs):
        for k, s in sides.items():
            a = timed(lambda: call(s, out=outs[k]))
            b = timed(lambda: call(s, out=ones[k], n=1))
            if it >= args.warmup:
                times[(k, "call")].append(a)
                times[(k, "grid")].append(b)
    for k in sides:
        d = res["directions"][k]
        d["call_ms"] = stats(times[(k, "call")], "ms")
        d["grid_build_ms"] = stats(times[(k, "grid")], "ms")
        d["search_counts_sum_ms"] = float(np.median(times[(k, "call")]) - np.median(times[(k, "grid")]))
        d["host_total_over_call"] = d["host"]["total_s"]["median_s"] * 1e3 / d["call_ms"]["median_ms"]
    # ---- the whole evaluation
    walls = []
    for it in range(args.warmup + 10):
        dt, got = wall(lambda: fusion.evaluate_cloud(pred, gt, max_dist=args.max_dist, thresholds=THRESHOLDS))
        if it >= args.warmup:
            walls.append(dt)
    res["evaluate_cloud"] = got
    res["evaluate_cloud_wall_s"] = stats(walls, "s")
    text = json.dumps(res, indent=1)
    with open(os.path.join(REPO, "profiles", "cloud_distance_timing.json"), "w") as f:
        f.write(text + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
