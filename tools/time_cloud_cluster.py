#!/usr/bin/env python3
"""Time the device DBSCAN of a fused cloud (mvs_cloud_cluster, fusion.cluster_cloud) on the synthetic 49-view 640 x 512
scan of tools/time_scan_fusion.py, with thresholds that keep every pixel (about a million points), inside the crop box of
tools/time_cloud_downsample.py, for eps at two and at four voxel edges.

  cluster, per eps   one _lib.cloud_cluster call on the resident cloud, device events around it; cell = the rule of
                     fusion.cluster_cloud, max(eps, distance_cell(box, P))
  host               scikit-learn's DBSCAN(algorithm="kd_tree", n_jobs=16) on the members, on the cloud already copied;
                     its labels must be the device's, every one
  scan_ds, scan_ds_clusters   fusion.reconstruct_scan end to end with downsample=... without / with clusters=... (eps two
                     voxel edges), alternating, host clock + synchronise

Figures are median [min, max].  Before anything is reported three cell sizes must give the same bytes.  The device figures
are written before the host yardstick starts (it needs minutes and gigabytes at the larger eps), and again after it.

    python tools/time_cloud_cluster.py [--runs 20] [--warmup 3] [--min-points 10] [--min-size 50] [--no-host] [--out FILE]
                                       [--calls-only N]
Writes profiles/cloud_cluster_timing.json.  --calls-only N builds the cloud, runs the device call N times (eps two voxel
edges) and writes nothing: the program to put under a kernel trace.
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
from time_cloud_downsample import BIN_CELLS, D, H, W, stats, wall  # noqa: E402
from time_cloud_outliers import timed  # noqa: E402
from time_scan_fusion import NVIEWS, V, write_scan  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, fusion, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.dataset_eval import EvalDataset  # noqa: E402

EPS_VOXELS = (2.0, 4.0)
HOST_JOBS = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-points", type=int, default=10)
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the scikit-learn yardstick")
    ap.add_argument("--host-max-neighbours", type=float, default=1.5e9,
                    help="skip the yardstick at an eps where scikit-learn would hold more neighbours than this (8 bytes each)")
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 10 or args.calls_only, "at least 10 timed runs"
    _lib.load()
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="mvs_cluster_", dir=args.tmp)

    def write(res):
        text = json.dumps(res, indent=1)
        for path in [os.path.join(REPO, "profiles", "cloud_cluster_timing.json")] + ([args.out] if args.out else []):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text + "\n")
        return text
    try:
        data, listfile = write_scan(root, H, W)
        ds = EvalDataset(data, listfile, "test", NVIEWS, D, 1.06, img_res=(H, W), dataset_name="dtu")
        model = MVSNet(refine=False)
        synthetic.randomize_bn_(model, seed=0, prob_gain=30.0)
        model = model.to(dev).eval()
        thr = dict(geomask=0, photomask=0.0, device=dev)
        vertices, colours = fusion.reconstruct_scan(model, ds, "scan1", **thr)
        P = len(vertices)
        finite = vertices[np.isfinite(vertices).all(axis=1)].astype(np.float64)
        lo, hi = np.quantile(finite, 0.05, axis=0).round(2), np.quantile(finite, 0.95, axis=0).round(2)
        v = float(f"{(np.prod(hi - lo) / BIN_CELLS) ** (1 / 3):.3g}")
        xyz = torch.from_numpy(vertices).to(dev)
        rule = lambda eps: max(eps, fusion.distance_cell((lo, hi), P))      # noqa: E731

        def call(eps, cell=None, out=None):
            return _lib.cloud_cluster(xyz, lo, hi, rule(eps) if cell is None else cell, eps, min_points=args.min_points,
                                      min_size=args.min_size, out=out)
        if args.calls_only:
            outs = call(2.0 * v)
            for _ in range(args.calls_only):
                call(2.0 * v, out=outs)
            torch.cuda.synchronize()
            print(f"{args.calls_only + 1} calls on P = {P}, eps {2.0 * v}, counts {outs[2].tolist()}, search grid "
                  f"{normals_ref.grid_shape(lo, hi, rule(2.0 * v))}")
            return
        member = normals_ref.members_of(vertices.astype(np.float64), lo, hi)
        ids = np.flatnonzero(member)
        res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "runs": args.runs,
               "shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D), "points": P, "members": int(member.sum()),
               "box_min": lo.tolist(), "box_max": hi.tolist(), "voxel_size": v, "min_points": args.min_points,
               "min_size": args.min_size, "eps": {}}
        device = {}
        for k in EPS_VOXELS:
            eps = k * v
            cell = rule(eps)
            t0 = timed(lambda: call(eps))                                       # the first call, reported apart
            outs = call(eps)
            for other in (2.0 * cell, 0.5 * cell):      # the same bytes for every cell size
                got = call(eps, cell=other)
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, got)), (eps, other)
            ts = [timed(lambda: call(eps, out=outs)) for _ in range(args.warmup + args.runs)][args.warmup:]
            counts = outs[2].tolist()
            assert counts[0] == len(ids)
            device[k] = outs[0].cpu().numpy()
            res["eps"][f"{k:g}_voxels"] = {
                "eps": eps, "cell": cell, "search_grid": normals_ref.grid_shape(lo, hi, cell), "counts": counts,
                "counts_are": ["members", "core", "border", "noise", "clusters", "kept", "largest"],
                "workspace_bytes": _lib.query_cluster_workspace(P, lo, hi, cell), "first_call_ms": t0,
                "call_ms": stats(ts, "ms"), "identical_bytes_for_cells": [cell, 2.0 * cell, 0.5 * cell]}
            print(f"eps {k:g} voxels: {json.dumps(res['eps'][f'{k:g}_voxels'])}", flush=True)
        # ---- the chain
        down = dict(voxel_size=v, box=(lo, hi), scale=0.01)
        with_c = dict(down, clusters=dict(eps=2.0 * v, min_points=args.min_points, min_size=args.min_size))
        times = {"scan_ds": [], "scan_ds_clusters": []}
        for it in range(args.warmup + 10):
            for name, d in (("scan_ds", down), ("scan_ds_clusters", with_c)):
                dt, got = wall(lambda: fusion.reconstruct_scan(model, ds, "scan1", downsample=d, **thr))
                assert len(got[0]) == P
                if it >= args.warmup:
                    times[name].append(dt)
                print(f"{'warm-up' if it < args.warmup else 'run'} {it} {name}: {dt:.4f} s", flush=True)
        assert got[4]["counts"].tolist() == res["eps"]["2_voxels"]["counts"]
        res["voxels_with_small_clusters_removed"] = len(got[2])
        res["wall"] = {name: stats(x, "s") for name, x in times.items()}
        res["host"] = "not run yet"
        print(write(res), flush=True)
        # ---- the host yardstick
        if args.no_host:
            res["host"] = "skipped (--no-host)"
        else:
            from sklearn.cluster import DBSCAN
            m = vertices[ids].astype(np.float64)
            res["host"] = {"method": f"sklearn.cluster.DBSCAN(algorithm='kd_tree', n_jobs={HOST_JOBS}) on the members, float64"}
            from scipy.spatial import cKDTree
            tree = cKDTree(m)
            sample = m[np.random.default_rng(0).integers(0, len(m), 2000)]
            for k in EPS_VOXELS:
                # scikit-learn holds every neighbourhood at once, 8 bytes a neighbour: estimated from 2,000 members first
                mean_nb = float(tree.query_ball_point(sample, k * v, return_length=True).mean())
                if mean_nb * len(m) > args.host_max_neighbours:
                    res["host"][f"{k:g}_voxels"] = {"not_run": f"about {mean_nb:.0f} neighbours per member, {mean_nb * len(m):.3g} "
                                                               f"in all, above --host-max-neighbours {args.host_max_neighbours:g}"}
                    print(f"host eps {k:g} voxels: {res['host'][f'{k:g}_voxels']['not_run']}", flush=True)
                    continue
                t = time.perf_counter()
                labels = DBSCAN(eps=k * v, min_samples=args.min_points, algorithm="kd_tree", n_jobs=HOST_JOBS).fit(m).labels_
                dt = time.perf_counter() - t
                differ = int((labels != device[k][ids]).sum())
                res["host"][f"{k:g}_voxels"] = {"seconds": dt, "labels_that_differ": differ,
                                                "over_device_call": dt * 1e3 / res["eps"][f"{k:g}_voxels"]["call_ms"]["median_ms"]}
                print(f"host eps {k:g} voxels: {dt:.2f} s, {differ} labels differ", flush=True)
                write(res)
                assert differ == 0, (k, differ)
        print(write(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
