#!/usr/bin/env python3
"""Time the statistical outlier removal of a fused cloud (mvs_cloud_outliers) on the synthetic 49-view 640 x 512 scan of
tools/time_scan_fusion.py, with thresholds that keep every pixel (about a million points), inside the crop box of
tools/time_cloud_downsample.py, beside mvs_cloud_normals on the same box, cell and number of neighbours: the two run the
same search, so the normals are the yardstick of the new call's time.

  outliers, normals   one _lib.cloud_outliers and one _lib.cloud_normals call on the resident cloud, ALTERNATING, device
                      events around each; the excess of the outliers' median over the normals' is held against the
                      spread (max - min) the normals show over those very runs
  host                the same definition on the host, on the cloud already copied: scipy.spatial.cKDTree (build + one
                      k-nearest query of every member) and numpy (mean distances, mean, standard deviation, mark)
  scan_ds, scan_ds_outliers   fusion.reconstruct_scan end to end with downsample=... without / with outliers=...,
                      alternating, host clock + synchronise

Figures are median [min, max].  Before anything is reported the device result is checked: the three counts and the
statistics against the host's (a k-d tree orders ties as it likes and numpy sums in its own order: the distances to a few
ulps, the statistics to 1e-12), the flags wherever the distance is not within 1e-9 of the threshold, and the same bytes
for every cell size.

    python tools/time_cloud_outliers.py [--runs 20] [--warmup 2] [--nb 20] [--std 2.0] [--out FILE] [--calls-only N]
Writes profiles/cloud_outliers_timing.json.  --calls-only N builds the cloud, runs the device call N times (cell 5) and
writes nothing: the program to put under a kernel trace.
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
import outliers_ref  # noqa: E402
from time_cloud_downsample import BIN_CELLS, D, H, W, stats, wall  # noqa: E402
from time_scan_fusion import NVIEWS, V, write_scan  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, fusion, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.dataset_eval import EvalDataset  # noqa: E402

CELLS = (2.5, 5.0, 10.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nb", type=int, default=20)
    ap.add_argument("--std", type=float, default=2.0)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 10 or args.calls_only, "at least 10 timed runs"
    _lib.load()
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="mvs_outliers_", dir=args.tmp)
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
        call = lambda cell, out=None: _lib.cloud_outliers(xyz, lo, hi, cell=cell, nb_neighbors=args.nb,     # noqa: E731
                                                          std_ratio=args.std, masked=True, out=out)
        normals = lambda out=None: _lib.cloud_normals(xyz, lo, hi, cell=5.0, knn=max(args.nb, 3), out=out)  # noqa: E731
        outs = call(5.0)
        n_outs = normals()
        if args.calls_only:
            for _ in range(args.calls_only):
                call(5.0, out=outs)
            torch.cuda.synchronize()
            print(f"{args.calls_only + 1} calls on P = {P}, nb {args.nb}, search grid {normals_ref.grid_shape(lo, hi, 5.0)}")
            return
        # ---- the result first
        dist, keep, masked, cnt, st = outs
        for cell in CELLS:          # the same bytes for every cell size
            other = call(cell)
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, other)), cell
        p = vertices.astype(np.float64)
        member = normals_ref.members_of(p, lo, hi)
        ids = np.flatnonzero(member)
        M = len(ids)
        assert cnt.tolist()[0] == M == n_outs[2].tolist()[0]
        from scipy.spatial import cKDTree

        def host_path():
            t0 = time.perf_counter()
            tree = cKDTree(p[ids])
            t1 = time.perf_counter()
            d, _ = tree.query(p[ids], k=min(args.nb, M), workers=-1)
            t2 = time.perf_counter()
            mean_d = d.reshape(M, -1).sum(axis=1) / d.reshape(M, -1).shape[1]
            x = mean_d[mean_d > 0]
            mean, std = x.mean(), x.std(ddof=1)
            kept = (mean_d > 0) & (mean_d < mean + args.std * std)
            t3 = time.perf_counter()
            return (t1 - t0, t2 - t1, t3 - t2), mean_d, (mean, std, mean + args.std * std), kept
        parts = []
        for it in range(3):
            dt, h_dist, h_stats, h_keep = host_path()
            parts.append(dt)
            print(f"host run {it}: tree {dt[0]:.3f} s, query {dt[1]:.3f} s, statistics + mark {dt[2]:.3f} s", flush=True)
        d_dist, d_keep, d_stats = dist.cpu().numpy(), keep.cpu().numpy(), st.cpu().numpy()
        assert (d_dist[~member] == -1.0).all() and not d_keep[~member].any()
        assert np.allclose(d_dist[ids], h_dist, rtol=1e-13, atol=0), float(np.abs(d_dist[ids] - h_dist).max())
        assert np.allclose(d_stats, h_stats, rtol=1e-12), (d_stats, h_stats)
        clear = np.abs(h_dist - h_stats[2]) > 1e-9 * h_stats[2]
        assert np.array_equal(d_keep[ids][clear], h_keep[clear])
        assert cnt.tolist()[1] == int((h_dist > 0).sum()) and abs(cnt.tolist()[2] - int(h_keep.sum())) <= int((~clear).sum())
        bits = masked.cpu().numpy().view(np.uint32)
        assert np.array_equal(bits, outliers_ref.masked_bits(vertices, d_keep))
        res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup,
               "shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D), "points": P, "nb_neighbors": args.nb, "std_ratio": args.std,
               "box_min": lo.tolist(), "box_max": hi.tolist(), "voxel_size": v, "counts": cnt.tolist(),
               "stats": d_stats.tolist(), "identical_bytes_for_cells": list(CELLS),
               "check": {"max_abs_dist_difference_from_the_k_d_tree": float(np.abs(d_dist[ids] - h_dist).max()),
                         "members_within_1e-9_of_the_threshold": int((~clear).sum())},
               "host": {"method": "scipy.spatial.cKDTree (build, query of every member with all cores) + numpy mean, std, mark",
                        "runs": 3, "tree_s": stats([x[0] for x in parts], "s"), "query_s": stats([x[1] for x in parts], "s"),
                        "statistics_mark_s": stats([x[2] for x in parts], "s"),
                        "total_s": stats([sum(x) for x in parts], "s")}}
        # ---- device calls, alternating
        t_out, t_nrm = [], []
        for it in range(3 + args.runs):
            a = timed(lambda: call(5.0, out=outs))
            b = timed(lambda: normals(out=n_outs))
            if it >= 3:
                t_out.append(a)
                t_nrm.append(b)
        res["outliers_call_ms"] = stats(t_out, "ms")
        res["normals_call_same_box_cell_knn_ms"] = stats(t_nrm, "ms")
        excess = float(np.median(t_out) - np.median(t_nrm))
        spread = float(max(t_nrm) - min(t_nrm))
        res["outliers_minus_normals_median_ms"] = excess
        res["normals_spread_max_minus_min_ms"] = spread
        res["outliers_within_the_normals_spread"] = bool(excess <= spread)
        res["outliers_call_by_cell_ms"] = {}
        for cell in CELLS:
            ts = [timed(lambda: call(cell, out=outs)) for _ in range(3 + args.runs)][3:]
            res["outliers_call_by_cell_ms"][str(cell)] = stats(ts, "ms")
        res["search_grid"] = {str(cell): normals_ref.grid_shape(lo, hi, cell) for cell in CELLS}
        res["outliers_workspace_bytes"] = {str(cell): _lib.query_outliers_workspace(P, lo, hi, cell) for cell in CELLS}
        # ---- the chain
        down = dict(voxel_size=v, box=(lo, hi), scale=0.01)
        with_o = dict(down, outliers=dict(nb_neighbors=args.nb, std_ratio=args.std, cell=5.0))
        times = {"scan_ds": [], "scan_ds_outliers": []}
        for it in range(args.warmup + 10):
            for k, d in (("scan_ds", down), ("scan_ds_outliers", with_o)):
                dt, got = wall(lambda: fusion.reconstruct_scan(model, ds, "scan1", downsample=d, **thr))
                assert len(got[0]) == P
                if it >= args.warmup:
                    times[k].append(dt)
                print(f"{'warm-up' if it < args.warmup else 'run'} {it} {k}: {dt:.4f} s", flush=True)
        assert got[4]["counts"].tolist() == cnt.tolist()
        res["voxels_with_outliers_removed"] = len(got[2])
        res["wall"] = {k: stats(x, "s") for k, x in times.items()}
        text = json.dumps(res, indent=1)
        with open(os.path.join(REPO, "profiles", "cloud_outliers_timing.json"), "w") as f:
            f.write(text + "\n")
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        print(text)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
