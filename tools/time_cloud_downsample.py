#!/usr/bin/env python3
"""Time the crop + voxel downsample of a fused cloud (mvs_cloud_downsample) on the synthetic 49-view 640 x 512 scan of
tools/time_scan_fusion.py, with thresholds that keep every pixel (the largest cloud the scan can give, about a million
points).  The box is the middle of that cloud (the 5 % .. 95 % quantile per axis) and the voxel size gives the box about
the cell count of the reference's bin at 5 mm (124 x 84 x 50).

  device          one _lib.cloud_downsample call on the resident cloud, device events around the enqueue
  copy_full       the packed full cloud to the host (what reconstruct_scan copies), host clock, ends in the copy's sync
  copy_small      the packed downsampled cloud to the host
  host_cloud_ref  the same cloud through tests/cloud_ref.py on the host, in this process (the cloud already copied): what a
                  user without the device step runs, Open3D or numpy
  scan, scan_ds   fusion.reconstruct_scan end to end without / with downsample=..., alternating, host clock + synchronise

Figures are median [min, max].  The device result is compared with cloud_ref (counts and colours exactly, coordinates
within cloud_ref's bound) before anything is reported.

    python tools/time_cloud_downsample.py [--runs 10] [--warmup 2] [--out FILE] [--calls-only N]
Writes profiles/cloud_downsample_timing.json.  --calls-only N builds the cloud, runs the device call N times and writes
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

import cloud_ref  # noqa: E402
from time_scan_fusion import NVIEWS, V, write_scan  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, fusion, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.dataset_eval import EvalDataset  # noqa: E402

H, W, D = 512, 640, 192
BIN_CELLS = 124 * 84 * 50


def stats(xs, unit):
    return {f"median_{unit}": float(np.median(xs)), f"min_{unit}": float(np.min(xs)), f"max_{unit}": float(np.max(xs)),
            "runs": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 10 or args.calls_only, "at least 10 timed runs"
    _lib.load()
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="mvs_cloud_", dir=args.tmp)
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
        n = cloud_ref.grid_shape(lo, hi, v)
        xyz, rgb = torch.from_numpy(vertices).to(dev), torch.from_numpy(colours).to(dev)
        out = _lib.cloud_downsample(xyz, rgb, lo, hi, v, scale=0.01)
        if args.calls_only:
            for _ in range(args.calls_only):
                _lib.cloud_downsample(xyz, rgb, lo, hi, v, scale=0.01, out=out)
            torch.cuda.synchronize()
            print(f"{args.calls_only + 1} calls on P = {P}, grid {n}, voxel {v}")
            return
        # the result first
        want = cloud_ref.downsample(vertices, colours, lo, hi, v, 0.01)
        Q = want["voxels"]
        assert out[2].tolist() == [want["kept"], Q]
        assert np.array_equal(out[1][:Q].cpu().numpy(), want["rgb"])
        err = np.abs(out[0][:Q].cpu().numpy().astype(np.float64) - want["mean"])
        assert (err <= want["bound"]).all()
        res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup,
               "shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D), "points": P, "kept": want["kept"], "voxels": Q,
               "box_min": lo.tolist(), "box_max": hi.tolist(), "voxel_size": v, "grid": n, "cells": int(np.prod(n)),
               "workspace_bytes": _lib.query_cloud_workspace(P, lo, hi, v), "largest_voxel_count": int(want["count"].max()),
               "matches_cloud_ref": True, "max_error_over_bound": float((err / want["bound"]).max())}
        # one device call, events around it
        ev = []
        for it in range(3 + 2 * args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.cloud_downsample(xyz, rgb, lo, hi, v, scale=0.01, out=out)
            b.record()
            b.synchronize()
            if it >= 3:
                ev.append(a.elapsed_time(b))
        res["device_call_ms"] = stats(ev, "ms")
        # the copies, and the host's own downsample of the copied cloud
        small = (out[0][:Q], out[1][:Q])
        times = {"copy_full": [], "copy_small": [], "host_cloud_ref": [], "scan": [], "scan_ds": []}
        for it in range(args.warmup + args.runs):
            for k, fn in (("copy_full", lambda: fusion._packed_to_host(xyz, rgb)),
                          ("copy_small", lambda: fusion._packed_to_host(*small))):
                dt, got = wall(fn)
                if it >= args.warmup:
                    times[k].append(dt)
            t0 = time.perf_counter()
            cloud_ref.downsample(vertices, colours, lo, hi, v, 0.01)
            if it >= args.warmup:
                times["host_cloud_ref"].append(time.perf_counter() - t0)
        down = dict(voxel_size=v, box=(lo, hi), scale=0.01)
        for it in range(args.warmup + args.runs):
            for k, fn in (("scan", lambda: fusion.reconstruct_scan(model, ds, "scan1", **thr)),
                          ("scan_ds", lambda: fusion.reconstruct_scan(model, ds, "scan1", downsample=down, **thr))):
                dt, got = wall(fn)
                assert len(got[0]) == P and (k == "scan" or len(got[2]) == Q)
                if it >= args.warmup:
                    times[k].append(dt)
                print(f"{'warm-up' if it < args.warmup else 'run'} {it} {k}: {dt:.4f} s", flush=True)
        res["wall"] = {k: stats(x, "s") for k, x in times.items()}
        res["d2h_bytes"] = {"full_cloud": 15 * P, "downsampled_cloud": 15 * Q, "counts": 16,
                            "reconstruct_scan": 15 * P + 4 * (V + 1),
                            "reconstruct_scan_with_downsample": 15 * P + 4 * (V + 1) + 15 * Q + 16}
        w = res["wall"]
        res["copy_saved_s_at_median"] = w["copy_full"]["median_s"] - w["copy_small"]["median_s"]
        res["device_step_below_copy_saved"] = bool(res["device_call_ms"]["max_ms"] * 1e-3 <
                                                   w["copy_full"]["min_s"] - w["copy_small"]["max_s"])
        res["host_path_s_at_median"] = w["copy_full"]["median_s"] + w["host_cloud_ref"]["median_s"]
        text = json.dumps(res, indent=1)
        with open(os.path.join(REPO, "profiles", "cloud_downsample_timing.json"), "w") as f:
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
