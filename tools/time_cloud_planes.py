#!/usr/bin/env python3
"""Time the plane segmentation of a fused cloud (mvs_cloud_planes, fusion.segment_planes) on the cloud the other cloud
tools use: the synthetic 49-view 640 x 512 scan with every pixel kept, about a million points.

  planes           _lib.cloud_planes at K = 1000 candidates for max_planes = 1 and 5, device events around each call,
                   alternating with the yardstick (b); also K = 64 at max_planes = 1: the count kernel tests one chunk of
                   64 candidates there, so (t_1000 - t_64) * 1024 / 960 estimates its time for the 1024 candidate slots
  (a) host         tests/planes_ref.py's vectorised numpy, one round (candidates and counts) on 16 threads over slices of
                   the candidates, on the same points; its counts are the device's, exactly, before anything is reported
  (b) distance     one _lib.cloud_distance search of the cloud against its resampled copy in the same run: the call less
                   the same call with ONE query (the grid build alone)
  (c) floor        K64 x M tests x 8 double-precision operations (3 products, 2 sums and a difference for s, a product
                   and a comparison for s * s <= thr) over the rate this card reaches in a register-only loop of the same
                   operations (mvs_test_planes_rate), measured here; the ratio floor / estimated count time is written down.
                   That kernel is only in a library built with `make PLANES_MEASURE=-DMVS_PLANES_MEASURE` (MVS_LIB_PATH may
                   point at such a build); without it (c) is left out and the JSON says so

Figures are median [min, max].
    python tools/time_cloud_planes.py [--runs 10] [--warmup 2] [--dist 2.0] [--out FILE] [--calls-only N]
Writes profiles/cloud_planes_timing.json.  --calls-only N builds the cloud, runs the max_planes = 5 call N times and writes
nothing: the program to put under a kernel trace.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import planes_ref as PR  # noqa: E402
from time_cloud_distance import bounding_box, clouds, timed  # noqa: E402
from time_cloud_downsample import stats  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, fusion  # noqa: E402

K, SEED, MIN_INLIERS, THREADS, OPS_PER_TEST = 1000, 0, 3, 16, 8


def host_round(q, t, threads=THREADS):
    """One round of planes_ref on `threads` threads: the candidates, then the counts over slices of them -> (counts, s)."""
    t0 = time.perf_counter()
    cand = PR.candidates(q, 0, K, SEED, t)
    cuts = np.linspace(0, K, threads + 1).astype(int)

    def part(k):
        e = slice(cuts[k], cuts[k + 1])
        return PR.counts_of(q, {name: v[e] for name, v in cand.items()}, chunk=2)
    with ThreadPoolExecutor(threads) as pool:
        counts = np.concatenate(list(pool.map(part, range(threads))))
    return counts, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dist", type=float, default=2.0)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    xyz_h, other_h = clouds(dev, args.tmp)
    xyz, other = torch.from_numpy(xyz_h).to(dev), torch.from_numpy(other_h).to(dev)
    lo, hi = bounding_box(xyz_h)

    def planes(rounds, k=K, extras=False):
        return _lib.cloud_planes(xyz, lo, hi, args.dist, num_candidates=k, max_planes=rounds, min_inliers=MIN_INLIERS, seed=SEED,
                                 cand_counts=extras)
    if args.calls_only:
        for _ in range(args.calls_only):
            planes(5)
        torch.cuda.synchronize()
        print(f"{args.calls_only} calls of 5 rounds at K = {K} on {len(xyz_h)} points")
        return
    raw = ctypes.CDLL(_lib.LIB_PATH)
    rate = getattr(raw, "mvs_test_planes_rate", None)
    if rate is not None:
        rate.restype, rate.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # ---- the result first: the device's counts of round 0 are the host's
    got = planes(5, extras=True)
    torch.cuda.synchronize()
    rounds, counts = got[1].cpu().numpy(), got[2].cpu().numpy()
    member = np.flatnonzero(np.isfinite(xyz_h).all(axis=1) & (xyz_h >= lo).all(axis=1) & (xyz_h <= hi).all(axis=1))
    q = xyz_h[member].astype(np.float64) - 0.5 * (lo + hi)
    host = []
    for it in range(3):
        host_counts, dt = host_round(q, args.dist)
        host.append(dt)
        print(f"host round {it}: {dt:.2f} s", flush=True)
    assert np.array_equal(host_counts, got[4][0].cpu().numpy()), "the device's candidate counts are not the reference's"
    M0 = int(rounds[0, 0])
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "runs": args.runs,
           "points": len(xyz_h), "members": int(counts[0]), "dist": args.dist, "num_candidates": K, "min_inliers": MIN_INLIERS,
           "rounds_of_the_5_plane_call": rounds.tolist(), "counts_of_the_5_plane_call": counts.tolist(),
           "workspace_bytes": _lib.query_planes_workspace(len(xyz_h), K),
           "not_measured": "Open3D's segment_plane (not installed); a real bin scan; K above 1000"}
    # ---- (c) the rate of the same operations in registers
    flops = None
    if rate is None:
        res["fp64_rate"] = "not built: the library has no mvs_test_planes_rate (make PLANES_MEASURE=-DMVS_PLANES_MEASURE)"
    else:
        table = torch.from_numpy(np.random.default_rng(1).normal(size=(64, 8))).to(dev)
        blocks, iters = 4096, 256
        out = torch.zeros(blocks * 4, dtype=torch.int32, device=dev)

        def rate_call():
            _lib.check(rate(table.data_ptr(), blocks, iters, out.data_ptr(), int(torch.cuda.current_stream(dev).cuda_stream)))
        rate_ms = [timed(rate_call) for _ in range(args.warmup + args.runs)][args.warmup:]
        tests = blocks * 256 * 4 * 64 * iters
        flops = OPS_PER_TEST * tests / (np.median(rate_ms) * 1e-3)
        res["fp64_rate"] = {"kernel": "planes_rate_kernel: 4 points per thread in registers, 64 candidates by uniform loads",
                            "blocks": blocks, "iters": iters, "tests": tests, "ops_per_test": OPS_PER_TEST, "ms": stats(rate_ms, "ms"),
                            "ops_per_second": flops}
    # ---- device calls, alternating with the yardstick
    cell = fusion.distance_cell((lo, hi), len(xyz_h))

    def distance(n=None):
        return _lib.cloud_distance(xyz, other if n is None else other[:n], lo, hi, cell, 20.0, ())
    keys = [("distance", "call"), ("distance", "grid"), ("planes", 1), ("planes", 5), ("planes", "K64")]
    times = {k: [] for k in keys}
    for it in range(args.warmup + args.runs):
        rec = {("distance", "call"): timed(distance), ("distance", "grid"): timed(lambda: distance(1)),
               ("planes", 1): timed(lambda: planes(1)), ("planes", 5): timed(lambda: planes(5)),
               ("planes", "K64"): timed(lambda: planes(1, k=64))}
        if it >= args.warmup:
            for k, v in rec.items():
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    search = med[("distance", "call")] - med[("distance", "grid")]
    count_ms = (med[("planes", 1)] - med[("planes", "K64")]) * 1024 / 960
    floor_ms = 1024 * M0 * OPS_PER_TEST / flops * 1e3 if flops else None
    res["distance"] = {"call_ms": stats(times[("distance", "call")], "ms"), "grid_build_ms": stats(times[("distance", "grid")], "ms"),
                       "search_ms": search}
    res["planes"] = {"max_planes_1_ms": stats(times[("planes", 1)], "ms"), "max_planes_5_ms": stats(times[("planes", 5)], "ms"),
                     "max_planes_1_K64_ms": stats(times[("planes", "K64")], "ms"),
                     "max_planes_1_over_the_distance_search": med[("planes", 1)] / search,
                     "max_planes_5_over_the_distance_search": med[("planes", 5)] / search,
                     "count_kernel_round_0_estimate_ms": count_ms, "count_kernel_floor_ms": floor_ms,
                     "floor_over_estimate": floor_ms / count_ms if flops else None, "tests_round_0": 1024 * M0,
                     "note": "the estimate is a difference of two calls; a kernel trace gives the count kernel's own time"}
    res["host"] = {"one_round_s": stats(host, "s"), "threads": THREADS,
                   "method": "planes_ref.candidates, then planes_ref.counts_of over 16 slices of the candidates, 2 candidates x M at a time",
                   "host_round_over_device_max_planes_1": float(np.median(host)) * 1e3 / med[("planes", 1)]}
    text = json.dumps(res, indent=1)
    with open(os.path.join(REPO, "profiles", "cloud_planes_timing.json"), "w") as f:
        f.write(text + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
