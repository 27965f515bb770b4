#!/usr/bin/env python3
"""Time the registration of a fused cloud onto a ground-truth cloud (mvs_cloud_register, fusion.register_cloud,
fusion.evaluate_cloud(register=...)) on the clouds of tools/time_cloud_distance.py: the synthetic 49-view 640 x 512 scan
with every pixel kept (the source, about a million points) against its jittered 95 % resampling (the target).

  distance         the yardstick, in the same process and run: one _lib.cloud_distance call, source -> target, and the same
                   call with ONE query (the grid build alone); search = the difference
  register         _lib.cloud_register with rel_fitness = rel_rmse = 0, so that every step is taken: max_iterations = 0 (the
                   grid and one evaluation) and max_iterations = 30 (31 evaluations, 30 solves), both modes, alternating
                   with the yardstick, device events around each; per iteration = (t_30 - t_0) / 30; overhead = per
                   iteration over the yardstick's search
  default          the call with the default criteria: how many iterations it runs and what it costs
  host             tests/register_ref.py's step with scipy's cKDTree (built once, query on 16 threads) in place of the brute
                   force: seconds per iteration over HOST_ITS iterations
  evaluate_cloud   fusion.evaluate_cloud with and without register, alternating, host clock around a call that ends in its
                   device-to-host copy

Figures are median [min, max].  Before anything is reported the device's first evaluation is checked against the host
tree's correspondences (equal wherever the tree's two nearest are not within 1e-12 of one another) and the result bytes
against a second cell size.

    python tools/time_cloud_register.py [--runs 10] [--warmup 2] [--max_dist 5] [--out FILE] [--calls-only N]
Writes profiles/cloud_register_timing.json.  --calls-only N builds the clouds, runs the 30-iteration call N times per mode
and writes nothing: the program to put under a kernel trace.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import register_ref as RR  # noqa: E402
from time_cloud_distance import bounding_box, clouds, timed  # noqa: E402
from time_cloud_downsample import stats, wall  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, fusion  # noqa: E402

ITS, HOST_ITS, KNN = 30, 3, 30


def host_iteration(tree, ids, T, src, tgt, nrm, lo, hi, max_dist):
    """One iteration of tests/register_ref.py's loop with the tree's nearest neighbour -> (T_next, idx)."""
    s = RR.image(T, src)
    d, j = tree.query(s, k=1, distance_upper_bound=max_dist, workers=16)
    ok = np.isfinite(d)
    si, qi = s[ok], tgt[ids[j[ok]]]
    terms = np.zeros((len(si), RR.TERMS))
    terms[:, 0] = terms[:, 1] = 1.0
    terms[:, 2] = d[ok] * d[ok]
    origin = 0.5 * (np.asarray(lo) + np.asarray(hi))
    if nrm is None:
        sp, qp = si - origin, qi - origin
        terms[:, 3:6], terms[:, 6:9] = sp, qp
        terms[:, 9:18] = (sp[:, :, None] * qp[:, None, :]).reshape(-1, 9)
    else:
        n = nrm[ids[j[ok]]]
        r = ((si - qi) * n).sum(axis=1)
        J = np.concatenate([np.cross(si, n), n], axis=1)
        iu = np.triu_indices(6)
        terms[:, 3:24] = J[:, iu[0]] * J[:, iu[1]]
        terms[:, 24:30] = J * r[:, None]
        terms[:, 30] = r * r
    sums = terms.sum(axis=0)
    sums[0] = len(src)
    return RR.compose(RR.step(sums, nrm is not None, origin), T), np.where(ok, ids[np.minimum(j, len(ids) - 1)], -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max_dist", type=float, default=5.0)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None, help="a second place for the JSON")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the scan's files go")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    _lib.load()
    dev = torch.device("cuda:0")
    src_h, tgt_h = clouds(dev, args.tmp)
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    lo, hi = bounding_box(tgt_h)
    lo, hi = lo - args.max_dist, hi + args.max_dist
    cell = fusion.distance_cell((lo, hi), len(tgt_h))
    nrm = fusion.estimate_normals(tgt, knn=KNN, box=(lo, hi))[0]
    torch.cuda.synchronize()
    modes = {"point_to_point": None, "point_to_plane": nrm}

    def register(mode, its, rel=0.0, c=None, indices=False):
        return _lib.cloud_register(tgt, src, lo, hi, cell if c is None else c, args.max_dist, target_normals=modes[mode],
                                   max_iterations=its, rel_fitness=rel, rel_rmse=rel, history=True, indices=indices)

    def distance(n=None):
        return _lib.cloud_distance(tgt, src if n is None else src[:n], lo, hi, cell, args.max_dist, ())
    if args.calls_only:
        for _ in range(args.calls_only):
            distance()
            for mode in modes:
                register(mode, ITS)
        torch.cuda.synchronize()
        print(f"{args.calls_only} calls per mode on {len(src_h)} / {len(tgt_h)} points")
        return
    # ---- the result first
    from scipy.spatial import cKDTree
    import normals_ref
    tgt64, src64, nrm64 = tgt_h.astype(np.float64), src_h.astype(np.float64), nrm.cpu().numpy().astype(np.float64)
    counted = np.isfinite(src64).all(axis=1)
    ids = np.flatnonzero(normals_ref.members_of(tgt64, lo, hi))
    t0 = time.perf_counter()
    tree = cKDTree(tgt64[ids])
    tree_s = time.perf_counter() - t0
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "runs": args.runs,
           "source_points": len(src_h), "target_points": len(tgt_h), "max_dist": args.max_dist, "cell": cell,
           "search_grid": normals_ref.grid_shape(lo, hi, cell), "normals_knn": KNN,
           "workspace_bytes": _lib.query_register_workspace(len(tgt_h), len(src_h), lo, hi, cell), "modes": {},
           "not_measured": "Open3D itself (not installed); a real bin scan against a CAD model"}
    first = register("point_to_point", 0, indices=True)
    d, j = tree.query(src64[counted], k=2, workers=16)
    clear = (d[:, 1] - d[:, 0] > 1e-12 * d[:, 1]) & (d[:, 0] <= args.max_dist)
    assert np.array_equal(first[5].cpu().numpy()[counted][clear], ids[j[clear, 0]])
    for mode in modes:
        a, b = register(mode, ITS), register(mode, ITS, c=2.0 * cell)
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a[:4], b[:4])), mode
        host, T = [], np.eye(4)
        for it in range(HOST_ITS):
            t0 = time.perf_counter()
            T, _ = host_iteration(tree, ids, T, src64[counted], tgt64, None if modes[mode] is None else nrm64, lo, hi, args.max_dist)
            host.append(time.perf_counter() - t0)
            print(f"{mode} host iteration {it}: {host[-1]:.3f} s", flush=True)
        dev_T = a[3][HOST_ITS, :16].reshape(4, 4).cpu().numpy()
        dflt = register(mode, ITS, rel=1e-6)
        res["modes"][mode] = {"counts_all_steps": a[1].tolist(), "stats_all_steps": a[2].tolist(),
                              "counts_default_criteria": dflt[1].tolist(), "stats_default_criteria": dflt[2].tolist(),
                              "host_iteration_s": stats(host, "s"), "host_tree_build_s": tree_s,
                              "host_method": "cKDTree(target members), query(k=1, distance_upper_bound=max_dist, workers=16), numpy sums and solve",
                              "max_abs_difference_of_T_after_the_host_iterations": float(np.abs(dev_T - T).max())}
    # ---- device calls, alternating
    times = {k: [] for k in [("distance", "call"), ("distance", "grid")] + [(m, w) for m in modes for w in ("its0", "its30", "default")]}
    for it in range(args.warmup + args.runs):
        rec = {("distance", "call"): timed(distance), ("distance", "grid"): timed(lambda: distance(1))}
        for mode in modes:
            rec[(mode, "its0")] = timed(lambda: register(mode, 0))
            rec[(mode, "its30")] = timed(lambda: register(mode, ITS))
            rec[(mode, "default")] = timed(lambda: register(mode, ITS, rel=1e-6))
        if it >= args.warmup:
            for k, v in rec.items():
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    search = med[("distance", "call")] - med[("distance", "grid")]
    res["distance"] = {"call_ms": stats(times[("distance", "call")], "ms"), "grid_build_ms": stats(times[("distance", "grid")], "ms"),
                       "search_counts_sum_ms": search}
    for mode in modes:
        per = (med[(mode, "its30")] - med[(mode, "its0")]) / ITS
        res["modes"][mode].update({"its0_ms": stats(times[(mode, "its0")], "ms"), "its30_ms": stats(times[(mode, "its30")], "ms"),
                                   "default_criteria_ms": stats(times[(mode, "default")], "ms"), "per_iteration_ms": per,
                                   "per_iteration_over_the_distance_search": per / search,
                                   "host_iteration_over_device_iteration": res["modes"][mode]["host_iteration_s"]["median_s"] * 1e3 / per})
    # ---- evaluate_cloud with and without, alternating
    walls = {"plain": [], "register": []}
    opt = dict(max_dist=args.max_dist, point_to_plane=True, knn=KNN)
    for it in range(1 + 3):
        for name, kw in (("plain", {}), ("register", dict(register=opt))):
            dt, got = wall(lambda: fusion.evaluate_cloud(src, tgt, max_dist=20.0, **kw))
            if it >= 1:
                walls[name].append(dt)
            if name == "register":
                res["evaluate_cloud_register"] = {k: got[k] for k in ("transformation", "register_fitness", "register_rmse", "overall")}
    res["evaluate_cloud_wall_s"] = {k: stats(v, "s") for k, v in walls.items()}
    text = json.dumps(res, indent=1)
    with open(os.path.join(REPO, "profiles", "cloud_register_timing.json"), "w") as f:
        f.write(text + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
