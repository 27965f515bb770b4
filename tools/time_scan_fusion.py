#!/usr/bin/env python3
"""Time one scan from images to the fused point cloud, through files and in memory, on a synthetic on-disk scan of 49
views (DTU layout, pair file with 6 sources per view, N = 5 views per depth map):

  files           eval_driver.save_depth_sharded (every depth / confidence map, camera and image to PFM, txt, PNG under
                  a temporary directory) and then fusion.filter_depth (reads them back, one mvs_filter_depth launch,
                  xyz_world and the masks to the host, numpy selection): the path before mvs_fuse_points existed
  files_reuse     the same with reuse_features=True (FeatureNet once per view, as reconstruct_scan runs it)
  memory          fusion.reconstruct_scan: nothing written but the PLY

at cfg2's size (640 x 512, D = 192) and at 1600 x 1184, D = 256.  The paths alternate in one process, --warmup runs
and then --runs timed runs each; wall clock is time.perf_counter around the call and a final device synchronise, and
the figures are median [min, max].  Every path writes its PLY; the files are compared byte for byte.  Thresholds:
geomask = 0 (random weights agree on no geometry) and the photomask that keeps --share of the pixels, taken from the
confidence maps of the warm-up run.

Also reported: the device time of one mvs_fuse_points call (its three kernels together, from events around the
enqueue, median of 20) on the scan's own masks and points; the bytes each path copies from the device to the host,
counted from the shapes; and the host time of decoding the 49 images alone, on one thread and on the 16 threads
reconstruct_scan uses.

    python tools/time_scan_fusion.py [--sizes cfg2,large] [--runs 5] [--warmup 1] [--out FILE]
Writes profiles/scan_fusion_timing.json (merging the sizes measured into what is there).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, data_io, fusion, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.dataset_eval import EvalDataset  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.eval_driver import save_depth_sharded, write_cam  # noqa: E402

SIZES = {"cfg2": dict(H=512, W=640, D=192), "large": dict(H=1184, W=1600, D=256)}
V, NVIEWS = 49, 5


def write_scan(root, H, W):
    """A DTU-style scan of V smooth random images written at the network size (the loader's rescale is the identity),
    cameras on a line, 6 sources per view."""
    data = os.path.join(root, "data")
    os.makedirs(os.path.join(data, "Cameras"))
    os.makedirs(os.path.join(data, "Rectified", "scan1"))
    rng = np.random.default_rng(0)
    K = np.array([[361.5 * W / 160, 0, W / 2], [0, 360.0 * H / 128, H / 2], [0, 0, 1]], np.float32)
    for v in range(V):
        img = (rng.random((H // 8, W // 8, 3)) * 255).astype(np.uint8)
        Image.fromarray(img).resize((W, H), Image.BILINEAR).save(
            os.path.join(data, "Rectified", "scan1", f"rect_{v + 1:03d}_3_r5000.png"), compress_level=1)
        E = np.eye(4, dtype=np.float32)
        E[0, 3], E[1, 3] = -30.0 * v, 5.0 * v
        write_cam(os.path.join(data, "Cameras", f"{v:08d}_cam.txt"), K, E, ["425.0", "2.5", "", ""])
    with open(os.path.join(data, "pair.txt"), "w") as f:
        f.write(f"{V}\n")
        for v in range(V):
            src = [(v + d) % V for d in (1, -1, 2, -2, 3, -3)]
            f.write(f"{v}\n{len(src)} " + " ".join(f"{s} 1.0" for s in src) + "\n")
    listfile = os.path.join(root, "list.txt")
    with open(listfile, "w") as f:
        f.write("scan1\n")
    return data, listfile


def stats(xs):
    return {"median_s": float(np.median(xs)), "min_s": float(np.min(xs)), "max_s": float(np.max(xs)), "runs": len(xs)}


def measure(name, runs, warmup, share, scratch_root):
    H, W, D = SIZES[name]["H"], SIZES[name]["W"], SIZES[name]["D"]
    h, w = H // 4, W // 4
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="mvs_scan_", dir=scratch_root)
    try:
        data, listfile = write_scan(root, H, W)
        pair = os.path.join(data, "pair.txt")
        ds = EvalDataset(data, listfile, "test", NVIEWS, D, 1.06, img_res=(H, W), dataset_name="dtu")
        model = MVSNet(refine=False)
        synthetic.randomize_bn_(model, seed=0, prob_gain=30.0)
        model = model.to(dev).eval()
        out = os.path.join(root, "out")
        thr = dict(geomask=0, photomask=0.8)

        def files(reuse):
            def go():
                shutil.rmtree(out, ignore_errors=True)
                save_depth_sharded(model, ds, out, device=dev, reuse_features=reuse)
                return fusion.filter_depth(os.path.join(out, "scan1"), pair, os.path.join(root, f"files{int(reuse)}.ply"), **thr)
            return go

        def memory():
            return fusion.reconstruct_scan(model, ds, "scan1", plyfilename=os.path.join(root, "memory.ply"), device=dev, **thr)

        paths = {"files": files(False), "files_reuse": files(True), "memory": memory}
        # the photomask that keeps `share` of the pixels, from the maps of a first pass through the files
        paths["files"]()
        conf = np.stack([data_io.read_pfm(os.path.join(out, "scan1", "confidence", f"{v:08d}.pfm"))[0] for v in range(V)])
        thr["photomask"] = float(np.quantile(conf, 1.0 - share))
        times = {k: [] for k in paths}
        points = {}
        for it in range(warmup + runs):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                vertices, _ = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                points[k] = len(vertices)
                if it >= warmup:
                    times[k].append(dt)
                print(f"[{name}] {'warm-up' if it < warmup else 'run'} {it} {k}: {dt:.3f} s, {len(vertices)} points", flush=True)
        plys = {k: open(os.path.join(root, f), "rb").read() for k, f in (("files", "files0.ply"), ("files_reuse", "files1.ply"),
                                                                          ("memory", "memory.ply"))}
        P = points["memory"]
        res = {"shape": dict(V=V, N=NVIEWS, H=H, W=W, D=D, h=h, w=w), "thresholds": dict(thr), "points": P,
               "share_selected": P / (V * h * w), "ply_bytes": len(plys["memory"]),
               "plys_byte_identical": bool(plys["files"] == plys["memory"] == plys["files_reuse"]),
               "wall": {k: stats(v) for k, v in times.items()}}
        m, f = res["wall"]["memory"], res["wall"]["files"]
        res["files_over_memory_at_median"] = f["median_s"] / m["median_s"]
        res["memory_range_entirely_below_files"] = bool(m["max_s"] < f["min_s"])
        # device-to-host bytes, from the shapes
        res["d2h_bytes"] = {"files": {"depth_and_confidence_maps": 2 * V * h * w * 4, "masks": V * 3 * h * w,
                                      "xyz_world": V * h * w * 3 * 8},
                            "memory": {"counts": (V + 1) * 4, "packed_points": 15 * P}}
        for k in ("files", "memory"):
            res["d2h_bytes"][k]["total"] = sum(res["d2h_bytes"][k].values())
        # host time of decoding the scan's images alone (part of every path)
        ds8 = EvalDataset(data, listfile, "test", NVIEWS, D, 1.06, img_res=(H, W), dataset_name="dtu", image_dtype="uint8")
        first = [ds8.view_plan(i)[1][0][0] for i in range(V)]
        t0 = time.perf_counter()
        imgs = [ds8.decode_view(p)[0] for p in first]
        res["decode_49_images_one_thread_s"] = time.perf_counter() - t0
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as pool:     # what reconstruct_scan does
            list(pool.map(ds8.decode_view, first))
        res["decode_49_images_16_threads_s"] = time.perf_counter() - t0
        # mvs_fuse_points alone, on the scan's own filter output
        depths = np.stack([data_io.read_pfm(os.path.join(out, "scan1", "depth_est", f"{v:08d}.pfm"))[0] for v in range(V)])
        cams = [fusion.read_camera_parameters(os.path.join(out, "scan1", "cams", f"{v:08d}_cam.txt")) for v in range(V)]
        pairs = [(m_[1], list(m_[2])) for m_ in ds.metas]
        filtered = fusion.filter_views(depths, conf, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), pairs,
                                       device=dev, **thr)
        images = torch.from_numpy(np.stack(imgs)).to(dev)
        ref_idx = torch.arange(V, dtype=torch.int32, device=dev)
        masks = filtered["masks"].view(torch.uint8)
        ev = []
        for it in range(3 + 20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, _, counts = _lib.fuse_points(filtered["xyz_world"], masks, images, ref_idx)
            b.record()
            b.synchronize()
            if it >= 3:
                ev.append(a.elapsed_time(b))
        assert int(counts[-1]) == P
        res["fuse_points_three_kernels_ms"] = {"median": float(np.median(ev)), "min": float(np.min(ev)), "max": float(np.max(ev)),
                                               "tiles": V * -(-(h * w) // _lib.FUSE_TILE),
                                               "bytes_read_and_written": 2 * V * h * w + P * (24 + 3 + 12 + 3)}
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="cfg2,large")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--share", type=float, default=0.2, help="share of the pixels the photomask keeps")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    _lib.load()
    target = os.path.join(REPO, "profiles", "scan_fusion_timing.json")
    doc = json.load(open(target)) if os.path.exists(target) else {}
    doc.update({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "files_under": args.tmp or tempfile.gettempdir(),
                "warmup": args.warmup})
    doc.setdefault("sizes", {})
    for name in args.sizes.split(","):
        doc["sizes"][name] = measure(name, args.runs, args.warmup, args.share, args.tmp)
        text = json.dumps(doc, indent=1)
        with open(target, "w") as f:
            f.write(text + "\n")
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
