#!/usr/bin/env python3
"""Throughput of ground-truth evaluation at 512x640, N=5, D=192 (fp32 volumes) on an in-memory training-format set
(items carry imgs, proj_matrices, depth_values, GT depth and mask), in three variants:
  (a) eval_gt.evaluate_depth: loader thread + copy stream, one masked HIP metrics pass per batch, one sync per run
  (b) the reference's test() loop restated: synchronous copies, model(...), then mvsnet_loss / AbsDepthError_metrics
      / Thres_metrics(1, 2, 4, 8) in torch with boolean indexing and one .item() per scalar (train.py:302-358)
  (c) the loop of (b) without the metrics (maps only), so that (b) - (c) is what the metric code costs per map
Usage: python tools/time_gt_eval.py [--n 200] [--batch_size 1] [--image_dtype uint8|float32] [--variants abc]
For kernel times run it under `rocprofv3 --kernel-trace --stats` with --variants a."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scene_3dreconstruction_mvsnet_amd import MVSNet, synthetic  # noqa: E402
from scene_3dreconstruction_mvsnet_amd.eval_gt import evaluate_depth  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--n", type=int, default=200)
p.add_argument("--batch_size", type=int, default=1)
p.add_argument("--image_dtype", default="uint8", choices=["uint8", "float32"])
p.add_argument("--variants", default="abc")
args = p.parse_args()

cfg = synthetic.CONFIGS["cfg2"]
N, H, W, D = cfg["nviews"], cfg["H"], cfg["W"], cfg["D"]
imgs, proj, dv = synthetic.make_inputs(N, H, W, D, seed=0, interval_scale=cfg["interval_scale"])
rng = np.random.default_rng(0)
gt = rng.uniform(float(dv[0, 0]), float(dv[0, -1]), size=(H // 4, W // 4)).astype(np.float32)
mask = (rng.random(size=(H // 4, W // 4)) < 0.7).astype(np.float32)
img_item = np.rint(imgs[0] * 255).astype(np.uint8) if args.image_dtype == "uint8" else imgs[0]


class Mem:
    def __len__(self):
        return args.n

    def __getitem__(self, i):
        return {"imgs": img_item, "proj_matrices": proj[0], "depth_values": dv[0], "depth": gt, "mask": mask}


dev = torch.device("cuda:0")
model = MVSNet(refine=False)
synthetic.randomize_bn_(model, seed=0)
model = model.to(dev).eval()


def reference_loop(ds, batch_size, with_metrics):
    """train.py test() restated: the scalars of test_sample, one .item() each, averaged per batch."""
    total, count = {}, 0
    with torch.no_grad():
        for start in range(0, len(ds), batch_size):
            items = [ds[i] for i in range(start, min(start + batch_size, len(ds)))]
            b = {k: torch.from_numpy(np.stack([it[k] for it in items])).to(dev) for k in items[0]}
            depth_est = model(b["imgs"], b["proj_matrices"], b["depth_values"])["depth"]
            if not with_metrics:
                continue
            depth_gt, m = b["depth"], b["mask"] > 0.5
            out = {"loss": F.smooth_l1_loss(depth_est[m], depth_gt[m], reduction="mean").item()}

            def per_image(f):
                return torch.stack([f(depth_est[i][m[i]], depth_gt[i][m[i]]) for i in range(len(items))]).mean()
            out["abs_depth_error"] = per_image(lambda e, g: torch.mean((e - g).abs())).item()
            for t in (1, 2, 4, 8):
                out[f"thres{t}mm_error"] = per_image(lambda e, g: torch.mean(((e - g).abs() > t).float())).item()
            total = out if not total else {k: total[k] + v for k, v in out.items()}
            count += 1
    torch.cuda.synchronize()
    return {k: v / count for k, v in total.items()} if count else None


runs = {"a": ("evaluate_depth", lambda: evaluate_depth(model, Mem(), batch_size=args.batch_size, device=dev)),
        "b": ("reference loop + metrics", lambda: reference_loop(Mem(), args.batch_size, True)),
        "c": ("reference loop, maps only", lambda: reference_loop(Mem(), args.batch_size, False))}
results = {}
for key in args.variants:
    name, fn = runs[key]
    fn()                        # warm-up: workspaces, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    dt = time.perf_counter() - t0
    results[key] = res
    print(f"({key}) {name}: {args.n / dt:.1f} maps/s ({dt / args.n * 1e3:.3f} ms per map, {args.n} maps, "
          f"batch {args.batch_size}, {args.image_dtype} images)", flush=True)
if "a" in results and "b" in results:
    print("a:", results["a"])
    print("b:", results["b"])
    for k, v in results["a"].items():
        assert abs(v - results["b"][k]) <= 1e-6 * max(1.0, abs(v)), (k, v, results["b"][k])
