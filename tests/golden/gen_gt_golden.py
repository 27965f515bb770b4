#!/usr/bin/env python3
"""Golden vectors for ground-truth evaluation (tests/golden/fx_gt.npz):
  * the REFERENCE's training-format readers (datasets/dtu_yao.py, datasets/blender.py MVSDataset) in val and test
    mode on the seeded trees of tests/synthetic_gt_dataset.py, with random.seed fixed before each constructor;
  * the REFERENCE's mvsnet_loss (models/mvsnet.py), AbsDepthError_metrics and Thres_metrics at 1/2/4/8 (utils.py)
    on seeded est / gt / mask arrays with the edge cases the HIP kernel must reproduce.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gt_golden.py
torchvision is not installed: a stub `torchvision.utils` is registered before utils.py is imported (only its
image-logging helpers use it)."""
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.environ.get("MVS_REFERENCE", "/root/reference"))
tv = types.ModuleType("torchvision")
tv.utils = types.ModuleType("torchvision.utils")
sys.modules.setdefault("torchvision", tv)
sys.modules.setdefault("torchvision.utils", tv.utils)

import torch  # noqa: E402

from synthetic_gt_dataset import write_blender, write_dtu_yao  # noqa: E402

import datasets.blender as ref_blender  # noqa: E402  (reference)
import datasets.dtu_yao as ref_dtu  # noqa: E402  (reference)
from models.mvsnet import mvsnet_loss  # noqa: E402  (reference)
from utils import AbsDepthError_metrics, Thres_metrics  # noqa: E402  (reference)

SEED = 0
NVIEWS, NDEPTHS, ISCALE = 3, 16, 1.06
# (format, mode, Nlights) whose light choice and length are recorded; items are recorded for the first four
CASES = (("dtu_yao", "val", "1:1"), ("dtu_yao", "test", "1:1"), ("blender", "val", "2:4"), ("blender", "test", "2:4"),
         ("blender", "test", "3:4"), ("blender", "test", "0:4"), ("blender", "test", "-3:4"))
ITEM_IDX = (0, 5, -1)


def metric_arrays():
    """est, gt, mask [3, 37, 53] float32: image 1 has no valid pixel; mask values of exactly 0.5 (not valid);
    errors exactly 1, 2, 4 and 8; inf in gt outside the mask; large errors for the 8 mm bin."""
    rng = np.random.default_rng(5)
    B, h, w = 3, 37, 53
    gt = rng.uniform(425.0, 470.0, size=(B, h, w)).astype(np.float32)
    est = (gt + rng.normal(0.0, 3.0, size=(B, h, w))).astype(np.float32)
    mask = rng.choice(np.array([0.0, 0.5, 127 / 255.0, 128 / 255.0, 1.0], np.float32), size=(B, h, w),
                      p=[0.2, 0.1, 0.1, 0.1, 0.5])
    mask[1] = np.where(mask[1] > 0.5, 0.5, mask[1])      # no valid pixel in image 1
    for k, t in enumerate((1.0, 2.0, 4.0, 8.0)):          # |e| == t exactly (integral depths)
        for b in (0, 2):
            gt[b, k, :8] = 440.0
            est[b, k, :4] = 440.0 + t
            est[b, k, 4:8] = 440.0 - t
            mask[b, k, :8] = 1.0
    est[2, 10:14, :] += 20.0                              # beyond 8 mm
    gt[0, 20, :] = np.where(mask[0, 20] > 0.5, gt[0, 20], np.inf)   # inf outside the mask
    gt[2, 21, :] = np.where(mask[2, 21] > 0.5, gt[2, 21], -np.inf)
    return est, gt, mask


def reference_metrics(out, est, gt, mask, prefix):
    e, g, m = torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)
    out[f"{prefix}_est"], out[f"{prefix}_gt"], out[f"{prefix}_mask"] = est, gt, mask
    out[f"{prefix}_loss"] = np.float32(mvsnet_loss(e, g, m).item())
    out[f"{prefix}_abs"] = np.float32(AbsDepthError_metrics(e, g, m > 0.5).item())
    out[f"{prefix}_thres"] = np.array([Thres_metrics(e, g, m > 0.5, t).item() for t in (1, 2, 4, 8)], np.float32)
    # per image: the values the batch means average (Thres_metrics of one image = count / n in fp32)
    per = []
    for b in range(est.shape[0]):
        sl = slice(b, b + 1)
        per.append([AbsDepthError_metrics(e[sl], g[sl], m[sl] > 0.5).item()] +
                   [Thres_metrics(e[sl], g[sl], m[sl] > 0.5, t).item() for t in (1, 2, 4, 8)] +
                   [mvsnet_loss(e[sl], g[sl], m[sl]).item()])
    out[f"{prefix}_per_image"] = np.array(per, np.float32)
    out[f"{prefix}_errormap"] = ((e - g).abs() * m).numpy()


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        roots = {"dtu_yao": os.path.join(d, "dtu"), "blender": os.path.join(d, "blender")}
        lists = {"dtu_yao": write_dtu_yao(roots["dtu_yao"]), "blender": write_blender(roots["blender"])}
        classes = {"dtu_yao": ref_dtu.MVSDataset, "blender": ref_blender.MVSDataset}
        for ci, (fmt, mode, nl) in enumerate(CASES):
            random.seed(SEED)
            ds = classes[fmt](roots[fmt], lists[fmt], mode, NVIEWS, NDEPTHS, ISCALE, pairfile="pair.txt", Nlights=nl)
            key = f"{fmt}_{mode}_{nl}"
            out[f"{key}_len"] = np.int64(len(ds))
            out[f"{key}_lights"] = np.array([m[1] for m in ds.metas], np.int64)
            if ci >= 4:
                continue
            for idx in ITEM_IDX:
                s = ds[idx]
                for k in ("imgs", "proj_matrices", "depth", "depth_values", "mask"):
                    if k != "imgs" or idx == ITEM_IDX[0]:   # random pixels do not compress: one sample's
                        out[f"{key}_{idx}_{k}"] = np.ascontiguousarray(s[k])
    est, gt, mask = metric_arrays()
    reference_metrics(out, est, gt, mask, "m")
    # a NaN error inside the mask (NaN estimate) next to an ordinary image
    est2, gt2, mask2 = est[[0, 2]].copy(), gt[[0, 2]].copy(), mask[[0, 2]].copy()
    est2[1, 30, 5] = np.nan
    mask2[1, 30, 5] = 1.0
    reference_metrics(out, est2, gt2, mask2, "nan")
    np.savez_compressed(os.path.join(HERE, "fx_gt.npz"), **out)
    print({k: getattr(v, "shape", v) for k, v in out.items() if not k.endswith(("imgs", "errormap"))})


if __name__ == "__main__":
    main()
