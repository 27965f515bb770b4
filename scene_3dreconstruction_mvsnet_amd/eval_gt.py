"""Ground-truth depth evaluation: the counterpart of the reference's `train.py --mode test` (train.py:228-238,
302-358), inference only.

evaluate_depth(model, dataset, batch_size) groups consecutive items into batches as
`DataLoader(shuffle=False, drop_last=False)` does (the last batch may be partial), runs the model on each batch
and returns the mean over batches of the test loop's scalars -- `loss` (mvsnet_loss, pooled over the batch),
`abs_depth_error` and `thres{1,2,4,8}mm_error` (per image, then the batch mean) -- the dict test() prints as
`final`.  As in the reference, the result depends on the batch size.  The metrics are one masked HIP pass per
batch (metrics.DepthMetricsAccumulator); the whole run synchronises once, at the end.

Loading reuses the eval driver's pipeline (decoder threads + loader thread copying on a side stream), with the GT
depth and mask travelling with each sample; `reuse_features=True` computes the maps from a FeatureNet bank
(eval_driver.FeatureSlots) with bit-identical results.

    python -m scene_3dreconstruction_mvsnet_amd.eval_gt --dataset dtu_yao --testpath DATA --testlist LIST \\
        --loadckpt model.ckpt [--NtestViews 5 --numdepth 192 --interval_scale 1.06 --batch_size 1 ...]
"""
from __future__ import annotations

import argparse
import queue
import threading

import torch

from .eval_driver import _check_reuse_features, _FeatureBank, _loaded, _loader
from .metrics import DepthMetricsAccumulator


def evaluate_depth(model, dataset, batch_size=1, device=None, decoders=16, reuse_features=False, feature_slots=64,
                   accumulator=None):
    """Mean over batches of the reference test loop's scalars (see the module docstring).  dataset[i] is a dict
    with imgs [N,3,H,W] (float32 or uint8), proj_matrices [N,4,4], depth_values [D], depth [h,w], mask [h,w]
    (dataset_gt.DtuYaoDataset / BlenderDataset).  `accumulator` (a fresh DepthMetricsAccumulator) lets the caller
    keep the per-image sums."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if len(dataset) == 0:
        raise ValueError("the dataset is empty")
    device = device or torch.device("cuda", torch.cuda.current_device())
    indices = list(range(len(dataset)))
    if reuse_features:   # refused before any work starts
        if not hasattr(dataset, "view_plan"):
            raise ValueError("reuse_features needs a dataset with view_plan() (image path of every view)")
        _check_reuse_features(model, dataset, indices[:1], feature_slots)
    model = model.to(device).eval()
    acc = DepthMetricsAccumulator(device=device) if accumulator is None else accumulator
    q: "queue.Queue" = queue.Queue(maxsize=4)
    with torch.cuda.device(device), torch.no_grad():
        copy_stream = torch.cuda.Stream(device)
        compute = torch.cuda.current_stream(device)
        th = threading.Thread(target=_loader, args=(dataset, indices, device, copy_stream, q, decoders, None, False,
                                                    feature_slots if reuse_features else 0),
                              kwargs={"extra_keys": ("depth", "mask")}, daemon=True)
        th.start()
        batch = []      # per item: device inputs [imgs, proj, dv] (plain) or the finished depth map (bank)
        gts = []        # per item: (GT depth [1,h,w], mask [1,h,w])
        bank = _FeatureBank(model, feature_slots, device)

        def flush():
            depth_gt = torch.cat([g for g, _ in gts]) if len(gts) > 1 else gts[0][0]
            mask = torch.cat([m for _, m in gts]) if len(gts) > 1 else gts[0][1]
            if reuse_features:
                depth_est = torch.cat(batch) if len(batch) > 1 else batch[0]
            else:   # one forward per batch, as the reference's loop calls it
                imgs, proj, dv = (torch.cat(t) if len(batch) > 1 else t[0] for t in zip(*batch))
                depth_est = model(imgs, proj, dv)["depth"]
            acc.update(depth_est, depth_gt, mask)
            batch.clear()
            gts.clear()

        for _, _, dev, plan in _loaded(q, compute):
            gts.append((dev[3], dev[4]))
            batch.append(dev[:3] if plan is None else bank.forward(dev, plan)["depth"])   # map by map, in sample order
            if len(gts) == batch_size:
                flush()
        if gts:
            flush()     # the partial last batch (drop_last=False)
        th.join()
        return acc.mean()


def main(argv=None):
    from .dataset_gt import find_dataset_def
    from .mvsnet import MVSNet, _load_checkpoint

    p = argparse.ArgumentParser(description="Score a checkpoint against ground-truth depth (train.py --mode test)")
    p.add_argument("--dataset", default="dtu_yao", choices=["dtu_yao", "blender"])
    p.add_argument("--testpath", required=True)
    p.add_argument("--testlist", default="lists/dtu/test.txt")
    p.add_argument("--pairfile", default="pair.txt")
    p.add_argument("--NtestViews", type=int, default=5)
    p.add_argument("--numdepth", type=int, default=192)
    p.add_argument("--interval_scale", type=float, default=1.06)
    p.add_argument("--Nlights", type=str, default="1:1")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--loadckpt", required=True)
    p.add_argument("--storage_dtype", default="f32", choices=["f32", "f16", "bf16"])
    p.add_argument("--reuse_features", action="store_true")
    args = p.parse_args(argv)
    ds = find_dataset_def(args.dataset)(args.testpath, args.testlist, "test", args.NtestViews, args.numdepth,
                                        args.interval_scale, pairfile=args.pairfile, Nlights=args.Nlights,
                                        image_dtype="uint8")
    model = MVSNet(refine=False)
    _load_checkpoint(model, args.loadckpt)
    model.storage_dtype = args.storage_dtype
    result = evaluate_depth(model, ds, batch_size=args.batch_size, reuse_features=args.reuse_features)
    print("final", result)
    return result


if __name__ == "__main__":
    main()
