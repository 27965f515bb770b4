#!/usr/bin/env python3
"""Time the training path at the training shape (reference train.py defaults: N = 3 views, 512 x 640 images ->
128 x 160 features, D = 192, B = 1) with device events after warm-up:

  cost_volume   forward + backward of the variance cost volume: training.cost_volume (HIP) against the torch
                autograd form written below (grid_sample + the reference's out-of-place sums, mvsnet.py:145-177)
  train_step    one whole optimisation step: training.train_sample on TrainableMVSNet against the same step with
                every stage in torch (FeatureNet, the torch cost volume, CostRegNet, softmax + depth regression)
  soft_argmin   forward + backward of training.soft_argmin against torch softmax + depth regression
  costreg       forward + backward of CostRegNet alone (training._costreg) at the training shape, costreg_impl "torch",
                "hip" and "hip_fused" alternating in the same process on the same seeded volume and upstream gradient;
                also BatchNorm3d forward + backward on a contiguous NCDHW and on a channels_last_3d volume
  train_step    (part of the same key) additionally times train_sample with costreg_impl = "hip" and "hip_fused"
  bn            per normalised CostRegNet layer at the training shape: training.batch_norm_relu forward + backward
                against nn.BatchNorm3d + relu (+ skip addition) on the same channels-last input, alternating, with the
                bytes the fused kernels move (3 or 4 sweeps forward, 5 backward) and the resulting TB/s

and the peak torch.cuda.max_memory_allocated of each.  Prints one JSON document (and writes it to --out).
    python tools/time_train_step.py [--warmup 3] [--iters 10] [--only cost_volume,train_step,soft_argmin,costreg,bn]
The costreg and train_step parts are also written to profiles/train_costreg_timing.json, and with the bn part to
profiles/train_fused_timing.json.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scene_3dreconstruction_mvsnet_amd import _lib, synthetic, training  # noqa: E402

DEV = torch.device("cuda:0")
N, H, W, D = 3, 512, 640, 192


# ---------------------------------------------------------------- the all-torch forms
def torch_cost_volume(feats, proj, dv):
    """feats [B,N,C,h,w], proj [B,N,4,4], dv [B,D] -> variance [B,C,D,h,w]: models/module.py:96-139 and the
    training branch of models/mvsnet.py:145-177 (grid under no_grad, out-of-place sums)."""
    B, n, C, h, w = feats.shape
    Dn = dv.shape[1]
    ref = feats[:, 0]
    ref_volume = ref.unsqueeze(2).repeat(1, 1, Dn, 1, 1)
    volume_sum = ref_volume
    volume_sq_sum = ref_volume ** 2
    del ref_volume
    for v in range(1, n):
        with torch.no_grad():
            pr = torch.matmul(proj[:, v], torch.inverse(proj[:, 0]))
            rot, trans = pr[:, :3, :3], pr[:, :3, 3:4]
            y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=DEV),
                                  torch.arange(w, dtype=torch.float32, device=DEV), indexing="ij")
            xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w, device=DEV)))
            xyz = xyz.unsqueeze(0).repeat(B, 1, 1)
            p = torch.matmul(rot, xyz).unsqueeze(2).repeat(1, 1, Dn, 1) * dv.view(B, 1, Dn, 1) + trans.view(B, 3, 1, 1)
            pxy = p[:, :2] / p[:, 2:3]
            gx = pxy[:, 0] / ((w - 1) / 2) - 1
            gy = pxy[:, 1] / ((h - 1) / 2) - 1
            grid = torch.stack((gx, gy), dim=3)
        warped = F.grid_sample(feats[:, v], grid.view(B, Dn * h, w, 2), mode="bilinear", padding_mode="zeros",
                               align_corners=False).view(B, C, Dn, h, w)
        volume_sum = volume_sum + warped
        volume_sq_sum = volume_sq_sum + warped ** 2
        del warped
    return volume_sq_sum.div_(n).sub_(volume_sum.div_(n).pow_(2))


def torch_soft_argmin(cost, dv):
    prob = F.softmax(cost, dim=1)
    return torch.sum(prob * dv.view(*dv.shape, 1, 1), 1)


def torch_train_step(model, opt, sample):
    """train_sample with every stage in torch (the reference's step, train.py:241-298, minus its logging)."""
    model.train()
    opt.zero_grad()
    imgs, proj, dv = sample["imgs"], sample["proj_matrices"], sample["depth_values"]
    feats = torch.stack([model.feature(imgs[:, v]) for v in range(imgs.shape[1])], dim=1)
    volume = torch_cost_volume(feats, proj, dv)
    cost = training._costreg(model.cost_regularization, volume).squeeze(1)
    depth = torch_soft_argmin(cost, dv)
    loss = training.mvsnet_loss(depth, sample["depth"], sample["mask"])
    loss.backward()
    opt.step()
    return loss


# ---------------------------------------------------------------- timing
def timed(fn, warmup, iters):
    """(median ms, min ms, peak bytes) of fn() over `iters` runs after `warmup`, each bracketed by events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated(DEV) - base
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
            "peak_bytes": int(peak)}


def timed_alternating(fns, warmup, iters):
    """The same figures for several callables run in turn (a, b, a, b, ...) in this process, so that clock and
    allocator state are shared; the peak is taken per callable in a pass of its own at the end."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = {}
    for k, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        fn()
        torch.cuda.synchronize()
        out[k] = {"median_ms": float(np.median(times[k])), "min_ms": float(np.min(times[k])),
                  "max_ms": float(np.max(times[k])), "peak_bytes": int(torch.cuda.max_memory_allocated(DEV) - base)}
    return out


def make_sample():
    imgs, proj, dv = synthetic.make_inputs(N, H, W, D, seed=1)
    rng = np.random.default_rng(2)
    gt = rng.uniform(dv[0, 10], dv[0, -10], size=(1, H // 4, W // 4)).astype(np.float32)
    mask = (rng.uniform(size=gt.shape) > 0.2).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return {"imgs": t(imgs), "proj_matrices": t(proj), "depth_values": t(dv), "depth": t(gt), "mask": t(mask)}


def bench_cost_volume(sample, warmup, iters):
    h, w = H // 4, W // 4
    feats = torch.randn((1, N, 32, h, w), generator=torch.Generator().manual_seed(0)).to(DEV).requires_grad_(True)
    g = torch.randn((1, 32, D, h, w), generator=torch.Generator().manual_seed(1)).to(DEV)
    proj, dv = sample["proj_matrices"], sample["depth_values"]

    def run(fn):
        def step():
            feats.grad = None
            fn(feats, proj, dv).backward(g)
        return step

    out = {"hip": timed(run(training.cost_volume), warmup, iters),
           "torch": timed(run(torch_cost_volume), warmup, iters)}
    # the HIP backward alone (the new kernel plus its zero-fill), for the atomic-byte floor below
    rt = _lib.relative_proj(proj[0])
    out["hip_backward_only"] = timed(lambda: _lib.warp_variance_backward(feats.detach()[0], rt, dv[0], g[0]),
                                     warmup, iters)
    # direct global atomics of a naive scatter: 4 taps x 32 channels x D x h x w per source view, 4 bytes each
    naive_bytes = 4 * 32 * D * h * w * (N - 1) * 4
    out["naive_atomic_bytes"] = naive_bytes
    out["naive_atomic_floor_ms_at_1.3TBps"] = naive_bytes / 1.3e12 * 1e3
    return out


def bench_soft_argmin(warmup, iters):
    h, w = H // 4, W // 4
    cost = (torch.randn((1, D, h, w), generator=torch.Generator().manual_seed(3)) * 5).to(DEV).requires_grad_(True)
    dv = torch.from_numpy(synthetic.depth_values(D))[None].to(DEV)
    gd = torch.randn((1, h, w), device=DEV)

    def hip():
        cost.grad = None
        training.soft_argmin(cost, dv)[0].backward(gd)

    def tor():
        cost.grad = None
        torch_soft_argmin(cost, dv).backward(gd)

    return {"hip": timed(hip, warmup, iters), "torch": timed(tor, warmup, iters)}


def bench_train_step(sample, warmup, iters):
    out = {}
    for name in ("hip", "torch"):
        torch.manual_seed(0)
        model = training.TrainableMVSNet(refine=False).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0)
        if name == "hip":
            out[name] = timed(lambda: training.train_sample(model, opt, sample), warmup, iters)
        else:
            out[name] = timed(lambda: torch_train_step(model, opt, sample), warmup, iters)
        del model, opt
        torch.cuda.empty_cache()
    # the same step with CostRegNet's convolutions in torch and in HIP, alternating
    steps = {}
    for impl in training.COSTREG_IMPLS:
        torch.manual_seed(0)
        model = training.TrainableMVSNet(refine=False).to(DEV)
        model.costreg_impl = impl
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0)
        steps[f"costreg_{impl}"] = (lambda m=model, o=opt: training.train_sample(m, o, sample))
    out.update(timed_alternating(steps, warmup, iters))
    a, b = out["costreg_torch"], out["costreg_hip"]
    out["hip_median_not_above_torch_median"] = bool(b["median_ms"] <= a["median_ms"])
    out["hip_fused_range_entirely_below_hip"] = bool(out["costreg_hip_fused"]["max_ms"] < b["min_ms"])
    return out


# CostRegNet's layers as convolutions: (Cin, Cout, level of the volume the 27-tap sum runs over)
_COSTREG_CONVS = ((32, 8, 0), (8, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 2), (32, 64, 3), (64, 64, 3),
                  (64, 32, 3), (32, 16, 2), (16, 8, 1), (8, 1, 0))


def costreg_gflop():
    """Forward + data gradient + weight gradient of the eleven 3x3x3 layers at the training shape, 2 FLOP per MAC."""
    d, h, w = D, H // 4, W // 4
    mac = sum(27 * ci * co * (d >> lv) * (h >> lv) * (w >> lv) for ci, co, lv in _COSTREG_CONVS)
    return {"forward_gmac": mac / 1e9, "conv0_forward_gmac": 27 * 32 * 8 * d * h * w / 1e9,
            "fwd_dgrad_wgrad_gflop": 3 * 2 * mac / 1e9, "ms_at_155_tflops": 3 * 2 * mac / 155e12 * 1e3}


def bench_costreg(warmup, iters):
    d, h, w = D, H // 4, W // 4
    volume = torch.randn((1, 32, d, h, w), generator=torch.Generator().manual_seed(0)).to(DEV).requires_grad_(True)
    g = torch.randn((1, 1, d, h, w), generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(0)
    cr = training.TrainableMVSNet(refine=False).to(DEV).train().cost_regularization

    def run(impl):
        def step():
            volume.grad = None
            cr.zero_grad(set_to_none=True)
            training._costreg(cr, volume, impl).backward(g)
        return step

    out = timed_alternating({impl: run(impl) for impl in training.COSTREG_IMPLS}, warmup, iters)
    out["flop"] = costreg_gflop()
    t, hp = out["torch"], out["hip"]
    out["speedup_median"] = t["median_ms"] / hp["median_ms"]
    out["hip_fused_range_entirely_below_hip"] = bool(out["hip_fused"]["max_ms"] < hp["min_ms"])
    out["hip_below_torch_and_ranges_disjoint"] = bool(hp["median_ms"] < t["median_ms"] and hp["max_ms"] < t["min_ms"])
    # BatchNorm3d (train mode) forward + backward on conv0's output, the two memory formats
    bn = torch.nn.BatchNorm3d(8).to(DEV).train()
    y = torch.randn((1, 8, d, h, w), generator=torch.Generator().manual_seed(2)).to(DEV)
    variants = {"bn_ncdhw": y.clone().requires_grad_(True),
                "bn_channels_last_3d": y.clone(memory_format=torch.channels_last_3d).requires_grad_(True)}
    gy = {k: torch.randn_like(v) for k, v in variants.items()}

    def bn_run(k):
        def step():
            variants[k].grad = None
            bn(variants[k]).backward(gy[k])
        return step

    out.update(timed_alternating({k: bn_run(k) for k in variants}, warmup, iters))
    return out


# the ten normalised layers: (name, C, level, has a skip)
_BN_LAYERS = (("conv0", 8, 0, False), ("conv1", 16, 1, False), ("conv2", 16, 1, False), ("conv3", 32, 2, False),
              ("conv4", 32, 2, False), ("conv5", 64, 3, False), ("conv6", 64, 3, False), ("conv7", 32, 2, True),
              ("conv9", 16, 1, True), ("conv11", 8, 0, True))


def bench_bn(warmup, iters):
    out = {}
    for name, C, lv, has_skip in _BN_LAYERS:
        d, h, w = D >> lv, (H // 4) >> lv, (W // 4) >> lv
        gen = torch.Generator().manual_seed(C + lv)
        cl = lambda: torch.randn((1, d, h, w, C), generator=gen).to(DEV).permute(0, 4, 1, 2, 3)  # noqa: E731
        x, g = cl().requires_grad_(True), cl()
        skip = cl().requires_grad_(True) if has_skip else None
        bn = torch.nn.BatchNorm3d(C).to(DEV).train()

        def hip():
            x.grad = None
            training.batch_norm_relu(x, bn, relu=True, skip=skip).backward(g)

        def tor():
            x.grad = None
            r = F.relu(bn(x), inplace=True)
            (r if skip is None else skip + r).backward(g)

        res = timed_alternating({"hip": hip, "torch": tor}, warmup, iters)
        vol = d * h * w * C * 4
        res["bytes_moved"] = ((4 if has_skip else 3) + 5) * vol
        res["hip_TBps_at_median"] = res["bytes_moved"] / (res["hip"]["median_ms"] * 1e-3) / 1e12
        res["quoted_peak_TBps"] = 8.0
        out[name] = res
        del x, g, skip
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="cost_volume,soft_argmin,train_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    _lib.load()
    sample = make_sample()
    res = {"shape": {"N": N, "H": H, "W": W, "D": D, "B": 1}, "warmup": args.warmup, "iters": args.iters,
           "device": torch.cuda.get_device_name(DEV), "torch": torch.__version__}
    t0 = time.time()
    for part in args.only.split(","):
        if part == "cost_volume":
            res[part] = bench_cost_volume(sample, args.warmup, args.iters)
        elif part == "soft_argmin":
            res[part] = bench_soft_argmin(args.warmup, args.iters)
        elif part == "train_step":
            res[part] = bench_train_step(sample, args.warmup, args.iters)
        elif part == "costreg":
            res[part] = bench_costreg(args.warmup, args.iters)
        elif part == "bn":
            res[part] = bench_bn(args.warmup, args.iters)
        else:
            raise SystemExit(f"unknown part {part!r}")
    res["wall_s"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    print(text)
    keep = {k: v for k, v in res.items() if k not in ("cost_volume", "soft_argmin")}
    if "costreg" in res or "train_step" in res:
        with open(os.path.join(REPO, "profiles", "train_costreg_timing.json"), "w") as f:
            f.write(json.dumps({k: v for k, v in keep.items() if k != "bn"}, indent=1) + "\n")
    if "costreg" in res or "train_step" in res or "bn" in res:
        with open(os.path.join(REPO, "profiles", "train_fused_timing.json"), "w") as f:
            f.write(json.dumps(keep, indent=1) + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
