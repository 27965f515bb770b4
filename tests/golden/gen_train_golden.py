#!/usr/bin/env python3
"""Golden vectors for one training step (tests/golden/fx_train.npz), from the REFERENCE's pure-torch model on CPU:
MVSNet(refine=False).train() with weights_seed0.npz, a seeded tiny scene (N = 3 views, D = 16, 64 x 96 images ->
16 x 24 features), mvsnet_loss against a seeded GT depth and mask, then backward().  Stored: the loss, the depth,
the gradients of the three feature maps (retain_grad), the full gradients of a few named parameters, the gradient
norm of every parameter, and every BN running statistic after the step's forward.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_train_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ.get("MVS_REFERENCE", "/root/reference"))

import torch  # noqa: E402

from models.mvsnet import MVSNet, mvsnet_loss  # noqa: E402  (reference)
from scene_3dreconstruction_mvsnet_amd import synthetic  # noqa: E402

N, H, W, D = 3, 64, 96, 16
# parameters whose whole gradient is stored (the rest: norms only)
FULL_GRADS = ("feature.feature.weight", "feature.feature.bias", "feature.conv0.conv.weight",
              "cost_regularization.conv0.conv.weight", "cost_regularization.conv0.bn.weight",
              "cost_regularization.conv11.0.weight", "cost_regularization.prob.weight",
              "cost_regularization.prob.bias")


def scene():
    imgs, proj, dv = synthetic.make_inputs(N, H, W, D, seed=3)
    rng = np.random.default_rng(11)
    h, w = H // 4, W // 4
    # a smooth GT inside the depth range, and a mask with invalid (0), borderline (0.5) and valid (1) pixels
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gt = dv[0, 3] + (dv[0, -4] - dv[0, 3]) * (0.5 + 0.4 * np.sin(xx / 5.0) * np.cos(yy / 4.0))
    gt = (gt + rng.normal(0.0, 0.5, size=(h, w)))[None].astype(np.float32)
    mask = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(1, h, w), p=[0.2, 0.1, 0.7])
    return imgs, proj, dv, gt, mask


def main():
    torch.manual_seed(0)
    with np.load(os.path.join(HERE, "weights_seed0.npz")) as z:
        weights = {k: torch.from_numpy(z[k].copy()) for k in z.files}
    model = MVSNet(refine=False)
    model.load_state_dict(weights)
    model.train()
    imgs, proj, dv, gt, mask = scene()
    feats = []

    def keep(_mod, _inp, out):
        out.retain_grad()
        feats.append(out)

    model.feature.register_forward_hook(keep)
    out = model(torch.from_numpy(imgs), torch.from_numpy(proj), torch.from_numpy(dv))
    loss = mvsnet_loss(out["depth"], torch.from_numpy(gt), torch.from_numpy(mask))
    loss.backward()
    rec = {"imgs": imgs, "proj": proj, "dv": dv, "gt": gt, "mask": mask,
           "loss": np.float32(loss.item()), "depth": out["depth"].detach().numpy(),
           "feat_grad": np.stack([f.grad[0].numpy() for f in feats]),
           "feats": np.stack([f.detach()[0].numpy() for f in feats])}
    names = []
    norms = []
    for name, p in model.named_parameters():
        names.append(name)
        norms.append(float(p.grad.double().norm()))
        if name in FULL_GRADS:
            rec["grad/" + name] = p.grad.numpy()
    rec["grad_norm_names"] = np.array(names)
    rec["grad_norms"] = np.array(norms, np.float64)
    for name, b in model.named_buffers():
        if "running_" in name:
            rec["bn/" + name] = b.numpy()
    path = os.path.join(HERE, "fx_train.npz")
    np.savez_compressed(path, **rec)
    print(f"{path}: {os.path.getsize(path)} bytes, loss {loss.item():.6f}")


if __name__ == "__main__":
    main()
