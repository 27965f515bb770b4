"""Depth error against ground truth: the scalars of the reference's test mode (train.py:228-238, 302-358).

Drop-ins under the reference's names and signatures, computed by one masked HIP pass (mvs_depth_metrics,
csrc/depth_metrics.hip) instead of boolean indexing and one host synchronisation per scalar:
  mvsnet_loss(depth_est, depth_gt, mask)               models/mvsnet.py:242-244  (pooled over the batch)
  AbsDepthError_metrics(depth_est, depth_gt, mask)     utils.py:151-158          (per image, then batch mean)
  Thres_metrics(depth_est, depth_gt, mask, thres)      utils.py:141-148          (per image, then batch mean)
They take CUDA tensors only and return 0-dim float32 CUDA tensors without synchronising.  An image without a
valid pixel gives NaN, as the reference's mean over an empty selection does.

DepthMetricsAccumulator replaces the test loop's `tensor2float` + DictAverageMeter (utils.py:105-125): update()
only enqueues, mean() copies every batch's sums to the host once and returns the dict test() prints as `final`.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

THRESHOLDS = (1, 2, 4, 8)
KEYS = ("loss", "abs_depth_error") + tuple(f"thres{t}mm_error" for t in THRESHOLDS)


def _sums(depth_est, depth_gt, mask, thresholds):
    for name, t in (("depth_est", depth_est), ("depth_gt", depth_gt), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA(ROCm) tensor: the metrics run in libmvs_hip, there is no CPU "
                               "implementation")
    return _lib.depth_metrics(depth_est, depth_gt, mask, thresholds)[0]


def mvsnet_loss(depth_est, depth_gt, mask):
    """smooth_l1_loss over every pixel of the batch with mask > 0.5 (models/mvsnet.py:242-244)."""
    s = _sums(depth_est, depth_gt, mask, ())
    return (s[:, 2].sum() / s[:, 0].sum()).to(torch.float32)


def AbsDepthError_metrics(depth_est, depth_gt, mask):  # noqa: N802 - the reference's name
    """Mean |est - gt| over each image's valid pixels, then the mean over the batch (utils.py:151-158)."""
    s = _sums(depth_est, depth_gt, mask, ())
    return (s[:, 1] / s[:, 0]).to(torch.float32).mean()


def Thres_metrics(depth_est, depth_gt, mask, thres):  # noqa: N802 - the reference's name
    """Fraction of each image's valid pixels with |est - gt| > thres, then the mean over the batch
    (utils.py:141-148).  The per-image fraction is count / n in fp32, as torch.mean(err_mask.float()) gives it."""
    assert isinstance(thres, (int, float))
    s = _sums(depth_est, depth_gt, mask, (thres,))
    return (s[:, 3].to(torch.float32) / s[:, 0].to(torch.float32)).mean()


def _div(a, b):
    return a / b if b != 0 else math.nan


def batch_scalars(sums, thresholds=THRESHOLDS):
    """One batch's rows [B, 3 + len(thresholds)] (host array of mvs_depth_metrics sums) -> the scalar dict of the
    reference's test_sample: loss pooled over the batch, the other scalars per image and then averaged."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != 3 + len(thresholds) or sums.shape[0] < 1:
        raise ValueError(f"sums must be [B, {3 + len(thresholds)}], got {sums.shape}")
    n = sums[:, 0]
    out = {"loss": _div(float(sums[:, 2].sum()), float(n.sum())),
           "abs_depth_error": float(np.mean([_div(float(a), float(c)) for a, c in zip(sums[:, 1], n)]))}
    for k, t in enumerate(thresholds):
        per_image = [float(np.float32(c) / np.float32(m)) if m != 0 else math.nan for c, m in zip(sums[:, 3 + k], n)]
        out[f"thres{t}mm_error"] = float(np.mean(per_image))
    return out


def final_scalars(sums, batch_sizes, thresholds=THRESHOLDS):
    """Every image's rows [M, 3 + len(thresholds)] in order plus the batch sizes that group them -> the mean over
    batches of batch_scalars (DictAverageMeter.mean(), utils.py:105-125); what test() prints as `final`."""
    sums = np.asarray(sums, dtype=np.float64)
    if sum(batch_sizes) != sums.shape[0]:
        raise ValueError(f"batch sizes add up to {sum(batch_sizes)}, but there are {sums.shape[0]} rows")
    if not batch_sizes:
        raise ValueError("no batch to average")
    total, start = None, 0
    for bs in batch_sizes:
        d = batch_scalars(sums[start:start + bs], thresholds)
        start += bs
        total = d if total is None else {k: total[k] + v for k, v in d.items()}
    return {k: v / len(batch_sizes) for k, v in total.items()}


class DepthMetricsAccumulator:
    """Collects the metric sums of consecutive batches on the device.  update() enqueues one mvs_depth_metrics pass
    on the current stream (rows land in a device buffer that grows as needed) and never synchronises; mean() makes
    the one device-to-host copy and returns final_scalars."""

    def __init__(self, thresholds=THRESHOLDS, device=None):
        self.thresholds = tuple(thresholds)
        self.device = device
        self.batch_sizes = []
        self._rows = None       # float64 [capacity, 3 + len(thresholds)]
        self._used = 0
        self._workspace = None

    def update(self, depth_est, depth_gt, mask):
        if depth_est.dim() == 2:
            depth_est, depth_gt, mask = depth_est[None], depth_gt[None], mask[None]
        B = depth_est.shape[0]
        dev = depth_est.device
        if not depth_est.is_cuda:
            raise RuntimeError("DepthMetricsAccumulator.update needs CUDA(ROCm) tensors")
        if self.device is None:
            self.device = dev
        K = 3 + len(self.thresholds)
        need = self._used + B
        if self._rows is None or need > self._rows.shape[0]:
            cap = max(64, need, 2 * (0 if self._rows is None else self._rows.shape[0]))
            rows = torch.empty((cap, K), dtype=torch.float64, device=dev)
            if self._used:
                rows[:self._used].copy_(self._rows[:self._used])   # stream-ordered, no sync
            self._rows = rows
        nbytes = _lib.query_metrics_workspace(B, depth_est.shape[1], depth_est.shape[2])
        if self._workspace is None or self._workspace.numel() < nbytes:
            self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.depth_metrics(depth_est, depth_gt, mask, self.thresholds, sums_out=self._rows[self._used:need],
                           workspace=self._workspace)
        self._used = need
        self.batch_sizes.append(B)

    def sums(self):
        """Every image's rows so far, on the host (one device-to-host copy)."""
        if self._rows is None:
            return np.zeros((0, 3 + len(self.thresholds)))
        return self._rows[:self._used].cpu().numpy()

    def mean(self):
        return final_scalars(self.sums(), self.batch_sizes, self.thresholds)
