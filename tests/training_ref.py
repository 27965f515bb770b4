"""Reference restatements shared by the training suites (tests/test_gpu_training.py, the cost-volume gradient
suites): the reference's warp + variance in torch, for autograd in any dtype, and float64 bookkeeping of the LDS
window each wave of warp_variance_bwd_kernel needs."""
import numpy as np
import torch
import torch.nn.functional as F

WAVE_WINDOW_TEXELS = 512   # kWinWave of csrc/train_backward.hip


def wave_window_areas(proj, dv, h, w):
    """Host-side bookkeeping in float64: for every wave of warp_variance_bwd_kernel (2 rows x 32 reference pixels x
    a slab of 8 depths) and source view, the area of the bounding box of its in-image bilinear taps -- the LDS window
    the wave needs.  Waves above WAVE_WINDOW_TEXELS add straight to global memory."""
    proj, dv = np.asarray(proj, np.float64), np.asarray(dv, np.float64)
    D = dv.shape[0]
    inv = np.linalg.inv(proj[0])
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), np.ones(h * w)])
    areas = []
    for v in range(1, proj.shape[0]):
        M = proj[v] @ inv
        P = (M[:3, :3] @ xyz)[:, None, :] * dv[None, :, None] + M[:3, 3][:, None, None]
        x0 = np.floor(P[0] / P[2] * w / (w - 1) - 0.5).reshape(D, h, w)
        y0 = np.floor(P[1] / P[2] * h / (h - 1) - 0.5).reshape(D, h, w)
        for d0 in range(0, D, 8):
            for r0 in range(0, h, 2):
                for c0 in range(0, w, 32):
                    X, Y = x0[d0:d0 + 8, r0:r0 + 2, c0:c0 + 32], y0[d0:d0 + 8, r0:r0 + 2, c0:c0 + 32]
                    near = (X >= -1) & (X < w) & (Y >= -1) & (Y < h)
                    xs = np.concatenate([X[near & (X >= 0)], X[near & (X + 1 < w)] + 1])
                    ys = np.concatenate([Y[near & (Y >= 0)], Y[near & (Y + 1 < h)] + 1])
                    if xs.size and ys.size:
                        areas.append((xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1))
    return np.array(areas)


def torch_variance(feats, rt, dv):
    """The reference's homo_warping + variance (models/module.py:96-139, mvsnet.py:145-177) in the dtype of feats,
    with the grid from the library's relative projections rt [(N-1),12]."""
    N, C, h, w = feats.shape
    D = dv.shape[0]
    y, x = torch.meshgrid(torch.arange(h, dtype=feats.dtype, device=feats.device),
                          torch.arange(w, dtype=feats.dtype, device=feats.device), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones_like(x).reshape(-1)))
    S = feats[0].unsqueeze(1).expand(C, D, h, w)
    Q = S ** 2
    for v in range(1, N):
        R, t = rt[v - 1, :9].view(3, 3).to(feats.dtype), rt[v - 1, 9:].to(feats.dtype)
        p = (R @ xyz).unsqueeze(1) * dv.to(feats.dtype).view(1, D, 1) + t.view(3, 1, 1)
        gx = p[0] / p[2] / ((w - 1) / 2) - 1
        gy = p[1] / p[2] / ((h - 1) / 2) - 1
        grid = torch.stack((gx, gy), dim=-1).view(1, D * h, w, 2)
        wv = F.grid_sample(feats[v:v + 1], grid, mode="bilinear", padding_mode="zeros",
                           align_corners=False).view(C, D, h, w)
        S = S + wv
        Q = Q + wv ** 2
    return Q / N - (S / N) ** 2
