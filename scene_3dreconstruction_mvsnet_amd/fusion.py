"""Depth-map filter / fusion on the GPU: the counterpart of the reference's `filter_depth`
(eval.py:590-800) and its helpers `reproject_with_depth` / `check_geometric_consistency`
(eval.py:508-585), `depth2pts_np` (eval.py:253-265), `save_mask` (eval.py:141-144)
(SURVEY.md §8 f3).

All reference views of a scan go through ONE launch of `mvs_filter_depth`; the numpy / cv2.remap
loops of the reference are not reproduced on the host.  What stays on the host is file I/O and the
boolean selection of the fused points (eval.py:753-759).

Differences from the reference, flagged rather than hidden:
  * cv2.remap is restated inside the kernel (1/32-pixel quantised bilinear, zero border); OpenCV is
    not importable here, so that one call is pinned only by the oracle's hand-computed cases.  The rest
    of the chain is pinned to the reference's own functions (tests/golden/fx_filter.npz).
  * the reference's PLY block (eval.py:789-800) raises AttributeError as written
    (`vertices_colors.dtype` on a list); `write_ply` emits what that block is evidently meant to
    produce through plyfile: binary little-endian vertices x,y,z (float) + red,green,blue (uchar).
"""
from __future__ import annotations

import os

import numpy as np
import torch
from PIL import Image

from . import _lib, data_io
from .dataset_eval import parse_pair_file


def read_camera_parameters(filename: str):
    """intrinsics 3x3, extrinsics 4x4 (float32) from a cams/*_cam.txt written by the depth stage;
    no /4 rescale (eval.py:89-104)."""
    with open(filename) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    extr = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intr = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intr, extr


def save_mask(filename: str, mask: np.ndarray) -> None:
    assert mask.dtype == np.bool_
    Image.fromarray(mask.astype(np.uint8) * 255).save(filename)


def _pad_pairs(pairs, n_view_filter):
    S = max(1, max(len(list(s)[:n_view_filter]) for _, s in pairs))
    ref = np.array([r for r, _ in pairs], np.int32)
    src = np.full((len(pairs), S), -1, np.int32)
    for i, (_, s) in enumerate(pairs):
        s = list(s)[:n_view_filter]
        src[i, :len(s)] = s
    return ref, src


def filter_views(depths, confs, intrinsics, extrinsics, pairs, n_view_filter=10, photomask=0.8,
                 geomask=3, condmask_pixel=1.0, condmask_depth=0.01, device=None):
    """Geometric + photometric filtering of every reference view in `pairs`.

    depths, confs [V,h,w] float32 (numpy or torch; index = view id), intrinsics [V,3,3],
    extrinsics [V,4,4] float32, pairs = [(ref_view, [src_view, ...]), ...] as read from pair.txt.
    Defaults are eval.py:45-49.  Returns torch tensors on the GPU:
      geo_sum [R,h,w] int32, depth_avg [R,h,w] float64, masks [R,3,h,w] bool (photo, geo, final),
      xyz_world [R,h*w,3] float64.
    """
    if not torch.cuda.is_available():
        raise RuntimeError("filter_views needs the GPU: libmvs_hip has no CPU implementation")
    device = device or torch.device("cuda", torch.cuda.current_device())
    depths = torch.as_tensor(np.asarray(depths) if not torch.is_tensor(depths) else depths,
                             dtype=torch.float32).to(device)
    confs = torch.as_tensor(np.asarray(confs) if not torch.is_tensor(confs) else confs,
                            dtype=torch.float32).to(device)
    V = depths.shape[0]
    ref, src = _pad_pairs(pairs, n_view_filter)
    if ref.min() < 0 or ref.max() >= V or src.max() >= V:
        raise RuntimeError(f"pair list names a view outside [0,{V})")
    ref_mats, pair_mats = _lib.filter_compose(intrinsics, extrinsics, ref, src)
    geo, avg, masks, xyz = _lib.filter_depth(
        depths, confs, torch.from_numpy(ref_mats).to(device), torch.from_numpy(pair_mats).to(device),
        torch.from_numpy(ref).to(device), torch.from_numpy(src).to(device),
        photomask, geomask, condmask_pixel, condmask_depth)
    return dict(geo_sum=geo, depth_avg=avg, masks=masks.bool(), xyz_world=xyz)


def write_ply(filename: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    rec = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
              "property float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nend_header\n" % len(rec))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def filter_depth(scan_out_folder: str, pair_file: str, plyfilename: str | None = None,
                 n_view_filter=10, photomask=0.8, geomask=3, condmask_pixel=1.0, condmask_depth=0.01,
                 device=None):
    """Filter + fuse one scan from the files the depth stage wrote under `scan_out_folder`
    (cams/, depth_est/, confidence/, images/ -- eval.py:626-630,677-678), write mask/*.png
    (eval.py:709-712) and optionally the fused cloud.  Returns (vertices float64 [P,3],
    colours uint8 [P,3])."""
    pairs = parse_pair_file(pair_file)
    views = sorted({r for r, _ in pairs} | {s for _, ss in pairs for s in list(ss)[:n_view_filter]})
    V = max(views) + 1
    depths = confs = None
    Ks = np.tile(np.eye(3, dtype=np.float32), (V, 1, 1))
    Es = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    for v in views:
        d = data_io.read_pfm(os.path.join(scan_out_folder, "depth_est", f"{v:08d}.pfm"))[0]
        if depths is None:
            depths = np.zeros((V,) + d.shape, np.float32)
            confs = np.zeros((V,) + d.shape, np.float32)
        depths[v] = d
        cfn = os.path.join(scan_out_folder, "confidence", f"{v:08d}.pfm")
        if os.path.exists(cfn):
            confs[v] = data_io.read_pfm(cfn)[0]
        Ks[v], Es[v] = read_camera_parameters(os.path.join(scan_out_folder, "cams", f"{v:08d}_cam.txt"))
    out = filter_views(depths, confs, Ks, Es, pairs, n_view_filter, photomask, geomask,
                       condmask_pixel, condmask_depth, device)
    masks = out["masks"].cpu().numpy()
    xyz = out["xyz_world"].cpu().numpy()
    os.makedirs(os.path.join(scan_out_folder, "mask"), exist_ok=True)
    vertices, colours = [], []
    h_d, w_d = depths.shape[1:]
    for i, (ref_view, _) in enumerate(pairs):
        photo, geo, final = masks[i]
        for tag, m in (("photo", photo), ("geo", geo), ("final", final)):
            save_mask(os.path.join(scan_out_folder, "mask", f"{ref_view:08d}_{tag}.png"), m)
        img = np.array(Image.open(os.path.join(scan_out_folder, "images", f"{ref_view:08d}.png")),
                       dtype=np.float32) / 255.0                                   # eval.py:130-134
        assert img.shape[:2] == (4 * h_d, 4 * w_d), "incompatible depth and image dimensions."
        vertices.append(xyz[i][final.reshape(-1)])                                 # eval.py:753
        colours.append((img[1::4, 1::4, :][final] * 255).astype(np.uint8))         # eval.py:755,759
    vertices = np.concatenate(vertices, 0)
    colours = np.concatenate(colours, 0)
    if plyfilename:
        write_ply(plyfilename, vertices, colours)
    return vertices, colours
