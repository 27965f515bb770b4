"""Depth-map filter / fusion on the GPU: the counterpart of the reference's `filter_depth`
(eval.py:590-800) and its helpers `reproject_with_depth` / `check_geometric_consistency`
(eval.py:508-585), `depth2pts_np` (eval.py:253-265), `save_mask` (eval.py:141-144)
(SURVEY.md §8 f3).

All reference views of a scan go through ONE launch of `mvs_filter_depth`; the numpy / cv2.remap
loops of the reference are not reproduced on the host.  In `filter_depth`, which works from the depth stage's files,
file I/O and the boolean selection of the fused points (eval.py:753-759) stay on the host.  `fuse_views` does that
selection on the device (mvs_fuse_points), and `reconstruct_scan` is the whole chain -- images of a scan in, its
coloured point cloud out -- without a file in between.  `downsample_cloud` is eval.py's last step for the bin-picking
datasets (eval.py:831-840: crop to the bin's outer box `bin_box`, voxel_down_sample, scale), on the device
(mvs_cloud_downsample); `reconstruct_scan(..., downsample=...)` appends it to the chain.  `estimate_normals` is
eval.py:817's pcd.estimate_normals() on the device (mvs_cloud_normals, include/mvs_normals_abi.h); the reference runs it
before the crop and the voxel filter, which carry the normals along, and so does `downsample=dict(normals=...)`.
`remove_outliers` is eval.py:495's pcd.remove_statistical_outlier() on the device (mvs_cloud_outliers,
include/mvs_outliers_abi.h), between the crop and the voxel filter: `downsample=dict(outliers=...)`, off by default.
`cloud_distance` and `evaluate_cloud` score a cloud against a ground-truth cloud on the device (mvs_cloud_distance,
include/mvs_distance_abi.h): accuracy, completeness, their mean, precision / recall / F-score.  The reference leaves this
to DTU's MATLAB code; `read_ply` reads the clouds back.
`cluster_cloud` labels the density-connected components of a cloud (DBSCAN with scikit-learn's and Open3D's labels) and
marks the clusters above a size, on the device (mvs_cloud_cluster, include/mvs_cluster_abi.h): the step the reference
leaves to the user of the cloud, and the remedy for small dense blobs of wrong depth; `downsample=dict(clusters=...)`,
off by default.
`segment_planes` takes the supporting planes out of a cloud by RANSAC, round after round (Open3D's segment_plane applied
repeatedly), on the device (mvs_cloud_planes, include/ext/mvs_planes_abi.h): on a bin scan the floor and the walls tie
every part into one cluster, so it runs before `cluster_cloud`; `downsample=dict(planes=...)`, off by default.

Differences from the reference, flagged rather than hidden:
  * cv2.remap is restated inside the kernel (1/32-pixel quantised bilinear, zero border); OpenCV is
    not importable here, so that one call is pinned only by the oracle's hand-computed cases.  The rest
    of the chain is pinned to the reference's own functions (tests/golden/fx_filter.npz).
  * the reference's PLY block (eval.py:789-800) raises AttributeError as written
    (`vertices_colors.dtype` on a list); `write_ply` emits what that block is evidently meant to
    produce through plyfile: binary little-endian vertices x,y,z (float) + red,green,blue (uchar).
  * normals (INTEGRATION.md has the list): the sign is specified -- towards the point's own camera -- where Open3D
    leaves it to its eigen-solver; only points inside a box are served, and the points whose neighbourhood a point
    outside the box could have changed are counted; the PLY's nx, ny, nz are float32 where Open3D writes doubles;
    the covariance is centred.  Open3D is not installed here: nothing was compared against it.
  * outliers: the reference drops the result of remove_statistical_outlier, so its cloud is unfiltered; here the step,
    when asked for, filters.  Ties, the order of every sum and the cases of fewer than two valid points are specified
    (INTEGRATION.md §6.4).
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


def write_ply(filename: str, xyz: np.ndarray, rgb: np.ndarray, normals: np.ndarray | None = None) -> None:
    """Binary little-endian vertices x, y, z (float), then nx, ny, nz (float) when `normals` [P,3] is given -- Open3D's
    property order --, then red, green, blue (uchar).  Without normals the file is what it always was."""
    nfields = [] if normals is None else [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    rec = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + nfields +
                   [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        if len(normals) != len(xyz):
            raise ValueError(f"write_ply: {len(normals)} normals for {len(xyz)} points")
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
              "property float y\nproperty float z\n%sproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nend_header\n" % (len(rec), "".join(f"property float {n}\n" for n, _ in nfields)))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(filename: str):
    """The counterpart of write_ply: (xyz [P,3] of the file's coordinate type, rgb uint8 [P,3] or None, normals [P,3] of
    their type or None) from a PLY in format binary_little_endian or ascii whose first element is `vertex` with scalar
    properties, x, y, z among them; red, green, blue (uchar) and nx, ny, nz are read when all three are there, every other
    property and every later element (faces) is ignored.  Anything else -- another format, a list property of the
    vertices, a short file -- raises ValueError.  read_ply(write_ply(...)) returns the arrays bit for bit."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    stop = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or stop < 0:
        raise ValueError(f"read_ply: {filename} has no PLY header")
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()]
    lines = [ln for ln in lines[1:] if ln and ln[0] not in ("comment", "obj_info")]
    if not lines or lines[0][0] != "format" or len(lines[0]) < 2 or lines[0][1] not in ("binary_little_endian", "ascii"):
        raise ValueError(f"read_ply: {filename}: format {' '.join(lines[0][1:2]) if lines else '?'!r} "
                         "(binary_little_endian or ascii)")
    binary = lines[0][1] == "binary_little_endian"
    if len(lines) < 2 or lines[1][:2] != ["element", "vertex"] or len(lines[1]) != 3 or not lines[1][2].isdigit():
        raise ValueError(f"read_ply: {filename}: the first element must be `element vertex <count>`")
    count = int(lines[1][2])
    fields = []
    for ln in lines[2:]:
        if ln[0] == "element":
            break
        if ln[0] != "property" or len(ln) != 3 or ln[1] not in _PLY_TYPES:
            raise ValueError(f"read_ply: {filename}: vertex property {' '.join(ln)!r} (scalar properties only)")
        if ln[2] in (n for n, _ in fields):
            raise ValueError(f"read_ply: {filename}: vertex property {ln[2]!r} is declared twice")
        fields.append((ln[2], "<" + _PLY_TYPES[ln[1]]))
    kinds = dict(fields)
    if not all(a in kinds for a in "xyz") or len({kinds[a] for a in "xyz"}) != 1 or kinds["x"][1] != "f":
        raise ValueError(f"read_ply: {filename}: the vertices need x, y, z of one floating-point type")
    body = data[stop + 1:]
    if binary:
        dtype = np.dtype(fields)
        if len(body) < count * dtype.itemsize:
            raise ValueError(f"read_ply: {filename}: {len(body)} bytes after the header, {count} vertices need "
                             f"{count * dtype.itemsize}")
        rec = np.frombuffer(body, dtype=dtype, count=count)
        column = {n: rec[n] for n in kinds}
    else:
        rows = [ln.split() for ln in body.decode("ascii", "replace").splitlines()[:count]]
        if len(rows) < count or any(len(r) != len(fields) for r in rows):
            raise ValueError(f"read_ply: {filename}: {count} vertex lines of {len(fields)} values each expected")
        column = {n: np.array([r[k] for r in rows], dtype=np.float64 if t[1] == "f" else np.int64).astype(t[1:])
                  for k, (n, t) in enumerate(fields)}

    def triple(names, what):
        if not any(n in kinds for n in names):
            return None
        if not all(n in kinds for n in names) or len({kinds[n] for n in names}) != 1:
            raise ValueError(f"read_ply: {filename}: {what} need {', '.join(names)} of one type")
        return np.stack([column[n] for n in names], axis=1)
    rgb = triple(("red", "green", "blue"), "colours")
    if rgb is not None and rgb.dtype != np.uint8:
        raise ValueError(f"read_ply: {filename}: red, green, blue must be uchar")
    normals = triple(("nx", "ny", "nz"), "normals")
    if normals is not None and normals.dtype.kind != "f":
        raise ValueError(f"read_ply: {filename}: nx, ny, nz must be floating-point")
    return triple(("x", "y", "z"), "points"), rgb, normals


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


_DECODE_THREADS = 16     # reconstruct_scan's image decoders (the eval driver's default)


def fuse_views(filtered, images, pairs_or_ref_idx, capacity=None):
    """The fused, coloured points of every reference view (eval.py:745-758) from what `filter_views` returned.

    filtered: the dict of filter_views (masks [R,3,h,w], xyz_world [R,h*w,3], on the GPU).  images: uint8 [V,H,W,3] or
    [V,3,H,W] (numpy or torch, host or device), index = view id; float32 [V,3,H,W] in [0,1] is converted on the
    device with (img*255).to(uint8), the depth stage's np.uint8(img*255) (eval.py:346-350).  pairs_or_ref_idx: the
    pair list handed to filter_views, or the image index of each reference view.  Returns (xyz float32 [P,3],
    rgb uint8 [P,3]) on the device, in the reference's order, and the per-view counts (numpy int32 [R]).  Reading the
    counts is the one host synchronisation.  capacity (default R*h*w, always enough) bounds the device buffers."""
    masks, xyz_world = filtered["masks"], filtered["xyz_world"]
    dev = xyz_world.device
    R, _, h, w = masks.shape
    images = torch.as_tensor(images) if not torch.is_tensor(images) else images
    if images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"fuse_views: images must be uint8 [V,H,W,3] / [V,3,H,W] or float32 [V,3,H,W], got "
                           f"{images.dtype} {tuple(images.shape)}")
    images = images.to(dev)
    if images.dtype == torch.float32:
        if images.shape[1] != 3:
            raise RuntimeError(f"fuse_views: float32 images must be [V,3,H,W], got {tuple(images.shape)}")
        images = (images * 255).to(torch.uint8)
    hwc = images.shape[1] != 3 and images.shape[3] == 3
    H, W = (images.shape[1], images.shape[2]) if hwc else (images.shape[2], images.shape[3])
    if (H, W) != (4 * h, 4 * w):
        raise RuntimeError(f"images are {H}x{W}, depth maps {h}x{w}: incompatible depth and image dimensions.")
    ref = [p[0] if isinstance(p, (tuple, list)) else p for p in
           (pairs_or_ref_idx.tolist() if torch.is_tensor(pairs_or_ref_idx) else list(pairs_or_ref_idx))]
    if len(ref) != R:
        raise RuntimeError(f"fuse_views: {len(ref)} reference views named, the filter produced {R}")
    ref_idx = torch.tensor([int(r) for r in ref], dtype=torch.int32).to(dev)
    xyz, rgb, counts = _lib.fuse_points(xyz_world, masks, images, ref_idx, capacity=capacity)
    counts = counts.cpu().numpy()
    total = int(counts[-1])
    if total > xyz.shape[0]:
        raise RuntimeError(f"fuse_views: the scan has {total} fused points, capacity is {xyz.shape[0]}")
    return xyz[:total], rgb[:total], counts[:-1]


def bin_box(dims=(0.57, 0.37, 0.22), delta=(0, 0, 0), wall=20.0, scale=1.0):
    """The outer box of the bin, the reference's bbox2 (get_o3d_frame_bbox, eval.py:188-213), as (min, max) in mm.

    dims: the bin's inner size in metres, delta: its offset in metres (both times 1000 * scale), wall: the wall
    thickness in mm (not scaled, as in the reference).  The bin is centred on the origin in x and y and stands on z = 0;
    the walls are added on every side but the open top.  The default is (-305, -205, -20), (305, 205, 220);
    delta=(0.08, 0.03, 0) is the reference's "overhead02" / "overhead03" setting."""
    size = np.asarray(dims, np.float64) * 1000 * scale
    shift = np.asarray(delta, np.float64) * 1000 * scale
    if size.shape != (3,) or shift.shape != (3,):
        raise ValueError(f"bin_box: dims and delta must hold 3 numbers each, got {dims!r} and {delta!r}")
    lo = np.array([-size[0] / 2, -size[1] / 2, 0.0]) + shift - wall
    hi = np.array([size[0] / 2, size[1] / 2, size[2]]) + shift + np.array([wall, wall, 0.0])
    return lo, hi


def estimate_normals(xyz, knn=30, box=None, cell=5.0, view_counts=None, centres=None, return_neighbours=False):
    """eval.py:817's pcd.estimate_normals() on the device (mvs_cloud_normals): a unit normal for every point of xyz
    (float32 or float64 [P,3], on the GPU) inside `box` = (min, max) from its `knn` nearest neighbours inside the box;
    points outside get (0, 0, 0).  box defaults to the bounding box of the finite points, which costs the one host
    synchronisation of this function (its six numbers travel in the kernel arguments); with a box given nothing
    synchronises.  cell: the search grid's cell edge, in the cloud's units -- it changes the time, never the result.
    view_counts (the per-view counts `fuse_views` returns, any integer sequence) and centres (float [R,3], the camera
    centres) turn each normal towards the camera of its point; the prefix of the counts is built on the device.  Without
    them the sign makes the normal's largest component positive.
    Returns (normals float32 [P,3], counts int64 [3]) on the device -- counts: points inside the box, those with an
    estimated normal, those whose knn-th neighbour is farther than the nearest face of the box (a point outside could
    have been nearer: grow the box until this is 0 for the whole cloud's answer) -- and, with return_neighbours, the
    neighbour indices int32 [P,knn] (ascending distance, then index; -1 pads) as a third item."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("estimate_normals: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    dev = xyz.device
    lo, hi = _finite_box(xyz) if box is None else box
    starts = ctr = None
    if (view_counts is None) != (centres is None):
        raise RuntimeError("estimate_normals: view_counts and centres must both be given or both be None")
    if view_counts is not None:
        counts = torch.as_tensor(np.asarray(view_counts.cpu() if torch.is_tensor(view_counts) else view_counts, np.int64))
        ctr = torch.as_tensor(np.asarray(centres.cpu() if torch.is_tensor(centres) else centres, np.float64))
        if counts.dim() != 1 or counts.shape[0] < 1 or tuple(ctr.shape) != (counts.shape[0], 3):
            raise RuntimeError(f"estimate_normals: view_counts must be [R], R >= 1, and centres [R,3]; got "
                               f"{tuple(counts.shape)} and {tuple(ctr.shape)}")
        with torch.cuda.device(dev):
            starts = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=dev)
            starts[1:] = torch.cumsum(counts.to(dev, non_blocking=True), 0)
            ctr = ctr.to(dev, non_blocking=True)
    normals, nbr, n = _lib.cloud_normals(xyz, lo, hi, cell=cell, knn=knn, view_starts=starts, centres=ctr,
                                         neighbours=return_neighbours)
    return (normals, n, nbr) if return_neighbours else (normals, n)


def remove_outliers(xyz, nb_neighbors=20, std_ratio=2.0, box=None, cell=5.0, masked=False):
    """eval.py:495's pcd.remove_statistical_outlier() on the device (mvs_cloud_outliers), among the points of xyz (float32
    or float64 [P,3], on the GPU) inside `box` = (min, max), default bin_box(): the reference crops first.  A point is kept
    iff it lies inside the box, its mean distance to its `nb_neighbors` nearest points there (itself among them) is positive,
    and that distance is below mean + std_ratio * std of those distances over the box.  cell: the search grid's cell edge,
    in the cloud's units -- it changes the time, never the result.
    Returns (keep bool [P], dist float64 [P]: the mean distances, -1 outside the box, counts int64 [3]: points inside the
    box, those with a positive distance, those kept, stats float64 [3]: mean, std, threshold), all on the device; nothing
    synchronises.  With masked=True a fifth item follows: xyz_masked, xyz with NaN in the rows that are not kept, which
    `downsample_cloud` and `estimate_normals` take in place of xyz (NaN points fall out of both) with colours and normals
    as they are; `xyz[keep]` is the compacted cloud."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("remove_outliers: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    lo, hi = bin_box() if box is None else box
    dist, keep, xyz_masked, counts, stats = _lib.cloud_outliers(xyz, lo, hi, cell=cell, nb_neighbors=nb_neighbors,
                                                                std_ratio=std_ratio, masked=masked)
    return (keep, dist, counts, stats, xyz_masked) if masked else (keep, dist, counts, stats)


DISTANCE_CELL_BUDGET = 1 << 24      # the most cells `cell=None` lets the search grid of cloud_distance have (64 MiB of counters)


def _finite_box(xyz):
    """The bounding box of the finite points, as host numbers: one synchronisation (estimate_normals' default)."""
    finite = xyz[torch.isfinite(xyz).all(dim=1)]
    if finite.shape[0] == 0:
        return (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    both = torch.stack([finite.min(dim=0).values, finite.max(dim=0).values]).double().cpu()      # the one sync
    return both[0].tolist(), both[1].tolist()


def distance_cell(box, P):
    """The cell edge cloud_distance picks for a box and P reference points: the edge at which the box holds about one
    cell per two points -- over the axes along which the box has an extent; 1.0 if it has none -- grown by a quarter at a
    time until the grid has at most DISTANCE_CELL_BUDGET cells.  Host arithmetic on host numbers."""
    ext = [float(h) - float(l) for l, h in zip(*box)]
    pos = [e for e in ext if e > 0.0]
    if not pos or not all(np.isfinite(pos)):
        return 1.0
    target = min(max(int(P) // 2, 1), DISTANCE_CELL_BUDGET // 4)
    cell = float(np.prod(pos) / target) ** (1.0 / len(pos))
    cell = max(cell, max(pos) * 2.0 ** -20)             # a sliver of a box: never more than 2^20 cells along an axis
    while np.prod([np.floor(e / cell) + 1.0 for e in ext]) > DISTANCE_CELL_BUDGET:
        cell *= 1.25
    return cell


def cloud_distance(query, ref, max_dist=float("inf"), thresholds=(), box=None, cell=None, return_indices=False):
    """For every point of `query` the distance to the nearest point of `ref` (both float32 or float64 [.,3] on the GPU,
    possibly the same tensor), on the device (mvs_cloud_distance, include/mvs_distance_abi.h): one direction of accuracy /
    completeness.  Only the points of `ref` inside `box` = (min, max) are searched; box defaults to the bounding box of
    ref's finite points, which costs the one host synchronisation of this function (with a box given nothing
    synchronises).  A query may lie anywhere.  cell: the search grid's cell edge, default distance_cell(box, P) -- it
    changes the time, never the result.
    Returns (dist float64 [N]: the distance; +inf where no point of ref in the box lies within max_dist; -1 for a query
    with a non-finite coordinate, counts int64 [2 + T]: the queries with finite coordinates, those within max_dist, those
    strictly below each of `thresholds` (at most 8), stats float64 [2]: the sum of the distances within max_dist, in a
    fixed order, and their mean), all on the device, and with return_indices a fourth item: idx int32 [N], the row of the
    nearest point in ref, the smallest on a tie, -1 where there is none."""
    for name, t in (("query", query), ("ref", ref)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"cloud_distance: {name} must be a CUDA(ROCm) tensor; there is no CPU implementation")
    lo, hi = _finite_box(ref) if box is None else box
    if cell is None:
        cell = distance_cell((lo, hi), ref.shape[0])
    dist, idx, counts, stats = _lib.cloud_distance(ref, query, lo, hi, cell, max_dist, thresholds, indices=return_indices)
    return (dist, counts, stats, idx) if return_indices else (dist, counts, stats)


def register_cloud(source, target, max_dist, target_normals=None, init=None, max_iterations=30, rel_fitness=1e-6,
                   rel_rmse=1e-6, box=None, cell=None):
    """The rigid transform that lays `source` onto `target` (both float32 or float64 [.,3] on the GPU) by iterative
    closest point on the device (mvs_cloud_register, include/ext/mvs_register_abi.h), with the semantics of Open3D's
    registration_icp: every iteration pairs each transformed source point with its nearest target point within max_dist
    and takes the rigid motion that brings the pairs closest -- point-to-plane with target_normals ([P,3], e.g.
    estimate_normals(target)[0]; their sign does not matter), point-to-point without.  It stops when fitness and rmse both
    change by less than rel_fitness and rel_rmse, after max_iterations, or when too few pairs are left.  A source row
    with a NaN is left out: a cluster is registered by passing the cloud with every other row set to NaN.  init: 4 x 4
    host numbers, default identity.  box = (min, max) limits the target points that are searched; it defaults to the
    bounding box of target's finite points grown by max_dist (one host synchronisation; with a box given nothing
    synchronises).  cell as in cloud_distance.
    Returns a dict of device tensors: transformation float64 [4,4] (apply it with transform_cloud), fitness (inliers /
    counted sources) and inlier_rmse float64 scalars, iterations and stop int64 scalars (stop: 1 converged,
    2 max_iterations, 3 degenerate; _lib.REGISTER_STOPS), history float64 [max_iterations + 1, 19]: the transform (16),
    fitness, rmse and inlier count of every evaluation, NaN after the last."""
    for name, t in (("source", source), ("target", target)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"register_cloud: {name} must be a CUDA(ROCm) tensor; there is no CPU implementation")
    if box is None:
        lo, hi = _finite_box(target)
        grow = float(max_dist) if np.isfinite(max_dist) and max_dist > 0 else 0.0
        lo, hi = [v - grow for v in lo], [v + grow for v in hi]
    else:
        lo, hi = box
    if cell is None:
        cell = distance_cell((lo, hi), target.shape[0])
    if target_normals is not None and isinstance(target_normals, torch.Tensor) and target_normals.dtype != target.dtype:
        target_normals = target_normals.to(target.dtype)
    T, counts, stats, history, _, _ = _lib.cloud_register(target, source, lo, hi, cell, max_dist, target_normals=target_normals,
                                                          init=init, max_iterations=max_iterations, rel_fitness=rel_fitness,
                                                          rel_rmse=rel_rmse, history=True)
    return dict(transformation=T, fitness=stats[0], inlier_rmse=stats[1], iterations=counts[2], stop=counts[3], history=history)


def transform_cloud(xyz, T):
    """R x + t for every row x of xyz ([P,3], any float dtype, any device) under the 4 x 4 transform T (a tensor or host
    numbers), computed in float64 and returned in xyz's dtype.  Plain torch."""
    T = torch.as_tensor(T, dtype=torch.float64).to(xyz.device).reshape(4, 4)
    return (xyz.double() @ T[:3, :3].T + T[:3, 3]).to(xyz.dtype)


def reduce_cell(box, P, min_dist):
    """The cell edge reduce_cloud picks: min_dist, so that a member's candidates are the 27 cells around it, but never
    below distance_cell(box, P), which keeps the grid inside DISTANCE_CELL_BUDGET however small min_dist is against the
    scene.  Host arithmetic on host numbers."""
    return max(float(min_dist), distance_cell(box, P))


def reduce_cloud(xyz, min_dist=0.2, seed=0, box=None, cell=None, max_rounds=64, masked=False):
    """DTU's point reduction (reducePts) on the device (mvs_cloud_reduce, include/mvs_reduce_abi.h): among the points of
    xyz (float32 or float64 [P,3], on the GPU) inside `box` = (min, max), visit the points in the order of a hash of
    (seed, index) and keep a point iff no point kept before it lies within min_dist, the bound included.  It is MATLAB's
    greedy pass with randperm replaced by the hash: the same distribution, not the same points as any MATLAB run.  box
    defaults to the bounding box of the finite points (one host synchronisation); cell, the search grid's cell edge,
    to reduce_cell(box, P, min_dist) -- it changes the time, never a byte.
    Returns (keep bool [P], counts int64 [4]: points inside the box, kept, undecided, rounds) on the device.  The counts
    are read once: if a point is still undecided after max_rounds (at most 256) rounds this raises, with the count in the
    message, and the caller raises max_rounds; about ten rounds serve a scan.  With masked=True a third item follows:
    xyz with NaN in the rows that are not kept, as `remove_outliers` gives it, so the cloud goes on without compaction."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("reduce_cloud: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    lo, hi = _finite_box(xyz) if box is None else box
    if cell is None:
        cell = reduce_cell((lo, hi), xyz.shape[0], min_dist)
    keep, counts = _lib.cloud_reduce(xyz, lo, hi, cell, min_dist, seed=seed, max_rounds=max_rounds)
    undecided = int(counts.cpu()[2])
    if undecided:
        raise RuntimeError(f"reduce_cloud: {undecided} points are still undecided after max_rounds = {max_rounds} rounds; "
                           "raise max_rounds (at most 256)")
    if not masked:
        return keep, counts
    return keep, counts, torch.where(keep[:, None], xyz, torch.full_like(xyz, float("nan")))


def cluster_cloud(xyz, eps, min_points=10, min_size=1, box=None, cell=None, masked=False):
    """DBSCAN on the device (mvs_cloud_cluster, include/mvs_cluster_abi.h): the density-connected components of the points
    of xyz (float32 or float64 [P,3], on the GPU) inside `box` = (min, max), with the labels scikit-learn's DBSCAN and
    Open3D's cluster_dbscan give: two points are neighbours within eps, the bound included; a core point has at least
    min_points neighbours, itself counted; clusters are numbered in the order of their first core point; a border point
    takes the smallest number among its core neighbours; -1 is noise, -2 a point outside the box.  keep marks the points
    of the clusters of at least min_size points (core and border counted): min_size drops the small dense blobs that
    `remove_outliers` cannot see.  box defaults to the bounding box of the finite points (one host synchronisation; with
    a box given nothing synchronises); cell, the search grid's cell edge, to max(eps, distance_cell(box, P)) -- it changes
    the time, never a byte.
    Returns (labels int32 [P], keep bool [P], counts int64 [7]: points inside the box, core, border, noise, clusters,
    kept points, size of the largest cluster) on the device.  With masked=True a fourth item follows: xyz with NaN in the
    rows that are not kept, as `remove_outliers` gives it, so the cloud goes on without compaction."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("cluster_cloud: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    lo, hi = _finite_box(xyz) if box is None else box
    if cell is None:
        cell = max(float(eps), distance_cell((lo, hi), xyz.shape[0]))
    labels, keep, counts = _lib.cloud_cluster(xyz, lo, hi, cell, eps, min_points=min_points, min_size=min_size)
    if not masked:
        return labels, keep, counts
    return labels, keep, counts, torch.where(keep[:, None], xyz, torch.full_like(xyz, float("nan")))


PLANES_DEFAULTS = dict(max_planes=1, num_candidates=1000, min_inliers=3, seed=0, remove=True)


def planes_options(opt):
    """The options of reconstruct_scan's plane stage, downsample['planes'], with their defaults: dict(dist, max_planes=1,
    num_candidates=1000, min_inliers=None -> 3, seed=0, remove=True); None stays None.  dist has no default."""
    if opt is None:
        return None
    opt = dict(opt)
    unknown = set(opt) - {"dist"} - set(PLANES_DEFAULTS)
    if unknown:
        raise ValueError(f"downsample['planes']: unknown keys {sorted(unknown)} (dist, max_planes, num_candidates, "
                         "min_inliers, seed, remove)")
    if "dist" not in opt:
        raise ValueError("downsample['planes'] needs dist, how far from a plane its points may lie, in the cloud's units")
    out = dict(PLANES_DEFAULTS, **opt)
    if out["min_inliers"] is None:
        out["min_inliers"] = 3
    return dict(dist=float(out["dist"]), max_planes=int(out["max_planes"]), num_candidates=int(out["num_candidates"]),
                min_inliers=int(out["min_inliers"]), seed=int(out["seed"]), remove=bool(out["remove"]))


def segment_planes(xyz, dist, max_planes=1, num_candidates=1000, min_inliers=None, seed=0, box=None, toward=None, masked=False):
    """The supporting planes of a cloud by RANSAC on the device (mvs_cloud_planes, include/ext/mvs_planes_abi.h): what
    Open3D's segment_plane gives when it is applied again and again to the rest.  Among the points of xyz (float32 or
    float64 [P,3], on the GPU) inside `box` = (min, max), every round draws num_candidates planes through three of the
    points that have no plane yet (by a hash of seed, round and candidate), takes the one with the most points within
    `dist`, refits it to those by least squares and gives the points within `dist` of the refitted plane its number.  It
    stops after max_planes rounds, when the best candidate has fewer than min_inliers points (default 3), or when fewer
    than three points are left.  toward: 3 host numbers, the side every normal is turned to (a camera, the bin's inside);
    without it the largest component of a normal is positive.  box defaults to the bounding box of the finite points (one
    host synchronisation; with a box given nothing synchronises).
    Returns (planes float64 [max_planes,4]: (n, d) of n . x + d = 0 with |n| = 1, NaN for rounds that gave none, labels
    int32 [P]: the plane's number, -1 on no plane, -2 outside the box, counts int64 [4]: points inside the box, planes
    found, points on planes, stop reason (1 max_planes, 2 no_plane, 3 exhausted; _lib.PLANES_STOPS), rounds int64
    [max_planes,4]: active points, winning candidate, its count, final inliers) on the device.  A plane is the P of
    select_cloud and evaluate_cloud(plane=).  With masked=True a fifth item follows: xyz with NaN in the rows that lie on
    a plane, ready for cluster_cloud and register_cloud."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("segment_planes: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    lo, hi = _finite_box(xyz) if box is None else box
    planes, rounds, counts, labels, _, _ = _lib.cloud_planes(xyz, lo, hi, dist, num_candidates=num_candidates,
                                                             max_planes=max_planes, min_inliers=3 if min_inliers is None else min_inliers,
                                                             seed=seed, toward=toward)
    if not masked:
        return planes, labels, counts, rounds
    return planes, labels, counts, rounds, torch.where((labels >= 0)[:, None], torch.full_like(xyz, float("nan")), xyz)


def select_cloud(xyz, obs_mask=None, plane=None):
    """DTU's observability mask and ground-plane filter on the device (mvs_cloud_select, include/mvs_reduce_abi.h).
    obs_mask = dict(mask=uint8 or bool [n0,n1,n2] (a tensor on xyz's device, or a numpy array), origin=(3,), res=float),
    e.g. read_obs_mask's: a point is observed iff the voxel round((p - origin) / res), halves away from zero, lies in the
    array and is set.  plane: 4 numbers, e.g. read_plane's: a point is above iff P . (x, y, z, 1) > 0.  Returns (keep bool
    [P]: every test that was asked for holds; False for a non-finite point, counts int64 [3]: finite points, observed
    ones, kept ones) on the device; nothing synchronises."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("select_cloud: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    mask = origin = None
    res = 1.0
    if obs_mask is not None:
        unknown = set(obs_mask) - {"mask", "origin", "res"}
        if unknown or not {"mask", "origin", "res"} <= set(obs_mask):
            raise ValueError(f"select_cloud: obs_mask must hold mask, origin and res, got {sorted(obs_mask)}")
        mask, res = obs_mask["mask"], float(obs_mask["res"])
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        mask = mask.to(xyz.device)
        origin = [float(v) for v in np.asarray(obs_mask["origin"], np.float64).reshape(-1)]
    if plane is not None:
        plane = [float(v) for v in np.asarray(plane, np.float64).reshape(-1)]
    return _lib.cloud_select(xyz, mask=mask, origin=origin, res=res, plane=plane)


def _read_arrays(path, names, who):
    """The named arrays of an .npz or a MATLAB .mat file."""
    if str(path).endswith(".npz"):
        with np.load(path) as f:
            missing = [k for k in names if k not in f.files]
            if missing:
                raise ValueError(f"{who}: {path} holds {sorted(f.files)}, not {missing}")
            return [np.asarray(f[k]) for k in names]
    if str(path).endswith(".mat"):
        try:
            from scipy.io import loadmat
        except ImportError as e:
            raise RuntimeError(f"{who}: reading {path} needs scipy (scipy.io.loadmat), which is not installed; "
                               "convert the file to .npz") from e
        f = loadmat(path)
        missing = [k for k in names if k not in f]
        if missing:
            raise ValueError(f"{who}: {path} holds {sorted(k for k in f if not k.startswith('__'))}, not {missing}")
        return [np.asarray(f[k]) for k in names]
    raise ValueError(f"{who}: {path} is neither .npz nor .mat")


def read_obs_mask(path):
    """DTU's ObsMask/ObsMaskN_10.mat, or an .npz with the same arrays ObsMask [n0,n1,n2], BB [2,3] and Res ->
    dict(mask=uint8 [n0,n1,n2], C-contiguous in that index order, origin=float64 (3,) = BB[0], res=float), what
    select_cloud and evaluate_cloud take.  A .mat file is read with scipy.io.loadmat."""
    mask, bb, res = _read_arrays(path, ("ObsMask", "BB", "Res"), "read_obs_mask")
    bb = np.asarray(bb, np.float64)
    if mask.ndim != 3 or bb.shape != (2, 3) or np.size(res) != 1:
        raise ValueError(f"read_obs_mask: {path}: ObsMask {mask.shape}, BB {bb.shape}, Res {np.shape(res)} "
                         "(need [n0,n1,n2], [2,3] and one number)")
    return dict(mask=np.ascontiguousarray(mask != 0).view(np.uint8), origin=bb[0].copy(), res=float(np.reshape(res, -1)[0]))


def read_plane(path):
    """DTU's ObsMask/PlaneN.mat, or an .npz with the same array P -> float64 (4,): the ground plane of select_cloud."""
    (plane,) = _read_arrays(path, ("P",), "read_plane")
    plane = np.asarray(plane, np.float64).reshape(-1)
    if plane.shape != (4,):
        raise ValueError(f"read_plane: {path}: P has {plane.size} numbers (need 4)")
    return plane


def evaluate_cloud(pred_xyz, gt_xyz, max_dist=20.0, thresholds=(1.0, 2.0, 5.0), box=None, cell=None, reduce=None,
                   obs_mask=None, plane=None, register=None):
    """The measure a reconstruction is judged by, both directions of `cloud_distance` on the device:
        accuracy      from every point of pred_xyz to the nearest point of gt_xyz
        completeness  from every point of gt_xyz to the nearest point of pred_xyz
    each as dict(mean, median, n, n_within, below): `n` points with finite coordinates, `n_within` of them with a
    neighbour within max_dist, mean and median (the lower one, the ((n_within + 1) // 2)-th smallest; NaN for none) over
    those, `below[t]` of them strictly nearer than thresholds[t]; and
        overall       (accuracy.mean + completeness.mean) / 2
        precision[t]  accuracy.below[t] / accuracy.n            recall[t]  completeness.below[t] / completeness.n
        fscore[t]     2 p r / (p + r), 0 when p + r == 0
    with max_dist and thresholds repeated, all plain Python numbers after one device-to-host copy.  A point farther than
    max_dist from the other cloud counts in n, in no mean and below no threshold.  `box` = (min, max) limits the points
    that are SEARCHED in either direction (default: each cloud's own bounding box, one host synchronisation per
    direction); the points that are scored are always all of the other cloud.  cell as in cloud_distance.

    With reduce, obs_mask and plane all None that is the whole of it: the definition of the distances, with clouds of
    different density or extent scored as they are.  The three options are the steps of DTU's evaluation, in its order:
        reduce    dict(min_dist=0.2, seed=0, gt=False, max_rounds=64): the reconstruction goes through `reduce_cloud`
                  first, with gt=True the ground truth too
        obs_mask  read_obs_mask's dict: accuracy is measured from the reduced reconstruction's OBSERVED points to the
                  whole ground truth
        plane     read_plane's four numbers: completeness is measured from the ground-truth points ABOVE the plane to the
                  whole reduced reconstruction (the observability mask does not thin the cloud that is searched)
    A filtered-out point is a NaN row of the query, which cloud_distance leaves uncounted.  The dict then gains
    `reduction`: the four counts of reduce_cloud per reduced cloud ("pred", "gt"), and `selection`: the three counts of
    select_cloud per direction ("accuracy", "completeness").
    What this still is not: DTU's tables.  MATLAB's randperm is replaced by a stated hash, so the kept points differ from
    those of any MATLAB run while their distribution is the same; nothing was compared against the MATLAB code or real
    DTU files; the per-scan tables are not built.

    register = dict(max_dist=..., point_to_plane=True, knn=30, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
    init=None) first lays the reconstruction onto the ground truth with `register_cloud` (ICP), for clouds that do not
    share a frame exactly: a laser scan, a CAD model, another rig.  Point-to-plane takes the ground truth's normals from
    `estimate_normals` over `knn` neighbours.  Everything above is then measured on the moved reconstruction, and the dict
    gains `transformation` (4 x 4), `register_fitness` and `register_rmse`.  Without it nothing changes."""
    thresholds = [float(t) for t in thresholds]
    T = len(thresholds)
    registered = None
    if register is not None:
        opt = dict(dict(point_to_plane=True, knn=30, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, init=None), **register)
        unknown = set(opt) - {"max_dist", "point_to_plane", "knn", "max_iterations", "rel_fitness", "rel_rmse", "init"}
        if unknown or "max_dist" not in opt:
            raise ValueError(f"evaluate_cloud: register needs max_dist and takes point_to_plane, knn, max_iterations, "
                             f"rel_fitness, rel_rmse, init (unknown: {sorted(unknown)})")
        for name, t in (("pred_xyz", pred_xyz), ("gt_xyz", gt_xyz)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"evaluate_cloud: {name} must be a CUDA(ROCm) tensor; there is no CPU implementation")
        normals = estimate_normals(gt_xyz, knn=opt["knn"])[0] if opt["point_to_plane"] and gt_xyz.shape[0] else None
        registered = register_cloud(pred_xyz, gt_xyz, opt["max_dist"], target_normals=normals, init=opt["init"],
                                    max_iterations=opt["max_iterations"], rel_fitness=opt["rel_fitness"],
                                    rel_rmse=opt["rel_rmse"])
        pred_xyz = transform_cloud(pred_xyz, registered["transformation"])
    pairs =((pred_xyz, gt_xyz), (gt_xyz, pred_xyz))
    dtu = reduce is not None or obs_mask is not None or plane is not None
    if dtu:
        reduction, selected = {}, []
        if reduce is not None:
            opt = dict(dict(min_dist=0.2, seed=0, gt=False, max_rounds=64), **reduce)
            unknown = set(opt) - {"min_dist", "seed", "gt", "max_rounds"}
            if unknown:
                raise ValueError(f"evaluate_cloud: reduce: unknown keys {sorted(unknown)} (min_dist, seed, gt, max_rounds)")
            also_gt = opt.pop("gt")
            _, reduction["pred"], pred_xyz = reduce_cloud(pred_xyz, masked=True, **opt)
            if also_gt:
                _, reduction["gt"], gt_xyz = reduce_cloud(gt_xyz, masked=True, **opt)
        queries = []
        for xyz, tests in ((pred_xyz, dict(obs_mask=obs_mask)), (gt_xyz, dict(plane=plane))):
            keep, counts = select_cloud(xyz, **tests)
            selected.append(counts)
            queries.append(torch.where(keep[:, None], xyz, torch.full_like(xyz, float("nan"))))
        pairs = ((queries[0], gt_xyz), (queries[1], pred_xyz))
    parts = []
    for query, ref in pairs:
        dist, counts, stats = cloud_distance(query, ref, max_dist=max_dist, thresholds=thresholds, box=box, cell=cell)
        if dist.shape[0]:
            within = (dist >= 0) & torch.isfinite(dist)
            ordered = torch.sort(torch.where(within, dist, torch.full_like(dist, float("inf")))).values
            k = torch.clamp((counts[1] + 1) // 2 - 1, min=0)
            median = torch.where(counts[1] > 0, ordered[k], torch.full_like(stats[0], float("nan")))
        else:
            median = torch.full_like(stats[0], float("nan"))
        parts += [counts.double(), stats, median.reshape(1)]
    if dtu:
        parts += [c.double() for c in selected] + [c.double() for c in reduction.values()]
    if registered is not None:
        parts += [registered["transformation"].reshape(16), registered["fitness"].reshape(1), registered["inlier_rmse"].reshape(1)]
    host = torch.cat(parts).cpu().tolist()                # the one copy; every count is below 2^31, exact as a double
    out = {}
    for name, v in (("accuracy", host[:T + 5]), ("completeness", host[T + 5:])):
        out[name] = dict(mean=v[T + 3], median=v[T + 4], n=int(v[0]), n_within=int(v[1]), below=[int(b) for b in v[2:2 + T]])
    acc, comp = out["accuracy"], out["completeness"]
    out["overall"] = (acc["mean"] + comp["mean"]) / 2
    out["precision"] = [b / acc["n"] if acc["n"] else 0.0 for b in acc["below"]]
    out["recall"] = [b / comp["n"] if comp["n"] else 0.0 for b in comp["below"]]
    out["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    out["max_dist"], out["thresholds"] = float(max_dist), thresholds
    if dtu:
        tail = [int(v) for v in host[2 * (T + 5):2 * (T + 5) + 6 + 4 * len(reduction)]]
        out["selection"] = dict(accuracy=tail[0:3], completeness=tail[3:6])
        out["reduction"] = {name: tail[6 + 4 * k:10 + 4 * k] for k, name in enumerate(reduction)}
    if registered is not None:
        out["transformation"] = [host[-18 + 4 * r:-14 + 4 * r] for r in range(4)]
        out["register_fitness"], out["register_rmse"] = host[-2], host[-1]
    return out


def downsample_cloud(xyz, rgb, voxel_size=5.0, box=None, scale=0.01, capacity=None, normals=None):
    """eval.py:831-840 on the device: crop the cloud to `box` = (min, max) (default bin_box(), in the cloud's units), keep
    the mean point and colour of every occupied voxel of size `voxel_size`, scale the coordinates.  xyz float32 or
    float64 [P,3], rgb uint8 [P,3], on the GPU.  Returns (xyz float32 [Q,3], rgb uint8 [Q,3]) on the device, voxels in
    ascending (iz, iy, ix).  Reading the two counts is the one host synchronisation.  capacity (default P, always
    enough) bounds the device buffers.  With normals (float32 [P,3] on the GPU, e.g. estimate_normals') a third tensor
    follows: float32 [Q,3], the mean of each voxel's normals, not renormalised, as Open3D's voxel filter leaves them
    (mvs_cloud_downsample_normals); the first two are the same bytes either way."""
    lo, hi = bin_box() if box is None else box
    if normals is None:
        out_xyz, out_rgb, counts = _lib.cloud_downsample(xyz, rgb, lo, hi, voxel_size, scale=scale, capacity=capacity)
    else:
        out_xyz, out_rgb, out_normals, counts = _lib.cloud_downsample_normals(xyz, rgb, normals, lo, hi, voxel_size,
                                                                              scale=scale, capacity=capacity)
    voxels = int(counts.cpu()[1])
    if voxels > out_xyz.shape[0]:
        raise RuntimeError(f"downsample_cloud: the cloud occupies {voxels} voxels, capacity is {out_xyz.shape[0]}")
    if normals is None:
        return out_xyz[:voxels], out_rgb[:voxels]
    return out_xyz[:voxels], out_rgb[:voxels], out_normals[:voxels]


def _packed_to_host(xyz, rgb):
    """Device points and colours -> host (float32 [P,3], uint8 [P,3]) in one copy."""
    P = xyz.shape[0]
    packed = torch.cat([xyz.reshape(-1).view(torch.uint8), rgb.reshape(-1)]).cpu().numpy()
    return packed[:12 * P].view(np.float32).reshape(P, 3), packed[12 * P:].reshape(P, 3)


def reconstruct_scan(model, dataset, scan=None, n_view_filter=10, photomask=0.8, geomask=3, condmask_pixel=1.0,
                     condmask_depth=0.01, plyfilename=None, batch=1, device=None, downsample=None):
    """eval.py's save_depth + filter_depth for one scan of an EvalDataset, in memory: every image is decoded once (as
    uint8), FeatureNet runs once per image, every reference view's depth and confidence map is computed from that
    feature bank, and the maps are filtered and fused on the device.  No file is written except the optional PLY; the
    packed points are the one device-to-host copy.  The cameras of the filter are the ones each sample carries for its
    reference view (what the depth stage writes to cams/).  `batch` maps go through one forward_features call.
    Returns (vertices float32 [P,3], colours uint8 [P,3]); the PLY equals `filter_depth`'s byte for byte.
    downsample=dict(voxel_size=5.0, box=None, scale=0.01, plyfilename=None) also runs `downsample_cloud` on the fused
    cloud while it is on the device; the return is then (vertices, colours, ds_vertices float32 [Q,3], ds_colours uint8
    [Q,3]) and the downsampled cloud goes to its own plyfilename through write_ply.
    downsample=dict(..., normals=dict(knn=30, margin=20.0, cell=5.0)) estimates the normals of the fused cloud first
    (eval.py:817 runs before the crop, eval.py:832), inside the crop box grown by `margin` on every side, each turned
    towards the camera of its own reference view (centre -R^T t of the extrinsics the sample carries); the downsample
    carries them, the small PLY gets nx, ny, nz, and the return gains two items: ds_normals float32 [Q,3] and the three
    counts of estimate_normals as a numpy array -- the last is the number of points inside the grown box that a point
    outside it could have served better.  The default margin is a guess (the reach of 30 neighbours on a dense scan),
    not measured on a real bin scan: watch that count.
    downsample=dict(..., outliers=dict(nb_neighbors=20, std_ratio=2.0, cell=5.0)) runs `remove_outliers` among the points
    inside the crop box between the normals (of the whole fused cloud, if asked for) and the voxel downsample, eval.py's
    order (817, 494-496); the downsample takes the masked cloud and the normals as they are.  The return gains one last
    item: dict(counts int64 [3], stats float64 [3], keep bool [P]) as numpy arrays, keep over the fused cloud.
    downsample=dict(..., clusters=dict(eps=E, min_points=10, min_size=1, cell=None)) runs `cluster_cloud` among the points
    inside the crop box after the outlier stage (on its masked cloud, if asked for) and before the voxel downsample, which
    takes the cloud with the noise and the clusters below min_size masked out too.  eps is in the cloud's units and has no
    default.  The return gains one last item, after the outliers' when both are asked for: dict(counts int64 [7], keep
    bool [P], labels int32 [P]) as numpy arrays over the fused cloud.
    downsample=dict(..., planes=dict(dist=D, max_planes=1, num_candidates=1000, min_inliers=None, seed=0, remove=True))
    runs `segment_planes` among the points inside the crop box after the outlier stage (on its masked cloud) and before
    the cluster stage: the bin's floor and walls, which would otherwise tie every part into one cluster.  With remove=True
    the cluster stage and the voxel downsample take the cloud without the plane points; with remove=False the points are
    labelled only.  dist is in the cloud's units and has no default.  The return gains one item, after the outliers' and
    before the clusters': dict(planes float64 [max_planes,4], rounds int64 [max_planes,4], counts int64 [4], labels int32
    [P]) as numpy arrays, labels over the fused cloud."""
    import copy
    normals_opt = outliers_opt = clusters_opt = planes_opt = None
    if downsample is not None:
        downsample = dict(downsample)
        ds_ply = downsample.pop("plyfilename", None)
        normals_opt = downsample.pop("normals", None)
        outliers_opt = downsample.pop("outliers", None)
        clusters_opt = downsample.pop("clusters", None)
        planes_opt = planes_options(downsample.pop("planes", None))
        unknown = set(downsample) - {"voxel_size", "box", "scale"}
        if unknown:
            raise ValueError(f"downsample: unknown keys {sorted(unknown)} (voxel_size, box, scale, plyfilename, normals, "
                             "outliers, planes, clusters)")
        if normals_opt is not None:
            normals_opt = dict(dict(knn=30, margin=20.0, cell=5.0), **normals_opt)
            unknown = set(normals_opt) - {"knn", "margin", "cell"}
            if unknown:
                raise ValueError(f"downsample['normals']: unknown keys {sorted(unknown)} (knn, margin, cell)")
        if outliers_opt is not None:
            outliers_opt = dict(dict(nb_neighbors=20, std_ratio=2.0, cell=5.0), **outliers_opt)
            unknown = set(outliers_opt) - {"nb_neighbors", "std_ratio", "cell"}
            if unknown:
                raise ValueError(f"downsample['outliers']: unknown keys {sorted(unknown)} (nb_neighbors, std_ratio, cell)")
        if clusters_opt is not None:
            clusters_opt = dict(dict(min_points=10, min_size=1, cell=None), **clusters_opt)
            unknown = set(clusters_opt) - {"eps", "min_points", "min_size", "cell"}
            if unknown:
                raise ValueError(f"downsample['clusters']: unknown keys {sorted(unknown)} (eps, min_points, min_size, cell)")
            if "eps" not in clusters_opt:
                raise ValueError("downsample['clusters'] needs eps, the neighbourhood radius in the cloud's units")
    for a in ("view_plan", "decode_view", "assemble", "metas"):
        if not hasattr(dataset, a):
            raise ValueError("reconstruct_scan needs a dataset with metas, view_plan(), decode_view() and assemble(), "
                             "e.g. dataset_eval.EvalDataset")
    if not all(hasattr(model, a) for a in ("extract_features", "forward_features")):
        raise ValueError("reconstruct_scan needs a model with extract_features / forward_features (MVSNet)")
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    scans = list(dict.fromkeys(m[0] for m in dataset.metas))
    if scan is None:
        if len(scans) != 1:
            raise ValueError(f"the dataset holds {len(scans)} scans: name one of {scans}")
        scan = scans[0]
    indices = [i for i, m in enumerate(dataset.metas) if m[0] == scan]
    if not indices:
        raise ValueError(f"scan {scan!r} is not in the dataset ({scans})")
    if getattr(dataset, "image_dtype", "uint8") != "uint8":
        dataset = copy.copy(dataset)          # same files and caches; the pixels stay bytes
        dataset.image_dtype = "uint8"
    pairs = [(dataset.metas[i][1], list(dataset.metas[i][2])) for i in indices]
    refs = [r for r, _ in pairs]
    if len(set(refs)) != len(refs):
        raise ValueError(f"scan {scan!r} lists a reference view twice")
    missing = sorted({s for _, ss in pairs for s in ss[:n_view_filter]} - set(refs))
    if missing:
        raise ValueError(f"views {missing} are filter sources of scan {scan!r} but no reference view: they get no depth map")
    # every image once, on a few threads (PIL's decoding releases the GIL)
    plans, paths = [], {}
    for i in indices:
        _, views = dataset.view_plan(i)
        ids = ([dataset.metas[i][1]] + list(dataset.metas[i][2]))[:len(views)]
        plans.append((i, ids))
        for vid, (img_path, _) in zip(ids, views):
            paths.setdefault(vid, img_path)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(_DECODE_THREADS, len(paths))) as pool:
        decoded = dict(zip(paths, pool.map(dataset.decode_view, paths.values())))
    pixels = {v: d[0] for v, d in decoded.items()}
    adjust = {v: d[1] for v, d in decoded.items()}
    samples = [(ids, dataset.assemble(i, [adjust[v] for v in ids])) for i, ids in plans]
    shapes = {tuple(np.asarray(a).shape) for a in pixels.values()}
    if len(shapes) != 1:
        raise ValueError(f"the views of scan {scan!r} differ in size: {sorted(shapes)}")
    if not torch.cuda.is_available():
        raise RuntimeError("reconstruct_scan needs the GPU: libmvs_hip has no CPU implementation")
    device = device or torch.device("cuda", torch.cuda.current_device())
    present = sorted(pixels)
    slot = {v: k for k, v in enumerate(present)}
    V = max(present) + 1
    Ks = np.tile(np.eye(3, dtype=np.float32), (V, 1, 1))
    Es = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    model = model.to(device).eval()
    with torch.cuda.device(device), torch.no_grad():
        imgs = torch.from_numpy(np.stack([np.asarray(pixels[v]) for v in present])).to(device)
        feats = model.extract_features(imgs)
        h, w = feats.shape[2], feats.shape[3]
        depths = torch.zeros((V, h, w), dtype=torch.float32, device=device)
        confs = torch.zeros((V, h, w), dtype=torch.float32, device=device)
        for g in range(0, len(samples), batch):
            group = samples[g:g + batch]
            same = all(s["proj_matrices"].shape == group[0][1]["proj_matrices"].shape and
                       s["depth_values"].shape == group[0][1]["depth_values"].shape for _, s in group)
            for chunk in ([group] if same else [[x] for x in group]):
                out = model.forward_features(
                    feats, [[slot[v] for v in ids] for ids, _ in chunk],
                    torch.from_numpy(np.stack([np.asarray(s["proj_matrices"], np.float32) for _, s in chunk])).to(device),
                    torch.from_numpy(np.stack([np.asarray(s["depth_values"], np.float32) for _, s in chunk])).to(device))
                for b, (ids, s) in enumerate(chunk):
                    depths[ids[0]] = out["depth"][b]
                    confs[ids[0]] = out["photometric_confidence"][b]
                    Ks[ids[0]], Es[ids[0]] = np.asarray(s["intrinsics"][0]), np.asarray(s["extrinsics"][0])
        filtered = filter_views(depths, confs, Ks, Es, pairs, n_view_filter, photomask, geomask, condmask_pixel,
                                condmask_depth, device)
        xyz, rgb, view_counts = fuse_views(filtered, imgs, [slot[r] for r in refs])
        normals = None
        if normals_opt is not None:
            lo, hi = bin_box() if downsample.get("box") is None else downsample["box"]
            grown = (np.asarray(lo, np.float64) - normals_opt["margin"], np.asarray(hi, np.float64) + normals_opt["margin"])
            E = Es[refs].astype(np.float64)
            centres = -np.einsum("rji,rj->ri", E[:, :3, :3], E[:, :3, 3])          # -R^T t
            normals, normal_counts = estimate_normals(xyz, knn=normals_opt["knn"], box=grown, cell=normals_opt["cell"],
                                                      view_counts=view_counts, centres=centres)
        ds_in = xyz
        if outliers_opt is not None:
            keep, _, out_counts, out_stats, ds_in = remove_outliers(xyz, box=downsample.get("box"), masked=True,
                                                                    **outliers_opt)
        if planes_opt is not None:
            crop = bin_box() if downsample.get("box") is None else downsample["box"]
            remove = planes_opt.pop("remove")
            pl_planes, pl_labels, pl_counts, pl_rounds, pl_masked = segment_planes(ds_in, box=crop, masked=True, **planes_opt)
            if remove:
                ds_in = pl_masked
        if clusters_opt is not None:
            crop = bin_box() if downsample.get("box") is None else downsample["box"]
            cl_labels, cl_keep, cl_counts, ds_in = cluster_cloud(ds_in, box=crop, masked=True, **clusters_opt)
        if normals_opt is not None:
            ds_xyz, ds_rgb, ds_nrm = downsample_cloud(ds_in, rgb, normals=normals, **downsample)
            ds_vertices, ds_colours = _packed_to_host(ds_xyz, ds_rgb)
            ds_normals, normal_counts = ds_nrm.cpu().numpy(), normal_counts.cpu().numpy()
        elif downsample is not None:
            ds_vertices, ds_colours = _packed_to_host(*downsample_cloud(ds_in, rgb, **downsample))
        if outliers_opt is not None:
            outliers = dict(counts=out_counts.cpu().numpy(), stats=out_stats.cpu().numpy(), keep=keep.cpu().numpy())
        if planes_opt is not None:
            planes = dict(planes=pl_planes.cpu().numpy(), rounds=pl_rounds.cpu().numpy(), counts=pl_counts.cpu().numpy(),
                          labels=pl_labels.cpu().numpy())
        if clusters_opt is not None:
            clusters = dict(counts=cl_counts.cpu().numpy(), keep=cl_keep.cpu().numpy(), labels=cl_labels.cpu().numpy())
        vertices, colours = _packed_to_host(xyz, rgb)      # the one copy of the full cloud
    if plyfilename:
        write_ply(plyfilename, vertices, colours)
    if downsample is None:
        return vertices, colours
    tail = (() if outliers_opt is None else (outliers,)) + (() if planes_opt is None else (planes,)) \
        + (() if clusters_opt is None else (clusters,))
    if normals_opt is None:
        if ds_ply:
            write_ply(ds_ply, ds_vertices, ds_colours)
        return (vertices, colours, ds_vertices, ds_colours) + tail
    if ds_ply:
        write_ply(ds_ply, ds_vertices, ds_colours, ds_normals)
    return (vertices, colours, ds_vertices, ds_colours, ds_normals, normal_counts) + tail
