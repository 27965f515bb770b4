"""Scans in, fused point clouds out: the counterpart of running the reference's eval.py (save_depth, then filter_depth
per scan), with nothing written but the PLY files.

    python -m scene_3dreconstruction_mvsnet_amd.reconstruct --testpath DATA --testlist LIST --loadckpt model.ckpt \\
        --outdir OUT [--pairfile pair.txt --numdepth 192 --interval_scale 1.06 --NviewGen 5 --NviewFilter 10
        --photomask 0.8 --geomask 3 --condmask_pixel 1.0 --condmask_depth 0.01 --dataset_name dtu]

Each scan of the list goes through fusion.reconstruct_scan and is written to OUT/mvsnet{scan_id:03d}_l3.ply, the name
eval.py gives it (scan_id = the first number in the scan's name).  eval.py picks the camera folder, the image path
pattern and the image size from a table keyed by --dataset_name; here they are the flags --cam_subfolder,
--img_subfolder and --img_res, with EvalDataset's defaults.

--downsample_mm V adds eval.py's last step for the bin-picking datasets (eval.py:831-840): the fused cloud is cropped to
the bin's outer box, voxel-downsampled at V and scaled by --cloud_scale on the device, and written to
OUT/<scan>/fused_dwnsmpld_<V>mm.ply, eval.py's name and place.  The box is --crop_box x0 y0 z0 x1 y1 z1 (in the cloud's
units), or the bin of --bin_dims / --bin_delta (metres, fusion.bin_box).  --normals_knn K (with --downsample_mm) adds
eval.py:817's estimate_normals: normals from K neighbours inside the box grown by --normals_margin_mm, turned towards each
point's camera, carried through the voxel filter and written as nx, ny, nz.  --outlier_knn K (with --downsample_mm) adds
eval.py:495's remove_statistical_outlier between the crop and the voxel filter: a point of the box whose mean distance to
its K nearest neighbours there is not below mean + --outlier_std standard deviations of those distances is dropped.
--cluster_eps E (with --downsample_mm) adds fusion.cluster_cloud after that and before the voxel filter: DBSCAN among the
points of the box with radius E (the cloud's units) and --cluster_min_points neighbours for a core point; the noise and the
clusters of fewer than --cluster_min_size points are dropped.
--segment_dist D (with --downsample_mm) adds fusion.segment_planes before the clustering: --segment_planes rounds of RANSAC
with --segment_candidates candidate planes each take the bin's floor and walls out (the points within D of each plane,
the cloud's units), so that the parts no longer hang together through them; --segment_keep labels the planes and removes
nothing; --segment_out FILE.npz ({scan} is replaced) receives the planes, the first as the array P that eval_cloud --plane reads
(not written when no plane is found; the largest component of its normal is positive, which decides the side --plane keeps).

--gt_ply PATH scores every scan's fused cloud (the full one, as it is written) against the ground-truth cloud of PATH on
the GPU and prints the result as `<scan>: score {json}`; --max_dist, --thresholds, --box, --cell and --json are eval_cloud's
(--json receives {scan: result}), and so are DTU's steps: --reduce_dist, --reduce_seed, --reduce_gt, --obs_mask FILE and
--plane FILE, and the ICP alignment before them: --register_dist D, --register_iters, --register_point_to_point.  PATH and
the two FILEs may hold `{scan}`.  Nothing else about the run changes.
"""
from __future__ import annotations

import argparse
import json
import os
import re

from .mvsnet import _load_checkpoint


def downsampled_name(voxel_mm):
    """eval.py:836's file name: fused_dwnsmpld_5mm.ply for 5 and 5.0, fused_dwnsmpld_2.5mm.ply for 2.5."""
    return f"fused_dwnsmpld_{voxel_mm:g}mm.ply"


def segment_options(args):
    """downsample['planes'] of the --segment_* flags, or None without --segment_dist."""
    if args.segment_dist is None:
        return None
    return dict(dist=args.segment_dist, max_planes=args.segment_planes, num_candidates=args.segment_candidates,
                min_inliers=3 if args.segment_min_inliers is None else args.segment_min_inliers, seed=args.segment_seed,
                remove=not args.segment_keep)


def write_planes(path, planes):
    """--segment_out: the arrays P (the first plane: fusion.read_plane reads it back, eval_cloud --plane applies it), planes,
    rounds and counts of reconstruct_scan's planes item.  Refused when no plane was found: P would be NaN, and the plane
    filter would read it without a word.  The sign of P is the segmentation's without `toward`: the largest component of
    the normal is positive, so the side select_cloud keeps (n . x + d > 0) is the side that component points to, not
    necessarily the scene's upper side; negate P where the other side is wanted."""
    import numpy as np
    if int(np.asarray(planes["counts"])[1]) < 1:
        raise ValueError(f"write_planes: no plane was found (counts {np.asarray(planes['counts']).tolist()}): nothing to write to {path}")
    np.savez(path, P=np.asarray(planes["planes"], np.float64)[0], planes=planes["planes"], rounds=planes["rounds"],
             counts=planes["counts"])


def main(argv=None):
    from . import MVSNet
    from .dataset_eval import EvalDataset
    from .eval_cloud import add_score_arguments, score
    from .fusion import bin_box, reconstruct_scan

    p = argparse.ArgumentParser(description="Reconstruct every scan of a list into a fused, coloured point cloud")
    p.add_argument("--testpath", required=True)
    p.add_argument("--testlist", required=True)
    p.add_argument("--pairfile", default="pair.txt")
    p.add_argument("--loadckpt", required=True)
    p.add_argument("--outdir", default="./outputs")
    p.add_argument("--numdepth", type=int, default=192)
    p.add_argument("--interval_scale", type=float, default=1.06)
    p.add_argument("--NviewGen", type=int, default=5)
    p.add_argument("--NviewFilter", type=int, default=10)
    p.add_argument("--photomask", type=float, default=0.8)
    p.add_argument("--geomask", type=int, default=3)
    p.add_argument("--condmask_pixel", type=float, default=1.0)
    p.add_argument("--condmask_depth", type=float, default=0.01)
    p.add_argument("--dataset_name", default="dtu")
    p.add_argument("--cam_subfolder", default="Cameras")
    p.add_argument("--img_subfolder", default="Rectified/{}/rect_{:0>3}_3_r5000.png")
    p.add_argument("--img_res", type=int, nargs=2, default=(512, 640), metavar=("H", "W"))
    p.add_argument("--downsample_mm", type=float, default=None, metavar="V",
                   help="also write OUT/<scan>/fused_dwnsmpld_<V>mm.ply: the cloud cropped to the box, one point per voxel of size V")
    p.add_argument("--crop_box", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="the box to keep, in the cloud's units (instead of --bin_dims / --bin_delta)")
    p.add_argument("--bin_dims", type=float, nargs=3, default=(0.57, 0.37, 0.22), metavar=("DX", "DY", "DZ"),
                   help="inner size of the bin in metres (eval.py's get_o3d_frame_bbox)")
    p.add_argument("--bin_delta", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"),
                   help="offset of the bin in metres (0.08 0.03 0 is eval.py's overhead02 / overhead03)")
    p.add_argument("--cloud_scale", type=float, default=0.01, help="factor on the downsampled coordinates (eval.py:839)")
    p.add_argument("--normals_knn", type=int, default=None, metavar="K",
                   help="with --downsample_mm: estimate normals from K neighbours (eval.py:817) and write nx, ny, nz")
    p.add_argument("--normals_margin_mm", type=float, default=20.0,
                   help="the neighbour search covers the box grown by this much (a guess; the tool prints how many points "
                        "a point outside could have served better)")
    p.add_argument("--outlier_knn", type=int, default=None, metavar="K",
                   help="with --downsample_mm: drop statistical outliers from K neighbours (eval.py:495) before the voxel filter")
    p.add_argument("--outlier_std", type=float, default=2.0, metavar="S",
                   help="a point is kept while its mean neighbour distance is below mean + S standard deviations")
    p.add_argument("--cluster_eps", type=float, default=None, metavar="E",
                   help="with --downsample_mm: label the density-connected clusters of the box (DBSCAN, radius E in the "
                        "cloud's units) and drop the noise and the small clusters before the voxel filter")
    p.add_argument("--cluster_min_points", type=int, default=10, metavar="M",
                   help="a core point has at least M points within E, itself counted")
    p.add_argument("--cluster_min_size", type=int, default=1, metavar="S",
                   help="a cluster is kept while it has at least S points (1 drops the noise only)")
    p.add_argument("--segment_dist", type=float, default=None, metavar="D",
                   help="with --downsample_mm: take the dominant planes of the box out before the clustering (RANSAC; a "
                        "point belongs to a plane within D, the cloud's units)")
    p.add_argument("--segment_planes", type=int, default=1, metavar="N", help="the most planes that are taken out")
    p.add_argument("--segment_candidates", type=int, default=1000, metavar="K", help="candidate planes tried per round")
    p.add_argument("--segment_min_inliers", type=int, default=None, metavar="N",
                   help="stop when the best candidate of a round has fewer points (default 3)")
    p.add_argument("--segment_seed", type=int, default=0)
    p.add_argument("--segment_keep", action="store_true", help="label the planes' points only, remove nothing")
    p.add_argument("--segment_out", default=None, metavar="FILE.npz",
                   help="write the planes there: P (the first, what --plane reads), planes, rounds, counts ({scan} is replaced)")
    p.add_argument("--gt_ply", default=None, metavar="PATH",
                   help="score each scan's fused cloud against this ground-truth PLY ({scan} is replaced by the scan's name)")
    add_score_arguments(p)
    args = p.parse_args(argv)
    if args.gt_ply is None and (args.box is not None or args.json is not None):
        p.error("--box and --json need --gt_ply")
    if args.gt_ply is None and (args.reduce_dist is not None or args.obs_mask is not None or args.plane is not None):
        p.error("--reduce_dist, --obs_mask and --plane need --gt_ply")
    if args.gt_ply is None and args.register_dist is not None:
        p.error("--register_dist needs --gt_ply")
    if args.reduce_dist is None and (args.reduce_gt or args.reduce_seed != 0):
        p.error("--reduce_seed and --reduce_gt need --reduce_dist")
    if len(args.thresholds) > 8:
        p.error("at most 8 --thresholds")
    if args.downsample_mm is None and args.crop_box is not None:
        p.error("--crop_box needs --downsample_mm")
    if args.downsample_mm is None and args.normals_knn is not None:
        p.error("--normals_knn needs --downsample_mm")
    if args.downsample_mm is None and args.outlier_knn is not None:
        p.error("--outlier_knn needs --downsample_mm")
    if args.downsample_mm is None and args.cluster_eps is not None:
        p.error("--cluster_eps needs --downsample_mm")
    if args.cluster_eps is None and (args.cluster_min_points != 10 or args.cluster_min_size != 1):
        p.error("--cluster_min_points and --cluster_min_size need --cluster_eps")
    if args.downsample_mm is None and args.segment_dist is not None:
        p.error("--segment_dist needs --downsample_mm")
    if args.segment_dist is None and (args.segment_planes != 1 or args.segment_candidates != 1000 or args.segment_seed != 0
                                      or args.segment_min_inliers is not None or args.segment_keep or args.segment_out):
        p.error("--segment_planes, --segment_candidates, --segment_min_inliers, --segment_seed, --segment_keep and "
                "--segment_out need --segment_dist")
    box = None
    if args.downsample_mm is not None:
        box = (args.crop_box[:3], args.crop_box[3:]) if args.crop_box else bin_box(args.bin_dims, args.bin_delta)
    ds = EvalDataset(args.testpath, args.testlist, "test", args.NviewGen, args.numdepth, args.interval_scale,
                     pairfile=args.pairfile, cam_subfolder=args.cam_subfolder, img_subfolder=args.img_subfolder,
                     img_res=tuple(args.img_res), dataset_name=args.dataset_name, image_dtype="uint8")
    model = MVSNet(refine=False)
    _load_checkpoint(model, args.loadckpt)
    os.makedirs(args.outdir, exist_ok=True)
    written, scores = [], {}
    for scan in dict.fromkeys(m[0] for m in ds.metas):
        scan_id = int(re.findall(r"\d+", scan)[0])
        ply = os.path.join(args.outdir, "mvsnet{:0>3}_l3.ply".format(scan_id))
        downsample = None
        if box is not None:
            os.makedirs(os.path.join(args.outdir, scan), exist_ok=True)
            small = os.path.join(args.outdir, scan, downsampled_name(args.downsample_mm))
            downsample = dict(voxel_size=args.downsample_mm, box=box, scale=args.cloud_scale, plyfilename=small)
            if args.normals_knn is not None:
                downsample["normals"] = dict(knn=args.normals_knn, margin=args.normals_margin_mm)
            if args.outlier_knn is not None:
                downsample["outliers"] = dict(nb_neighbors=args.outlier_knn, std_ratio=args.outlier_std)
            if segment_options(args) is not None:
                downsample["planes"] = segment_options(args)
            if args.cluster_eps is not None:
                downsample["clusters"] = dict(eps=args.cluster_eps, min_points=args.cluster_min_points,
                                              min_size=args.cluster_min_size)
        got = reconstruct_scan(model, ds, scan, n_view_filter=args.NviewFilter, photomask=args.photomask,
                               geomask=args.geomask, condmask_pixel=args.condmask_pixel,
                               condmask_depth=args.condmask_depth, plyfilename=ply, downsample=downsample)
        print(f"{scan}: {len(got[0])} points -> {ply}")
        written.append(ply)
        if downsample:
            print(f"{scan}: {len(got[2])} voxels of {args.downsample_mm:g} -> {small}")
            written.append(small)
            if args.normals_knn is not None:
                members, estimated, open_ = (int(x) for x in got[5])
                print(f"{scan}: normals of {estimated} of {members} points in the grown box; {open_} of them could have "
                      f"had a nearer neighbour outside it")
            if args.outlier_knn is not None:
                outliers = got[-1 - (args.cluster_eps is not None) - (args.segment_dist is not None)]
                members, valid, kept = (int(x) for x in outliers["counts"])
                print(f"{scan}: {kept} of {members} points in the box kept ({valid} with a neighbour elsewhere; mean distance "
                      f"below {outliers['stats'][2]:g})")
            if args.segment_dist is not None:
                planes = got[-2] if args.cluster_eps is not None else got[-1]
                members, found, on_planes, stop = (int(x) for x in planes["counts"])
                print(f"{scan}: {found} planes among {members} points in the box hold {on_planes} of them"
                      f"{' (labelled, not removed)' if args.segment_keep else ''}")
                if args.segment_out and found == 0:
                    print(f"{scan}: no plane was found, --segment_out is not written")
                elif args.segment_out:
                    write_planes(args.segment_out.replace("{scan}", scan), planes)
                    written.append(args.segment_out.replace("{scan}", scan))
            if args.cluster_eps is not None:
                members, core, border, noise, clusters, kept, largest = (int(x) for x in got[-1]["counts"])
                print(f"{scan}: {clusters} clusters among {members} points in the box ({core} core, {border} border, {noise} "
                      f"noise; the largest has {largest}); {kept} points kept")
        if args.gt_ply is not None:
            from .fusion import read_ply
            scores[scan] = score(got[0], read_ply(args.gt_ply.replace("{scan}", scan))[0], args, scan=scan)
            print(f"{scan}: score {json.dumps(scores[scan], sort_keys=True)}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(scores, f, indent=1, sort_keys=True)
    return written


if __name__ == "__main__":
    main()
