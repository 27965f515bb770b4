"""Training-format datasets with ground-truth depth: the readers behind the reference's test mode
(`train.py --mode test`, train.py:113-118), for the two formats it reads, datasets/dtu_yao.py and
datasets/blender.py.

Written from the reference's behaviour, not its code.  Both take the reference's constructor
arguments `(datapath, listfile, mode, nviews, ndepths, interval_scale, pairfile=, Nlights=)` and return
the reference's item dict `imgs [N,3,H,W], proj_matrices [N,4,4], depth [h,w], depth_values [D], mask [h,w]`
(float32, the same bits).  Common to both:
  * pair file `{Cameras|Cameras_512x640}/{pairfile}` (the format of dataset_eval.parse_pair_file), the same
    for every scan of the list file; one sample per (scan, viewpoint, light)
  * reference view + the first nviews-1 source views; proj = [[K @ E[:3,:4]], [E[3]]] in float32
  * cam file as dataset_eval.parse_cam_file; depth_values from the REFERENCE view's cam file
  * image, mask: PIL pixels as float32 / 255; GT depth: the PFM as float32
The formats differ in:
  | | dtu_yao | blender |
  | lights | 7 per viewpoint | Nlights "n:tot", drawn with random.sample (below) |
  | intrinsics | as stored | rows 0-1 divided by 4 |
  | GT depth and mask | as stored | subsampled [::4, ::4] |
  | depth_values | arange(min, interval*D + min, interval) | arange(min, min + interval*(D-0.5), interval) |
  | image | Rectified/{scan}_train/rect_{vid+1:03}_{light}_r5000.png | Rectified_512x640/{scan}/rect_C{vid:03}_L{light:02}.png |
Blender's light choice per viewpoint (in scan, viewpoint order): Nlights 0 -> light 0; negative -> light
-Nlights; otherwise mode "val" samples 2 of range(Nlights) and "test" Nlights of range(tot).  The draws come from
random.Random(seed), or from the module-level `random` when seed is None, as the reference does: with
`random.seed(s)` before the reference's constructor, seed=s reproduces its choice.

Added, as EvalDataset has them: image_dtype="uint8" (the decoded pixels; the drop-in MVSNet divides by 255 on
the device, bit-identically) and view_plan(idx) (image paths, keyed by light, for the feature bank).
"""
from __future__ import annotations

import os
import random

import numpy as np
from PIL import Image

from .data_io import read_pfm
from .dataset_eval import parse_cam_file, parse_pair_file


class _GTDataset:
    _cam_dir = None

    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, pairfile="pair.txt",
                 Nlights="1:1", image_dtype="float32", seed=None):
        if mode not in ("val", "test"):
            raise ValueError(f"mode must be 'val' or 'test' (training is out of scope), got {mode!r}")
        if image_dtype not in ("float32", "uint8"):
            raise ValueError(f"image_dtype must be 'float32' or 'uint8', got {image_dtype!r}")
        self.datapath, self.listfile, self.mode = datapath, listfile, mode
        self.nviews, self.ndepths, self.interval_scale = nviews, ndepths, interval_scale
        self.pairfile, self.image_dtype = pairfile, image_dtype
        self._parse_lights(Nlights)
        self._rng = random if seed is None else random.Random(seed)
        with open(listfile) as f:
            scans = [ln.rstrip() for ln in f.readlines()]
        self.metas = []
        for scan in scans:
            for ref, src in parse_pair_file(os.path.join(datapath, self._cam_dir, pairfile)):
                for light in self._lights():
                    self.metas.append((scan, light, ref, src))

    def _parse_lights(self, Nlights):
        pass

    def __len__(self):
        return len(self.metas)

    def view_ids(self, idx):
        scan, light, ref, src = self.metas[idx]
        return [ref] + src[:self.nviews - 1]

    def view_plan(self, idx):
        """-> (None, [(image path, cam path), ...]) of sample idx, reference view first.  The image path carries
        the light, so it identifies the pixels (the key of eval_driver's feature bank)."""
        scan, light, _, _ = self.metas[idx]
        return None, [(self._image_path(scan, vid, light), self._cam_path(vid)) for vid in self.view_ids(idx)]

    def _cam_path(self, vid):
        return os.path.join(self.datapath, self._cam_file.format(vid))

    def _read_image(self, path):
        img = Image.open(path)
        if self.image_dtype == "uint8":
            return np.asarray(img, dtype=np.uint8)
        return np.array(img, dtype=np.float32) / 255.

    def _read_mask(self, path):
        m = np.array(Image.open(path), dtype=np.float32) / 255.
        if m.ndim != 2:
            raise ValueError(f"{path}: the mask must be a single-channel image, got an array of shape {m.shape}")
        return m

    def __getitem__(self, idx):
        scan, light, _, _ = self.metas[idx]
        imgs, projs = [], []
        depth = mask = depth_values = None
        for i, vid in enumerate(self.view_ids(idx)):
            imgs.append(self._read_image(self._image_path(scan, vid, light)))
            intr, extr, dmin, dint = parse_cam_file(self._cam_path(vid), self.interval_scale)
            intr = self._intrinsics(intr)
            proj = extr.copy()
            proj[:3, :4] = np.matmul(intr, proj[:3, :4])
            projs.append(proj)
            if i == 0:
                depth_values = self._depth_values(dmin, dint)
                mask = self._read_mask(self._mask_path(scan, vid))
                depth = np.array(read_pfm(self._depth_path(scan, vid))[0], dtype=np.float32)
                mask, depth = self._gt_view(mask), self._gt_view(depth)
        return {"imgs": np.stack(imgs).transpose([0, 3, 1, 2]),
                "proj_matrices": np.stack(projs),
                "depth": depth,
                "depth_values": depth_values,
                "mask": mask}


class DtuYaoDataset(_GTDataset):
    """The DTU training set as preprocessed by Yao et al. (reference datasets/dtu_yao.py): 7 lights per viewpoint,
    GT at the feature resolution (128x160 for 512x640 images)."""
    _cam_dir = "Cameras"
    _cam_file = "Cameras/train/{:0>8}_cam.txt"

    def _lights(self):
        return range(7)

    def _image_path(self, scan, vid, light):
        return os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light))

    def _mask_path(self, scan, vid):
        return os.path.join(self.datapath, "Depths/{}_train/depth_visual_{:0>4}.png".format(scan, vid))

    def _depth_path(self, scan, vid):
        return os.path.join(self.datapath, "Depths/{}_train/depth_map_{:0>4}.pfm".format(scan, vid))

    def _intrinsics(self, intr):
        return intr

    def _depth_values(self, dmin, dint):
        return np.arange(dmin, dint * self.ndepths + dmin, dint, dtype=np.float32)

    def _gt_view(self, a):
        return a


class BlenderDataset(_GTDataset):
    """The Blender-rendered training format (reference datasets/blender.py): lights drawn per viewpoint, GT at the
    image resolution, subsampled by 4 to the feature resolution."""
    _cam_dir = "Cameras_512x640"
    _cam_file = "Cameras_512x640/{:0>8}_cam.txt"

    def _parse_lights(self, Nlights):
        n, tot = str(Nlights).split(":")[:2]
        self.Nlights = int(n.replace("(", "").replace(")", ""))
        self.TotLights = int(tot)

    def _lights(self):
        if self.Nlights == 0:
            return [0]
        if self.Nlights < 0:
            return [-self.Nlights]
        if self.mode == "val":
            if self.Nlights < 2:
                raise ValueError(f"mode 'val' draws 2 of Nlights lights, got Nlights={self.Nlights}")
            return self._rng.sample(range(self.Nlights), k=2)
        if self.Nlights > self.TotLights:
            raise ValueError(f"Nlights={self.Nlights} exceeds the {self.TotLights} lights of the dataset")
        return self._rng.sample(range(self.TotLights), k=self.Nlights)

    def _image_path(self, scan, vid, light):
        return os.path.join(self.datapath, "Rectified_512x640/{}/rect_C{:0>3}_L{:0>2}.png".format(scan, vid, light))

    def _mask_path(self, scan, vid):
        return os.path.join(self.datapath, "Depths_512x640/{}/depth_mask_{:0>3}.png".format(scan, vid))

    def _depth_path(self, scan, vid):
        return os.path.join(self.datapath, "Depths_512x640/{}/depth_map_{:0>3}.pfm".format(scan, vid))

    def _intrinsics(self, intr):
        intr[:2, :] = intr[:2, :] / 4.0     # feature scale
        return intr

    def _depth_values(self, dmin, dint):
        return np.arange(dmin, dmin + dint * (self.ndepths - 0.5), dint, dtype=np.float32)

    def _gt_view(self, a):
        return a[::4, ::4]


DATASETS = {"dtu_yao": DtuYaoDataset, "blender": BlenderDataset}


def find_dataset_def(name):
    """The reader class of a train.py `--dataset` name (reference datasets/__init__.py)."""
    if name not in DATASETS:
        raise ValueError(f"unknown dataset {name!r}; one of {sorted(DATASETS)}")
    return DATASETS[name]
