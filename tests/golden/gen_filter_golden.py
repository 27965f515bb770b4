#!/usr/bin/env python3
"""Golden vectors for the depth-map filter / fusion step (tests/golden/fx_filter.npz): the REFERENCE's own
reproject_with_depth, check_geometric_consistency (eval.py:508-585) and depth2pts_np (eval.py:253-265) on the fixture
scenes of tests/filter_ref.py, plus the reference's float32 np.linalg.inv / np.matmul camera products.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_filter_golden.py

eval.py is imported as a module with sys.argv cut to one entry (it parses its arguments at import) and with stub
modules for what is not installed: `plyfile` (PlyData, PlyElement), `open3d`, `torchvision.utils`, and `cv2`, whose
`remap` is oracle.filter_oracle.remap_linear -- the ONE call of the filter that is not the reference's own code here
(eval.py:540); everything else recorded below is computed by the reference's functions on the numpy this container
links.  The per-view combination (eval.py:692-706: the int32 mask sum, `sum(list) + ref` over `sum + 1`, the `>=`
geo mask, the `>` photo mask of eval.py:660 and their logical_and) sits inside a function that reads files; those few
numpy expressions are restated in `combine` below.  Nothing else of the reference's text is copied anywhere."""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.environ.get("MVS_REFERENCE", "/root/reference"))

from oracle import filter_oracle as fo  # noqa: E402

import filter_ref as R  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)
    return sys.modules[name]


def _remap(src, map_x, map_y, interpolation=None):
    return fo.remap_linear(np.ascontiguousarray(src, np.float32), map_x, map_y)


_stub("plyfile", PlyData=object, PlyElement=object)
_stub("open3d")
tv = _stub("torchvision")
tv.utils = _stub("torchvision.utils")
_stub("cv2", remap=_remap, INTER_LINEAR=1)
sys.argv = sys.argv[:1]
with contextlib.redirect_stdout(io.StringIO()):
    import eval as ev  # noqa: E402  (reference)


def combine(masks, d_reps, ref_depth, confidence, photomask, geomask):
    """eval.py:660, 692, 699, 702, 706 restated (see the module docstring)."""
    geo_mask_sum = 0
    for m in masks:
        geo_mask_sum += m.astype(np.int32)
    with np.errstate(all="ignore"):
        depth_est_averaged = (sum(d_reps) + ref_depth) / (geo_mask_sum + 1)
    photo_mask = confidence > photomask
    geo_mask = geo_mask_sum >= geomask
    return geo_mask_sum, depth_est_averaged, photo_mask, geo_mask, np.logical_and(photo_mask, geo_mask)


def record(out, sc):
    name, th, d, c, K, E = sc["name"], sc["th"], sc["depths"], sc["confs"], sc["Ks"], sc["Es"]
    ev.args.condmask_pixel, ev.args.condmask_depth = th["condmask_pixel"], th["condmask_depth"]
    out[f"{name}/depths"], out[f"{name}/confs"], out[f"{name}/Ks"], out[f"{name}/Es"] = d, c, K, E
    ref_idx, src_idx = R.abi_rows(sc)
    out[f"{name}/pair_ref"], out[f"{name}/pair_src"] = ref_idx, src_idx
    for k, v in th.items():
        out[f"{name}/{k}"] = np.asarray(v)
    for ref, srcs in sc["pairs"]:
        masks, d_reps = [], []
        for j, s in enumerate(srcs[:th["n_view_filter"]]):
            a = (d[ref].copy(), K[ref], E[ref], d[s].copy(), K[s], E[s])
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                d_rep, x_rep, y_rep, x_src, y_src = ev.reproject_with_depth(*a)
                mask, d_masked, _, _ = ev.check_geometric_consistency(*a)
            p = f"{name}/{ref}_{j}/"
            out[p + "mask"], out[p + "depth_reprojected"] = mask, d_rep
            out[p + "x_reprojected"], out[p + "y_reprojected"], out[p + "x_src"], out[p + "y_src"] = x_rep, y_rep, x_src, y_src
            masks.append(mask)
            d_reps.append(d_masked)
        gs, avg, photo, geo, final = combine(masks, d_reps, d[ref], c[ref], th["photomask"], th["geomask"])
        assert avg.dtype == np.float64 and gs.dtype == np.int32
        with np.errstate(all="ignore"):
            xyz = ev.depth2pts_np(avg, K[ref], E[ref])
        p = f"{name}/{ref}/"
        out[p + "geo_mask_sum"], out[p + "depth_est_averaged"], out[p + "xyz_world"] = gs, avg, xyz
        out[p + "photo_mask"], out[p + "geo_mask"], out[p + "final_mask"] = photo, geo, final
    if name == "distinctK":     # the float32 products mvs_filter_compose restates, as this container's numpy forms them
        V = len(K)
        out[f"{name}/inv_K"] = np.stack([np.linalg.inv(K[v]) for v in range(V)])
        out[f"{name}/inv_R"] = np.stack([np.linalg.inv(E[v][:3, :3]) for v in range(V)])
        out[f"{name}/E_inv_E"] = np.stack([np.stack([np.matmul(E[a], np.linalg.inv(E[b])) for b in range(V)])
                                           for a in range(V)])      # [a][b] = E_a inv(E_b)
        assert out[f"{name}/inv_K"].dtype == np.float32 and out[f"{name}/E_inv_E"].dtype == np.float32


def main():
    out = {}
    for name in R.FIXTURE_SCENES:
        record(out, R.scene(name))
    fn = os.path.join(HERE, "fx_filter.npz")
    np.savez_compressed(fn, **out)
    print(len(out), "arrays,", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
