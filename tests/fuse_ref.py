"""The fused point cloud of a scan in numpy: the yardstick of the mvs_fuse_points tests.

It restates the end of the reference's filter_depth (eval.py:745-758) the way fusion.filter_depth does on the host:
boolean indexing of each view's float64 points and of img[1::4, 1::4] with the final mask, the colour arithmetic
float32(u) / 255 * 255 truncated to uint8, concatenation over the views, and the float64 -> '<f4' assignment of the PLY
writer.  Nothing here knows how the kernels tile, scan or rank.
"""
import numpy as np


def colour_roundtrip(u8):
    """What the reference does to a decoded pixel before it reaches the PLY: np.array(img, float32) / 255 on loading
    (eval.py:130-134), * 255 and astype(uint8) on fusing (eval.py:759)."""
    return ((np.asarray(u8, dtype=np.float32) / 255.0) * 255).astype(np.uint8)


def fuse(xyz_world, masks, images, ref_idx, hwc=True):
    """xyz_world float64 [R,h*w,3]; masks [R,3,h,w] (plane 2 selects, != 0); images uint8 [V,4h,4w,3] (hwc) or
    [V,3,4h,4w]; ref_idx [R].  -> (xyz '<f4' [P,3], rgb uint8 [P,3], counts int32 [R+1]: per view, then the total).
    A ref_idx outside [0, V) gives its view no point."""
    xyz_world, masks, images = np.asarray(xyz_world), np.asarray(masks), np.asarray(images)
    R, V = masks.shape[0], images.shape[0]
    h, w = masks.shape[2:]
    vertices, colours, counts = [], [], []
    for r in range(R):
        v = int(ref_idx[r])
        final = masks[r, 2] != 0
        if v < 0 or v >= V:
            counts.append(0)
            continue
        img = images[v] if hwc else images[v].transpose(1, 2, 0)
        assert img.shape[:2] == (4 * h, 4 * w), "incompatible depth and image dimensions."
        img = np.array(img, dtype=np.float32) / 255.0
        vertices.append(xyz_world[r][final.reshape(-1)])
        colours.append((img[1::4, 1::4, :][final] * 255).astype(np.uint8))
        counts.append(int(final.sum()))
    xyz = np.concatenate(vertices, 0) if vertices else np.zeros((0, 3), np.float64)
    rgb = np.concatenate(colours, 0) if colours else np.zeros((0, 3), np.uint8)
    out = np.empty((len(xyz), 3), dtype="<f4")
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, 0], out[:, 1], out[:, 2] = xyz[:, 0], xyz[:, 1], xyz[:, 2]      # as write_ply assigns its fields
    return out, rgb, np.array(counts + [sum(counts)], np.int32)
