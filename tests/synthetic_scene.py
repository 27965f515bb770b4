"""Synthetic multi-view depth maps of a tilted plane for the filter / fusion tests (no reference
data is available offline).  Cameras are DTU-like at feature scale; every view's depth map is the
analytic ray/plane intersection times a smooth view-dependent perturbation of a few 0.1 %, so that
the 1 % relative-depth and 1 px reprojection checks (eval.py:574-582) both pass and fail somewhere.

Options (the defaults leave every output bit-identical to the scenes the first filter tests were written on):
`k_spread` > 0 gives every view its own intrinsics (focal lengths varied by that relative amount, principal points
moved by up to 2 * k_spread of the image size) and `skew` sets K[0,1], so that K_ref and K_src -- and their
inverses -- can be told apart; `rot` (radians, std of the two rotation angles) and `baseline` (a factor on the camera
translations) widen the views until reprojections leave the source image; `roll` (radians per view
index) turns view v about its optical axis by roll * (v + 1), which leaves no structural zero in the rotation; `noise=0` gives exact plane depths (up to
float32 rounding), every world point then lies on PLANE_N . X = PLANE_C."""
import numpy as np

PLANE_N = np.array([0.2, 0.1, 1.0])
PLANE_C = 700.0


def make_scene(V=6, h=64, w=80, seed=0, noise=0.006, rot=0.04, k_spread=0.0, skew=0.0, baseline=1.0,
               roll=0.0):
    rng = np.random.default_rng(seed)
    K = np.array([[361.5 * w / 160, 0, w / 2], [0, 360.0 * h / 128, h / 2], [0, 0, 1]], np.float64)
    Ks = np.tile(K.astype(np.float32), (V, 1, 1))
    if k_spread or skew:
        krng = np.random.default_rng(seed + 7919)       # its own stream: the draws below stay where they were
        for v in range(V):
            Kv = K.copy()
            Kv[0, 0] *= 1 + k_spread * krng.uniform(-1, 1)
            Kv[1, 1] *= 1 + k_spread * krng.uniform(-1, 1)
            Kv[0, 2] += 2 * k_spread * w * krng.uniform(-1, 1)
            Kv[1, 2] += 2 * k_spread * h * krng.uniform(-1, 1)
            Kv[0, 1] = skew * (1 + 0.5 * krng.uniform(-1, 1))
            Ks[v] = Kv.astype(np.float32)
    Es = np.zeros((V, 4, 4), np.float32)
    n, c = PLANE_N, PLANE_C
    depths = np.zeros((V, h, w), np.float32)
    confs = np.zeros((V, h, w), np.float32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for v in range(V):
        a, b = rot * rng.standard_normal(2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Ry @ Rx
        if roll:
            g = roll * (v + 1)
            R = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]]) @ R
        t = np.array([-25.0 * v + 60, 6.0 * v - 15, 3.0 * rng.standard_normal()])
        if baseline != 1.0:
            t = t * baseline
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, t
        Es[v] = E.astype(np.float32)
        E64 = Es[v].astype(np.float64)
        Rf, tf = E64[:3, :3], E64[:3, 3]
        dirs = np.linalg.inv(Ks[v].astype(np.float64)) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        Rt = np.linalg.inv(Rf)
        d = (c + n @ (Rt @ tf)) / (n @ (Rt @ dirs))
        ph = rng.uniform(0, 6.28, 2)
        pert = 1 + noise * np.sin(xs.ravel() * 0.21 + ph[0]) * np.cos(ys.ravel() * 0.17 + ph[1])
        depths[v] = (d * pert).reshape(h, w).astype(np.float32)
        confs[v] = (0.5 + 0.5 * np.sin(xs * 0.13 + v) * np.cos(ys * 0.11 - v)).astype(np.float32)
    pairs = [(v, [s for s in np.roll(np.arange(V), -v)[1:]]) for v in range(V)]
    pairs = [(int(r), [int(s) for s in ss]) for r, ss in pairs]
    return depths, confs, Ks, Es, pairs
