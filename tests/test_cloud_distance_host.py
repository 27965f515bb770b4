"""Host-side checks of the cloud-to-cloud distance (include/mvs_distance_abi.h, csrc/cloud_distance.hip, fusion.read_ply,
fusion.evaluate_cloud's arithmetic, the command lines): none needs a GPU.  Every refusal is decided before the first HIP
call, so the fake device pointers are never dereferenced; the refusals run in a child process that sees no device
(HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty), where a call the library failed to refuse would come back as
MVS_ERR_HIP (4) instead of reaching hardware."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for path in (REPO, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import distance_ref  # noqa: E402
import normals_ref  # noqa: E402
import outliers_ref  # noqa: E402
import refusals  # noqa: E402

from refusals import BAD_DTYPE, BAD_SHAPE, BIN, HIP, INF, NAN, NULL, OK, WORKSPACE  # noqa: E402

# ---------------------------------------------------------------- the refusal cases (shared by the child and the tests)
GOOD = dict(ref_dtype=0, query_dtype=0, P=5000, N=3000, box_min=BIN[0], box_max=BIN[1], cell=5.0, max_dist=20.0, thresholds=(1.0, 2.0, 5.0))
CASES = [(f"null {p}", {p: None}, NULL, "NULL") for p in ("ref_xyz", "query_xyz", "box_min", "box_max", "thresholds", "dist_out", "counts_out", "stats_out", "workspace")]
CASES += [
    ("idx_out may be NULL", dict(idx_out=None, workspace_bytes=0), WORKSPACE, "workspace"),
    ("thresholds may be NULL at T == 0", dict(thresholds=None, T=0, workspace_bytes=0), WORKSPACE, "workspace"),
    ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"),
    ("N < 0", dict(N=-1), BAD_SHAPE, "N = -1"),
    ("N = 2^31", dict(N=1 << 31), BAD_SHAPE, "N = 2147483648"),
    ("N = 2^40", dict(N=1 << 40), BAD_SHAPE, "2^31"),
    ("T = 9", dict(thresholds=(1.0,) * 9), BAD_SHAPE, "T = 9"),
    ("T = -1", dict(T=-1), BAD_SHAPE, "T = -1"),
    ("T = 8 is legal", dict(thresholds=(1.0,) * 8, workspace_bytes=0), WORKSPACE, "workspace"),
    ("max_dist nan", dict(max_dist=NAN), BAD_SHAPE, "max_dist"),
    ("max_dist < 0", dict(max_dist=-1.0), BAD_SHAPE, "max_dist"),
    ("max_dist -inf", dict(max_dist=-INF), BAD_SHAPE, "max_dist"),
    ("max_dist inf is legal", dict(max_dist=INF, workspace_bytes=0), WORKSPACE, "workspace"),
    ("max_dist 0 is legal", dict(max_dist=0.0, workspace_bytes=0), WORKSPACE, "workspace"),
    ("threshold nan", dict(thresholds=(1.0, NAN)), BAD_SHAPE, "thresholds[1]"),
    ("threshold < 0", dict(thresholds=(-0.5,)), BAD_SHAPE, "thresholds[0]"),
    ("threshold inf", dict(thresholds=(1.0, 2.0, INF)), BAD_SHAPE, "thresholds[2]"),
    ("threshold 0 is legal", dict(thresholds=(0.0,), workspace_bytes=0), WORKSPACE, "workspace"),
    ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("cell < 0", dict(cell=-5.0), BAD_SHAPE, "cell"),
    ("cell nan", dict(cell=NAN), BAD_SHAPE, "cell"),
    ("cell inf", dict(cell=INF), BAD_SHAPE, "cell"),
    ("box nan", dict(box_min=(NAN, 0, 0)), BAD_SHAPE, "box axis 0"),
    ("box -inf", dict(box_min=(0, -INF, 0)), BAD_SHAPE, "box axis 1"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("one axis of 3e9", dict(box_min=(0, 0, 0), box_max=(3e9, 0, 0), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("ref dtype 2", dict(ref_dtype=2), BAD_DTYPE, "dtype 2"),
    ("query dtype -1", dict(query_dtype=-1), BAD_DTYPE, "dtype -1"),
    ("one byte short", dict(workspace_bytes="need-1"), WORKSPACE, "workspace"),
    ("the normals' size is too small", dict(workspace_bytes="normals"), WORKSPACE, "workspace"),
    ("no workspace", dict(workspace_bytes=0), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace_bytes="need", workspace="plus4"), WORKSPACE, "aligned"),
    ("everything right reaches HIP", dict(workspace_bytes="need"), HIP, ""),
    ("the other dtype pair reaches HIP", dict(workspace_bytes="need", ref_dtype=1, query_dtype=1), HIP, ""),
    ("mixed dtypes reach HIP", dict(workspace_bytes="need", ref_dtype=0, query_dtype=1), HIP, ""),
    ("P == 0 reaches HIP", dict(P=0, workspace_bytes="need"), HIP, ""),
    ("N == 0 reaches HIP", dict(N=0, workspace_bytes="need"), HIP, ""),
]
Q_CASES = [
    ("null box_min", dict(box_min=None), NULL, "NULL"), ("null box_max", dict(box_max=None), NULL, "NULL"),
    ("null bytes", dict(bytes=None), NULL, "NULL"), ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"), ("N < 0", dict(N=-7), BAD_SHAPE, "N = -7"),
    ("N = 2^31", dict(N=1 << 31), BAD_SHAPE, "2^31"), ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("cell nan", dict(cell=NAN), BAD_SHAPE, "cell"), ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("fine", dict(), OK, ""), ("P == 0 and N == 0 are fine", dict(P=0, N=0), OK, ""),
]


REFUSALS = {
    "mvs_cloud_distance": dict(
        good=dict(GOOD, T=lambda a: len(a["thresholds"])), host=dict(refusals.BOX, thresholds=ctypes.c_double),
        optional=("idx_out",), cases=CASES,
        sizes=dict(need=lambda a: distance_ref.workspace_bytes(a["P"], a["N"], a["box_min"], a["box_max"], a["cell"]),
                   normals=lambda a: normals_ref.workspace_bytes(a["P"], a["box_min"], a["box_max"], a["cell"]))),
    "mvs_query_distance_workspace": dict(good=GOOD, host=refusals.BOX, cases=Q_CASES),
}


@pytest.mark.parametrize("ep,cases", [("distance", CASES), ("query", Q_CASES)])
def test_every_refusal_comes_with_its_status_and_its_message(ep, cases):
    name, = [n for n, spec in REFUSALS.items() if spec["cases"] is cases and ep in n]
    refusals.check(sys.modules[__name__], (name,))


# ---------------------------------------------------------------- declarations
from scene_3dreconstruction_mvsnet_amd import _lib, eval_cloud, fusion, reconstruct  # noqa: E402


def test_distance_symbols_are_the_declarations_of_the_distance_header():
    src = refusals.check_header("mvs_distance_abi.h", _lib.DISTANCE_SYMBOLS)
    assert list(_lib.DISTANCE_SYMBOLS) == ["mvs_query_distance_workspace", "mvs_cloud_distance"]
    assert '#include "mvs_abi.h"' in src and '#include "mvs_outliers_abi.h"' in src
    for name, value in (("MVS_DISTANCE_THRESHOLDS_MAX", _lib.DISTANCE_THRESHOLDS_MAX), ("MVS_DISTANCE_SCALARS", _lib.DISTANCE_SCALARS)):
        assert refusals.define(src, name) == value == getattr(distance_ref, name[13:])
    assert "mvs_distance_abi.h" in refusals.header_text("mvs_abi.h")
    assert "observability mask" in src and "nothing here was compared against the MATLAB code" in src


# ---------------------------------------------------------------- workspace formula
@pytest.mark.parametrize("P,N,lo,hi,cell", [(5000, 3000, BIN[0], BIN[1], 5.0), (0, 3000, BIN[0], BIN[1], 5.0),
                                            (5000, 0, BIN[0], BIN[1], 5.0), (0, 0, BIN[0], BIN[1], 5.0),
                                            (7, 1, BIN[0], BIN[1], 2.5), (7, 2, BIN[0], BIN[1], 2.5),
                                            (4097, 1024, (-300, -200, -50), (300, 200, 150), 7.3),
                                            (4097, 1025, (-300, -200, -50), (300, 200, 150), 7.3),
                                            (3, (1 << 20) + 5, (0, 0, 0), (0, 0, 0), 1.0),
                                            ((1 << 31) - 1, (1 << 31) - 1, (0, 0, 0), (1289, 1289, 1289), 1.0)])
def test_distance_workspace_query_agrees_with_the_headers_formula(P, N, lo, hi, cell):
    want = distance_ref.workspace_bytes(P, N, lo, hi, cell)
    assert _lib.query_distance_workspace(P, N, lo, hi, cell) == want and want % 8 == 0
    # the grid part is exactly the normals' query over P; the rest depends on N alone, as the outliers' does on its P
    assert want - _lib.query_normals_workspace(P, lo, hi, cell) == 8 * outliers_ref.partial_sums(N) + 64
    assert want - _lib.query_normals_workspace(P, lo, hi, cell) == (_lib.query_outliers_workspace(N, lo, hi, cell)
                                                                    - _lib.query_normals_workspace(N, lo, hi, cell))
    levels = {0: 0, 1: 0, 2: 1, 1024: 1, 1025: 3}
    if N in levels:
        assert outliers_ref.partial_sums(N) == levels[N]
    with pytest.raises(_lib.MvsError) as e:
        _lib.query_distance_workspace(P, N, (0, 0, 0), (1290, 1290, 1290), 1.0)      # 1291^3 >= 2^31
    assert e.value.code == BAD_SHAPE


# ---------------------------------------------------------------- the yardstick against an independent formulation
def _scene(P, N, seed):
    """A noisy plane with scattered points as the reference, another sampling of it as the queries, a quarter of them
    scattered through a volume that reaches well outside the box; continuous coordinates: no ties."""
    rng = np.random.default_rng(seed)
    r = np.column_stack([rng.uniform(-100, 100, P), rng.uniform(-60, 60, P), rng.normal(10, 0.5, P)])
    far = rng.choice(P, P // 20, replace=False)
    r[far] = rng.uniform([-130, -90, -40], [130, 90, 90], (len(far), 3))
    r[7] = np.nan
    q = np.column_stack([rng.uniform(-100, 100, N), rng.uniform(-60, 60, N), rng.normal(10, 0.5, N)])
    out = rng.choice(N, N // 4, replace=False)
    q[out] = rng.uniform([-300, -200, -150], [300, 200, 200], (len(out), 3))
    q[3] = np.inf
    return r, q, ((-120.0, -80.0, -30.0), (120.0, 80.0, 80.0))


@pytest.mark.parametrize("P,N,max_dist,seed", [(1500, 900, np.inf, 1), (700, 2000, 25.0, 2), (300, 300, 3.0, 3)])
def test_the_yardstick_against_a_kd_tree(P, N, max_dist, seed):
    from scipy.spatial import cKDTree
    r, q, (lo, hi) = _scene(P, N, seed)
    got = distance_ref.distance(r, q, lo, hi, max_dist, (1.0, 5.0))
    member = normals_ref.members_of(r, lo, hi)
    assert np.array_equal(got["member"], member) and 0 < member.sum() < P
    counted = np.isfinite(q).all(axis=1)
    outside = counted & ~normals_ref.members_of(q, lo, hi)
    assert 0 < outside.sum() < counted.sum() < N                       # queries partly outside the box, one not counted
    assert (got["dist"][~counted] == -1.0).all() and (got["idx"][~counted] == -1).all()
    ids = np.flatnonzero(member)
    d, j = cKDTree(r[ids]).query(q[counted], k=1, distance_upper_bound=max_dist)
    found = np.isfinite(d)
    want_idx = np.where(found, ids[np.minimum(j, len(ids) - 1)], -1)
    assert np.array_equal(got["idx"][counted], want_idx)               # continuous coordinates: the nearest is unique
    assert np.array_equal(np.isfinite(got["dist"][counted]), found)
    if np.isfinite(max_dist):
        assert 0 < found.sum() < len(found)                            # the cap has queries on both sides
    # the tree's distance is sqrt of a sum of three squares in another order: each square carries the rounding of its
    # difference twice and its own (3 u), each of the two sums one more (2 u), the square root halves that and adds its
    # own: below 4 ulps for either side, 8 * 2^-52 between them -- the bound of test_cloud_outliers_host.py's yardstick
    assert np.allclose(got["dist"][counted][found], d[found], rtol=8 * 2.0 ** -52, atol=0)
    within = counted.copy()
    within[counted] = found
    assert got["counts"] == [int(counted.sum()), int(found.sum()), int((within & (got["dist"] < 1.0)).sum()),
                             int((within & (got["dist"] < 5.0)).sum())]
    assert got["counts"][1] >= got["counts"][3] >= got["counts"][2] > 0
    x = np.where(within, got["dist"], 0.0)
    assert got["stats"][0] == outliers_ref.tree_sum(x) and got["stats"][1] == got["stats"][0] / found.sum()
    assert np.isclose(got["stats"][1], d[found].mean(), rtol=1e-13)


def test_the_yardstick_on_cases_with_known_answers():
    box = ((-10, -10, -10), (10, 10, 10))
    D = distance_ref.distance
    # duplicates in the reference -> the smaller index; a 3-4-5 triangle: exact
    r = np.array([[50.0, 0, 0], [3.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0], [np.nan, 0, 0]])
    got = D(r, [[3.0, 0, 0], [0.0, 0, 0], [3.0, 4.0, 0.0]], *box)
    assert got["idx"].tolist() == [1, 1, 3] and got["dist"].tolist() == [0.0, 3.0, 3.0]
    assert got["counts"] == [3, 3] and got["stats"].tolist() == [(0.0 + 3.0) + (3.0 + 0.0), 6.0 / 3]
    got = D(r, [[3.0, -4.0, 0.0]], *box)
    assert got["idx"].tolist() == [1] and got["dist"].tolist() == [4.0]
    # the point outside the box would have been nearer: it is not found
    got = D(r, [[49.0, 0, 0]], *box)
    assert got["idx"].tolist() == [1] and got["dist"].tolist() == [46.0]
    # midway between two lattice points -> the smaller index, whichever comes first in the array
    lattice = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0], [2.0, 2.0, 0]])
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        got = D(lattice[perm], [[1.0, 0, 0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0]], *box)
        assert got["idx"].tolist() == [min(perm.index(0), perm.index(1)), 0, min(perm.index(1), perm.index(3))]
        assert got["dist"].tolist() == [1.0, np.sqrt(2.0), 1.0]
    # d2 exactly max_dist^2 -> within; one ulp more -> +inf
    got = D([[0.0, 0, 0]], [[3.0, 4.0, 0.0]], *box, max_dist=5.0)
    assert got["dist"].tolist() == [5.0] and got["counts"] == [1, 1]
    got = D([[0.0, 0, 0]], [[3.0, 4.0, 0.0]], *box, max_dist=np.nextafter(5.0, 0.0))
    assert got["dist"].tolist() == [np.inf] and got["idx"].tolist() == [-1] and got["counts"] == [1, 0]
    got = D([[0.0, 0, 0]], [[np.nextafter(3.0, 4.0), 4.0, 0.0]], *box, max_dist=5.0)
    assert got["dist"].tolist() == [np.inf]
    # max_dist = 0 -> only coincident points
    got = D(lattice, [[2.0, 2.0, 0.0], [2.0, 2.0, 5e-324], [1.0, 1.0, 1.0]], *box, max_dist=0.0, thresholds=(0.0, 1.0))
    assert got["dist"].tolist() == [0.0, 0.0, np.inf] and got["idx"].tolist() == [3, 3, -1]      # 5e-324 squared is 0
    assert got["counts"] == [3, 2, 0, 2] and got["stats"].tolist() == [0.0, 0.0]
    # M = 0: every counted query gets +inf; NaN / inf queries -> -1
    for ref in (np.zeros((0, 3)), [[50.0, 0, 0], [np.nan, 0, 0]]):
        got = D(ref, [[0.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, 0, 0]], *box, thresholds=(1.0,))
        assert got["dist"].tolist() == [np.inf, -1.0, -1.0, -1.0, np.inf] and (got["idx"] == -1).all()
        assert got["counts"] == [2, 0, 0] and got["stats"].tolist() == [0.0, 0.0]
    # no queries
    got = D(lattice, np.zeros((0, 3)), *box, thresholds=(1.0, 2.0))
    assert got["counts"] == [0, 0, 0, 0] and got["stats"].tolist() == [0.0, 0.0] and got["dist"].shape == (0,)
    # thresholds are strict
    got = D([[0.0, 0, 0]], [[1.0, 0, 0], [2.0, 0, 0], [0.0, 0, 0]], *box, thresholds=(0.0, 1.0, np.nextafter(1.0, 2.0), 2.0))
    assert got["counts"] == [3, 3, 0, 1, 2, 2]
    # a member on the box's face is one; one ulp outside is not
    got = D([[10.0, 0, 0], [np.nextafter(10.0, 11.0), 5.0, 0]], [[10.0, 5.0, 0.0]], *box)
    assert got["idx"].tolist() == [0] and got["dist"].tolist() == [5.0]
    assert distance_ref.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0 and distance_ref.lower_median([3.0, 1.0, 2.0]) == 2.0
    assert np.isnan(distance_ref.lower_median([]))


# ---------------------------------------------------------------- the Python layer, before any GPU work
def test_read_ply_returns_what_write_ply_wrote_bit_for_bit(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.normal(size=(257, 3)).astype(np.float32)
    xyz[0] = [np.nan, -0.0, np.inf]
    xyz.view(np.uint32)[1, 0] = 0x7FC12345                    # a NaN payload
    rgb = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    nrm = rng.normal(size=(257, 3)).astype(np.float32)
    path = str(tmp_path / "a.ply")
    fusion.write_ply(path, xyz, rgb)
    x, c, n = fusion.read_ply(path)
    assert n is None and x.dtype == np.float32 and x.tobytes() == xyz.tobytes() and c.dtype == np.uint8 and np.array_equal(c, rgb)
    fusion.write_ply(path, xyz, rgb, nrm)
    x, c, n = fusion.read_ply(path)
    assert x.tobytes() == xyz.tobytes() and np.array_equal(c, rgb) and n.dtype == np.float32 and n.tobytes() == nrm.tobytes()
    fusion.write_ply(path, xyz[:0], rgb[:0])
    x, c, n = fusion.read_ply(path)
    assert x.shape == (0, 3) and c.shape == (0, 3) and n is None


def _write(path, text, body=b""):
    with open(path, "wb") as f:
        f.write(text.encode("ascii") + body)
    return path


def test_read_ply_reads_ascii_doubles_extra_properties_and_ignores_later_elements(tmp_path):
    head = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty double x\nproperty double y\n"
            "property double z\nproperty float quality\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    path = _write(str(tmp_path / "a.ply"), head + "0 0.5 1 0.25 1 2 3\n1e-3 -2 3.25 0 255 0 7\n4 5 6 1 9 8 7\n3 0 1 2\n")
    x, c, n = fusion.read_ply(path)
    assert x.dtype == np.float64 and x.tolist() == [[0.0, 0.5, 1.0], [1e-3, -2.0, 3.25], [4.0, 5.0, 6.0]]
    assert c.tolist() == [[1, 2, 3], [255, 0, 7], [9, 8, 7]] and n is None
    # binary, properties in another order, a face element behind the vertices
    rec = np.zeros(2, dtype=[("nx", "<f4"), ("x", "<f8"), ("ny", "<f4"), ("y", "<f8"), ("nz", "<f4"), ("z", "<f8"), ("k", "<i2")])
    rec["x"], rec["y"], rec["z"] = [1.5, 2.5], [3.5, 4.5], [5.5, 6.5]
    rec["nx"], rec["ny"], rec["nz"] = [0, 1], [0, 0], [1, 0]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float nx\nproperty double x\nproperty float ny\n"
            "property double y\nproperty float nz\nproperty double z\nproperty short k\nelement face 1\n"
            "property list uchar int vertex_indices\nend_header\n")
    x, c, n = fusion.read_ply(_write(path, head, rec.tobytes() + b"\x03\x00\x00\x00\x00"))
    assert x.tolist() == [[1.5, 3.5, 5.5], [2.5, 4.5, 6.5]] and c is None and n.tolist() == [[0, 0, 1], [1, 0, 0]]


@pytest.mark.parametrize("text,body,message", [
    ("plx\nformat ascii 1.0\nelement vertex 0\nend_header\n", b"", "no PLY header"),
    ("ply\nformat ascii 1.0\nelement vertex 0\n", b"", "no PLY header"),
    ("ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
     b"", "binary_big_endian"),
    ("ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n", b"", "first element"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty list uchar float x\nend_header\n", b"", "scalar properties only"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty half x\nend_header\n", b"", "scalar properties only"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n1 2\n", b"", "x, y, z"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty double y\nproperty float z\nend_header\n1 2 3\n", b"",
     "one floating-point type"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty int x\nproperty int y\nproperty int z\nend_header\n1 2 3\n", b"",
     "floating-point"),
    ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n", b"",
     "vertex lines"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2\n", b"",
     "vertex lines"),
    ("ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
     b"\0" * 23, "24"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty float red\n"
     "property float green\nproperty float blue\nend_header\n1 2 3 4 5 6\n", b"", "uchar"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
     "end_header\n1 2 3 4\n", b"", "red, green, blue"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float x\nproperty float y\nproperty float z\n"
     "end_header\n1 2 3 4\n", b"", "declared twice"),
])
def test_read_ply_refuses_what_it_does_not_read(tmp_path, text, body, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        fusion.read_ply(_write(str(tmp_path / "bad.ply"), text, body))


def test_evaluate_clouds_arithmetic_on_a_hand_made_pair():
    """The reference's dict on two small clouds whose every number can be written down."""
    gt = np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [100.0, 0, 0]])
    pred = np.array([[0.0, 3.0, 0.0], [10.0, 0.0, 4.0], [20.0, 0.5, 0.0], [np.nan, 0, 0], [20.0, 0.0, 0.0]])
    got = distance_ref.evaluate(pred, gt, max_dist=20.0, thresholds=(1.0, 3.5))
    # accuracy: pred -> gt: 3, 4, 0.5, (not counted), 0; completeness: gt -> pred: 3, 4, 0, (80: beyond max_dist)
    assert got["accuracy"] == dict(mean=((3.0 + 4.0) + (0.5 + 0.0)) / 4, median=0.5, n=4, n_within=4, below=[2, 3])
    assert got["completeness"] == dict(mean=((3.0 + 4.0) + (0.0 + 0.0)) / 3, median=3.0, n=4, n_within=3, below=[1, 2])
    assert got["overall"] == (7.5 / 4 + 7.0 / 3) / 2
    assert got["precision"] == [0.5, 0.75] and got["recall"] == [0.25, 0.5]
    assert got["fscore"] == [2 * 0.5 * 0.25 / 0.75, 2 * 0.75 * 0.5 / 1.25]
    assert got["max_dist"] == 20.0 and got["thresholds"] == [1.0, 3.5]
    # nothing within anything: means 0, medians NaN, F-score 0 without a division by zero
    got = distance_ref.evaluate(pred[:1], gt[3:], max_dist=1.0, thresholds=(1.0,))
    assert got["accuracy"]["mean"] == 0.0 and np.isnan(got["accuracy"]["median"]) and got["fscore"] == [0.0]
    got = distance_ref.evaluate(np.zeros((0, 3)), gt, thresholds=(1.0,))
    assert got["accuracy"]["n"] == 0 and got["precision"] == [0.0] and got["completeness"]["n_within"] == 0


def test_the_cell_rule_stays_within_its_budget():
    for box, P in ((BIN, 1 << 20), (BIN, 1), (BIN, 0), (((0, 0, 0), (1e6, 1e-3, 1.0)), 1 << 22), (((0, 0, 0), (1.0, 1.0, 0.0)), 5000),
                   (((-1e9, -1e9, -1e9), (1e9, 1e9, 1e9)), (1 << 31) - 1)):
        cell = fusion.distance_cell(box, P)
        n = normals_ref.grid_shape(*box, cell)
        assert cell > 0 and n[0] * n[1] * n[2] <= fusion.DISTANCE_CELL_BUDGET, (box, P, cell, n)
        _lib.query_distance_workspace(P, 1, *box, cell)               # the library admits it
    assert fusion.distance_cell(((1.0, 2.0, 3.0), (1.0, 2.0, 3.0)), 77) == 1.0
    n = normals_ref.grid_shape(*BIN, fusion.distance_cell(BIN, 1 << 20))
    assert (1 << 17) < n[0] * n[1] * n[2] < (1 << 20)                 # about one cell per two points


def test_python_functions_refuse_host_tensors_and_bad_options():
    import torch
    xyz = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        _lib.cloud_distance(xyz, xyz, *BIN, 5.0, 20.0, ())
    with pytest.raises(RuntimeError, match="query must be a CUDA"):
        fusion.cloud_distance(xyz, xyz)
    with pytest.raises(RuntimeError, match="CUDA"):
        fusion.evaluate_cloud(xyz, xyz)
    for argv in (["--box", "0", "0", "0", "1", "1", "1"], ["--json", "x.json"], ["--gt_ply", "g.ply", "--thresholds"] + ["1"] * 9):
        with pytest.raises(SystemExit):     # the score options without a ground truth are refused while the arguments are parsed
            reconstruct.main(["--testpath", "x", "--testlist", "y", "--loadckpt", "z"] + argv)
    with pytest.raises(SystemExit):
        eval_cloud.main(["--pred", "a.ply"])
    with pytest.raises(SystemExit):
        eval_cloud.main(["--pred", "a.ply", "--gt", "b.ply", "--thresholds"] + ["1"] * 9)


def test_the_command_lines_take_the_score_flags(monkeypatch, tmp_path):
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def parse(self, argv=None):
        args = real(self, argv)
        seen.update(vars(args))
        return args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    common = ["--testpath", "/nonexistent/x", "--testlist", "/nonexistent/y", "--loadckpt", "/nonexistent/z"]
    with pytest.raises(Exception):          # there is no dataset at x: whatever stops the run, the arguments were parsed
        reconstruct.main(common + ["--gt_ply", "gt_{scan}.ply", "--max_dist", "7.5", "--thresholds", "0.5", "1", "--box", "0",
                                   "1", "2", "3", "4", "5", "--cell", "2", "--json", "out.json"])
    assert seen["gt_ply"] == "gt_{scan}.ply" and seen["max_dist"] == 7.5 and seen["thresholds"] == [0.5, 1.0]
    assert seen["box"] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and seen["cell"] == 2.0 and seen["json"] == "out.json"
    seen.clear()
    with pytest.raises(Exception):
        reconstruct.main(common)
    assert seen["gt_ply"] is None and seen["max_dist"] == 20.0 and tuple(seen["thresholds"]) == (1.0, 2.0, 5.0)
    assert seen["box"] is None and seen["cell"] is None and seen["json"] is None
    seen.clear()
    with pytest.raises(Exception):          # no such file
        eval_cloud.main(["--pred", str(tmp_path / "none.ply"), "--gt", str(tmp_path / "none2.ply"), "--max_dist", "3",
                         "--thresholds", "0.25", "--json", str(tmp_path / "o.json")])
    assert seen["pred"].endswith("none.ply") and seen["max_dist"] == 3.0 and seen["thresholds"] == [0.25]
    assert seen["box"] is None and seen["json"].endswith("o.json")
