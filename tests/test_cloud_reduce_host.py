"""Host-side checks of DTU's point reduction, observability mask and plane (include/mvs_reduce_abi.h,
csrc/cloud_reduce.hip, tests/reduce_ref.py, fusion.read_obs_mask / read_plane, the command lines): none needs a GPU.
Every refusal is decided before the first HIP call, so the fake device pointers are never dereferenced; the refusals run
in a child process that sees no device (HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty), where a call the library
failed to refuse would come back as MVS_ERR_HIP (4) instead of reaching hardware."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for path in (REPO, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import normals_ref  # noqa: E402
import reduce_ref as RR  # noqa: E402
import refusals  # noqa: E402

from refusals import BAD_DTYPE, BAD_SHAPE, BIN, HIP, INF, NAN, NULL, OK, WORKSPACE  # noqa: E402

# ---------------------------------------------------------------- the refusal cases (shared by the child and the tests)
GOOD = dict(dtype=0, P=5000, box_min=BIN[0], box_max=BIN[1], cell=5.0, min_dist=0.2, seed=0, max_rounds=64)
CASES = [(f"null {p}", {p: None}, NULL, "NULL") for p in ("xyz", "box_min", "box_max", "keep_out", "counts_out", "workspace")]
CASES += [
    ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"),
    ("P = 2^31 - 1 is legal", dict(P=(1 << 31) - 1, workspace_bytes=0), WORKSPACE, "workspace"),
    ("min_dist nan", dict(min_dist=NAN), BAD_SHAPE, "min_dist"),
    ("min_dist < 0", dict(min_dist=-0.2), BAD_SHAPE, "min_dist"),
    ("min_dist inf", dict(min_dist=INF), BAD_SHAPE, "min_dist"),
    ("min_dist -inf", dict(min_dist=-INF), BAD_SHAPE, "min_dist"),
    ("min_dist 0 is legal", dict(min_dist=0.0, workspace_bytes=0), WORKSPACE, "workspace"),
    ("min_dist 1e300 is legal", dict(min_dist=1e300, workspace_bytes=0), WORKSPACE, "workspace"),
    ("max_rounds 0", dict(max_rounds=0), BAD_SHAPE, "max_rounds = 0"),
    ("max_rounds -1", dict(max_rounds=-1), BAD_SHAPE, "max_rounds = -1"),
    ("max_rounds 257", dict(max_rounds=257), BAD_SHAPE, "max_rounds = 257"),
    ("max_rounds 1 is legal", dict(max_rounds=1, workspace_bytes=0), WORKSPACE, "workspace"),
    ("max_rounds 256 is legal", dict(max_rounds=256, workspace_bytes=0), WORKSPACE, "workspace"),
    ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("cell < 0", dict(cell=-5.0), BAD_SHAPE, "cell"),
    ("cell nan", dict(cell=NAN), BAD_SHAPE, "cell"),
    ("cell inf", dict(cell=INF), BAD_SHAPE, "cell"),
    ("box nan", dict(box_min=(NAN, 0, 0)), BAD_SHAPE, "box axis 0"),
    ("box -inf", dict(box_min=(0, -INF, 0)), BAD_SHAPE, "box axis 1"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("1290^3 cells are legal", dict(box_min=(0, 0, 0), box_max=(1289, 1289, 1289), cell=1.0, workspace_bytes=0), WORKSPACE, "workspace"),
    ("one axis of 3e9", dict(box_min=(0, 0, 0), box_max=(3e9, 0, 0), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("dtype 2", dict(dtype=2), BAD_DTYPE, "dtype 2"),
    ("dtype -1", dict(dtype=-1), BAD_DTYPE, "dtype -1"),
    ("one byte short", dict(workspace_bytes="need-1"), WORKSPACE, "workspace"),
    ("the normals' size is too small", dict(workspace_bytes="normals"), WORKSPACE, "workspace"),
    ("no workspace", dict(workspace_bytes=0), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace_bytes="need", workspace="plus4"), WORKSPACE, "aligned"),
    ("everything right reaches HIP", dict(workspace_bytes="need"), HIP, ""),
    ("f64 reaches HIP", dict(workspace_bytes="need", dtype=1), HIP, ""),
    ("the largest seed reaches HIP", dict(workspace_bytes="need", seed=(1 << 64) - 1), HIP, ""),
    ("P == 0 reaches HIP", dict(P=0, workspace_bytes="need"), HIP, ""),
]
Q_CASES = [
    ("null box_min", dict(box_min=None), NULL, "NULL"), ("null box_max", dict(box_max=None), NULL, "NULL"),
    ("null bytes", dict(bytes=None), NULL, "NULL"), ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"), ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("cell nan", dict(cell=NAN), BAD_SHAPE, "cell"), ("cell inf", dict(cell=INF), BAD_SHAPE, "cell"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("fine", dict(), OK, ""), ("P == 0 is fine", dict(P=0), OK, ""), ("P = 2^31 - 1 is fine", dict(P=(1 << 31) - 1), OK, ""),
]
S_GOOD = dict(dtype=0, P=5000, n=(12, 10, 8), origin=(-3.0, 2.0, 0.5), res=10.0, plane=(0.0, 0.0, 1.0, -2.0))
S_CASES = [(f"null {p}", {p: None}, NULL, "NULL") for p in ("xyz", "keep_out", "counts_out")]
S_CASES += [
    ("a mask with a null n", dict(n=None), NULL, "NULL n or origin"),
    ("a mask with a null origin", dict(origin=None), NULL, "NULL n or origin"),
    ("no mask: n and origin may be NULL", dict(obs_mask=None, n=None, origin=None), HIP, ""),
    ("no plane", dict(plane=None), HIP, ""),
    ("neither", dict(obs_mask=None, n=None, origin=None, plane=None), HIP, ""),
    ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"),
    ("P = 2^31 - 1 reaches HIP", dict(P=(1 << 31) - 1), HIP, ""),
    ("P == 0 reaches HIP", dict(P=0), HIP, ""),
    ("n[1] = 0", dict(n=(12, 0, 8)), BAD_SHAPE, "n[1] = 0"),
    ("n[2] < 0", dict(n=(12, 10, -8)), BAD_SHAPE, "n[2] = -8"),
    ("2^31 voxels", dict(n=(1 << 11, 1 << 10, 1 << 10)), BAD_SHAPE, "2^31 voxels"),
    ("2^31 - 1 voxels reach HIP", dict(n=((1 << 31) - 1, 1, 1)), HIP, ""),
    ("one voxel reaches HIP", dict(n=(1, 1, 1)), HIP, ""),
    ("res 0", dict(res=0.0), BAD_SHAPE, "res"),
    ("res < 0", dict(res=-10.0), BAD_SHAPE, "res"),
    ("res nan", dict(res=NAN), BAD_SHAPE, "res"),
    ("res inf", dict(res=INF), BAD_SHAPE, "res"),
    ("res 0 without a mask", dict(res=0.0, obs_mask=None, n=None, origin=None), BAD_SHAPE, "res"),
    ("origin nan", dict(origin=(0.0, NAN, 0.0)), BAD_SHAPE, "origin[1]"),
    ("origin inf", dict(origin=(0.0, 0.0, -INF)), BAD_SHAPE, "origin[2]"),
    ("plane nan", dict(plane=(NAN, 0.0, 1.0, 0.0)), BAD_SHAPE, "plane[0]"),
    ("plane inf", dict(plane=(0.0, 0.0, 1.0, INF)), BAD_SHAPE, "plane[3]"),
    ("dtype 2", dict(dtype=2), BAD_DTYPE, "dtype 2"),
    ("dtype -1", dict(dtype=-1), BAD_DTYPE, "dtype -1"),
    ("everything right reaches HIP", dict(), HIP, ""),
    ("f64 reaches HIP", dict(dtype=1), HIP, ""),
]


def _bytes_of(ref):
    return lambda a: ref.workspace_bytes(a["P"], a["box_min"], a["box_max"], a["cell"])


REFUSALS = {
    "mvs_cloud_reduce": dict(good=GOOD, host=refusals.BOX, cases=CASES,
                             sizes=dict(need=_bytes_of(RR), normals=_bytes_of(normals_ref))),
    "mvs_query_reduce_workspace": dict(good=GOOD, host=refusals.BOX, cases=Q_CASES),
    "mvs_cloud_select": dict(good=S_GOOD, host=dict(n=ctypes.c_int, origin=ctypes.c_double, plane=ctypes.c_double),
                             optional=("obs_mask", "plane"), cases=S_CASES),
}


@pytest.mark.parametrize("ep,cases", [("reduce", CASES), ("query", Q_CASES), ("select", S_CASES)])
def test_every_refusal_comes_with_its_status_and_its_message(ep, cases):
    name, = [n for n, spec in REFUSALS.items() if spec["cases"] is cases and ep in n]
    refusals.check(sys.modules[__name__], (name,))


# ---------------------------------------------------------------- declarations
from scene_3dreconstruction_mvsnet_amd import _lib, eval_cloud, fusion, reconstruct  # noqa: E402


def test_reduce_symbols_are_the_declarations_of_the_reduce_header():
    src = refusals.check_header("mvs_reduce_abi.h", _lib.REDUCE_SYMBOLS)
    assert list(_lib.REDUCE_SYMBOLS) == ["mvs_query_reduce_workspace", "mvs_cloud_reduce", "mvs_cloud_select"]
    assert '#include "mvs_abi.h"' in src and '#include "mvs_normals_abi.h"' in src
    assert refusals.define(src, "MVS_REDUCE_ROUNDS_MAX") == 256 == _lib.REDUCE_ROUNDS_MAX == RR.ROUNDS_MAX
    assert "Likewise include/mvs_reduce_abi.h" in refusals.header_text("mvs_abi.h")
    # what is still not DTU's is said where the contract is
    assert "randperm is replaced by the hash" in src and "nothing here was compared against the MATLAB code" in src
    assert "per-scan tables are not built" in src


# ---------------------------------------------------------------- workspace formula
@pytest.mark.parametrize("P,lo,hi,cell", [(5000, BIN[0], BIN[1], 5.0), (0, BIN[0], BIN[1], 5.0), (1, BIN[0], BIN[1], 2.5),
                                          (7, BIN[0], BIN[1], 2.5), (4097, (-300, -200, -50), (300, 200, 150), 7.3),
                                          (3, (0, 0, 0), (0, 0, 0), 1.0), ((1 << 31) - 1, (0, 0, 0), (1289, 1289, 1289), 1.0)])
def test_reduce_workspace_query_agrees_with_the_headers_formula(P, lo, hi, cell):
    want = RR.workspace_bytes(P, lo, hi, cell)
    assert _lib.query_reduce_workspace(P, lo, hi, cell) == want and want % 8 == 0
    # the grid part is exactly the normals' query; the rest is one 32-bit word per point and the counters
    assert want - _lib.query_normals_workspace(P, lo, hi, cell) == 8 * ((P + 1) // 2) + 8 * (256 + 2)
    with pytest.raises(_lib.MvsError) as e:
        _lib.query_reduce_workspace(P, (0, 0, 0), (1290, 1290, 1290), 1.0)      # 1291^3 >= 2^31
    assert e.value.code == BAD_SHAPE


# ---------------------------------------------------------------- the yardstick
def test_the_keys_are_splitmix64():
    assert tuple(int(k) for k in RR.keys(3, 0)) == RR.FIRST_KEYS_SEED0 == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4,
                                                                           0x06C45D188009454F)
    # the stream does not depend on how many keys are drawn, and another seed is another stream
    assert np.array_equal(RR.keys(1000, 7)[:10], RR.keys(10, 7)) and not np.array_equal(RR.keys(10, 7), RR.keys(10, 8))
    # seed + (i + 1) * golden: seed = golden at i is seed = 0 at i + 1, and the sum wraps modulo 2^64
    assert np.array_equal(RR.keys(5, 0x9E3779B97F4A7C15), RR.keys(6, 0)[1:])
    assert int(RR.keys(1, (1 << 64) - 0x9E3779B97F4A7C15)[0]) == 0          # z = 0 stays 0 through every step
    assert len(set(RR.keys(100000, 0).tolist())) == 100000


def _independent_and_maximal(xyz, mask, lo, hi, min_dist):
    """By brute force, without the keys: no two kept members are near; every removed member has a kept near member."""
    p = np.asarray(xyz, np.float64)
    member = normals_ref.members_of(p, lo, hi)
    assert not mask[~member].any()
    m = p[member]
    k = mask[member]
    with np.errstate(over="ignore"):
        d = m[None, :, :] - m[:, None, :]
        near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= np.float64(min_dist) * np.float64(min_dist)
    np.fill_diagonal(near, False)
    assert not near[np.ix_(k, k)].any(), "two kept members are near"
    assert near[np.ix_(~k, k)].any(axis=1).all(), "a removed member has no kept near member"


def _clouds():
    rng = np.random.default_rng(11)
    box = ((0.0, 0.0, 0.0), (5.0, 5.0, 1.0))
    surface = np.column_stack([rng.uniform(-0.2, 5.2, 1500), rng.uniform(-0.2, 5.2, 1500), rng.uniform(0.4, 0.6, 1500)])
    surface[3] = np.nan
    surface[4, 1] = np.inf
    for min_dist in (0.05, 0.15, 0.4):
        yield f"surface {min_dist}", surface, box, min_dist
    f32 = surface.astype(np.float32)
    yield "float32 input", f32, box, 0.15
    gx, gy, gz = np.meshgrid(np.arange(12) * 0.25, np.arange(10) * 0.25, np.arange(3) * 0.25, indexing="ij")
    lattice = np.column_stack([gx.ravel(), gy.ravel(), gz.ravel()])
    yield "lattice at its spacing", lattice, box, 0.25                    # the bound is inclusive: the 6 neighbours are near
    yield "lattice one ulp below", lattice, box, float(np.nextafter(0.25, 0.0))      # nobody is near
    dup = np.vstack([surface[:300], surface[100:250], surface[100:150]])
    yield "duplicates", dup, box, 0.1
    yield "duplicates at 0", dup, box, 0.0
    yield "one cell", surface[:200], box, 100.0                           # everybody is near everybody: one survivor
    yield "nothing", np.zeros((0, 3)), box, 0.2
    yield "no members", surface[:50] + 100.0, box, 0.2


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D])
def test_the_rounds_reach_the_sequential_greedy_mask(seed):
    for what, xyz, (lo, hi), min_dist in _clouds():
        want, n_kept = RR.reduce_sequential(xyz, lo, hi, min_dist, seed)
        mask, counts = RR.reduce_rounds(xyz, lo, hi, min_dist, seed, max_rounds=64)
        member = normals_ref.members_of(xyz, lo, hi)
        print(what, counts)
        assert np.array_equal(mask, want), what
        assert counts[:3] == [int(member.sum()), n_kept, 0] and counts[1] == mask.sum(), what
        assert counts[3] == RR.depth(xyz, lo, hi, min_dist, seed) <= 16, what
        assert (counts[3] == 0) == (counts[0] == 0), what
        _independent_and_maximal(xyz, mask, lo, hi, min_dist)
        if what == "lattice one ulp below" or what == "nothing":
            assert counts[1] == counts[0] and counts[3] == (1 if counts[0] else 0)
        if what == "lattice at its spacing":
            assert counts[1] < counts[0] // 2
        if what == "one cell":
            assert counts[1] == 1 and counts[3] == 2                      # round 1 keeps the smallest key, round 2 removes the rest
            ids = np.flatnonzero(member)
            h = RR.keys(len(xyz), seed)[ids]
            assert mask[ids[np.lexsort((ids, h))[0]]]
        if what == "duplicates at 0":
            first = {}
            ids = np.flatnonzero(member)
            h = RR.keys(len(xyz), seed)
            for i in sorted(ids, key=lambda i: (int(h[i]), i)):
                first.setdefault(np.asarray(xyz[i], np.float64).tobytes(), i)
            assert sorted(first.values()) == np.flatnonzero(mask).tolist()      # exactly the duplicates of a lower key go


def test_a_cap_on_the_rounds_leaves_the_rest_undecided():
    _, xyz, (lo, hi), min_dist = next(c for c in _clouds() if c[0] == "surface 0.15")
    full, counts = RR.reduce_rounds(xyz, lo, hi, min_dist)
    assert counts[3] >= 5 and counts[2] == 0
    last = None
    for cap in (1, 2, 3, counts[3] - 1, counts[3], counts[3] + 1):
        mask, c = RR.reduce_rounds(xyz, lo, hi, min_dist, max_rounds=cap)
        assert c[3] == min(cap, counts[3]) and (c[2] == 0) == (cap >= counts[3]) and c[0] == counts[0]
        assert not (mask & ~full).any() and c[1] == mask.sum()          # what is kept early stays kept
        assert last is None or (c[1] >= last[1] and c[2] <= last[2])
        last = c
    assert np.array_equal(mask, full)


def test_select_on_cases_with_known_answers():
    mask = np.zeros((3, 4, 5), np.uint8)
    mask[1, 2, 3] = mask[0, 0, 0] = mask[2, 3, 4] = 1
    obs = dict(mask=mask, origin=(10.0, 20.0, 30.0), res=2.0)
    pts = np.array([[12.0, 24.0, 36.0],        # voxel (1, 2, 3): set
                    [13.0, 24.0, 36.0],        # x offset 1.5 -> 2: (2, 2, 3) is not set
                    [12.999, 24.0, 36.0],      # 1.4995 -> 1
                    [11.0, 25.0, 37.0],        # 0.5, 2.5, 3.5 -> 1, 3, 4: not set
                    [9.0, 20.0, 30.0],         # -0.5 -> -1: outside
                    [9.001, 19.001, 29.001],   # -0.4995 -> -0 = 0: voxel (0, 0, 0)
                    [14.0, 26.0, 38.0],        # the last voxel (2, 3, 4)
                    [15.0, 26.0, 38.0],        # 2.5 -> 3: one voxel outside
                    [14.0, 28.0, 38.0], [14.0, 26.0, 40.0], [np.nan, 24.0, 36.0], [12.0, np.inf, 36.0]])
    keep, counts = RR.select(pts, obs_mask=obs)
    assert keep.tolist() == [True, False, True, False, False, True, True, False, False, False, False, False]
    assert counts == [10, 4, 4]
    assert RR.mround([0.5, -0.5, 1.5, -1.5, 2.4999, -0.4999, 0.0]).tolist() == [1.0, -1.0, 2.0, -2.0, 2.0, -0.0, 0.0]
    plane = (0.0, 0.0, 1.0, -36.0)             # z > 36, strictly
    keep, counts = RR.select(pts, plane=plane)
    assert keep.tolist() == [False, False, False, True, False, False, True, True, True, True, False, False]
    assert counts == [10, 10, 5]
    keep, counts = RR.select(pts, obs_mask=obs, plane=plane)
    assert keep.tolist() == [False] * 6 + [True] + [False] * 5 and counts == [10, 4, 1]
    keep, counts = RR.select(pts)
    assert keep.tolist() == [True] * 10 + [False] * 2 and counts == [10, 10, 10]
    assert RR.select(np.zeros((0, 3)), obs_mask=obs, plane=plane)[1] == [0, 0, 0]


def test_evaluate_with_the_options_on_a_hand_made_pair():
    gt = np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [20.0, 0, -5.0]])
    pred = np.array([[0.0, 3.0, 0.0], [0.0, 3.0, 0.0], [10.0, 0.0, 4.0], [20.0, 0.5, 0.0], [np.nan, 0, 0]])
    plain = RR.evaluate(pred, gt, thresholds=(1.0, 3.5))
    assert "reduction" not in plain and plain["accuracy"]["n"] == 4
    got = RR.evaluate(pred, gt, thresholds=(1.0, 3.5), reduce=dict(min_dist=0.1), plane=(0.0, 0.0, 1.0, 1.0))
    assert got["reduction"] == dict(pred=[4, 3, 0, 2]) and got["selection"] == dict(accuracy=[3, 3, 3], completeness=[4, 4, 3])
    assert got["accuracy"]["n"] == 3 and got["accuracy"]["mean"] == (3.0 + 4.0 + 0.5) / 3
    assert got["completeness"]["n"] == 3 and got["completeness"]["mean"] == (3.0 + 4.0 + 0.5) / 3      # (20, 0, -5) is below
    mask = np.ones((3, 1, 1), np.uint8)
    mask[1] = 0                                 # the voxel around x = 10 was not observed
    got = RR.evaluate(pred, gt, thresholds=(1.0,), obs_mask=dict(mask=mask, origin=(0.0, 0.0, 0.0), res=10.0))
    assert got["selection"]["accuracy"] == [4, 3, 3] and got["accuracy"]["n"] == 3 and got["completeness"]["n"] == 4
    assert got["reduction"] == {}
    both = RR.evaluate(pred, gt, thresholds=(1.0,), reduce=dict(min_dist=6.0, gt=True))
    assert both["reduction"]["gt"][:3] == [4, 3, 0] and both["completeness"]["n"] == 3


# ---------------------------------------------------------------- the Python layer, before any GPU work
def test_read_obs_mask_and_read_plane_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 2, (12, 10, 8)).astype(bool)
    bb = np.array([[-71.5, -120.25, 500.0], [1.0, 2.0, 3.0]])
    plane = np.array([0.1, -0.2, 0.97, -640.5])
    path = str(tmp_path / "ObsMask1_10.npz")
    np.savez(path, ObsMask=np.asfortranarray(mask), BB=bb, Res=np.float64(10.0))
    got = fusion.read_obs_mask(path)
    assert got["mask"].dtype == np.uint8 and got["mask"].flags.c_contiguous and np.array_equal(got["mask"], mask.astype(np.uint8))
    assert got["origin"].tolist() == bb[0].tolist() and got["res"] == 10.0 and type(got["res"]) is float
    np.savez(str(tmp_path / "Plane1.npz"), P=plane.reshape(4, 1))
    assert fusion.read_plane(str(tmp_path / "Plane1.npz")).tolist() == plane.tolist()
    with pytest.raises(ValueError, match="BB"):
        np.savez(str(tmp_path / "bad.npz"), ObsMask=mask, Res=10.0)
        fusion.read_obs_mask(str(tmp_path / "bad.npz"))
    with pytest.raises(ValueError, match="need 4"):
        np.savez(str(tmp_path / "bad2.npz"), P=plane[:3])
        fusion.read_plane(str(tmp_path / "bad2.npz"))
    with pytest.raises(ValueError, match="neither"):
        fusion.read_plane(str(tmp_path / "plane.txt"))


def test_read_obs_mask_and_read_plane_read_matlab_files(tmp_path):
    sio = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(6)
    mask = rng.integers(0, 2, (5, 7, 3)).astype(bool)
    bb = np.array([[-71.5, -120.25, 500.0], [1.0, 2.0, 3.0]])
    plane = np.array([0.1, -0.2, 0.97, -640.5])
    sio.savemat(str(tmp_path / "ObsMask1_10.mat"), dict(ObsMask=mask, BB=bb, Res=10.0))       # MATLAB: logical, 2x3, 1x1
    sio.savemat(str(tmp_path / "Plane1.mat"), dict(P=plane.reshape(4, 1)))
    got = fusion.read_obs_mask(str(tmp_path / "ObsMask1_10.mat"))
    assert got["mask"].dtype == np.uint8 and got["mask"].flags.c_contiguous and np.array_equal(got["mask"], mask.astype(np.uint8))
    assert got["origin"].tolist() == bb[0].tolist() and got["res"] == 10.0
    assert fusion.read_plane(str(tmp_path / "Plane1.mat")).tolist() == plane.tolist()


def test_the_cell_rule_of_the_reduction_stays_within_the_budget():
    for box, P, min_dist in ((BIN, 1 << 22, 0.2), (BIN, 1, 0.2), (BIN, 0, 0.0), (((0, 0, 0), (1e6, 1e-3, 1.0)), 1 << 22, 1e-6),
                             (BIN, 5000, 1e4), (((1.0, 2.0, 3.0), (1.0, 2.0, 3.0)), 77, 0.2)):
        cell = fusion.reduce_cell(box, P, min_dist)
        n = normals_ref.grid_shape(*box, cell)
        assert cell >= min_dist and cell > 0 and n[0] * n[1] * n[2] <= fusion.DISTANCE_CELL_BUDGET, (box, P, min_dist, cell, n)
        _lib.query_reduce_workspace(P, *box, cell)                    # the library admits it
    assert fusion.reduce_cell(BIN, 5000, 1e4) == 1e4 and fusion.reduce_cell(BIN, 1 << 22, 0.2) > 0.2


def test_python_functions_refuse_host_tensors_and_bad_options():
    import torch
    xyz = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        _lib.cloud_reduce(xyz, *BIN, 5.0, 0.2)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        _lib.cloud_select(xyz)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        fusion.reduce_cloud(xyz)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        fusion.select_cloud(xyz, plane=(0, 0, 1, 0))
    for kw in (dict(reduce=dict(min_dist=0.2)), dict(plane=(0.0, 0.0, 1.0, 0.0)),
               dict(obs_mask=dict(mask=np.ones((2, 2, 2), np.uint8), origin=(0, 0, 0), res=1.0)), dict()):
        with pytest.raises(RuntimeError, match="CUDA"):             # the new keywords are refused like the old ones
            fusion.evaluate_cloud(xyz, xyz, **kw)
    common = ["--testpath", "x", "--testlist", "y", "--loadckpt", "z"]
    for argv in (["--reduce_dist", "0.2"], ["--obs_mask", "m.npz"], ["--plane", "p.npz"],
                 ["--gt_ply", "g.ply", "--reduce_gt"], ["--gt_ply", "g.ply", "--reduce_seed", "3"]):
        with pytest.raises(SystemExit):     # the DTU options without a ground truth, or without a reduction to apply them to
            reconstruct.main(common + argv)


def test_the_command_lines_take_the_dtu_flags(monkeypatch, tmp_path):
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def parse(self, argv=None):
        args = real(self, argv)
        seen.update(vars(args))
        return args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    with pytest.raises(Exception):          # no such file: whatever stops the run, the arguments were parsed
        eval_cloud.main(["--pred", str(tmp_path / "none.ply"), "--gt", str(tmp_path / "none2.ply"), "--reduce_dist", "0.2",
                         "--reduce_seed", "7", "--reduce_gt", "--obs_mask", "m.npz", "--plane", "p.mat"])
    assert seen["reduce_dist"] == 0.2 and seen["reduce_seed"] == 7 and seen["reduce_gt"] is True
    assert seen["obs_mask"] == "m.npz" and seen["plane"] == "p.mat"
    seen.clear()
    with pytest.raises(Exception):
        eval_cloud.main(["--pred", str(tmp_path / "none.ply"), "--gt", str(tmp_path / "none2.ply")])
    assert seen["reduce_dist"] is None and seen["reduce_seed"] == 0 and seen["reduce_gt"] is False
    assert seen["obs_mask"] is None and seen["plane"] is None
    # the keywords the options turn into; {scan} in the two file names
    np.savez(str(tmp_path / "Plane_scan9.npz"), P=np.array([0.0, 0.0, 1.0, -2.0]))
    args = argparse.Namespace(reduce_dist=0.2, reduce_seed=7, reduce_gt=True, obs_mask=None, plane=str(tmp_path / "Plane_{scan}.npz"))
    kw = eval_cloud.dtu_options(args, scan="scan9")
    assert kw["reduce"] == dict(min_dist=0.2, seed=7, gt=True) and kw["obs_mask"] is None
    assert kw["plane"].tolist() == [0.0, 0.0, 1.0, -2.0]
    none = argparse.Namespace(reduce_dist=None, reduce_seed=0, reduce_gt=False, obs_mask=None, plane=None)
    assert eval_cloud.dtu_options(none) == dict(reduce=None, obs_mask=None, plane=None)
