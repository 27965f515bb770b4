"""mvs_cloud_normals / mvs_cloud_downsample_normals / fusion.estimate_normals / reconstruct_scan(downsample=dict(normals=...))
on the GPU, held to tests/normals_ref.py: the neighbour indices and the three counts exactly, the normals within the angle
bound normals_ref derives (eigenvector perturbation over the gap + float32 rounding), the Rayleigh quotient and the sign
rule for every member without exception.  The buffers of the two entry points lie between guards and are poisoned."""
import functools
import os

import numpy as np
import pytest
import torch

import cloud_ref
import guarded as G
from cloud_testing import DEV, assert_guarded_coverage, cu, dataset, read_ply
import normals_ref as NR
from conftest import load_weights
from scene_3dreconstruction_mvsnet_amd import _lib, fusion

pytestmark = pytest.mark.gpu
BOX = ((-290.0, -190.0, -60.0), (290.0, 190.0, 160.0))        # inside the 600 x 400 scene: some points fall out
DTYPES = {"f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def noisy_scene(P, seed=0):
    """Half the points on the plane z = 0 of a 600 x 400 footprint, half on a hemisphere of radius 100 standing on it,
    0.3 units of Gaussian noise, rounded to float32 -> float32 [P,3] (read-only)."""
    rng = np.random.default_rng(seed)
    half = P // 2
    plane = np.column_stack([rng.uniform(-300, 300, half), rng.uniform(-200, 200, half), np.zeros(half)])
    d = rng.normal(size=(P - half, 3))
    d[:, 2] = np.abs(d[:, 2])
    dome = 100.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (np.vstack([plane, dome]) + rng.normal(0.0, 0.3, (P, 3)))[rng.permutation(P)].astype(np.float32)
    xyz.setflags(write=False)
    return xyz


CAMERAS = dict(view_starts=lambda P: [0, P // 3, P], centres=[[0.0, 0.0, 500.0], [0.0, 0.0, -500.0]])


@functools.lru_cache(maxsize=None)
def scene_ref(P, knn, cameras=False):
    kw = dict(view_starts=CAMERAS["view_starts"](P), centres=CAMERAS["centres"]) if cameras else {}
    return NR.estimate(noisy_scene(P), *BOX, knn, **kw)


def run(xyz, box, knn, cell=5.0, view_starts=None, centres=None, nbr=True):
    """-> (normals float32 [P,3], nbr int32 [P,knn], counts list) as numpy, through the ctypes wrapper."""
    vs = None if view_starts is None else cu(np.asarray(view_starts, np.int64))
    ct = None if centres is None else cu(np.asarray(centres, np.float64))
    n, b, c = _lib.cloud_normals(cu(xyz), box[0], box[1], cell=cell, knn=knn, view_starts=vs, centres=ct, neighbours=nbr)
    torch.cuda.synchronize()
    return n.cpu().numpy(), (b.cpu().numpy() if nbr else None), c.tolist()


def assert_exact(got, want, what):
    n, b, c = got
    assert c == want["counts"], (what, c, want["counts"])
    assert b.dtype == np.int32 and b.shape == want["nbr"].shape
    bad = np.flatnonzero((b != want["nbr"]).any(axis=1))
    assert bad.size == 0, (what, f"{bad.size} rows of neighbours differ, first {bad[0]}: {b[bad[0]].tolist()} / "
                                 f"{want['nbr'][bad[0]].tolist()}")
    assert n.dtype == np.float32 and (n[~want["member"]].view(np.uint32) == 0).all(), what       # exact +0.0
    assert np.isfinite(n).all()


def assert_normals(n, want, xyz, what, view_starts=None, centres=None):
    """Unit length, Rayleigh quotient, sign rule for every member; the angle wherever the gap allows."""
    mem = np.flatnonzero(want["member"])
    v = n[mem].astype(np.float64)
    length = np.linalg.norm(v, axis=1)
    # three components rounded to float32, each by at most 2^-25, of a vector that is a unit vector to a few 2^-53
    assert (np.abs(length - 1.0) <= np.sqrt(3) * 2.0 ** -25 + 2.0 ** -50).all(), (what, np.abs(length - 1).max())
    live = ~want["degenerate"][mem]
    C, w = want["cov"][mem], want["eig"][mem]
    rq = np.einsum("pi,pij,pj->p", v, C, v) / (length * length)
    over = live & (rq > w[:, 0] + want["rayleigh_slack"][mem])
    print(f"{what}: members {len(mem)}, Rayleigh excess / slack max "
          f"{float(((rq - w[:, 0])[live] / want['rayleigh_slack'][mem][live]).max()) if live.any() else 0.0:.3g}")
    assert not over.any(), (what, int(over.sum()))
    assert np.array_equal(n[mem][~live], want["normals"][mem][~live].astype(np.float32)), what      # (0, 0, +-1) exactly
    # sign
    view = want["view"][mem]
    if centres is not None:
        c = np.asarray(centres, np.float64)[np.maximum(view, 0)] - np.asarray(xyz, np.float64)[mem]
        dot = (v * c).sum(axis=1)
        # n is the signed double vector rounded to float32: the dot moves by at most |c| sqrt(3) 2^-25
        assert (dot[view >= 0] >= -np.linalg.norm(c[view >= 0], axis=1) * np.sqrt(3) * 2.0 ** -25).all(), what
    free = view < 0
    # the largest component is positive: after the rounding the largest positive one is within 2^-24 of the largest
    assert (v[free].max(axis=1) >= np.abs(v[free]).max(axis=1) - 2.0 ** -24).all(), what
    # angle, where the yardstick's eigenvector is determined
    gate = live & ((w[:, 1] - w[:, 0]) >= 0.05 * w[:, 2])
    ang = NR.angle_between(v[gate], want["normals"][mem][gate])
    print(f"{what}: angle / bound max {float((ang / want['angle_bound'][mem][gate]).max()):.3g}; left out by the gap gate "
          f"{100.0 * (1 - gate.sum() / max(live.sum(), 1)):.2f} %")
    assert (ang <= want["angle_bound"][mem][gate]).all(), (what, float(ang.max()))
    assert (live & ~gate).sum() <= 0.02 * len(mem), what
    # and on the yardstick's side; a member whose own rule is a near-tie (a dot product or two components within the
    # two solvers' 1e-15 of each other) may differ, which at these sizes is none or one
    same = (v[gate] * want["normals"][mem][gate]).sum(axis=1) > 0
    assert (~same).sum() <= 1, (what, int((~same).sum()))


# ---------------------------------------------------------------- exactness of the neighbours and the counts
@pytest.mark.parametrize("P,knn", [(4000, 30), (4000, 8), (1500, 30), (4097, 64)])
def test_noisy_scene_neighbours_counts_and_normals(P, knn):
    xyz = noisy_scene(P)
    want = scene_ref(P, knn)
    got = run(xyz, BOX, knn)
    assert_exact(got, want, f"scene P={P} knn={knn}")
    assert 0 < want["counts"][2] < want["counts"][0] < P          # conditions on the inputs: every count has work to do
    assert_normals(got[0], want, xyz, f"scene P={P} knn={knn}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_noisy_scene_with_two_cameras_on_opposite_sides(dtype):
    P, knn = 1500, 30
    xyz = noisy_scene(P).astype(DTYPES[dtype])
    want = scene_ref(P, knn, cameras=True)
    vs, ct = CAMERAS["view_starts"](P), CAMERAS["centres"]
    got = run(xyz, BOX, knn, view_starts=vs, centres=ct)
    assert_exact(got, want, f"cameras {dtype}")
    assert_normals(got[0], want, xyz, f"cameras {dtype}", vs, ct)
    plain = scene_ref(P, knn)
    flipped = (want["normals"] * plain["normals"]).sum(axis=1) < 0
    assert 0.2 < flipped[want["member"]].mean() < 0.8              # the rule bites: the second camera looks from below
    # a view table that covers only the middle: the rest takes the camera-free rule
    vs2 = [P // 4, P // 2, 3 * P // 4]
    want2 = NR.estimate(xyz, *BOX, knn, view_starts=vs2, centres=ct)
    got2 = run(xyz, BOX, knn, view_starts=vs2, centres=ct)
    assert_exact(got2, want2, "partial views")
    assert (want2["view"][want2["member"]] < 0).sum() > 100
    assert_normals(got2[0], want2, xyz, "partial views", vs2, ct)


def test_f64_points_that_are_no_float32():
    rng = np.random.default_rng(3)
    xyz = noisy_scene(1500).astype(np.float64) + rng.uniform(-1e-4, 1e-4, (1500, 3))
    assert not np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)
    want = NR.estimate(xyz, *BOX, 30)
    got = run(xyz, BOX, 30)
    assert_exact(got, want, "f64")
    assert_normals(got[0], want, xyz, "f64")


TWO_PASS_BOX, TWO_PASS_CELL = ((0.0, 0.0, 0.0), (48.0, 48.0, 32.0)), 0.375      # 0.375 is exact in binary


@functools.lru_cache(maxsize=None)
def two_pass_scene():
    """Two clusters of 200 points, each strictly inside a 3-unit cube of TWO_PASS_BOX: one at the low corner, one with z in
    [28, 31]; each two tilted sheets of 10 x 10 jittered lattice points one unit apart, so that five neighbours determine a
    normal -> (xyz float32 [400,3] (read-only), linear cell index int64 [400], the yardstick at knn = 5)."""
    rng = np.random.default_rng(6)
    i, j, k = (g.reshape(-1).astype(np.float64) for g in np.meshgrid(np.arange(10), np.arange(10), np.arange(4), indexing="ij"))
    sheet = np.column_stack([0.2 + 0.28 * i, 0.2 + 0.28 * j, 0.8 + (k % 2)]) + rng.normal(0.0, [0.03, 0.03, 0.01], (400, 3))
    sheet[:, 2] += 0.3 * (sheet[:, 0] - 1.5)
    corners = np.where((k < 2)[:, None], [0.0, 0.0, 0.0], [40.0, 40.0, 28.0])     # sheets 0, 1 low, sheets 2, 3 high
    assert (sheet > 0.04).all() and (sheet < 2.96).all()
    xyz = (corners + sheet)[rng.permutation(400)].astype(np.float32)
    xyz.setflags(write=False)
    n = NR.grid_shape(*TWO_PASS_BOX, TWO_PASS_CELL)
    c = np.floor((xyz.astype(np.float64) - np.asarray(TWO_PASS_BOX[0])) / TWO_PASS_CELL).astype(np.int64)
    return xyz, (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0], NR.estimate(xyz, *TWO_PASS_BOX, 5)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_knn_grid_of_more_tiles_than_one_pass_of_the_tile_scan(dtype):
    """1,398 tiles of cell counts: the tile scan's second pass starts from the carry of its first, and every member of the
    upper cluster takes its offset from there."""
    xyz, linear, want = two_pass_scene()
    n = NR.grid_shape(*TWO_PASS_BOX, TWO_PASS_CELL)
    assert n == [129, 129, 86]
    tiles = -(-(n[0] * n[1] * n[2]) // _lib.NORMALS_TILE)
    assert n[0] * n[1] * n[2] == 1431126 and tiles == 1398 > _lib.CLOUD_SCAN_WIDTH      # the scan width is one for all grids
    first_pass = _lib.CLOUD_SCAN_WIDTH * _lib.NORMALS_TILE                               # cells the first pass covers
    assert want["member"].all() and (linear < first_pass).sum() >= 100 and (linear >= first_pass).sum() >= 100
    got = run(xyz.astype(DTYPES[dtype]), TWO_PASS_BOX, 5, cell=TWO_PASS_CELL)
    assert_exact(got, want, f"two passes {dtype}")
    assert_normals(got[0], want, xyz, f"two passes {dtype}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_integer_lattice_ties_are_decided_by_index(dtype):
    g = np.stack(np.meshgrid(np.arange(16.0), np.arange(16.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    xyz = g[np.random.default_rng(1).permutation(len(g))].astype(DTYPES[dtype])
    box = ((0.0, 0.0, 0.0), (15.0, 15.0, 2.0))                 # every outer point lies exactly on a face
    for knn, cell in ((30, 1.0), (8, 2.5), (64, 16.0)):
        want = NR.estimate(xyz, *box, knn)
        assert want["counts"][0] == 768
        assert_exact(run(xyz, box, knn, cell=cell), want, f"lattice knn={knn} cell={cell}")


def test_every_point_duplicated():
    xyz = np.repeat(noisy_scene(1500)[:700], 2, axis=0)[np.random.default_rng(2).permutation(1400)]
    want = NR.estimate(xyz, *BOX, 30)
    got = run(xyz, BOX, 30)
    assert_exact(got, want, "duplicates")
    mem = np.flatnonzero(want["member"])
    twin = want["nbr"][mem, :2]
    assert (np.sort(twin, axis=1) == twin).all() and (xyz[twin[:, 0]] == xyz[twin[:, 1]]).all()     # twins lead, lower index first


def test_points_exactly_on_the_box_faces_and_just_outside():
    rng = np.random.default_rng(4)
    lo, hi = np.array([-8.0, -4.0, 0.0]), np.array([8.0, 4.0, 2.0])
    xyz = rng.uniform(lo - 1, hi + 1, (600, 3)).astype(np.float32)
    xyz[:120] = rng.uniform(lo, hi, (120, 3)).astype(np.float32)           # the rows put on the faces lie inside otherwise
    for a in range(3):
        xyz[40 * a:40 * a + 20, a] = lo[a]
        xyz[40 * a + 20:40 * a + 40, a] = hi[a]
        xyz[120 + 20 * a:130 + 20 * a, a] = np.nextafter(np.float32(lo[a]), np.float32(-np.inf))
        xyz[130 + 20 * a:140 + 20 * a, a] = np.nextafter(np.float32(hi[a]), np.float32(np.inf))
    want = NR.estimate(xyz, lo, hi, 10)
    on_face = want["member"] & ((xyz == lo) | (xyz == hi)).any(axis=1)
    assert on_face.sum() >= 120 and (~want["member"][120:180]).all()
    for cell in (1.0, 0.7, 16.0):
        assert_exact(run(xyz, (lo, hi), 10, cell=cell), want, f"faces cell={cell}")


@pytest.mark.parametrize("knn", [3, 30])
def test_few_members(knn):
    """M = 0, 1, 2, 3, knn - 1, knn, knn + 1 members among points outside the box."""
    rng = np.random.default_rng(6)
    for M in sorted({0, 1, 2, 3, knn - 1, knn, knn + 1}):
        xyz = rng.uniform(50, 60, (knn + 9, 3)).astype(np.float32)          # all outside
        inside = rng.choice(len(xyz), M, replace=False)
        xyz[inside] = rng.uniform(0, 10, (M, 3)).astype(np.float32)
        want = NR.estimate(xyz, (0, 0, 0), (10, 10, 10), knn)
        assert want["counts"][0] == M and want["counts"][1] == (M if M >= 3 else 0)
        for cell in (20.0, 3.0):
            got = run(xyz, ((0, 0, 0), (10, 10, 10)), knn, cell=cell)
            assert_exact(got, want, f"M={M} knn={knn} cell={cell}")
            if M < 3:
                assert np.array_equal(got[0][inside], np.tile(np.float32([0, 0, 1]), (M, 1)))


def test_nan_and_inf_rows_are_no_members():
    xyz = noisy_scene(1500).copy()
    rng = np.random.default_rng(7)
    rows = rng.choice(1500, 90, replace=False)
    xyz[rows[:30], rng.integers(0, 3, 30)] = np.nan
    xyz[rows[30:60], rng.integers(0, 3, 30)] = np.inf
    xyz[rows[60:], rng.integers(0, 3, 30)] = -np.inf
    want = NR.estimate(xyz, *BOX, 30)
    assert not want["member"][rows].any()
    got = run(xyz, BOX, 30)
    assert_exact(got, want, "non-finite")
    assert_normals(got[0], want, xyz, "non-finite")


def test_an_empty_cloud_gives_three_zero_counts():
    n, b, c = run(np.zeros((0, 3), np.float32), BOX, 30)
    assert c == [0, 0, 0] and n.shape == (0, 3) and b.shape == (0, 30)


# ---------------------------------------------------------------- exact normals
def test_lattice_planes_coincident_points_and_the_sign_rule_give_exact_normals():
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), indexing="ij"), -1).reshape(-1, 2)
    low = np.column_stack([g, np.zeros(len(g))])
    high = np.column_stack([g, np.full(len(g), 100.0)])            # two z-planes far apart: neighbours stay in the plane
    heap = np.tile([5.5, 5.5, 50.0], (12, 1))                      # twelve coincident points in between
    xyz = np.vstack([low, high, heap]).astype(np.float32)
    box = ((-1.0, -1.0, -1.0), (12.0, 12.0, 101.0))
    want = NR.estimate(xyz, *box, 9)
    got = run(xyz, box, 9, cell=4.0)
    assert_exact(got, want, "planes")
    assert want["degenerate"][288:].all() and not want["degenerate"][:288].any()
    assert np.array_equal(got[0], np.tile(np.float32([0, 0, 1]), (300, 1)))        # no camera: the largest component positive
    # a camera between the planes: the lower plane looks up, the upper one down; the heap lies below the camera
    vs, ct = [0, 300], [[5.0, 5.0, 60.0]]
    got = run(xyz, box, 9, cell=4.0, view_starts=vs, centres=ct)
    assert_exact(got, NR.estimate(xyz, *box, 9, view_starts=vs, centres=ct), "planes, camera")
    assert np.array_equal(got[0][:144], np.tile(np.float32([0, 0, 1]), (144, 1)))
    assert np.array_equal(got[0][144:288], np.tile(np.float32([0, 0, -1]), (144, 1)))
    assert np.array_equal(got[0][288:], np.tile(np.float32([0, 0, 1]), (12, 1)))
    assert (np.signbit(got[0][144:288, :2]) | (got[0][144:288, :2] == 0)).all()


def test_a_box_whose_faces_certify_some_members_and_not_others():
    """A dense slab: members deep inside have their 8 neighbours well within the distance to the nearest face, members
    near a face do not -> counts_out[2] is neither 0 nor M."""
    rng = np.random.default_rng(8)
    xyz = rng.uniform(-12, 12, (5000, 3)).astype(np.float32)
    box = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))
    want = NR.estimate(xyz, *box, 8)
    M, _, open_ = want["counts"]
    assert 0.2 * M < open_ < 0.8 * M
    assert_exact(run(xyz, box, 8, cell=2.0), want, "slab")


# ---------------------------------------------------------------- determinism
def test_every_cell_size_two_runs_and_two_streams_give_identical_bytes():
    P, knn = 4000, 30
    x = cu(noisy_scene(P))
    vs, ct = cu(np.asarray(CAMERAS["view_starts"](P), np.int64)), cu(np.asarray(CAMERAS["centres"], np.float64))
    span = max(b - a for a, b in zip(*BOX))
    call = lambda cell: _lib.cloud_normals(x, *BOX, cell=cell, knn=knn, view_starts=vs, centres=ct, neighbours=True)   # noqa: E731
    runs = [call(c) for c in (span, 50.0, 5.0, 7.3, 5.0)]          # one cell (two per axis), ..., the same again
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        runs.append(call(5.0))
    side.synchronize()
    torch.cuda.synchronize()
    assert NR.grid_shape(*BOX, span) == [2, 1, 1] and NR.grid_shape(*BOX, 7.3) == [80, 53, 31]
    assert runs[0][2].tolist() == scene_ref(P, knn, cameras=True)["counts"]
    for other in runs[1:]:
        for u, v in zip(runs[0], other):
            assert torch.equal(G.raw_bytes(u), G.raw_bytes(v))


def test_cloud_normals_enqueues_without_a_host_synchronisation():
    x = cu(noisy_scene(1500))
    _lib.cloud_normals(x, *BOX, knn=8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n, b, c = _lib.cloud_normals(x, *BOX, knn=8)
        fusion.estimate_normals(x, knn=8, box=BOX)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert b is None and c.tolist() == scene_ref(1500, 8)["counts"]


# ---------------------------------------------------------------- guarded buffers
GUARDED_ENTRIES = {"mvs_cloud_normals": "test_normals_buffers_between_guards_under_every_poison",
                   "mvs_cloud_downsample_normals": "test_downsample_normals_buffers_between_guards_under_every_poison"}


def test_every_device_entry_point_of_the_normals_header_has_a_guarded_case():
    assert_guarded_coverage("mvs_normals_abi.h", GUARDED_ENTRIES, globals())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_normals_buffers_between_guards_under_every_poison(dtype):
    P, knn = 1500, 30
    xyz = noisy_scene(P).astype(DTYPES[dtype])
    want = scene_ref(P, knn, cameras=True)
    vs, ct = np.asarray(CAMERAS["view_starts"](P), np.int64), np.asarray(CAMERAS["centres"], np.float64)
    arena = G.Arena(32 << 20, DEV)
    seen = []

    def fn(a):
        ins = [a.put(cu(t), name=n) for t, n in ((xyz, "xyz"), (vs, "view_starts"), (ct, "centres"))]
        with a.intercept(_lib):       # normals, neighbours, counts are carved as `out`, the workspace as `scratch`
            n, b, c = _lib.cloud_normals(ins[0], *BOX, cell=5.0, knn=knn, view_starts=ins[1], centres=ins[2], neighbours=True)
        torch.cuda.synchronize()
        if isinstance(a, G.Arena):
            roles = sorted(r.role for r in a.carved)
            assert roles == ["in"] * 3 + ["out"] * 3 + ["scratch"], roles
            ws = [r for r in a.carved if r.role == "scratch"][0]
            assert ws.tensor.numel() == _lib.query_normals_workspace(P, *BOX, 5.0) == NR.workspace_bytes(P, *BOX, 5.0)
            seen.append(a.poison)
        return n, b, c

    guard_bytes = G.guarded_and_plain(arena, fn)
    assert seen == list(G.POISONS) and guard_bytes >= 14 * G.MIN_GUARD
    n, b, c = fn(G.Plain(DEV))
    assert_exact((n.cpu().numpy(), b.cpu().numpy(), c.tolist()), want, f"guarded {dtype}")


# ---------------------------------------------------------------- the downsample that carries normals
def ds_inputs(P, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-330, -230, -30], [330, 230, 60], (P, 3))
    rgb = rng.integers(0, 256, (P, 3), dtype=np.uint8)
    nrm = rng.normal(size=(P, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[::97] = [2.5, -3.0, np.nan]                    # clamped to 1, -1, and counted as 0
    nrm[5::101] = 0.0                                  # what estimate_normals gives a point outside its box
    return xyz, rgb, nrm


BIN = ((-305.0, -205.0, -20.0), (305.0, 205.0, 220.0))


def run_ds(xyz, rgb, nrm, v=5.0, scale=0.01, capacity=None, out=None):
    r = _lib.cloud_downsample_normals(cu(xyz), cu(rgb), cu(nrm), *BIN, v, scale=scale, capacity=capacity, out=out)
    torch.cuda.synchronize()
    return r


def assert_mean_normals(got, xyz, nrm, v, what):
    want = NR.voxel_mean_normals(xyz, nrm, *BIN, v)
    got = got.astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    big = np.maximum(np.abs(want), np.abs(got))
    ulp32 = np.where(big == 0, 2.0 ** -149, np.maximum(np.ldexp(1.0, np.frexp(big)[1] - 24), 2.0 ** -149))
    err = np.abs(got - want)
    print(f"{what}: {len(want)} voxels, max error / (2^-31 + ulp32 / 2) = {float((err / (2.0 ** -31 + ulp32 / 2)).max()):.3f}")
    assert (err <= 2.0 ** -31 + ulp32 / 2).all(), (what, float(err.max()))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("P", [1, 1025, 20011])
def test_downsample_with_normals_equals_the_plain_one_and_the_fp64_mean(P, dtype):
    xyz, rgb, nrm = ds_inputs(P, P)
    xyz = xyz.astype(DTYPES[dtype])
    xyz[0] = [12.3, -45.6, 7.8]
    x, c, n, cnt = run_ds(xyz, rgb, nrm)
    px, pc, pcnt = _lib.cloud_downsample(cu(xyz), cu(rgb), *BIN, 5.0, scale=0.01)
    torch.cuda.synchronize()
    Q = int(cnt[1])
    assert cnt.tolist() == pcnt.tolist() and Q >= 1 and (P == 1 or Q < int(cnt[0]) < P)
    assert torch.equal(G.raw_bytes(x[:Q]), G.raw_bytes(px[:Q])) and torch.equal(c[:Q], pc[:Q])
    assert_mean_normals(n[:Q].cpu().numpy(), xyz, nrm, 5.0, f"downsample normals P={P} {dtype}")
    # a shuffled copy, its colours and normals shuffled alike: the same bytes
    perm = np.random.default_rng(1).permutation(P)
    x2, c2, n2, cnt2 = run_ds(xyz[perm], rgb[perm], nrm[perm])
    assert cnt2.tolist() == cnt.tolist()
    for u, w in ((x, x2), (c, c2), (n, n2)):
        assert torch.equal(G.raw_bytes(u[:Q]), G.raw_bytes(w[:Q]))


def test_downsample_with_normals_respects_the_capacity():
    xyz, rgb, nrm = ds_inputs(5000, 8)
    full = run_ds(xyz, rgb, nrm)
    total = int(full[3][1])
    assert total > 1024 + 64
    for capacity in (total + 5, total, total - 1, 0):
        big_x = torch.full((total + 8, 3), 777.0, dtype=torch.float32, device=DEV)
        big_c = torch.full((total + 8, 3), 0x5A, dtype=torch.uint8, device=DEV)
        big_n = torch.full((total + 8, 3), 555.0, dtype=torch.float32, device=DEV)
        counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        run_ds(xyz, rgb, nrm, capacity=capacity, out=(big_x[:capacity], big_c[:capacity], big_n[:capacity], counts))
        assert counts.tolist() == full[3].tolist(), capacity
        m = min(capacity, total)
        for big, ref, fill in ((big_x, full[0], 777.0), (big_c, full[1], 0x5A), (big_n, full[2], 555.0)):
            assert torch.equal(G.raw_bytes(big[:m]), G.raw_bytes(ref[:m])) and bool((big[m:] == fill).all()), capacity
    x, c, n, cnt = run_ds(xyz, rgb, nrm, capacity=0)        # no buffers given: NULL outputs go to the library
    assert n.shape == (0, 3) and cnt.tolist() == full[3].tolist()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_downsample_normals_buffers_between_guards_under_every_poison(dtype):
    P = 5000
    xyz, rgb, nrm = ds_inputs(P, 12)
    xyz = xyz.astype(DTYPES[dtype])
    arena = G.Arena(64 << 20, DEV)
    seen = []

    def fn(a):
        ins = [a.put(cu(t), name=k) for t, k in ((xyz, "xyz"), (rgb, "rgb"), (nrm, "normals"))]
        with a.intercept(_lib):
            x, c, n, cnt = _lib.cloud_downsample_normals(*ins, *BIN, 5.0, scale=0.01)
        torch.cuda.synchronize()
        Q = int(cnt[1])
        if isinstance(a, G.Arena):
            roles = sorted(r.role for r in a.carved)
            assert roles == ["in"] * 3 + ["out"] * 4 + ["scratch"], roles
            ws = [r for r in a.carved if r.role == "scratch"][0]
            assert ws.tensor.numel() == _lib.query_cloud_normals_downsample_workspace(P, *BIN, 5.0)
            for t in (x, c, n):         # beyond the voxels nothing is written: the poison is still there
                assert bool((G.raw_bytes(t[Q:]) == a.poison).all())
            seen.append(a.poison)
        return x[:Q], c[:Q], n[:Q], cnt

    G.guarded_and_plain(arena, fn)
    assert seen == list(G.POISONS)
    x, c, n, cnt = fn(G.Plain(DEV))
    assert_mean_normals(n.cpu().numpy(), xyz, nrm, 5.0, f"guarded {dtype}")
    want = cloud_ref.downsample(xyz, rgb, *BIN, 5.0, 0.01)
    assert cnt.tolist() == [want["kept"], want["voxels"]] and np.array_equal(c.cpu().numpy(), want["rgb"])


# ---------------------------------------------------------------- the Python layer
def test_estimate_normals_defaults_to_the_bounding_box_of_the_finite_points():
    xyz = noisy_scene(1500).copy()
    xyz[7] = [np.nan, 0.0, 0.0]
    xyz[9] = [0.0, np.inf, 0.0]
    ok = np.isfinite(xyz).all(axis=1)
    lo, hi = xyz[ok].min(axis=0).astype(np.float64), xyz[ok].max(axis=0).astype(np.float64)
    want = NR.estimate(xyz, lo, hi, 8)
    n, cnt, nbr = fusion.estimate_normals(cu(xyz), knn=8, return_neighbours=True)
    assert cnt.tolist() == want["counts"] and want["counts"][0] == 1498
    assert_exact((n.cpu().numpy(), nbr.cpu().numpy(), cnt.tolist()), want, "bounding box")
    # per-view counts and centres as fuse_views and the cameras give them
    counts, ct = np.array([500, 0, 1000], np.int32), np.array([[0, 0, 500.0], [9, 9, 9.0], [0, 0, -500.0]])
    n2, cnt2 = fusion.estimate_normals(cu(xyz), knn=8, box=(lo, hi), view_counts=counts, centres=ct)
    want2 = NR.estimate(xyz, lo, hi, 8, view_starts=[0, 500, 500, 1500], centres=ct)
    assert_exact((n2.cpu().numpy(), want2["nbr"], cnt2.tolist()), want2, "views")
    assert_normals(n2.cpu().numpy(), want2, xyz, "views", [0, 500, 500, 1500], ct)
    with pytest.raises(RuntimeError, match="both be given"):
        fusion.estimate_normals(cu(xyz), view_counts=counts)
    with pytest.raises(_lib.MvsError) as e:
        _lib.cloud_normals(cu(xyz), lo, hi, knn=65)
    assert e.value.code == 1


# ---------------------------------------------------------------- the chain
def test_reconstruct_scan_with_normals_equals_the_steps_by_hand(tmp_path):
    ds, model, _ = dataset(tmp_path)
    thr = dict(geomask=0, photomask=0.0, device=DEV)        # thresholds that keep every pixel
    plain = fusion.reconstruct_scan(model, ds, "scan1", **thr)
    finite = plain[0][np.isfinite(plain[0]).all(axis=1)].astype(np.float64)
    lo, hi = np.quantile(finite, 0.1, axis=0), np.quantile(finite, 0.9, axis=0)
    v = float((hi - lo).max() / 12)
    margin, cell = 2 * v, v
    small, small_n, full, full_n = (str(tmp_path / f) for f in ("small.ply", "small_n.ply", "full.ply", "full_n.ply"))
    base = fusion.reconstruct_scan(model, ds, "scan1", plyfilename=full,
                                   downsample=dict(voxel_size=v, box=(lo, hi), scale=0.01, plyfilename=small), **thr)
    got = fusion.reconstruct_scan(model, ds, "scan1", plyfilename=full_n,
                                  downsample=dict(voxel_size=v, box=(lo, hi), scale=0.01, plyfilename=small_n,
                                                  normals=dict(knn=8, margin=margin, cell=cell)), **thr)
    # without `normals` everything is what it was; with them the first four items and the full PLY are the same bytes
    assert len(plain) == 2 and len(base) == 4 and len(got) == 6
    for a, b in zip(base, got[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert open(full, "rb").read() == open(full_n, "rb").read()
    # the steps by hand, on the returned full cloud
    refs = [m[1] for m in ds.metas if m[0] == "scan1"]
    per_view = 24 * 32
    assert len(plain[0]) == len(refs) * per_view
    E = np.stack([np.asarray(ds[i]["extrinsics"][0], np.float64) for i, m in enumerate(ds.metas) if m[0] == "scan1"])
    centres = np.stack([-e[:3, :3].T @ e[:3, 3] for e in E])
    x, c = cu(plain[0]), cu(plain[1])
    nrm, cnt = fusion.estimate_normals(x, knn=8, box=(lo - margin, hi + margin), cell=cell,
                                       view_counts=[per_view] * len(refs), centres=centres)
    hx, hc, hn = fusion.downsample_cloud(x, c, voxel_size=v, box=(lo, hi), scale=0.01, normals=nrm)
    assert got[4].dtype == np.float32 and got[4].shape == got[2].shape and len(got[4]) > 20
    assert got[4].tobytes() == hn.cpu().numpy().tobytes() and got[2].tobytes() == hx.cpu().numpy().tobytes()
    assert got[5].tolist() == cnt.tolist() and 0 < got[5][0] <= len(plain[0]) and got[5][1] == got[5][0]
    # and against the yardstick: every normal looks at its own camera
    want = NR.estimate(plain[0], lo - margin, hi + margin, 8, view_starts=np.arange(len(refs) + 1) * per_view, centres=centres)
    assert cnt.tolist() == want["counts"]
    assert_normals(nrm.cpu().numpy(), want, plain[0], "chain", list(np.arange(len(refs) + 1) * per_view), centres)
    # the PLY holds the returned arrays bit for bit; the file without normals is today's
    px, pc, pn = read_ply(small_n, normals=True)
    assert px.tobytes() == got[2].tobytes() and pc.tobytes() == got[3].tobytes() and pn.tobytes() == got[4].tobytes()
    body = lambda path: open(path, "rb").read()      # noqa: E731
    assert b"property float nx" not in body(small) and len(body(small_n)) > len(body(small))


def test_the_command_line_flag_writes_the_same_file(tmp_path):
    from scene_3dreconstruction_mvsnet_amd import reconstruct
    ds, model, listfile = dataset(tmp_path)
    torch.save({"model": {k: torch.from_numpy(v) for k, v in load_weights().items()}}, str(tmp_path / "model.ckpt"))
    out = tmp_path / "plys"
    common = ["--testpath", os.path.join(str(tmp_path), "data"), "--testlist", listfile, "--loadckpt",
              str(tmp_path / "model.ckpt"), "--outdir", str(out), "--numdepth", "16", "--NviewGen", "3", "--img_res", "96", "128",
              "--geomask", "0", "--photomask", "0.0"]
    # a box around the middle of the first scan's cloud, 10 voxels along its longest edge
    fx = fusion.reconstruct_scan(model, ds, "scan1", geomask=0, photomask=0.0, device=DEV)[0].astype(np.float64)
    lo, hi = np.quantile(fx, 0.15, axis=0).round(1), np.quantile(fx, 0.85, axis=0).round(1)
    v = float(((hi - lo).max() / 10).round(2))
    box = [float(b) for b in (*lo, *hi)]
    flags = ["--downsample_mm", repr(v), "--cloud_scale", "1", "--crop_box"] + [repr(b) for b in box]
    plain = reconstruct.main(common + flags)
    before = [open(p, "rb").read() for p in plain]
    written = reconstruct.main(common + flags + ["--normals_knn", "8", "--normals_margin_mm", repr(2 * v)])
    assert [os.path.relpath(p, str(out)) for p in written] == [os.path.relpath(p, str(out)) for p in plain]
    assert [open(p, "rb").read() for p in written[::2]] == before[::2]           # the full clouds are what they were
    got = fusion.reconstruct_scan(model, ds, "scan1", geomask=0, photomask=0.0, device=DEV,
                                  downsample=dict(voxel_size=v, box=(box[:3], box[3:]), scale=1.0,
                                                  normals=dict(knn=8, margin=2 * v)))
    px, pc, pn = read_ply(written[1], normals=True)
    assert len(px) == len(got[2]) > 20 and np.isfinite(pn).all() and (np.linalg.norm(pn, axis=1) <= 1 + 1e-6).all()
    assert px.tobytes() == got[2].tobytes() and pc.tobytes() == got[3].tobytes() and pn.tobytes() == got[4].tobytes()
