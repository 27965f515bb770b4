"""Host-side checks of the plane segmentation (include/ext/mvs_planes_abi.h, csrc/cloud_planes.hip,
csrc/cloud_planes_fit.h, fusion.segment_planes, the command line): none needs a GPU.

The header lives in include/ext/ and its table is `_lib._ABI_EXT`, outside the tables tests/refusals.py and
tests/wrapper_contract.py are bound to, so this file applies their checks itself with their helpers, the way
tests/test_cloud_register_host.py does: the prototypes against the argument types, the refusals in a child that sees no
device (`python tests/test_cloud_planes_host.py child`, started through tests/gpu_child.py), every pointer's extent and
the wrapper's defective calls against the recording stand-in.  The fit header runs as a stand-alone host program under
the address and undefined-behaviour sanitizers; tests/planes_ref.py is held to the planted scene of the issue."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for path in (REPO, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import planes_ref as PR  # noqa: E402
import refusals  # noqa: E402

from refusals import BAD_DTYPE, BAD_SHAPE, BIN, HIP, INF, NAN, NULL, OK, WORKSPACE  # noqa: E402

HEADER = "ext/mvs_planes_abi.h"

# ---------------------------------------------------------------- the refusal cases (shared by the child and the tests)
GOOD = dict(dtype=0, P=5000, box_min=BIN[0], box_max=BIN[1], dist=1.5, num_candidates=1000, max_planes=3, min_inliers=50,
            seed=7, toward=(0.0, 0.0, 1000.0))
SHORT = dict(workspace_bytes=0)      # a legal call is recognised by the refusal that comes last: the workspace's
CASES = [(f"null {p}", {p: None}, NULL, "NULL") for p in ("xyz", "box_min", "box_max", "planes_out", "rounds_out",
                                                          "counts_out", "labels_out", "workspace")]
CASES += [(f"{p} may be NULL", dict(SHORT, **{p: None}), WORKSPACE, "workspace") for p in ("toward", "cand_counts_out", "sums_out")]
CASES += [
    ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"),
    ("K = 0", dict(num_candidates=0), BAD_SHAPE, "num_candidates = 0"),
    ("K < 0", dict(num_candidates=-5), BAD_SHAPE, "num_candidates = -5"),
    ("K = 8193", dict(num_candidates=8193), BAD_SHAPE, "num_candidates = 8193"),
    ("K = 1 is legal", dict(SHORT, num_candidates=1), WORKSPACE, "workspace"),
    ("K = 8192 is legal", dict(SHORT, num_candidates=8192), WORKSPACE, "workspace"),
    ("max_planes 0", dict(max_planes=0), BAD_SHAPE, "max_planes = 0"),
    ("max_planes < 0", dict(max_planes=-1), BAD_SHAPE, "max_planes = -1"),
    ("max_planes 65", dict(max_planes=65), BAD_SHAPE, "max_planes = 65"),
    ("max_planes 64 is legal", dict(SHORT, max_planes=64), WORKSPACE, "workspace"),
    ("min_inliers 2", dict(min_inliers=2), BAD_SHAPE, "min_inliers = 2"),
    ("min_inliers < 0", dict(min_inliers=-1), BAD_SHAPE, "min_inliers = -1"),
    ("min_inliers 3 is legal", dict(SHORT, min_inliers=3), WORKSPACE, "workspace"),
    ("dist nan", dict(dist=NAN), BAD_SHAPE, "dist"),
    ("dist < 0", dict(dist=-0.5), BAD_SHAPE, "dist"),
    ("dist inf", dict(dist=INF), BAD_SHAPE, "dist"),
    ("dist 0 is legal", dict(SHORT, dist=0.0), WORKSPACE, "workspace"),
    ("toward nan", dict(toward=(0.0, NAN, 0.0)), BAD_SHAPE, "toward[1]"),
    ("toward inf", dict(toward=(0.0, 0.0, INF)), BAD_SHAPE, "toward[2]"),
    ("box nan", dict(box_min=(NAN, 0, 0)), BAD_SHAPE, "box axis 0"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("a flat box is legal", dict(SHORT, box_min=(0, 0, 0), box_max=(0, 0, 0)), WORKSPACE, "workspace"),
    ("dtype 2", dict(dtype=2), BAD_DTYPE, "dtype 2"),
    ("dtype -1", dict(dtype=-1), BAD_DTYPE, "dtype -1"),
    ("one byte short", dict(workspace_bytes="need-1"), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace_bytes="need", workspace="plus4"), WORKSPACE, "aligned"),
    ("everything right reaches HIP", dict(workspace_bytes="need"), HIP, ""),
    ("f64 without the optional pointers reaches HIP", dict(workspace_bytes="need", dtype=1, toward=None, cand_counts_out=None,
                                                           sums_out=None), HIP, ""),
    ("P == 0 reaches HIP", dict(P=0, workspace_bytes="need"), HIP, ""),
]
Q_CASES = [
    ("null bytes", dict(bytes=None), NULL, "NULL"), ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"), ("K = 0", dict(num_candidates=0), BAD_SHAPE, "num_candidates"),
    ("K < 0", dict(num_candidates=-1), BAD_SHAPE, "num_candidates"), ("K = 8193", dict(num_candidates=8193), BAD_SHAPE, "num_candidates"),
    ("max_planes 0", dict(max_planes=0), BAD_SHAPE, "max_planes"), ("max_planes < 0", dict(max_planes=-3), BAD_SHAPE, "max_planes"),
    ("max_planes 65", dict(max_planes=65), BAD_SHAPE, "max_planes"),
    ("fine", dict(), OK, ""), ("P == 0 is fine", dict(P=0), OK, ""), ("the largest is fine", dict(P=(1 << 31) - 1, num_candidates=8192, max_planes=64), OK, ""),
]
OPTIONAL = ("toward", "cand_counts_out", "sums_out")
# not named REFUSALS: the tables of that name are held to the headers of include/*.h (tests/test_abi_domain_host.py)
PLANES_REFUSALS = {
    "mvs_cloud_planes": dict(good=GOOD, host=dict(refusals.BOX, toward=ctypes.c_double), optional=OPTIONAL, cases=CASES,
                             sizes=dict(need=lambda a: PR.workspace_bytes(a["P"], a["num_candidates"]))),
    "mvs_query_planes_workspace": dict(good=GOOD, cases=Q_CASES),
}


def child():
    """tests/refusals.py's child over the header of include/ext/: the same records, the same call builder."""
    from scene_3dreconstruction_mvsnet_amd import _lib
    lib = _lib.load()
    protos = refusals.prototypes(HEADER)

    def sentinel():
        assert lib.mvs_query_feature_workspace(1, 3, 2, ctypes.byref(ctypes.c_size_t(0))) == BAD_SHAPE
        return lib.mvs_last_error_string().decode("utf-8", "replace")
    for name, spec in PLANES_REFUSALS.items():
        for lab, ov, want, _ in spec["cases"]:
            before = sentinel()
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=None, err="")), flush=True)      # about to call
            got, err = refusals.call(lib, protos, name, spec, ov)
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=got, err=err, stale=err == before)), flush=True)


_child = {}


def records():
    import gpu_child
    if not _child:
        r = gpu_child.run_once(("planes refusals",), ["test_cloud_planes_host.py", "child"], timeout=300, gpu=False)
        _child["r"], _child["records"] = r, {(rec["ep"], rec["case"]): rec for rec in r.records("R ")}
    return _child["r"], _child["records"]


@pytest.mark.parametrize("name", list(PLANES_REFUSALS))
def test_every_refusal_comes_with_its_status_and_its_message_in_a_child_without_a_device(name):
    r, recs = records()
    spec = PLANES_REFUSALS[name]
    labels = [c[0] for c in spec["cases"]]
    assert len(set(labels)) == len(labels)
    bad = [f"{lab}: {why}" for lab, _, want, text in spec["cases"] for why in [refusals.wrong(recs.get((name, lab)), want, text)] if why]
    assert not bad, f"{len(bad)} of {len(labels)} cases:\n" + "\n".join(bad)
    assert r.returncode == 0, r.stderr[-2000:]


def test_every_pointer_and_count_of_the_prototypes_has_its_cases():
    """what tests/test_abi_domain_host.py asks of the headers of include/*.h"""
    protos = refusals.prototypes(HEADER)
    assert set(protos) == set(PLANES_REFUSALS)
    for name, params in protos.items():
        spec = PLANES_REFUSALS[name]
        nulled = {k for _, ov, code, _ in spec["cases"] if code == NULL for k, v in ov.items() if v is None}
        for kind, p in params:
            if kind == "ptr" and p != "stream":
                assert p in nulled or p in spec.get("optional", ()), (name, p)
            if kind in ("long long", "int") and p != "dtype":
                assert any(p in ov and isinstance(ov[p], int) and ov[p] < 0 for _, ov, code, _ in spec["cases"] if code == BAD_SHAPE), (name, p)
        for p in spec.get("optional", ()):
            assert any(ov.get(p, 0) is None and p in ov and code != NULL for _, ov, code, _ in spec["cases"]), (name, p)


# ---------------------------------------------------------------- declarations
from scene_3dreconstruction_mvsnet_amd import _lib, fusion, reconstruct  # noqa: E402


def test_planes_symbols_are_the_declarations_of_the_planes_header():
    declared = [name for name, _ in refusals.declarations(HEADER)]
    assert declared == list(_lib._ABI_EXT[HEADER]) == list(_lib.PLANES_SYMBOLS) == ["mvs_query_planes_workspace", "mvs_cloud_planes"]
    assert sorted(_lib._ABI_EXT) == sorted("ext/" + f for f in os.listdir(os.path.join(REPO, "include", "ext")))
    assert sorted(_lib._ABI) == refusals.HEADERS                     # the other table is untouched by this one
    others = refusals.HEADERS + [h for h in _lib._ABI_EXT if h != HEADER]
    for other in others:
        table = _lib._ABI.get(other) or _lib._ABI_EXT[other]
        assert not set(declared) & set(table), other
        assert not set(declared) & {name for name, _ in refusals.declarations(other)}, other
    kinds = refusals.header_argtypes(HEADER)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert _lib._ABI_EXT[HEADER][name] == kinds[name], name
        assert list(getattr(_lib.load(), name).argtypes) == kinds[name], name
        assert getattr(_lib.load(), name).restype is ctypes.c_int and hasattr(raw, name), name
    src = refusals.header_text(HEADER)
    for name, value in (("CANDIDATES_MAX", _lib.PLANES_CANDIDATES_MAX), ("SUMS", _lib.PLANES_SUMS), ("TILE", _lib.PLANES_TILE),
                        ("GROUP", _lib.PLANES_GROUP), ("FANIN", _lib.PLANES_FANIN), ("SCALARS", _lib.PLANES_SCALARS)):
        assert refusals.define(src, "MVS_PLANES_" + name) == value == getattr(PR, name), name
    assert refusals.define(src, "MVS_PLANES_MAX") == _lib.PLANES_MAX == PR.PLANES_MAX
    assert refusals.define(src, "MVS_PLANES_JACOBI_SWEEPS") == PR.JACOBI_SWEEPS
    for code, word in _lib.PLANES_STOPS.items():
        assert refusals.define(src, "MVS_PLANES_STOP_" + word.upper()) == code == getattr(PR, word.upper())
    assert "moves to include/" in src and "Nothing here was compared against Open3D" in src
    for value in PR.KEY_CHECK:                                        # the header states the hash again, with its check values
        assert f"0x{value:016X}" in src
    assert all(f"0x{value:016X}" in refusals.header_text("mvs_reduce_abi.h") for value in PR.KEY_CHECK)


# ---------------------------------------------------------------- workspace formula
@pytest.mark.parametrize("P,K", [(0, 1), (1, 1), (1023, 64), (1024, 65), (1025, 1000), (256, 63), (257, 8192), (65536, 128),
                                 (65537, 129), (1 << 24, 1000), ((1 << 24) + 1, 1000), ((1 << 31) - 1, 8192)])
def test_planes_workspace_query_agrees_with_the_headers_formula(P, K):
    want = PR.workspace_bytes(P, K)
    assert _lib.query_planes_workspace(P, K) == want and want % 8 == 0
    assert _lib.query_planes_workspace(P, K, max_planes=64) == want      # it does not depend on it
    shapes = {0: [], 1: [1], 256: [1], 257: [2, 1], 65536: [256, 1], 65537: [257, 2, 1], (1 << 24) + 1: [65537, 257, 2, 1]}
    if P in shapes:
        assert PR.levels(P) == shapes[P]
    assert PR.tree_depth(0) == 0 and PR.tree_depth(256) == 8 and PR.tree_depth(257) == 16 and PR.tree_depth(65537) == 24


# ---------------------------------------------------------------- the hash and the yardstick
def test_the_key_is_the_hash_of_the_reduce_header_with_its_check_values():
    import reduce_ref
    assert tuple(int(PR.key(0, i)) for i in range(3)) == PR.KEY_CHECK
    assert [int(v) for v in PR.key(0, np.arange(3))] == list(PR.KEY_CHECK)
    rng = np.random.default_rng(0)
    for seed, i in zip(rng.integers(0, 1 << 63, 20).tolist() + [(1 << 64) - 1], rng.integers(0, 1 << 40, 21).tolist()):
        z = (seed + (i + 1) * 0x9E3779B97F4A7C15) % (1 << 64)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
        assert int(PR.key(seed, i)) == z ^ (z >> 31)
    for seed in (0, 5, (1 << 64) - 3):                                # the reduce yardstick's own statement of it
        assert (reduce_ref.keys(50, seed) == PR.key(seed, np.arange(50))).all()


def test_the_tree_sum_is_the_pairing_of_the_register_tree_and_within_its_bound():
    import register_ref as RR
    rng = np.random.default_rng(1)
    for P in (1, 255, 256, 257, 65536, 65537, 70000):
        x = rng.normal(size=(P, 3)) * 10.0 ** rng.integers(-3, 4, (P, 3))
        tree, exact = PR.tree_sums(x), RR.exact_sums(x)
        assert (np.abs(tree - exact) <= PR.sum_bound(x)).all() and (PR.sum_bound(x) < 1e-12 * np.abs(x).sum(axis=0)).all()
        if P <= 32:          # one group of the register tree is the same balanced sum
            assert tree.tobytes() == RR.tree_sums(x).tobytes()
    assert PR.tree_sums(np.ones((70000, 1)))[0] == 70000.0


@pytest.mark.parametrize("P,K", [(4096, 256), (1500, 128)])
def test_the_reference_finds_the_three_planted_planes_and_then_stops_for_want_of_a_plane(P, K):
    xyz, truth = PR.planted_scene(P)
    assert xyz.dtype == np.float32 and len(xyz) == P
    for seed in (0, 1, 2):
        got = PR.segment(xyz, *PR.SCENE_BOX, 1.5, K, max_planes=4, min_inliers=50, seed=seed)
        assert got["counts"].tolist()[:2] == [P, 3] and got["counts"][3] == PR.NO_PLANE, got["counts"]
        assert 11 <= got["rounds"][3, 2] <= 23 and got["rounds"][3, 3] == -1 and np.isnan(got["planes"][3]).all()
        assert got["margin"] >= 1e-9
        axes = sorted(int(np.argmax(np.abs(pl[:3]))) for pl in got["planes"][:3])
        assert axes == [0, 1, 2]
        for r in range(3):
            pl = got["planes"][r]
            axis = int(np.argmax(np.abs(pl[:3])))
            planted = {2: 0, 0: 1, 1: 2}[axis]                        # floor: z, the walls: x, y
            assert np.abs(np.abs(pl[:3]) - np.eye(3)[axis]).max() < 2e-3, pl
            # of its planted points that no earlier plane took (a wall's points within t of the floor lie on both),
            # and of all of them nearly as many: at P = 1500 the second wall keeps 222 of its 225
            held = ((got["labels"] == r) & (truth == planted)).sum()
            free = ((truth == planted) & ~((got["labels"] >= 0) & (got["labels"] < r))).sum()
            assert held >= 0.99 * free and held >= 0.985 * (truth == planted).sum(), (seed, r, held, free)
            assert got["winners"][r]["fitted"] and got["winners"][r]["residual"] <= 1e-9
            # the eigenvector by another road, within the bound of the fit's own rounding
            other, w = PR.fit_eigh(got["sums"][r], got["rounds"][r, 2], np.array([0.0, 0.0, 710.0]))
            bound = PR.plane_bound(got["sums"][r], np.zeros(9), got["rounds"][r, 2], (0.0, 0.0, 710.0), got["winners"][r]["residual"])
            assert (np.abs(other - pl) <= bound).all(), (np.abs(other - pl), bound)
        # the labels are a function of the planes: feeding the planes back changes nothing
        again = PR.segment(xyz, *PR.SCENE_BOX, 1.5, K, max_planes=4, min_inliers=50, seed=seed, planes=got["planes"])
        assert (again["labels"] == got["labels"]).all() and (again["cand_counts"] == got["cand_counts"]).all()


def test_the_reference_on_degenerate_clouds():
    box = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))
    line = np.column_stack([np.arange(40.0) * 0.25 - 5, np.arange(40.0) * 0.5 - 9.5, np.arange(40.0) * -0.125])
    got = PR.segment(line, *box, 0.1, 64, max_planes=2, min_inliers=3)
    assert got["counts"].tolist() == [40, 0, 0, PR.NO_PLANE] and (got["cand_counts"][0] == 0).all() and got["rounds"][0].tolist() == [40, 0, 0, -1]
    assert PR.segment(line[:2], *box, 0.1, 8)["counts"].tolist() == [2, 0, 0, PR.EXHAUSTED]
    assert PR.segment(line[:0], *box, 0.1, 8)["counts"].tolist() == [0, 0, 0, PR.EXHAUSTED]
    gx, gy = np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij")
    sheet = np.column_stack([gx.ravel(), gy.ravel(), np.full(30, 2.0)])
    got = PR.segment(sheet, *box, 0.0, 32, max_planes=3, min_inliers=3)      # every valid candidate counts all 30: the first wins
    valid = np.flatnonzero(got["cand_counts"][0] == 30)
    assert got["rounds"][0].tolist() == [30, valid[0], 30, 30] and got["counts"].tolist() == [30, 1, 30, PR.EXHAUSTED]
    assert got["planes"][0].tolist() == [0.0, 0.0, 1.0, -2.0] and got["rounds"][1, 0] == 0
    for toward, sign in (((0.0, 0.0, 9.0), 1.0), ((0.0, 0.0, -9.0), -1.0)):
        got = PR.segment(sheet, *box, 0.0, 32, toward=toward)
        assert (got["planes"][0] == sign * np.array([0.0, 0.0, 1.0, -2.0])).all()


# ---------------------------------------------------------------- the fit header, under the host sanitizers
CXX = "/opt/rocm/llvm/bin/clang++"      # the host compiler of the toolchain that builds the library


@pytest.fixture(scope="module")
def fit_lines(tmp_path_factory):
    """tests/planes_fit_host.cpp: csrc/cloud_planes_fit.h as a stand-alone host program built with the address and
    undefined-behaviour sanitizers (nothing is preloaded, nothing is loaded into Python, no GPU)."""
    assert os.path.exists(CXX), CXX
    exe = tmp_path_factory.mktemp("fit") / "planes_fit_host"
    subprocess.run([CXX, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "scene_3dreconstruction_mvsnet_amd", "csrc"),
                    os.path.join(REPO, "tests", "planes_fit_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    out = []
    for ln in lines[:-1]:
        tag, _, rest = ln.partition(" ")
        left, _, right = rest.partition(" -> ")
        assert tag == "fit"
        left, right = [float.fromhex(t) for t in left.split()], [float.fromhex(t) for t in right.split()]
        out.append(dict(sums=np.array(left[:9]), m=left[9], o=np.array(left[10:13]), toward=left[14:17] if left[13] else None,
                        cand=np.array(left[17:25]), fitted=right[0], plane=np.array(right[1:])))
    return out


def test_the_fit_header_gives_the_yardsticks_plane_bit_for_bit_and_eighs_within_the_bound(fit_lines):
    assert len(fit_lines) == 13
    fitted = 0
    for k, c in enumerate(fit_lines):
        want, ok, residual = PR.fit(c["sums"], c["m"], c["o"], c["toward"], (c["cand"][:3], c["cand"][5:8]))
        assert c["fitted"] == float(ok), k
        # the same operations in the same order: the same bits (libm's sqrt and the divisions are correctly rounded)
        assert (c["plane"] + 0.0).tobytes() == (want + 0.0).tobytes(), (k, c["plane"], want)
        assert abs(np.linalg.norm(c["plane"][:3]) - 1) < 8 * PR.U
        if c["toward"] is not None:
            assert c["plane"][:3] @ np.array(c["toward"]) + c["plane"][3] >= 0, k
        else:
            assert c["plane"][int(np.argmax(np.abs(c["plane"][:3])))] > 0, k
        if ok:
            fitted += 1
            w = np.linalg.eigvalsh(np.array(PR.covariance(c["sums"], c["m"])[1]))
            if w[1] - w[0] > 1e-6 * max(w[2], 1e-300):               # the plane is unique: all but the line and the point
                other, _ = PR.fit_eigh(c["sums"], c["m"], c["o"], c["toward"])
                bound = PR.plane_bound(c["sums"], np.zeros(9), c["m"], c["o"], residual)
                assert (np.abs(other - c["plane"]) <= bound).all(), (k, np.abs(other - c["plane"]), bound)
    assert fitted == 10
    p0, p1, p2 = (c["plane"] for c in fit_lines[:3])
    assert np.abs(p0[:3] - np.array([-0.1, 0.2, 1.0]) / np.sqrt(1.05)).max() < 1e-3 and abs(p0[3] + 603.0 / np.sqrt(1.05)) < 0.05
    assert (p1 == p0).all() and (p2 == -p0).all()                    # toward above: as it is; below: negated
    for c in fit_lines[4:6]:                                         # the wall x = -285, with or without toward
        assert np.abs(c["plane"] - [1.0, 0.0, 0.0, 285.0]).max() < 1e-9
    assert fit_lines[7]["plane"].tolist() == [1.0, 0.0, 0.0, -3.0]   # coincident points: the lowest axis
    assert fit_lines[8]["plane"].tolist() == [-1.0, 0.0, 0.0, 3.0]   # and turned to the side of toward
    for c in fit_lines[10:]:                                         # not finite: the candidate's plane n / |n| through q^0 + o
        assert c["fitted"] == 0.0 and np.abs(np.abs(c["plane"][:3]) - [0.0, 0.6, 0.8]).max() < 4 * PR.U


# ---------------------------------------------------------------- the wrapper's calls against the recording stand-in
def test_the_wrapper_hands_over_only_pointers_the_entry_point_can_take():
    """tests/wrapper_contract.py's harness on the wrapper of this header: the prototype and the extents of the header are
    lent to its tables for the duration of this test and taken back."""
    import torch
    import wrapper_contract as WC
    name = "mvs_cloud_planes"
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    extents = dict(WC._BOX, xyz=WC._xyz("dtype", "P"), toward=WC.HOSTP_NULL,
                   planes_out=WC.Ptr(f64, lambda a: a["max_planes"] * 32), rounds_out=WC.Ptr(i64, lambda a: a["max_planes"] * 32),
                   counts_out=WC.Ptr(i64, lambda a: 32), labels_out=WC.Ptr(i32, lambda a: a["P"] * 4),
                   cand_counts_out=WC.Ptr(i32, lambda a: a["max_planes"] * a["num_candidates"] * 4, True),
                   sums_out=WC.Ptr(f64, lambda a: a["max_planes"] * 72, True), workspace=WC.WS)
    protos = refusals.prototypes(HEADER)
    assert {p for kind, p in protos[name] if kind == "ptr" and p != "stream"} == set(extents)      # every pointer's extent

    def build(m):
        return dict(WC.BOX, xyz=WC._cloud(m), dist=0.5, num_candidates=70, max_planes=3, min_inliers=4, seed=5,
                    toward=(0.0, 0.0, 9.0), cand_counts=True, sums=True,
                    out=(m.f(3, 4, dtype=f64), m.ints([[0] * 4] * 3, i64), m.ints([0] * 4, i64), m.ints([0] * 64),
                         m.ints([[0] * 70] * 3), m.f(3, 9, dtype=f64)))
    roles = dict(xyz="in", **{f"out[{k}]": "out" for k in range(6)})
    case = WC.Unaligned("cloud_planes", _lib.cloud_planes, build, roles, [name])
    saved = WC.DEVICE_ENTRIES, WC.FORWARDED
    WC.PROTOS[name], WC.EXTENTS[name] = protos[name], extents
    WC.DEVICE_ENTRIES, WC.FORWARDED = saved[0] + (name,), saved[1] + ("mvs_query_planes_workspace",)
    try:
        verdict, detail, called = WC.run_case(case, "fake")
        assert (verdict, called) == ("honest", [name]), detail
        rows = WC.table_rows(case)
        assert len(rows) >= 7 * 6
        for leaf, defect in rows:
            want = WC.default_expectation(roles[leaf], defect)
            verdict, detail, _ = WC.run_case(case, "fake", leaf, defect)
            if leaf == "xyz" and defect == "dtype:float64":                     # either dtype is the header's
                want = "honest"
            assert verdict == want, (leaf, defect, verdict, detail)
    finally:
        del WC.PROTOS[name], WC.EXTENTS[name]
        WC.DEVICE_ENTRIES, WC.FORWARDED = saved
    assert name not in WC.PROTOS and name not in WC.EXTENTS and name not in WC.DEVICE_ENTRIES


# ---------------------------------------------------------------- the Python layer, before any GPU work
def test_python_functions_refuse_host_tensors_and_bad_options():
    import torch
    xyz = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        _lib.cloud_planes(xyz, *BIN, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        fusion.segment_planes(xyz, 1.0)
    with pytest.raises(SystemExit):
        reconstruct.main(["--testpath", "x", "--testlist", "y", "--loadckpt", "z", "--segment_planes", "2"])      # needs --segment_dist
    with pytest.raises(ValueError, match="dist"):
        fusion.planes_options(dict(max_planes=2))
    with pytest.raises(ValueError, match="unknown"):
        fusion.planes_options(dict(dist=1.0, ransac_n=3))
    assert fusion.planes_options(dict(dist=2)) == dict(dist=2.0, max_planes=1, num_candidates=1000, min_inliers=3, seed=0, remove=True)
    assert fusion.planes_options(None) is None


def test_the_command_line_takes_the_segment_flags(monkeypatch, tmp_path):
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def parse(self, argv=None):
        args = real(self, argv)
        seen.update(vars(args))
        return args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    base = ["--testpath", "/nonexistent/x", "--testlist", "/nonexistent/y", "--loadckpt", "/nonexistent/z"]
    with pytest.raises(Exception):          # no such file: whatever stops the run, the arguments were parsed
        reconstruct.main(base + ["--downsample_mm", "5", "--segment_dist", "1.5", "--segment_planes", "3", "--segment_candidates", "500",
                                 "--segment_min_inliers", "40", "--segment_seed", "9", "--segment_keep",
                                 "--segment_out", str(tmp_path / "planes.npz")])
    assert (seen["segment_dist"], seen["segment_planes"], seen["segment_candidates"], seen["segment_min_inliers"],
            seen["segment_seed"], seen["segment_keep"]) == (1.5, 3, 500, 40, 9, True)
    assert reconstruct.segment_options(argparse.Namespace(**seen)) == dict(dist=1.5, max_planes=3, num_candidates=500,
                                                                          min_inliers=40, seed=9, remove=False)
    seen.clear()
    with pytest.raises(Exception):
        reconstruct.main(base)
    assert seen["segment_dist"] is None and seen["segment_planes"] == 1 and seen["segment_candidates"] == 1000
    assert reconstruct.segment_options(argparse.Namespace(**seen)) is None


def test_the_npz_of_segment_out_reads_back_as_a_plane_file(tmp_path):
    planes = np.array([[0.0, 0.0, 1.0, -600.0], [1.0, 0.0, 0.0, 285.0]])
    path = str(tmp_path / "planes.npz")
    reconstruct.write_planes(path, dict(planes=planes, rounds=np.zeros((2, 4), np.int64), counts=np.array([9, 2, 7, 1])))
    assert list(fusion.read_plane(path)) == [0.0, 0.0, 1.0, -600.0]
    with np.load(path) as z:
        assert sorted(z.files) == ["P", "counts", "planes", "rounds"] and (z["planes"] == planes).all()
    none = str(tmp_path / "none.npz")
    with pytest.raises(ValueError, match="no plane"):      # a NaN plane would pass through eval_cloud --plane unnoticed
        reconstruct.write_planes(none, dict(planes=np.full((2, 4), np.nan), rounds=np.full((2, 4), -1), counts=np.array([9, 0, 0, 2])))
    assert not os.path.exists(none)


if __name__ == "__main__":
    if sys.argv[1:2] == ["child"]:
        child()
