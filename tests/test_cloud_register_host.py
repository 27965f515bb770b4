"""Host-side checks of the rigid registration (include/ext/mvs_register_abi.h, csrc/cloud_register.hip,
csrc/cloud_register_solve.h, fusion.register_cloud, the command lines): none needs a GPU.

The header lives in include/ext/ and its table is `_lib._ABI_EXT`, outside the tables tests/refusals.py and
tests/wrapper_contract.py are bound to, so this file applies their checks itself with their helpers: the prototypes
against the argument types, the refusals in a child that sees no device (`python tests/test_cloud_register_host.py child`,
started through tests/gpu_child.py), every pointer's extent and the wrapper's defective calls against the recording
stand-in.  The solver header runs as a stand-alone host program under the address and undefined-behaviour sanitizers."""
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

import normals_ref  # noqa: E402
import refusals  # noqa: E402
import register_ref as RR  # noqa: E402

from refusals import BAD_DTYPE, BAD_SHAPE, BIN, HIP, INF, NAN, NULL, OK, WORKSPACE  # noqa: E402

HEADER = "ext/mvs_register_abi.h"
EYE = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0)

# ---------------------------------------------------------------- the refusal cases (shared by the child and the tests)
GOOD = dict(target_dtype=0, source_dtype=0, P=5000, N=3000, box_min=BIN[0], box_max=BIN[1], cell=5.0, max_dist=20.0,
            init=EYE, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6)
SHORT = dict(workspace_bytes=0)      # a legal call is recognised by the refusal that comes last: the workspace's
CASES = [(f"null {p}", {p: None}, NULL, "NULL") for p in ("target_xyz", "source_xyz", "box_min", "box_max", "transform_out",
                                                          "counts_out", "stats_out", "workspace")]
CASES += [(f"{p} may be NULL", dict(SHORT, **{p: None}), WORKSPACE, "workspace")
          for p in ("target_normals", "init", "history_out", "system_out", "idx_out")]
CASES += [
    ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"),
    ("N < 0", dict(N=-1), BAD_SHAPE, "N = -1"),
    ("N = 2^31", dict(N=1 << 31), BAD_SHAPE, "N = 2147483648"),
    ("max_iterations -1", dict(max_iterations=-1), BAD_SHAPE, "max_iterations = -1"),
    ("max_iterations 1001", dict(max_iterations=1001), BAD_SHAPE, "max_iterations = 1001"),
    ("max_iterations 0 is legal", dict(SHORT, max_iterations=0), WORKSPACE, "workspace"),
    ("max_iterations 1000 is legal", dict(SHORT, max_iterations=1000), WORKSPACE, "workspace"),
    ("max_dist nan", dict(max_dist=NAN), BAD_SHAPE, "max_dist"),
    ("max_dist < 0", dict(max_dist=-1.0), BAD_SHAPE, "max_dist"),
    ("max_dist inf is legal", dict(SHORT, max_dist=INF), WORKSPACE, "workspace"),
    ("max_dist 0 is legal", dict(SHORT, max_dist=0.0), WORKSPACE, "workspace"),
    ("rel_fitness nan", dict(rel_fitness=NAN), BAD_SHAPE, "rel_fitness"),
    ("rel_fitness < 0", dict(rel_fitness=-1e-9), BAD_SHAPE, "rel_fitness"),
    ("rel_rmse nan", dict(rel_rmse=NAN), BAD_SHAPE, "rel_rmse"),
    ("rel_rmse < 0", dict(rel_rmse=-1.0), BAD_SHAPE, "rel_rmse"),
    ("criteria 0 are legal", dict(SHORT, rel_fitness=0.0, rel_rmse=0.0), WORKSPACE, "workspace"),
    ("init nan", dict(init=EYE[:5] + (NAN,) + EYE[6:]), BAD_SHAPE, "init[5]"),
    ("init inf", dict(init=EYE[:3] + (INF,) + EYE[4:]), BAD_SHAPE, "init[3]"),
    ("init last row 0 0 0 2", dict(init=EYE[:15] + (2.0,)), BAD_SHAPE, "last row"),
    ("init last row 1 0 0 1", dict(init=EYE[:12] + (1.0, 0, 0, 1.0)), BAD_SHAPE, "last row"),
    ("any upper block is legal", dict(SHORT, init=(2.0, 1, 0, 5, 0, 0, 0, -3, 0, 0, 0, 0, 0, 0, 0, 1.0)), WORKSPACE, "workspace"),
    ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("cell nan", dict(cell=NAN), BAD_SHAPE, "cell"),
    ("cell inf", dict(cell=INF), BAD_SHAPE, "cell"),
    ("box nan", dict(box_min=(NAN, 0, 0)), BAD_SHAPE, "box axis 0"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("min > max", dict(box_min=(306, -205, -20)), BAD_SHAPE, "box axis 0"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("target dtype 2", dict(target_dtype=2), BAD_DTYPE, "dtype 2"),
    ("source dtype -1", dict(source_dtype=-1), BAD_DTYPE, "dtype -1"),
    ("one byte short", dict(workspace_bytes="need-1"), WORKSPACE, "workspace"),
    ("the distance's size is too small", dict(workspace_bytes="normals"), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace_bytes="need", workspace="plus4"), WORKSPACE, "aligned"),
    ("everything right reaches HIP", dict(workspace_bytes="need"), HIP, ""),
    ("f64 and point-to-point reach HIP", dict(workspace_bytes="need", target_dtype=1, source_dtype=1, target_normals=None), HIP, ""),
    ("P == 0 reaches HIP", dict(P=0, workspace_bytes="need"), HIP, ""),
    ("N == 0 reaches HIP", dict(N=0, workspace_bytes="need"), HIP, ""),
]
Q_CASES = [
    ("null box_min", dict(box_min=None), NULL, "NULL"), ("null box_max", dict(box_max=None), NULL, "NULL"),
    ("null bytes", dict(bytes=None), NULL, "NULL"), ("P < 0", dict(P=-1), BAD_SHAPE, "P = -1"),
    ("P = 2^31", dict(P=1 << 31), BAD_SHAPE, "2^31"), ("N < 0", dict(N=-7), BAD_SHAPE, "N = -7"),
    ("N = 2^31", dict(N=1 << 31), BAD_SHAPE, "2^31"), ("cell 0", dict(cell=0.0), BAD_SHAPE, "cell"),
    ("max_iterations -1", dict(max_iterations=-1), BAD_SHAPE, "max_iterations"),
    ("max_iterations 1001", dict(max_iterations=1001), BAD_SHAPE, "max_iterations"),
    ("box inf", dict(box_max=(305, 205, INF)), BAD_SHAPE, "box axis 2"),
    ("1291^3 cells", dict(box_min=(0, 0, 0), box_max=(1290, 1290, 1290), cell=1.0), BAD_SHAPE, "2^31 cells"),
    ("fine", dict(), OK, ""), ("P == 0 and N == 0 are fine", dict(P=0, N=0), OK, ""),
]
OPTIONAL = ("target_normals", "init", "history_out", "system_out", "idx_out")
# not named REFUSALS: the tables of that name are held to the headers of include/*.h (tests/test_abi_domain_host.py)
REGISTER_REFUSALS = {
    "mvs_cloud_register": dict(
        good=GOOD, host=dict(refusals.BOX, init=ctypes.c_double), optional=OPTIONAL, cases=CASES,
        sizes=dict(need=lambda a: RR.workspace_bytes(a["P"], a["N"], a["box_min"], a["box_max"], a["cell"]),
                   normals=lambda a: normals_ref.workspace_bytes(a["P"], a["box_min"], a["box_max"], a["cell"]))),
    "mvs_query_register_workspace": dict(good=GOOD, host=refusals.BOX, cases=Q_CASES),
}


def child():
    """tests/refusals.py's child over the header of include/ext/: the same records, the same call builder."""
    from scene_3dreconstruction_mvsnet_amd import _lib
    lib = _lib.load()
    protos = refusals.prototypes(HEADER)

    def sentinel():
        assert lib.mvs_query_feature_workspace(1, 3, 2, ctypes.byref(ctypes.c_size_t(0))) == BAD_SHAPE
        return lib.mvs_last_error_string().decode("utf-8", "replace")
    for name, spec in REGISTER_REFUSALS.items():
        for lab, ov, want, _ in spec["cases"]:
            before = sentinel()
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=None, err="")), flush=True)      # about to call
            got, err = refusals.call(lib, protos, name, spec, ov)
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=got, err=err, stale=err == before)), flush=True)


_child = {}


def records():
    import gpu_child
    if not _child:
        r = gpu_child.run_once(("register refusals",), ["test_cloud_register_host.py", "child"], timeout=300, gpu=False)
        _child["r"], _child["records"] = r, {(rec["ep"], rec["case"]): rec for rec in r.records("R ")}
    return _child["r"], _child["records"]


@pytest.mark.parametrize("name", list(REGISTER_REFUSALS))
def test_every_refusal_comes_with_its_status_and_its_message_in_a_child_without_a_device(name):
    r, recs = records()
    spec = REGISTER_REFUSALS[name]
    labels = [c[0] for c in spec["cases"]]
    assert len(set(labels)) == len(labels)
    bad = [f"{lab}: {why}" for lab, _, want, text in spec["cases"] for why in [refusals.wrong(recs.get((name, lab)), want, text)] if why]
    assert not bad, f"{len(bad)} of {len(labels)} cases:\n" + "\n".join(bad)
    assert r.returncode == 0, r.stderr[-2000:]


def test_every_pointer_and_count_of_the_prototypes_has_its_cases():
    """what tests/test_abi_domain_host.py asks of the headers of include/*.h"""
    protos = refusals.prototypes(HEADER)
    assert set(protos) == set(REGISTER_REFUSALS)
    for name, params in protos.items():
        spec = REGISTER_REFUSALS[name]
        nulled = {k for _, ov, code, _ in spec["cases"] if code == NULL for k, v in ov.items() if v is None}
        for kind, p in params:
            if kind == "ptr" and p != "stream":
                assert p in nulled or p in spec.get("optional", ()), (name, p)
            if kind in ("long long", "int") and p not in ("target_dtype", "source_dtype"):
                assert any(p in ov and isinstance(ov[p], int) and ov[p] < 0 for _, ov, code, _ in spec["cases"] if code == BAD_SHAPE), (name, p)
        # an optional pointer is shown to be optional: NULL, and the call goes on to the workspace check
        for p in spec.get("optional", ()):
            assert any(ov.get(p, 0) is None and p in ov and code != NULL for _, ov, code, _ in spec["cases"]), (name, p)


# ---------------------------------------------------------------- declarations
from scene_3dreconstruction_mvsnet_amd import _lib, eval_cloud, fusion, reconstruct  # noqa: E402


def test_register_symbols_are_the_declarations_of_the_register_header():
    """refusals.check_header's assertions, for the table of include/ext/"""
    declared = [name for name, _ in refusals.declarations(HEADER)]
    assert declared == list(_lib._ABI_EXT[HEADER]) == list(_lib.REGISTER_SYMBOLS) == ["mvs_query_register_workspace", "mvs_cloud_register"]
    assert sorted(_lib._ABI_EXT) == sorted("ext/" + f for f in os.listdir(os.path.join(REPO, "include", "ext")))
    assert sorted(_lib._ABI) == refusals.HEADERS                     # the other table is untouched by this one
    for other in refusals.HEADERS:
        assert not set(declared) & set(_lib._ABI[other]), other
        assert not set(declared) & {name for name, _ in refusals.declarations(other)}, other
    kinds = refusals.header_argtypes(HEADER)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert _lib._ABI_EXT[HEADER][name] == kinds[name], name
        assert list(getattr(_lib.load(), name).argtypes) == kinds[name], name
        assert getattr(_lib.load(), name).restype is ctypes.c_int and hasattr(raw, name), name
    src = refusals.header_text(HEADER)
    for name, value in (("ITERATIONS_MAX", _lib.REGISTER_ITERATIONS_MAX), ("TERMS", _lib.REGISTER_TERMS),
                        ("HISTORY", _lib.REGISTER_HISTORY), ("GROUP", _lib.REGISTER_GROUP), ("FANIN", _lib.REGISTER_FANIN),
                        ("SCALARS", _lib.REGISTER_SCALARS)):
        assert refusals.define(src, "MVS_REGISTER_" + name) == value == getattr(RR, name), name
    assert refusals.define(src, "MVS_REGISTER_JACOBI_SWEEPS") == RR.JACOBI_SWEEPS
    for code, word in _lib.REGISTER_STOPS.items():
        assert refusals.define(src, "MVS_REGISTER_STOP_" + word.upper()) == code == getattr(RR, word.upper())
    assert "moves to include/" in src and "Nothing here was compared against Open3D" in src


# ---------------------------------------------------------------- workspace formula
@pytest.mark.parametrize("P,N,lo,hi,cell", [(5000, 3000, BIN[0], BIN[1], 5.0), (0, 3000, BIN[0], BIN[1], 5.0),
                                            (5000, 0, BIN[0], BIN[1], 5.0), (0, 0, BIN[0], BIN[1], 5.0),
                                            (7, 1, BIN[0], BIN[1], 2.5), (7, 32, BIN[0], BIN[1], 2.5), (7, 33, BIN[0], BIN[1], 2.5),
                                            (4097, 32 * 256, (-300, -200, -50), (300, 200, 150), 7.3),
                                            (4097, 32 * 256 + 1, (-300, -200, -50), (300, 200, 150), 7.3),
                                            (3, 32 * 256 * 256 + 1, (0, 0, 0), (0, 0, 0), 1.0),
                                            ((1 << 31) - 1, (1 << 31) - 1, (0, 0, 0), (1289, 1289, 1289), 1.0)])
def test_register_workspace_query_agrees_with_the_headers_formula(P, N, lo, hi, cell):
    want = RR.workspace_bytes(P, N, lo, hi, cell)
    assert _lib.query_register_workspace(P, N, lo, hi, cell) == want and want % 8 == 0
    assert _lib.query_register_workspace(P, N, lo, hi, cell, max_iterations=0) == want      # it does not depend on it
    assert want - _lib.query_normals_workspace(P, lo, hi, cell) == 8 * 31 * sum(RR.levels(N)) + 512
    shapes = {0: [], 1: [1], 32: [1], 33: [2, 1], 8192: [256, 1], 8193: [257, 2, 1], 2097153: [65537, 257, 2, 1]}
    if N in shapes:
        assert RR.levels(N) == shapes[N]
    assert RR.tree_depth(0) == 0 and RR.tree_depth(32) == 5 and RR.tree_depth(33) == 13 and RR.tree_depth(8193) == 21


# ---------------------------------------------------------------- the yardstick against independent formulations
def _surface(P, seed, jitter=0.0, lattice=False):
    """P points of a curved sheet with its unit normals; lattice: on a 20-column lattice of spacing 0.3 x 0.2 instead of
    scattered, so that no two points are nearer than 0.2"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-3, 3, P), rng.uniform(-2, 2, P)
    if lattice:
        u, v = -2.85 + 0.3 * (np.arange(P) % 20), -1.9 + 0.2 * (np.arange(P) // 20)
    xyz = np.column_stack([u, v, 0.4 * np.sin(u) * np.cos(1.3 * v) + 0.05 * u * v])
    n = np.column_stack([-(0.4 * np.cos(u) * np.cos(1.3 * v) + 0.05 * v), -(-0.52 * np.sin(u) * np.sin(1.3 * v) + 0.05 * u), np.ones(P)])
    return xyz + rng.normal(0, jitter, xyz.shape), n / np.linalg.norm(n, axis=1, keepdims=True)


def test_the_tree_sum_is_the_pairing_of_the_outliers_tree_and_within_its_bound():
    import outliers_ref
    rng = np.random.default_rng(0)
    for N in (1, 31, 32, 33, 63, 64, 65, 8192, 8193, 70000):
        x = rng.normal(size=(N, 3)) * 10.0 ** rng.integers(-3, 4, (N, 3))
        tree, exact = RR.tree_sums(x), RR.exact_sums(x)
        assert (np.abs(tree - exact) <= RR.sum_bound(x)).all() and (RR.sum_bound(x) < 1e-12 * np.abs(x).sum(axis=0)).all()
        if N <= 32:      # one group: the balanced pairwise sum of mvs_outliers_abi.h itself
            assert all(tree[k] == outliers_ref.tree_sum(x[:, k]) for k in range(3))
    ones = np.ones((70000, 1))
    assert RR.tree_sums(ones)[0] == 70000.0


def test_kabsch_agrees_with_scipy_and_the_step_recovers_a_known_motion():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    for deg in (0.5, 30.0, 179.0):
        rot = Rotation.from_rotvec(np.deg2rad(deg) * np.array([0.6, 0.0, 0.8]))
        s = rng.normal(size=(300, 3)) * (3, 2, 1)
        q = rot.apply(s) + rng.normal(0, 0.01, s.shape)
        S = (s - s.mean(0)).T @ (q - q.mean(0))
        R = RR.kabsch(S)
        want = Rotation.align_vectors(q - q.mean(0), s - s.mean(0))[0].as_matrix()
        assert np.abs(R - want).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        # the eigenvector of Horn's matrix is the same rotation
        w, V = np.linalg.eigh(RR.horn_matrix(S))
        assert np.abs(Rotation.from_quat(np.roll(V[:, -1], -1)).as_matrix() - R).max() < 1e-12
    # a mirrored cloud: the unconstrained optimum is a reflection, the determinant fix gives the proper rotation
    S = (s - s.mean(0)).T @ ((s * (-1, 1, 1)) - (s * (-1, 1, 1)).mean(0))
    assert abs(np.linalg.det(RR.kabsch(S)) - 1) < 1e-12
    # one step from exact correspondences: point-to-point lands on the motion, point-to-plane close to it
    tgt, nrm = _surface(400, 5, lattice=True)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rotation.from_rotvec([0.01, -0.02, 0.015]).as_matrix(), (0.02, -0.01, 0.03)
    src = RR.image(np.linalg.inv(T), tgt)
    box = ((-4.0, -3.0, -2.0), (4.0, 3.0, 2.0))
    for normals, tol in ((None, 1e-12), (nrm, 2e-3)):
        ev = RR.evaluate(np.eye(4), src, tgt, normals, *box, 0.5)
        assert (ev["idx"] == np.arange(400)).all()
        dT = RR.step(RR.exact_sums(ev["terms"]), normals is not None, (0.0, 0.0, 0.0))
        assert np.abs(dT - T).max() < tol, np.abs(dT - T).max()


def test_the_loop_on_the_cpu_converges_counts_and_stops_as_the_header_says():
    tgt, nrm = _surface(400, 7, lattice=True)
    box = ((-4.0, -3.0, -2.0), (4.0, 3.0, 2.0))
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rotation.from_rotvec(np.deg2rad(2.0) * np.array([0, 0.6, 0.8])).as_matrix(), (0.05, 0.02, -0.03)
    src = RR.image(np.linalg.inv(T), tgt[::2])
    src[5] = np.nan
    for normals in (None, nrm):
        got = RR.icp(src, tgt, *box, 0.5, normals=normals, max_iterations=40, bounds=True)
        assert got["counts"][0] == 199 and got["counts"][3] == RR.CONVERGED and got["counts"][2] < 40
        assert np.abs(got["T"] - T).max() < 1e-6 and got["stats"][0] == 1.0 and got["stats"][1] < 1e-6
        assert np.isnan(got["history"][got["counts"][2] + 1:]).all() and np.isfinite(got["history"][:got["counts"][2] + 1]).all()
        assert got["bound"].max() < 1e-9 and got["gap"] > 0
    far = RR.icp(src + 100.0, tgt, *box, 0.5, max_iterations=5)
    assert far["counts"] == [199, 0, 0, RR.DEGENERATE] and (far["T"] == np.eye(4)).all()
    zero = RR.icp(src, tgt, *box, 0.5, max_iterations=0)
    assert zero["counts"][2:] == [0, RR.MAX_ITERATIONS] and (zero["T"] == np.eye(4)).all()
    same = RR.icp(tgt, tgt, *box, 0.5, normals=nrm, max_iterations=5)
    assert same["counts"][2:] == [1, RR.CONVERGED] and (same["T"] == np.eye(4)).all() and same["stats"].tolist() == [1.0, 0.0]


# ---------------------------------------------------------------- the solver header, under the host sanitizers
CXX = "/opt/rocm/llvm/bin/clang++"      # the host compiler of the toolchain that builds the library


@pytest.fixture(scope="module")
def solver_lines(tmp_path_factory):
    """tests/register_solve_host.cpp: csrc/cloud_register_solve.h as a stand-alone host program built with the address and
    undefined-behaviour sanitizers (nothing is preloaded, nothing is loaded into Python, no GPU)."""
    assert os.path.exists(CXX), CXX
    exe = tmp_path_factory.mktemp("solve") / "register_solve_host"
    subprocess.run([CXX, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "scene_3dreconstruction_mvsnet_amd", "csrc"),
                    os.path.join(REPO, "tests", "register_solve_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    out = {}
    for ln in lines[:-1]:
        tag, _, rest = ln.partition(" ")
        left, _, right = rest.partition(" -> ")
        out.setdefault(tag, []).append(([float.fromhex(t) for t in left.split()], [float.fromhex(t) for t in right.split()]))
    return out


def test_the_ldlt_solve_against_numpy_within_the_solve_bound(solver_lines):
    cases = solver_lines["ldlt"]
    assert len(cases) == 13
    solved = conds = 0
    for left, right in cases:
        A, b, ok, x = np.array(left[:36]).reshape(6, 6), np.array(left[36:]), right[0], np.array(right[1:])
        d = RR.ldlt_pivots(A)
        assert ok == float(len(d) == 6 and all(v > 0 for v in d))        # the same operations, the same pivots, the same verdict
        cond = np.linalg.cond(A)
        if ok and cond < 1e13:
            want = np.linalg.solve(A, -b)
            g = 19 * RR.U
            bound = 2 * 6 * g * cond * np.linalg.norm(want) / (1 - 2 * 6 * g * cond)        # both solves' backward errors
            assert np.linalg.norm(x - want) <= bound, (cond, np.linalg.norm(x - want), bound)
            solved += 1
            conds = max(conds, cond)
    assert solved >= 11 and conds > 1e8 and any(right[0] == 0.0 for _, right in cases)


def test_horns_rotation_against_kabsch_up_to_179_degrees_and_on_mirrored_sets(solver_lines):
    cases = solver_lines["horn"]
    assert len(cases) == 20
    worst = 0.0
    for k, (left, right) in enumerate(cases):
        S, ok, R = np.array(left).reshape(3, 3), right[0], np.array(right[1:]).reshape(3, 3)
        assert ok == 1.0
        assert np.abs(R @ R.T - np.eye(3)).max() < 64 * RR.U and abs(np.linalg.det(R) - 1) < 64 * RR.U      # proper, always
        lam = np.linalg.eigvalsh(RR.horn_matrix(S))
        Nf = np.linalg.norm(RR.horn_matrix(S), "fro")
        if lam[-1] - lam[-2] > 1e-6 * Nf:                                  # the optimum is unique: all but the collinear set
            dN = 2 * 60 * 8 * RR.U * Nf
            dq = dN / (lam[-1] - lam[-2] - dN)
            bound = 2 * dq * (1 + dq) + 16 * RR.U
            err = np.abs(R - RR.kabsch(S)).max()
            assert err <= bound, (k, err, bound)
            worst = max(worst, err / bound)
        else:
            assert k == 19
        # optimal in any case: no rotation has a larger trace(R S)
        assert np.trace(R @ S) >= np.trace(RR.kabsch(S) @ S) - 1e-12 * Nf
    print("worst error / bound of Horn's rotation:", worst)


def test_the_matrix_of_a_6_vector_the_product_and_the_two_steps(solver_lines):
    for left, right in solver_lines["vec6"]:
        assert np.abs(np.array(right).reshape(4, 4) - RR.vector6_to_matrix(left)).max() <= 16 * RR.U
    assert solver_lines["vec6"][0][1] == np.eye(4).reshape(-1).tolist()                      # x = 0 is the identity exactly
    for left, right in solver_lines["compose"]:
        A, B = np.array(left[:16]).reshape(4, 4), np.array(left[16:]).reshape(4, 4)
        assert np.array(right).tobytes() == RR.compose(A, B).reshape(-1).tobytes()           # the same operations, the same bits
    assert len(solver_lines["plane"]) == 3 and len(solver_lines["point"]) == 2
    for left, right in solver_lines["plane"][:2]:
        sums, dT = np.array(left), np.array(right[1:]).reshape(4, 4)
        assert right[0] == 1.0
        bound = RR.plane_step_bound(sums, np.zeros(31))
        assert (np.abs(dT - RR.step(sums, True, None)) <= bound).all(), (np.abs(dT - RR.step(sums, True, None)) / bound).max()
    sums = np.array(solver_lines["plane"][2][0])
    d = RR.ldlt_pivots(RR.plane_system(sums)[0])
    assert solver_lines["plane"][2][1][0] == float(len(d) == 6 and all(v > 0 for v in d))
    for left, right in solver_lines["point"]:
        sums, o, dT = np.array(left[:31]), np.array(left[31:]), np.array(right[1:]).reshape(4, 4)
        assert right[0] == 1.0
        bound = RR.point_step_bound(sums, np.zeros(31), o)
        assert (np.abs(dT - RR.step(sums, False, o)) <= bound).all(), (np.abs(dT - RR.step(sums, False, o)) / bound).max()


# ---------------------------------------------------------------- the wrapper's calls against the recording stand-in
def test_the_wrapper_hands_over_only_pointers_the_entry_point_can_take():
    """tests/wrapper_contract.py's harness on the one wrapper of the table of include/ext/: the prototype and the extents
    of the header are lent to its tables for the duration of this test and taken back."""
    import torch
    import wrapper_contract as WC
    name = "mvs_cloud_register"
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    extents = dict(WC._BOX, target_xyz=WC._xyz("target_dtype", "P"),
                   target_normals=WC.Ptr(lambda a: f64 if a["target_dtype"] == 1 else f32,
                                         lambda a: a["P"] * 3 * (8 if a["target_dtype"] == 1 else 4), True),
                   source_xyz=WC._xyz("source_dtype", "N"), init=WC.HOSTP_NULL, transform_out=WC.Ptr(f64, lambda a: 128),
                   counts_out=WC.Ptr(i64, lambda a: 32), stats_out=WC.Ptr(f64, lambda a: 16),
                   history_out=WC.Ptr(f64, lambda a: (a["max_iterations"] + 1) * 19 * 8, True),
                   system_out=WC.Ptr(f64, lambda a: a["max_iterations"] * 31 * 8, True),
                   idx_out=WC.Ptr(i32, lambda a: a["N"] * 4, True), workspace=WC.WS)
    protos = refusals.prototypes(HEADER)
    assert {p for kind, p in protos[name] if kind == "ptr" and p != "stream"} == set(extents)      # every pointer's extent

    def build(m):
        return dict(WC.BOX, target=WC._cloud(m), source=WC._cloud(m, 32), cell=2.0, max_dist=4.0, target_normals=m.f(64, 3),
                    init=np.eye(4), max_iterations=3, history=True, systems=True, indices=True,
                    out=(m.f(4, 4, dtype=f64), m.ints([0] * 4, i64), m.f(2, dtype=f64), m.f(4, 19, dtype=f64),
                         m.f(3, 31, dtype=f64), m.ints([0] * 32)))
    roles = dict(target="in", source="in", target_normals="in", **{f"out[{k}]": "out" for k in range(6)})
    case = WC.Unaligned("cloud_register", _lib.cloud_register, build, roles, [name])
    saved = WC.DEVICE_ENTRIES, WC.FORWARDED
    WC.PROTOS[name], WC.EXTENTS[name] = protos[name], extents
    WC.DEVICE_ENTRIES, WC.FORWARDED = saved[0] + (name,), saved[1] + ("mvs_query_register_workspace",)
    try:
        verdict, detail, called = WC.run_case(case, "fake")
        assert (verdict, called) == ("honest", [name]), detail
        rows = WC.table_rows(case)
        assert len(rows) >= 9 * 6
        for leaf, defect in rows:
            want = WC.default_expectation(roles[leaf], defect)
            verdict, detail, _ = WC.run_case(case, "fake", leaf, defect)
            # a target of another dtype or length: its normals no longer fit it; a shorter source: neither does out's idx
            if leaf == "source" and defect == "dtype:float64":                  # either dtype is the header's
                want = "honest"
            assert verdict == want, (leaf, defect, verdict, detail)
        assert WC.run_case(case, "fake", "target_normals", "dtype:float64")[0] == "refused"      # normals of another dtype
    finally:
        del WC.PROTOS[name], WC.EXTENTS[name]
        WC.DEVICE_ENTRIES, WC.FORWARDED = saved
    assert name not in WC.PROTOS and name not in WC.EXTENTS and name not in WC.DEVICE_ENTRIES


# ---------------------------------------------------------------- the Python layer, before any GPU work
def test_python_functions_refuse_host_tensors_and_bad_options():
    import torch
    xyz = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="xyz must be a CUDA"):
        _lib.cloud_register(xyz, xyz, *BIN, 5.0, 20.0)
    with pytest.raises(RuntimeError, match="source must be a CUDA"):
        fusion.register_cloud(xyz, xyz, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        fusion.evaluate_cloud(xyz, xyz, register=dict(max_dist=1.0))
    with pytest.raises(ValueError, match="max_dist"):
        fusion.evaluate_cloud(xyz, xyz, register=dict(knn=5))
    with pytest.raises(ValueError, match="unknown"):
        fusion.evaluate_cloud(xyz, xyz, register=dict(max_dist=1.0, scale=True))
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    moved = fusion.transform_cloud(torch.tensor([[1.0, 0.0, 0.0], [float("nan"), 0, 0]]), T)
    assert moved.dtype == torch.float32 and moved[0].tolist() == [1.0, 3.0, 3.0] and torch.isnan(moved[1]).all()
    with pytest.raises(SystemExit):
        reconstruct.main(["--testpath", "x", "--testlist", "y", "--loadckpt", "z", "--register_dist", "2"])      # needs --gt_ply


def test_the_command_lines_take_the_register_flags(monkeypatch, tmp_path):
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def parse(self, argv=None):
        args = real(self, argv)
        seen.update(vars(args))
        return args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    with pytest.raises(Exception):          # no such file: whatever stops the run, the arguments were parsed
        eval_cloud.main(["--pred", str(tmp_path / "a.ply"), "--gt", str(tmp_path / "b.ply"), "--register_dist", "2.5",
                         "--register_iters", "12", "--register_point_to_point"])
    assert seen["register_dist"] == 2.5 and seen["register_iters"] == 12 and seen["register_point_to_point"] is True
    args = argparse.Namespace(**seen)
    assert eval_cloud.register_options(args) == dict(max_dist=2.5, max_iterations=12, point_to_plane=False)
    seen.clear()
    with pytest.raises(Exception):
        eval_cloud.main(["--pred", str(tmp_path / "a.ply"), "--gt", str(tmp_path / "b.ply")])
    assert seen["register_dist"] is None and seen["register_iters"] == 30 and seen["register_point_to_point"] is False
    assert eval_cloud.register_options(argparse.Namespace(**seen)) is None
    seen["register_iters"] = 5
    with pytest.raises(SystemExit):
        eval_cloud.register_options(argparse.Namespace(**seen))
    seen.clear()
    with pytest.raises(Exception):
        reconstruct.main(["--testpath", "/nonexistent/x", "--testlist", "/nonexistent/y", "--loadckpt", "/nonexistent/z",
                          "--gt_ply", "g.ply", "--register_dist", "4"])
    assert seen["register_dist"] == 4.0 and seen["register_iters"] == 30


if __name__ == "__main__":
    if sys.argv[1:2] == ["child"]:
        child()
