"""The GPU checks of mvs_cloud_register, run as a child of tests/test_gpu_cloud_register.py (through tests/gpu_child.py):

    python tests/register_check.py GROUP        GROUP: edges | sums | dense | loop | evaluate

Every check prints one record, `R {"check": name, "ok": bool, "why": text, ...figures}`; a check that fails does not stop
the ones after it, a HIP error ends the child at once with a non-zero status.  The scenes are seeded and built here; the
references are tests/register_ref.py's, on the CPU.  Nothing is run twice to make it pass and nothing is made to fault."""
import json
import os
import sys
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _path in (REPO, HERE):
    if _path not in sys.path:
        sys.path.insert(0, _path)

import guarded as G  # noqa: E402
import register_ref as RR  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, fusion  # noqa: E402

DEV = torch.device("cuda:0")
BOX = ((-4.0, -3.0, -2.0), (4.0, 3.0, 2.0))
NAMES = ("T", "counts", "stats", "history", "systems", "idx")


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def surface(P, seed, dtype=np.float64):
    """P seeded points of a curved sheet inside BOX and their unit normals."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-3, 3, P), rng.uniform(-2, 2, P)
    xyz = np.column_stack([u, v, 0.4 * np.sin(u) * np.cos(1.3 * v) + 0.05 * u * v])
    n = np.column_stack([-(0.4 * np.cos(u) * np.cos(1.3 * v) + 0.05 * v), 0.52 * np.sin(u) * np.sin(1.3 * v) - 0.05 * u, np.ones(P)])
    return xyz.astype(dtype), (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(dtype)


def motion(degrees, axis, t):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.deg2rad(degrees) * np.asarray(axis, float) / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = t
    return T


def run(target, source, box=BOX, cell=0.25, max_dist=0.5, normals=None, init=None, its=5, rel=1e-6, tensors=False):
    out = _lib.cloud_register(target if torch.is_tensor(target) else cu(target), source if torch.is_tensor(source) else cu(source),
                              box[0], box[1], cell, max_dist, target_normals=None if normals is None else cu(normals), init=init,
                              max_iterations=its, rel_fitness=rel, rel_rmse=rel, history=True, systems=True, indices=True)
    torch.cuda.synchronize()
    if tensors:
        return out
    got = {k: v.cpu().numpy() for k, v in zip(NAMES, out)}
    assert got["T"].shape == (4, 4) and got["history"].shape == (its + 1, 19) and got["systems"].shape == (its, 31)
    return got


def same_bytes(a, b):
    return all(torch.equal(G.raw_bytes(u), G.raw_bytes(v)) for u, v in zip(a, b))


# ---------------------------------------------------------------- edges
def check_empty_and_single_clouds():
    tgt, nrm = surface(200, 1)
    out = {}
    for name, t, s in (("N=0", tgt, tgt[:0]), ("P=0", tgt[:0], tgt[:5]), ("both", tgt[:0], tgt[:0])):
        for its in (0, 4):
            got = run(t, s, its=its)
            want = [0 if len(s) == 0 else 5, 0, 0, RR.DEGENERATE if its else RR.MAX_ITERATIONS]
            assert got["counts"].tolist() == want and (got["T"] == np.eye(4)).all() and got["stats"].tolist() == [0.0, 0.0], (name, its, got)
            assert (got["history"][0] == list(np.eye(4).reshape(-1)) + [0.0, 0.0, 0.0]).all() and np.isnan(got["history"][1:]).all()
            assert np.isnan(got["systems"]).all() and (got["idx"] == -1).all()
    # one source, one member: a pair is too few for a step, and is evaluated all the same
    got = run(np.array([[1.0, 0.5, 0.25]]), np.array([[1.0, 0.5, 0.5]]), its=3)
    assert got["counts"].tolist() == [1, 1, 0, RR.DEGENERATE] and got["stats"].tolist() == [1.0, 0.25] and got["idx"].tolist() == [0]
    got = run(tgt, tgt[7:8], normals=nrm, its=3)
    assert got["counts"].tolist() == [1, 1, 0, RR.DEGENERATE] and got["stats"].tolist() == [1.0, 0.0] and got["idx"].tolist() == [7]
    got = run(tgt[:1], tgt[:40], max_dist=np.inf, its=3)          # forty sources on one member: S is zero, any rotation is optimal
    assert got["counts"][:2].tolist() == [40, 40] and np.isfinite(got["T"]).all() and (got["idx"] == 0).all()
    return out


def check_sources_beyond_max_dist_and_zero_iterations():
    tgt, nrm = surface(500, 2)
    init = motion(3.0, (0, 0, 1), (0.01, 0.02, 0.0))
    for normals in (None, nrm):
        got = run(tgt, tgt[:100] + (0.0, 0.0, 50.0), normals=normals, init=init, its=6)
        assert got["counts"].tolist() == [100, 0, 0, RR.DEGENERATE] and got["T"].tobytes() == init.tobytes()
        assert got["stats"].tolist() == [0.0, 0.0] and (got["idx"] == -1).all() and np.isnan(got["history"][1:]).all()
        got = run(tgt, tgt[:100], normals=normals, init=init, its=0)
        ev = RR.evaluate(init, tgt[:100], tgt, normals, *BOX, 0.5)
        sums = RR.exact_sums(ev["terms"])
        assert got["counts"].tolist() == [100, int(sums[1]), 0, RR.MAX_ITERATIONS] and got["T"].tobytes() == init.tobytes()
        assert (got["idx"] == ev["idx"]).all() and got["systems"].shape == (0, 31)
        assert got["stats"][0] == RR.fitness_rmse(sums)[0] and abs(got["stats"][1] - RR.fitness_rmse(sums)[1]) <= 1e-14
    return {}


def check_a_source_aliasing_the_target():
    tgt, nrm = surface(700, 3, np.float32)
    for normals in (None, nrm):
        t = cu(tgt)
        out = run(t, t, normals=normals, its=9, tensors=True)
        got = {k: v.cpu().numpy() for k, v in zip(NAMES, out)}
        assert got["counts"].tolist() == [700, 700, 1, RR.CONVERGED], got["counts"]
        assert (got["T"] == np.eye(4)).all() and got["stats"].tolist() == [1.0, 0.0] and (got["idx"] == np.arange(700)).all()
        assert np.isfinite(got["history"][:2]).all() and np.isnan(got["history"][2:]).all()
        assert np.isfinite(got["systems"][:1]).all() and np.isnan(got["systems"][1:]).all()
    return {}


def check_ties_and_nan_rows():
    # a source midway between two members takes the smaller index, wherever that member stands in the array
    lattice = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0], [2.0, 2.0, 0], [0.0, 0.0, 2.0], [2.0, 2.0, 2.0]])
    src = np.array([[1.0, 0, 0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0], [np.nan, 0, 0], [0.0, np.inf, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 1.0]])
    box = ((-1.0, -1.0, -1.0), (3.0, 3.0, 3.0))
    for perm in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [1, 3, 0, 5, 2, 4]):
        for cell in (0.5, 1.0, 100.0):
            got = run(lattice[perm], src, box=box, cell=cell, max_dist=5.0, its=0)
            ev = RR.evaluate(np.eye(4), src, lattice[perm], None, *box, 5.0)
            assert got["idx"].tolist() == ev["idx"].tolist(), (perm, cell, got["idx"], ev["idx"])
            assert got["idx"][0] == min(perm.index(0), perm.index(1)) and got["idx"][3] == -1 and got["idx"][4] == -1
            assert got["counts"][:2].tolist() == [5, 5]
    # NaN rows are not counted: a cloud with every other row blanked registers like the rows that are left
    tgt, nrm = surface(900, 4)
    T = motion(1.0, (1, 2, 3), (0.02, -0.01, 0.015))
    src = RR.image(np.linalg.inv(T), tgt[:400])
    blank = src.copy()
    blank[1::2] = np.nan
    a, b = run(tgt, blank, normals=nrm, its=8), run(tgt, src[0::2], normals=nrm, its=8)
    assert a["counts"].tolist() == b["counts"].tolist() and a["counts"][0] == 200 and (a["idx"][1::2] == -1).all()
    assert (a["idx"][0::2] == b["idx"]).all() and np.abs(a["T"] - b["T"]).max() < 1e-12 and np.abs(a["T"] - T).max() < 1e-6
    return {}


def check_exact_lattice_probes():
    """Integer coordinates, axis-aligned normals, identity init: every term and every partial sum is an integer far below
    2^53, so the sums have one value whatever the order and system_out's row 0 is the reference's, bit for bit."""
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(-8.0, 9.0), np.arange(-6.0, 7.0), indexing="ij")
    step = np.where(gx.ravel() > 0, 2.0, 0.0)
    tgt = np.column_stack([gx.ravel(), gy.ravel(), step])
    nrm = np.zeros_like(tgt)
    nrm[:, 2] = 1.0
    nrm[gx.ravel() == 1] = (1.0, 0.0, 0.0)                                 # the riser of the step
    nrm[gy.ravel() == 3] = (0.0, 1.0, 0.0)                                 # and a row that faces along y: three families of planes
    src = tgt[rng.permutation(len(tgt))[:150]] + rng.integers(-1, 2, (150, 3)) * (0.0, 0.0, 1.0) + (rng.random(150) < 0.1)[:, None] * (0.0, 0.0, 20.0)
    box = ((-8.0, -6.0, -2.0), (8.0, 6.0, 4.0))
    out = {}
    for name, normals in (("point", None), ("plane", nrm)):
        for dt in (np.float32, np.float64):
            got = run(tgt.astype(dt), src.astype(dt), box=box, cell=1.0, max_dist=1.5, normals=None if normals is None else normals.astype(dt), its=1)
            ev = RR.evaluate(np.eye(4), src, tgt, normals, *box, 1.5)
            want = RR.exact_sums(ev["terms"])
            assert (ev["terms"] == np.round(ev["terms"] * 4) / 4).all() and 0 < want[1] < want[0] == 150
            assert RR.step(want, normals is not None, (0.0, 0.0, 1.0)) is not None and got["counts"][2] == 1, got["counts"]
            # + 0.0: a sum of zeros of either sign is a zero of either sign; every other value has one representation
            assert (got["systems"][0] + 0.0).tobytes() == (want + 0.0).tobytes(), (name, got["systems"][0], want)
            assert (got["history"][0, 16:] == [want[1] / want[0], np.sqrt(want[2] / want[1]), want[1]]).all()
            out[name] = int(want[1])
    return out


def check_refusals_on_the_device_build():
    tgt, nrm = surface(100, 6)
    t, s = cu(tgt), cu(tgt[:10])
    for kw, code in ((dict(cell=-1.0), 1), (dict(cell=float("nan")), 1), (dict(box_min=(5.0, 0, 0)), 1)):
        args = dict(box_min=BOX[0], box_max=BOX[1], cell=0.25)
        args.update(kw)
        try:
            _lib.cloud_register(t, s, args["box_min"], args["box_max"], args["cell"], 0.5)
            raise AssertionError(f"{kw} was not refused")
        except _lib.MvsError as e:
            assert e.code == code, (kw, e)
    for kw, text in ((dict(max_iterations=-1), "max_iterations"), (dict(max_iterations=1001), "max_iterations"), (dict(rel_rmse=-1.0), "rel_rmse"),
                     (dict(init=np.full((4, 4), np.nan)), "init"), (dict(init=2 * np.eye(4)), "init"), (dict(init=np.eye(3)), "init"),
                     (dict(init=cu(np.eye(4))), "host"), (dict(target_normals=cu(nrm).float()), "target_normals"),
                     (dict(target_normals=cu(nrm[:50])), "target_normals")):
        try:
            _lib.cloud_register(t, s, *BOX, 0.25, 0.5, **kw)
            raise AssertionError(f"{list(kw)} was not refused")
        except RuntimeError as e:
            assert text in str(e) and not isinstance(e, _lib.MvsError), (kw, e)
    try:
        _lib.cloud_register(t, s, *BOX, 0.25, -0.5)
        raise AssertionError("max_dist < 0 was not refused")
    except RuntimeError as e:
        assert "max_dist" in str(e)
    torch.cuda.synchronize()
    return {}


def check_determinism_and_no_host_synchronisation():
    tgt, nrm = surface(3000, 7, np.float32)
    src = RR.image(np.linalg.inv(motion(2.0, (1, 1, 3), (0.03, -0.02, 0.02))), tgt[:1100].astype(np.float64)).astype(np.float32)
    t, s, n = cu(tgt), cu(src), cu(nrm)
    out = {}
    for name, normals in (("point", None), ("plane", n)):
        call = lambda cell: _lib.cloud_register(t, s, *BOX, cell, 0.5, target_normals=normals, max_iterations=6, history=True,  # noqa: E731
                                                systems=True, indices=True)
        runs = [call(c) for c in (0.25, 0.25, 0.1, 100.0)]           # two runs, a finer grid, one cell
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            runs.append(call(0.25))
        side.synchronize()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            runs.append(call(0.25))
            reg = fusion.register_cloud(s, t, 0.5, target_normals=normals, max_iterations=6, box=BOX, cell=0.25)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        for k, other in enumerate(runs[1:]):
            assert same_bytes(runs[0], other), (name, k)
        assert same_bytes((reg["transformation"], reg["history"]), (runs[0][0], runs[0][3]))
        assert reg["iterations"].item() == runs[0][1][2].item() and reg["stop"].item() == runs[0][1][3].item()
        assert reg["fitness"].item() == runs[0][2][0].item() and reg["inlier_rmse"].item() == runs[0][2][1].item()
        out[name] = runs[0][1].tolist()
        assert out[name][2] >= 2 and out[name][1] > 1000
    return out


def check_guarded_buffers():
    tgt, nrm = surface(1500, 8, np.float32)
    src = RR.image(np.linalg.inv(motion(1.0, (0, 1, 3), (0.02, 0.01, 0.0))), tgt[:333].astype(np.float64))
    out = {}
    for name, P, N, normals, extras in (("plane", 1500, 333, nrm, True), ("point", 1500, 333, None, False), ("P=0", 0, 33, None, True),
                                        ("N=1", 65, 1, None, True)):
        arena = G.Arena(32 << 20, DEV)
        seen = []

        def fn(a):
            t = a.put(cu(tgt[:P]), name="target") if P else cu(tgt[:P])
            s = a.put(cu(src[:N]), name="source")
            nn = None if normals is None else a.put(cu(normals), name="normals")
            with a.intercept(_lib):
                outs = _lib.cloud_register(t, s, *BOX, 0.25, 0.5, target_normals=nn, max_iterations=5, history=extras,
                                           systems=extras, indices=extras)
            torch.cuda.synchronize()
            if isinstance(a, G.Arena):
                roles = sorted(rec.role for rec in a.carved)
                assert roles == ["in"] * ((1 if P else 0) + 1 + (normals is not None)) + ["out"] * (6 if extras else 3) + ["scratch"], roles
                ws = [rec for rec in a.carved if rec.role == "scratch"][0]
                assert ws.tensor.numel() == RR.workspace_bytes(P, N, *BOX, 0.25)
                seen.append(a.poison)
            return outs
        guard_bytes = G.guarded_and_plain(arena, fn)
        assert seen == list(G.POISONS) and guard_bytes >= 8 * G.MIN_GUARD
        out[name] = fn(G.Plain(DEV))[1].tolist()
    assert out["plane"][3] == RR.CONVERGED or out["plane"][2] == 5
    return out


# ---------------------------------------------------------------- the sums at the boundaries of their tree
def check_reduction_boundaries():
    """N around one wave's and one block's share of sources, at one more than one level-1 partial sum covers and at one
    more than two levels cover.  Most sources of the long clouds are NaN rows, which cost no search; the counted ones sit
    at the ends of the groups and of the blocks.  system_out's row 0 against fsum within the sum bound."""
    tgt, nrm = surface(2000, 9)
    T = motion(1.5, (1, 0, 2), (0.02, 0.02, -0.01))
    pool = RR.image(np.linalg.inv(T), tgt)
    out = {}
    worst = 0.0
    for N in (31, 32, 33, 63, 64, 65, 255, 256, 257, 32 * 256 - 1, 32 * 256, 32 * 256 + 1, 32 * 256 * 256 + 1):
        rng = np.random.default_rng(N)
        if N <= 300:
            src = pool[rng.permutation(2000)[:N]]
        else:
            src = np.full((N, 3), np.nan)
            rows = np.unique(np.concatenate([rng.integers(0, N, 600), np.arange(0, 70), np.arange(N - 70, N),
                                             np.arange(8150, min(8250, N)), np.arange(N // 2 - 40, N // 2 + 40)]))
            src[rows] = pool[rng.integers(0, 2000, len(rows))]
        for normals in (None, nrm):
            got = run(tgt, src, normals=normals, its=1, max_dist=0.5)
            ev = RR.evaluate(np.eye(4), src, tgt, normals, *BOX, 0.5)
            exact, bound = RR.exact_sums(ev["terms"]), RR.sum_bound(ev["terms"])
            assert got["counts"][2] == 1 and got["history"][0, 18] == exact[1], (N, got["counts"])      # idx is evaluation 1's
            err = np.abs(got["systems"][0] - exact)
            assert (err <= bound).all(), (N, normals is not None, (err / np.maximum(bound, 1e-300)).max())
            assert (got["systems"][0][:2] == exact[:2]).all() and exact[1] > 25
            if N <= 32 * 256 + 1:      # the tree itself, literally: the same bytes
                assert got["systems"][0].tobytes() == RR.tree_sums(ev["terms"]).tobytes(), N
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        out[str(N)] = RR.levels(N)
    out["worst_ratio"] = worst
    return out


# ---------------------------------------------------------------- one step against the reference, dense
DENSE_SEED, DENSE_ITS = 11, 6


def dense_scene(dtype):
    tgt, nrm = surface(3000, DENSE_SEED, dtype)
    src, _ = surface(2000, DENSE_SEED + 1)
    src = RR.image(np.linalg.inv(motion(2.0, (1, -1, 3), (0.04, -0.03, 0.02))), src).astype(dtype)
    return tgt, nrm, src


def check_dense(dtype, plane):
    dtype = dict(f32=np.float32, f64=np.float64)[dtype]
    tgt, nrm, src = dense_scene(dtype)
    normals = nrm if plane else None
    origin = 0.5 * (np.asarray(BOX[0]) + np.asarray(BOX[1]))
    got = run(tgt, src, normals=normals, its=DENSE_ITS, rel=0.0)          # rel = 0: every step is taken
    assert got["counts"][2:].tolist() == [DENSE_ITS, RR.MAX_ITERATIONS]
    worst_sum = worst_step = 0.0
    gap = 1.0
    for k in range(DENSE_ITS + 1):
        Tk = got["history"][k, :16].reshape(4, 4)
        ev = RR.evaluate(Tk, src, tgt, normals, *BOX, 0.5, second=True)
        gap = min(gap, ev["gap"])
        assert ev["gap"] >= 1e-9, (k, ev["gap"])                           # the reference alone: no correspondence is a toss-up
        one = run(tgt, src, normals=normals, init=Tk, its=0)               # Evaluate(T_k) by itself: its correspondences
        assert (one["idx"] == ev["idx"]).all(), (k, int((one["idx"] != ev["idx"]).sum()))
        exact, bound = RR.exact_sums(ev["terms"]), RR.sum_bound(ev["terms"])
        fit, rmse = RR.fitness_rmse(exact)
        assert got["history"][k, 16] == fit and got["history"][k, 18] == exact[1] and abs(got["history"][k, 17] - rmse) <= 4 * RR.U * rmse + bound[2] / (2 * exact[1] * rmse)
        if k == DENSE_ITS:
            assert (got["idx"] == ev["idx"]).all()
            break
        err = np.abs(got["systems"][k] - exact)
        assert (err <= bound).all(), (k, (err / np.maximum(bound, 1e-300)).max())
        worst_sum = max(worst_sum, float((err[bound > 0] / bound[bound > 0]).max()))
        want = RR.compose(RR.step(exact, plane, origin), Tk)
        tb = RR.step_bound(exact, bound, plane, origin, Tk)
        terr = np.abs(got["history"][k + 1, :16].reshape(4, 4) - want)
        assert (terr[:3] <= tb[:3]).all(), (k, (terr[:3] / tb[:3]).max())
        worst_step = max(worst_step, float((terr[:3] / tb[:3]).max()))
    return dict(worst_sum_ratio=worst_sum, worst_step_ratio=worst_step, gap=gap, inliers=int(got["counts"][1]))


# ---------------------------------------------------------------- the whole loop
LOOP_SEED = 21


def loop_scene():
    """The source is a rigid image of a subset of the target: 5 degrees of rotation and a translation of two cells."""
    tgt, nrm = surface(3000, LOOP_SEED)
    T = motion(5.0, (1, 2, 6), (0.2, -0.1, 0.05))
    return tgt, nrm, RR.image(np.linalg.inv(T), tgt[::2]), T


def check_loop(plane):
    tgt, nrm, src, T = loop_scene()
    normals = nrm if plane else None
    cell, max_dist = 0.1, 0.6
    assert np.abs(T[:3, 3]).max() == 2 * cell
    got = run(tgt, src, normals=normals, cell=cell, max_dist=max_dist, its=50)
    ref = RR.icp(src, tgt, *BOX, max_dist, normals=normals, max_iterations=50, bounds=True)
    assert ref["counts"][3] == RR.CONVERGED and ref["counts"][2] < 50 and ref["gap"] >= 1e-9 and ref["margin"] > 1e-3, ref["counts"]
    assert got["counts"].tolist() == ref["counts"], (got["counts"], ref["counts"])
    err = np.abs(got["T"] - ref["T"])
    ratio = float((err[:3] / ref["bound"][:3]).max())
    assert (err[:3] <= ref["bound"][:3]).all() and (got["T"][3] == [0, 0, 0, 1]).all(), ratio
    assert (got["idx"] == ref["idx"]).all() and np.abs(got["T"] - T).max() < 1e-6
    assert got["stats"][0] == ref["stats"][0] and abs(got["stats"][1] - ref["stats"][1]) <= 1e-12
    return dict(iterations=int(got["counts"][2]), worst_ratio=ratio, bound=float(ref["bound"].max()), error=float(err.max()),
                gap=ref["gap"], margin=ref["margin"])


# ---------------------------------------------------------------- evaluate_cloud
def check_evaluate_cloud():
    tgt, _ = surface(3000, 31, np.float32)
    rng = np.random.default_rng(32)      # the reconstruction: 2500 of the ground truth's points, each off by a little noise
    pred = (tgt[np.sort(rng.choice(3000, 2500, replace=False))].astype(np.float64) + rng.normal(0, 0.004, (2500, 3))).astype(np.float32)
    T = motion(1.0, (2, 1, 5), (0.03, -0.02, 0.02))
    moved = RR.image(np.linalg.inv(T), pred.astype(np.float64)).astype(np.float32)
    kw = dict(max_dist=1.0, thresholds=(0.02, 0.05, 0.1))
    base = fusion.evaluate_cloud(cu(pred), cu(tgt), **kw)
    again = fusion.evaluate_cloud(cu(pred), cu(tgt), register=None, **kw)
    assert json.dumps(base, sort_keys=True) == json.dumps(again, sort_keys=True) and "transformation" not in base
    unreg = fusion.evaluate_cloud(cu(moved), cu(tgt), **kw)
    out = dict(base=base["overall"], unregistered=unreg["overall"])
    for p2p in (True, False):
        got = fusion.evaluate_cloud(cu(moved), cu(tgt), register=dict(max_dist=0.5, point_to_plane=p2p, knn=20, max_iterations=40), **kw)
        Tg = np.array(got["transformation"])
        # the alignment is off T by dT: a point at radius <= 5 moves by at most |dR| 5 + |dt|, and a distance to the
        # nearest point of the other cloud changes by at most that much; so do both means
        slack = np.abs(Tg[:3, :3] - T[:3, :3]).sum(axis=1).max() * 5.0 + np.abs(Tg[:3, 3] - T[:3, 3]).max() + 1e-6      # float32 coordinates
        assert slack < 0.005 and got["register_fitness"] > 0.99 and got["register_rmse"] < 0.1, (slack, got)
        assert abs(got["overall"] - base["overall"]) <= slack and abs(unreg["overall"] - base["overall"]) > 10 * slack
        assert got["accuracy"]["n"] == base["accuracy"]["n"] and set(got) - set(base) == {"transformation", "register_fitness", "register_rmse"}
        out["plane" if p2p else "point"] = dict(overall=got["overall"], slack=float(slack), fitness=got["register_fitness"])
    return out


GROUPS = {
    "edges": [check_empty_and_single_clouds, check_sources_beyond_max_dist_and_zero_iterations, check_a_source_aliasing_the_target,
              check_ties_and_nan_rows, check_exact_lattice_probes, check_refusals_on_the_device_build,
              check_determinism_and_no_host_synchronisation, check_guarded_buffers],
    "sums": [check_reduction_boundaries],
    "dense": [(check_dense, dt, plane) for dt in ("f32", "f64") for plane in (False, True)],
    "loop": [(check_loop, False), (check_loop, True)],
    "evaluate": [check_evaluate_cloud],
}


def name_of(check):
    if not isinstance(check, tuple):
        return check.__name__
    return check[0].__name__ + "".join(f"[{a}]" for a in check[1:])


def main(group):
    _lib.load()
    for check in GROUPS[group]:
        fn, args = (check[0], check[1:]) if isinstance(check, tuple) else (check, ())
        rec = dict(check=name_of(check), ok=False, why="")
        try:
            rec.update(fn(*args) or {})
            rec["ok"] = True
        except Exception as e:      # noqa: BLE001
            rec["why"] = traceback.format_exc()[-3000:]
            if any(t in str(e) for t in ("HIP error", "libmvs_hip status 4:")):      # nothing more on this GPU
                print("R " + json.dumps(rec), flush=True)
                raise
        print("R " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
