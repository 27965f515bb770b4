"""The z-chunk and depth-slab splits the launchers pick at run time, at the cheapest shape of every case category.

tests/zchunks.py asks the library's planner for each launcher's split; here the CU count of the device under test chooses, per launcher,
the cheapest volume (D, h, w) of every category its kernel treats differently (one chunk, ragged last chunks of 0, 1
or 2 planes mod 3 after chunks of 0, 1 or 2 mod 3, for conv11_prob odd chunks and a one-plane last chunk), and each
case runs against the CPU oracle.  The split of every case is in its test id: <launcher>-<form>-<categories>-
D<D>h<h>w<w>-zc<ZC>n<chunks>l<last>.

Kernel selection is read once per process, so the cases run in child processes (tests/zchunk_check.py), one per
environment, each checking all of its cases; the test of a case reports that case's verdict.  Every case is small
enough (at most about 0.7 M voxels at 80 .. 304 CUs) for the whole-volume oracle.

The tap-cache warp's slab depends on D alone: D = 288 and 632 take slab 44, D = 312 and 320 slab 36, which no other
test reaches.  Those run in both block orders against the oracle; the fp32 volume must also equal the plain kernel's
(MVS_WARP_TC=0) bit for bit, and so must the tc16 volumes (16-bit feature copy, MVS_FEAT16=1) the plain 16-bit kernel's
(MVS_WARP_TC16=0).
"""
import json
import os

import numpy as np
import pytest
import torch

import gpu_child
import zchunks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _device_cus():
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(0).multi_processor_count
    return 256   # collected without a GPU: the tests are deselected there


CUS = _device_cus()
PERSIST_CUS = 4   # MVS_PERSIST_CUS for conv1z's long chunks: 4 "CUs" split a single column into about 4 chunks
PERSIST_MIN_ZC = 24

# (launcher, form, storage, environment, CU count the search sees, smallest ZC of interest)
FORMS = [
    ("conv11_prob", "split", "f32", {}, CUS, 0),
    ("conv11_prob", "priv", "f32", {"MVS_TAIL_SPLIT": "0"}, CUS, 0),
    ("conv11_prob", "f16", "f16", {}, CUS, 0),
    ("conv11_prob", "bf16", "bf16", {}, CUS, 0),
    ("conv1z", "f32", "f32", {"MVS_CONV1Z": "1"}, CUS, 0),
    # chunks of >= 24 planes (the unrolled loop runs 8+ times) at a few thousand voxels: only through MVS_PERSIST_CUS
    ("conv1z", "persist4", "f32", {"MVS_CONV1Z": "1", "MVS_PERSIST_CUS": str(PERSIST_CUS)}, PERSIST_CUS,
     PERSIST_MIN_ZC),
] + [(f"convz16-{layer}", st, st, {"MVS_CONVZ16": "1"}, CUS, 0) for layer in (1, 2, 3) for st in ("f16", "bf16")] \
  + [("conv0z16", st, st, {"MVS_CONV0Z16": "1"}, CUS, 0) for st in ("f16", "bf16")]


def _env_key(env):
    return tuple(sorted(env.items()))


def _chunk_cases():
    cases = []
    for name, form, storage, env, cus, min_zc in FORMS:
        by_shape = {}
        for cat, shape in sorted(zchunks.cheapest_cases(name, cus, min_zc).items()):
            by_shape.setdefault(shape, []).append(cat)
        for shape, cats in sorted(by_shape.items(), key=lambda kv: kv[0][0] * kv[0][1] * kv[0][2]):
            s = zchunks.LAUNCHERS[name](*shape, cus)
            D, h, w = shape
            cid = f"{name}-{form}-{'+'.join(cats)}-D{D}h{h}w{w}-zc{s.zc}n{s.n}l{s.last}"
            op = "conv11_prob" if name == "conv11_prob" else "layer"
            layer = {"conv1z": 1, "conv0z16": 0}.get(name, int(name[-1]) if name.startswith("convz16") else None)
            cases.append({"id": cid, "op": op, "storage": storage, "layer": layer, "shape": list(shape),
                          "env": env, "save": None})
    return cases


TC_DEPTHS = (288, 632, 312, 320)   # slab 44, 44, 36, 36
# (form, volume storage, environment); each runs in both block orders
TC_FORMS = [("tc-f32", "f32", {}), ("tc-f16", "f16", {}), ("tc-bf16", "bf16", {}),
            ("tc16-f16", "f16", {"MVS_FEAT16": "1"}), ("tc16-bf16", "bf16", {"MVS_FEAT16": "1"})]
# the plain kernels the tap-cache volumes are compared with
PLAIN = {"tc-f32": {"MVS_WARP_TC": "0"}, "tc16-f16": {"MVS_FEAT16": "1", "MVS_WARP_TC16": "0"},
         "tc16-bf16": {"MVS_FEAT16": "1", "MVS_WARP_TC16": "0"}}


def _warp_cases():
    cases = []
    for D in TC_DEPTHS:
        s = zchunks.tc_slab(D, 16, 24)
        for form, storage, env in TC_FORMS:
            for df in ("1", "0"):
                cases.append({"id": f"{form}-df{df}-D{D}-slab{s.zc}n{s.n}l{s.last}", "op": "warp", "storage": storage,
                              "layer": None, "shape": [D, 16, 24], "env": dict(env, MVS_WARP_DEPTH_FASTEST=df),
                              "form": form, "save": None})
            if form in PLAIN:
                cases.append({"id": f"{form}-plain-D{D}", "op": "warp", "storage": storage, "layer": None,
                              "shape": [D, 16, 24], "env": PLAIN[form], "form": form, "save": None})
    return cases


CHUNK_CASES = _chunk_cases()
WARP_CASES = _warp_cases()
ALL_CASES = {c["id"]: c for c in CHUNK_CASES + WARP_CASES}
assert len(ALL_CASES) == len(CHUNK_CASES) + len(WARP_CASES)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Runs each environment's cases in one child, on first use: {env key: {case id: verdict}}."""
    tmp = tmp_path_factory.mktemp("zchunks")
    keys = sorted({_env_key(c["env"]) for c in ALL_CASES.values()})
    for i, key in enumerate(keys):
        with open(tmp / f"env{i}.cases.json", "w") as f:
            json.dump([dict(c, save=str(tmp / f"{c['id']}.npy")) for c in ALL_CASES.values()
                       if _env_key(c["env"]) == key], f)

    def get(case):
        key = _env_key(case["env"])
        stem = tmp / f"env{keys.index(key)}"
        r = gpu_child.run_once(("zchunks", key), ["zchunk_check.py", f"{stem}.cases.json", f"{stem}.out.json"],
                               env=case["env"], timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(f"{stem}.out.json") as f:
            return json.load(f)[case["id"]], tmp / f"{case['id']}.npy"

    return get


@pytest.mark.parametrize("cid", [c["id"] for c in CHUNK_CASES])
def test_z_chunk_split_matches_oracle(results, cid):
    verdict, _ = results(ALL_CASES[cid])
    assert verdict["ok"], verdict["msg"]


@pytest.mark.parametrize("cid", [c["id"] for c in WARP_CASES if "-plain-" not in c["id"]])
def test_tap_cache_slab_matches_oracle_and_plain_kernel(results, cid):
    case = ALL_CASES[cid]
    verdict, vol = results(case)
    assert verdict["ok"], verdict["msg"]
    if case["form"] in PLAIN:
        plain_case = ALL_CASES[f"{case['form']}-plain-D{case['shape'][0]}"]
        plain_verdict, plain_vol = results(plain_case)
        assert plain_verdict["ok"], plain_verdict["msg"]
        a, b = np.load(vol), np.load(plain_vol)
        assert a.shape == b.shape
        assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} elements differ from the plain kernel's"
