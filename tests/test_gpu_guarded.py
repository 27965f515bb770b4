"""Where the kernels read and write: every device output, workspace and input of the library's entry points between
guard bands, outputs and workspaces poisoned three ways before the call (tests/guarded.py).  A case passes when its
outputs are the same bytes under the three poisons and equal to a plain call's, no guard byte changed and no input
changed; tests/guard_check.py lists the cases and runs them.

Kernel selection is read once per process, so the cases run in child processes, one per environment: every
environment of probe_check.CASES (CostRegNet's layers in every kernel form, at the ragged shapes of probes.GEOM),
every environment of warp_ref_check.ENVS (warp + variance), the environments of the run-time z-chunk splits
(test_gpu_zchunks.FORMS, one shape per category of zchunks.cheapest_cases at this device's CU count), and the default
environment for everything else.  Each child has its own time limit, writes its verdicts to a JSON file and runs at
most once; what ends the run after a child is the suite's one rule, in tests/gpu_child.py.
"""
import json
import os
import re

import pytest

import gpu_child
import guard_check
import probe_check
import test_gpu_zchunks as Z
import warp_ref_check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240   # seconds, per environment
CHILD_FAILED = "(child)"   # key of a child's own failure among its verdicts


def _zchunk_cases():
    """The run-time splits: test_gpu_zchunks.CHUNK_CASES holds, per launcher and form, the cheapest shape of every
    category (one-plane last chunk, ragged chunks, the persistent conv1 form) at this device's CU count."""
    out = []
    for c in Z.CHUNK_CASES:
        entry = "mvs_conv11_prob" if c["op"] == "conv11_prob" else "mvs_conv_layer"
        out.append({"id": "zchunk-" + c["id"], "entries": [entry], "env": c["env"], "kind": "zchunk",
                    "args": {"op": c["op"], "layer": c["layer"], "storage": c["storage"], "shape": c["shape"]}})
    return out


CASES = {c["id"]: c for c in guard_check.STATIC_CASES + _zchunk_cases()}


def _env_key(env):
    return tuple(sorted(env.items()))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Runs each environment's cases in one child, on first use: {env key: {case id: verdict}}."""
    tmp = tmp_path_factory.mktemp("guarded")
    keys = sorted({_env_key(c["env"]) for c in CASES.values()})
    for i, key in enumerate(keys):
        with open(tmp / f"env{i}.cases.json", "w") as f:
            json.dump([c for c in CASES.values() if _env_key(c["env"]) == key], f)

    def get(case):
        key = _env_key(case["env"])
        stem = tmp / f"env{keys.index(key)}"
        # guard_check.py ends with status 2 after a HIP error: like a signal or a time limit, that ends the run
        r = gpu_child.run_once(("guarded", key), ["guard_check.py", f"{stem}.cases.json", f"{stem}.out.json"],
                               env=case["env"], timeout=CHILD_TIMEOUT, hip_error_status=2)
        try:
            with open(f"{stem}.out.json") as f:
                verdicts = json.load(f)
        except (OSError, ValueError):
            verdicts = {}
        if r.returncode != 0:      # the child never runs twice: the cases without a verdict fail with its output
            verdicts[CHILD_FAILED] = f"guard_check ended with status {r.returncode}:\n" + \
                r.stdout[-2000:] + r.stderr[-4000:]
        return verdicts

    return get


@pytest.mark.parametrize("cid", list(CASES))
def test_guards_inputs_and_poisons(results, cid):
    case = CASES[cid]
    verdicts = results(case)
    assert cid in verdicts, verdicts.get(CHILD_FAILED, "the child wrote no verdict for this case")
    v = verdicts[cid]
    print(f"{'+'.join(case['entries'])} env={case['env']} shape={v['shape']} guard_bytes={v['guard_bytes']} "
          f"exempt={v['exempt']}")
    assert v["ok"], v["msg"]
    assert v["exempt"] == 0.0      # include/mvs_abi.h declares no element of any output unspecified
    assert v["guard_bytes"] > 0 or case["kind"] == "module"


def device_entry_points():
    """The mvs_* functions of include/mvs_abi.h that take a device output or a workspace: every declaration but the
    version / error-string calls, the mvs_query_* size queries and the host-only functions (their comment says HOST)."""
    with open(os.path.join(os.path.dirname(HERE), "include", "mvs_abi.h")) as f:
        src = f.read()
    names = re.findall(r"^(?:int|const char\*)\s+(mvs_\w+)\s*\(", src, re.M)
    host_only = {"mvs_abi_version", "mvs_last_error_string", "mvs_pack_weights", "mvs_pack_feature_weights",
                 "mvs_filter_compose"}
    for n in host_only:
        assert n in names, n
    for words in ("HOST function.  Folds eval-mode BatchNorm3d", "mvs_pack_feature_weights (HOST pointers)",
                  "mvs_filter_compose (HOST pointers only, no GPU work)"):
        assert words in src, words      # the header's own words for the three host-only functions
    return [n for n in names if n not in host_only and not n.startswith("mvs_query_")]


def test_every_device_entry_point_has_a_case():
    names = device_entry_points()
    assert len(names) >= 26 and "mvs_warp_variance" in names and "mvs_volume_relayout" in names
    covered = {e for c in CASES.values() for e in c["entries"]}
    missing = [n for n in names if n not in covered]
    assert not missing, f"no guarded case for {missing}"
    assert covered <= set(names), sorted(covered - set(names))


def test_every_environment_has_a_case():
    have = {_env_key(c["env"]) for c in CASES.values()}
    for table in (probe_check.CASES, warp_ref_check.ENVS):
        for name, spec in table.items():
            assert _env_key(spec["env"]) in have, name
            ids = [c for c in CASES.values() if _env_key(c["env"]) == _env_key(spec["env"])]
            assert ids
    for name, c in probe_check.CASES.items():
        for layer in c["layers"]:
            for st in c["storages"]:
                cid = f"conv-{name}-tail-{st}" if layer == "tail" else f"conv-{name}-layer{layer}-{st}"
                assert cid in CASES, cid
    for *_, env, _, _ in Z.FORMS:
        assert _env_key(env) in have, env
