"""The C ABI driven from a plain-C host process (tools/c_abi_demo/demo.c: gcc + HIP runtime API, no
Python / torch in that process): same numbers as the oracle, errors as status codes."""
import os
import subprocess

import numpy as np
import pytest

import gpu_child
from conftest import REPO, rel_l1
from oracle import oracle as orc
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic

pytestmark = pytest.mark.gpu


def test_plain_c_host_runs_depth_infer(tmp_path):
    demo = os.path.join(REPO, "tools", "c_abi_demo", "demo")
    if not os.path.exists(demo):
        subprocess.check_call(["make", "-C", os.path.dirname(demo)])
    N, D, h, w = 3, 16, 24, 40
    feats = synthetic.random_features(N, 32, h, w, seed=4)
    proj = synthetic.cameras(N, h, w, yaw_deg=1.0)
    dv = synthetic.depth_values(D)
    sd = synthetic.random_costreg_state(seed=4)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([N, D, h, w], np.int32).tobytes())
        for a in (feats, proj, dv):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for key in _lib.CONV_WEIGHT_KEYS:
            f.write(np.ascontiguousarray(sd[key], np.float32).tobytes())
        for pre in _lib.BN_PREFIXES:
            for suffix in ("weight", "bias", "running_mean", "running_var"):
                f.write(np.ascontiguousarray(sd[f"{pre}.{suffix}"], np.float32).tobytes())
        f.write(np.ascontiguousarray(sd["prob.bias"], np.float32).tobytes())
    r = gpu_child.run([demo, _lib.LIB_PATH, fin, fout], timeout=120, python=False)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "must be positive multiples of 8" in r.stdout      # the bad-shape message came back as text
    out = np.fromfile(fout, np.float32).reshape(2, h, w)
    depth_o, conf_o = orc.depth_infer(feats, proj, dv, sd)
    assert rel_l1(out[0], depth_o) < 1e-5
    assert (np.abs(out[1] - conf_o) > 5e-3).mean() < 0.02


def test_rccl_backend_initialises_and_gathers_on_this_box(tmp_path):
    """bench.py --gpus N initialises torch.distributed with backend "nccl" (= RCCL) and gathers the
    per-rank maps with all_gather_into_tensor; a one-GPU box can only run the 1-rank form of exactly
    those calls, which still exercises the RCCL init path and the device-tensor collective."""
    code = (
        "import os, torch, torch.distributed as dist\n"
        "os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29533')\n"
        "dev = torch.device('cuda', 0); torch.cuda.set_device(dev)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)\n"
        "src = torch.arange(2 * 2 * 8 * 8, dtype=torch.float32, device=dev).reshape(2, 2, 8, 8)\n"
        "out = torch.empty_like(src)\n"
        "dist.all_gather_into_tensor(out, src)\n"
        "dist.barrier(); torch.cuda.synchronize()\n"
        "assert torch.equal(out, src)\n"
        "t = torch.tensor([1.5], dtype=torch.float64, device=dev); dist.all_reduce(t, op=dist.ReduceOp.MAX)\n"
        "assert float(t.item()) == 1.5\n"
        "dist.destroy_process_group(); print('rccl ok')\n")
    r = gpu_child.run(["-c", code], env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"}, timeout=240)
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stdout + r.stderr
