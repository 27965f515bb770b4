#!/usr/bin/env python3
"""Child-process helper: every warp + variance kernel form against the fp64 reference and the derived bound of
tests/warp_ref.py, under ONE kernel-selection environment (read once per process by options() in mvs_host.hip).
Usage: warp_ref_check.py <environment> <work dir>; the parent (test_gpu_warp_ref.py) sets ENVS[environment]["env"].

Per case and storage type: mvs_relative_proj against relative_proj64, mvs_warp_variance against variance64 from the rt
the GPU produced (NaN pattern exact, |error| <= bound elsewhere); in the default environment also mvs_homo_warp
against warp64 and the training forward against mvs_warp_variance's bits.  Prints one verdict line per case, writes
the raw volumes to <work dir>/<environment>/ (the parent compares tap-cache and plain forms bit for bit), and ends with
one JSON line: the worst error / bound per case and over all.  The fp64 references are cached in <work dir>/ref, so
that the environments of one test run compute each only once.

Which kernel an environment reaches at the cases' sizes (csrc/warp_variance.hip launch_warp_variance /
launch_warp_variance16, csrc/warp_variance_tc.hip launch_tc2_dt):
  default: warp_variance_tc2<DT, F32, NV = N - 1> for N = 2..5, warp_variance_kernel<DT, false> for N = 1 and N > 5
  MVS_WARP_TC=0: warp_variance_kernel<DT, false> for every N
  MVS_WARP_DEPTH_FASTEST=1: the same kernels in the depth-slab-fastest block order (warp_variance_kernel<DT, true>);
      =0 forces the pixel-fastest order on the tap-cache form (the default at these sizes, a no-op for the plain form)
  MVS_FEAT16=1 (16-bit volumes only): nchw_to_c8<DT> narrows the feature copy; warp_variance_tc2<DT, DT, NV>, or with
      MVS_WARP_TC16=0 (and for N = 1, N > 5) warp_variance16_kernel<DT, ...>.  MVS_WARP_TC16=0 without MVS_FEAT16
      selects nothing else than the default (the fp32-feature path is steered by MVS_WARP_TC).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import warp_ref as W  # noqa: E402

DEV = "cuda:0"
ALL3, B16 = ("f32", "f16", "bf16"), ("f16", "bf16")
DF, TC, TC16, F16 = "MVS_WARP_DEPTH_FASTEST", "MVS_WARP_TC", "MVS_WARP_TC16", "MVS_FEAT16"

ENVS = {
    "default": dict(env={}, storages=ALL3),
    "tc0": dict(env={TC: "0"}, storages=ALL3),
    "df1": dict(env={DF: "1"}, storages=ALL3),
    "df1_tc0": dict(env={DF: "1", TC: "0"}, storages=ALL3),
    "df0": dict(env={DF: "0"}, storages=("f32",)),
    "tc16_0": dict(env={TC16: "0"}, storages=B16),
    "feat16": dict(env={F16: "1"}, storages=B16),
    "feat16_df1": dict(env={F16: "1", DF: "1"}, storages=B16),
    "feat16_tc16_0": dict(env={F16: "1", TC16: "0"}, storages=B16),
    "feat16_tc16_0_df1": dict(env={F16: "1", TC16: "0", DF: "1"}, storages=B16),
}
# tap-cache environment -> the plain-kernel environment whose volumes must be the same bits, case by case
IDENTICAL = {"default": "tc0", "df1": "df1_tc0", "df0": "tc0", "tc16_0": "tc0", "feat16": "feat16_tc16_0",
             "feat16_df1": "feat16_tc16_0_df1"}

# every kernel of csrc/warp_variance.hip and csrc/warp_variance_tc.hip, and every template instantiation they launch
# (whitespace removed; MVS_TC2(NV) is the launcher's macro for the four view counts) -> one (environment, case, storage)
# that reaches it ("*": every case).  test_warp_ref_host.py parses the sources: a new kernel or instantiation without
# an entry here fails the CPU suite.
KERNELS = {
    "relative_proj_kernel": ("default", "*", "f32"),
    "nchw_to_c8_kernel": ("default", "*", "f32"),
    "warp_variance_kernel": ("tc0", "*", "f32"),
    "warp_variance16_kernel": ("feat16_tc16_0", "*", "f16"),
    "warp_variance_tc2_kernel": ("default", "dtu_n5", "f32"),
    "homo_warp_kernel": ("default", "odd", "f32"),
}
INSTANTIATIONS = {
    "nchw_to_c8_kernel<MVS_F32>": ("default", "*", "f32"),
    "nchw_to_c8_kernel<MVS_F16>": ("feat16", "*", "f16"),
    "nchw_to_c8_kernel<MVS_BF16>": ("feat16", "*", "bf16"),
    "warp_variance_kernel<MVS_F32,false>": ("tc0", "*", "f32"),
    "warp_variance_kernel<MVS_F16,false>": ("tc0", "*", "f16"),
    "warp_variance_kernel<MVS_BF16,false>": ("tc0", "*", "bf16"),
    "warp_variance_kernel<MVS_F32,true>": ("df1_tc0", "*", "f32"),
    "warp_variance_kernel<MVS_F16,true>": ("df1_tc0", "*", "f16"),
    "warp_variance_kernel<MVS_BF16,true>": ("df1_tc0", "*", "bf16"),
    "warp_variance16_kernel<MVS_F16,false>": ("feat16_tc16_0", "*", "f16"),
    "warp_variance16_kernel<MVS_BF16,false>": ("feat16_tc16_0", "*", "bf16"),
    "warp_variance16_kernel<MVS_F16,true>": ("feat16_tc16_0_df1", "*", "f16"),
    "warp_variance16_kernel<MVS_BF16,true>": ("feat16_tc16_0_df1", "*", "bf16"),
    "warp_variance_tc2_kernel<DT,FDT,NV,CPT,0,1>": ("default", "dtu_n5", "f32"),
    "launch_tc2_dt<MVS_F32,MVS_F32>": ("default", "dtu_n5", "f32"),
    "launch_tc2_dt<MVS_F16,MVS_F32>": ("default", "dtu_n5", "f16"),
    "launch_tc2_dt<MVS_BF16,MVS_F32>": ("default", "dtu_n5", "bf16"),
    "launch_tc2_dt<MVS_F16,MVS_F16>": ("feat16", "dtu_n5", "f16"),
    "launch_tc2_dt<MVS_BF16,MVS_BF16>": ("feat16", "dtu_n5", "bf16"),
    "MVS_TC2(1)": ("default", "dtu_n2", "f32"),
    "MVS_TC2(2)": ("default", "dtu_n3", "f32"),
    "MVS_TC2(3)": ("default", "dtu_n4", "f32"),
    "MVS_TC2(4)": ("default", "dtu_n5", "f32"),
}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def cached_ref(work, name, c, rt, storage, feat16):
    """variance_bound for (case, rt, feature rounding), its fp32 part cached on disk; the storage half-ulp is added here"""
    fmode = storage if feat16 else "f32"
    key = hashlib.sha1(np.ascontiguousarray(rt).tobytes()).hexdigest()[:12]
    path = os.path.join(work, "ref", "%s_%s_%s.npz" % (name, fmode, key))
    if os.path.exists(path):
        with np.load(path) as z:
            ref = {k: z[k] for k in z.files}
    else:
        feats = W.round_storage(c["feats"], storage) if feat16 else c["feats"]      # MVS_FEAT16=1: RNE-narrowed features
        ref = W.variance_bound(feats, rt, c["dv"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, **ref)
        os.replace(tmp, path)
    if storage != "f32":
        with np.errstate(invalid="ignore"):
            ref["bound"] = ref["bound"] + W.ulp_storage(np.abs(ref["var"]) + ref["bound"], storage) / 2
        ref["storage_max"] = W.STORAGE_MAX[storage]
    return ref


def main():
    from scene_3dreconstruction_mvsnet_amd import _lib, training

    envname, work = sys.argv[1], sys.argv[2]
    spec = ENVS[envname]
    for k, v in spec["env"].items():
        assert os.environ.get(k) == v, "the parent must set %s=%s" % (k, v)
    outdir = os.path.join(work, envname)
    os.makedirs(outdir, exist_ok=True)
    feat16_env = spec["env"].get(F16) == "1"
    ratios, failures = {}, []

    def verdict(tag, ratio, problems):
        ratios[tag] = ratio
        print("%-28s %s  error / bound = %.4f" % (tag, "FAIL" if problems else "ok", ratio), flush=True)
        failures.extend("%s: %s" % (tag, p) for p in problems)

    for name, (builder, _) in W.CASES.items():
        c = builder()
        N, Cn, h, w = c["feats"].shape
        D = len(c["dv"])
        rt_dev = _lib.relative_proj(cu(c["proj"]))
        rt = rt_dev.cpu().numpy()[:max(N - 1, 0)] if N > 1 else np.zeros((0, 12), np.float32)
        if N > 1:
            want, bnd = W.relative_proj64(c["proj"]), W.relative_proj_bound(c["proj"])
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.where(bnd > 0, np.abs(rt.astype(np.float64) - want) / bnd, np.where(rt == want, 0.0, np.inf))
            verdict(name + "/relative_proj", float(r.max()), [] if r.max() <= 1 else ["relative_proj off: %s" % r.max()])
        for storage in spec["storages"]:
            dt = _lib.dtype_code(storage)
            ws = _lib.alloc_workspace(N, Cn, D, h, w, DEV, dt)
            var = _lib.warp_variance(cu(c["feats"]), rt_dev, cu(c["dv"]), ws, dt)
            torch.cuda.synchronize()
            raw = var.cpu()
            got = _lib.from_c8(raw.float()).numpy()
            np.save(os.path.join(outdir, "%s_%s.npy" % (name, storage)), got)
            ref = cached_ref(work, name, c, rt, storage, feat16_env and storage != "f32")
            ratio, problems = W.compare(got, ref)
            verdict("%s/%s" % (name, storage), ratio, problems)
            if storage == "f32" and name in W.TRAINING_CASES:
                tv = training.cost_volume(cu(c["feats"])[None], cu(c["proj"])[None], cu(c["dv"])[None])[0].cpu().numpy()
                same = np.array_equal(tv, got, equal_nan=True)
                verdict(name + "/training", 0.0, [] if same else ["training forward differs from mvs_warp_variance"])

    if envname == "default":
        lib = _lib.load()
        for name, c in W.homo_cases().items():
            Cn, h, w = c["fea"].shape
            D = len(c["dv"])
            rt_dev = _lib.relative_proj(cu(c["proj"]))
            out = torch.empty((Cn, D, h, w), dtype=torch.float32, device=DEV)
            fea, dv = cu(c["fea"]), cu(c["dv"])
            _lib.check(lib.mvs_homo_warp(fea.data_ptr(), rt_dev.data_ptr(), dv.data_ptr(), out.data_ptr(), Cn, D, h, w,
                                         _lib._stream(out.device)))
            torch.cuda.synchronize()
            wv, e, lo, na = W.warp_bound(c["fea"], rt_dev.cpu().numpy()[0], c["dv"])
            ratio, problems = W.compare(out.cpu().numpy(), dict(var=wv, bound=e, loose=lo, nan=na))
            verdict("homo_warp/" + name, ratio, problems)

    worst = max(ratios.values())
    print(json.dumps({"env": envname, "worst": worst, "ratios": ratios, "failures": failures}))
    for f in failures:
        print("FAILED", f, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
