#!/usr/bin/env python3
"""Child-process helper: NaN and infinity through the CostRegNet kernels, the soft-argmin and the chain, against the
contract of tests/nonfinite_ref.py (R1 never hide, R2 nothing else moves, R3 bounded spread).
Usage: nonfinite_check.py layers <case> | softargmin | chain.  `layers` runs under ONE kernel-selection environment, the
case table of probe_check.py (the parent, test_gpu_nonfinite.py, sets CASES[case]["env"]).
Prints one JSON line with the worst R2 ratio and the widest observed spread per layer and storage next to the table's
extent, lists every violation with its first offending index and exits non-zero if there is one."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import nonfinite_ref as N  # noqa: E402
import probes as P  # noqa: E402
import softargmin_ref as sar  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from probe_check import CASES, DEV, cu, run_layer, run_tail  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic  # noqa: E402


def check_layers(name):
    case = CASES[name]
    for k, v in case["env"].items():
        assert os.environ.get(k) == v, f"case {name} needs {k}={v} in the environment"
    sd = synthetic.random_costreg_state(seed=13)
    blob = _lib.pack_weights(sd).to(DEV)
    chk = N.Checker()
    extents = {}
    for storage in case["storages"]:
        rng = np.random.default_rng(29)
        for layer in case["layers"]:
            key = f"{layer}:{storage}"
            extent = extents[key] = N.case_extent(name, layer)
            if layer == "tail":
                w9, sh9 = P.folded(sd, 9)
                for pname, x, skip in N.tail_patterns(rng, storage):
                    got = run_tail(x, skip, blob, storage)
                    ref, bound, touched = N.tail_reference(x, skip, w9, sh9, sd["prob.weight"], sd["prob.bias"], storage)
                    chk.check(key, pname, got, ref, bound, touched, extent)
                continue
            wf, sh = P.folded(sd, layer)
            wino = case["wino"].get(layer)
            for pname, x, skip in N.layer_patterns(layer, rng, storage):
                got = run_layer(layer, x, skip, blob, storage)
                ref, bound, touched = N.layer_reference(layer, x, skip, wf, sh, storage, wino,
                                                        case.get("arith", "mfma16"))
                if layer == 10:
                    ref, bound = ref[0], bound[0]
                chk.check(key, pname, got, ref, bound, touched, extent)
    torch.cuda.synchronize()
    print(json.dumps({"case": name, "ratios": {k: round(v, 4) for k, v in chk.ratios.items()},
                      "spread": {k: [list(v), list(extents[k])] for k, v in chk.spreads.items()}}))
    return chk.failures


def check_softargmin():
    failures, ratios = [], {}
    for form in sar.FORMS:
        c = N.softargmin_case(form)
        D = c["cost"].shape[0]
        assert sar.launch_form(D, c["h"] * c["w"])[0] == form
        depth, conf = _lib.softargmin_conf(cu(c["cost"].reshape(D, c["h"], c["w"])), cu(c["dv"]))
        pix = np.concatenate(list(c["pixels"].values()))
        rd, rc, problems = N.check_softargmin(depth.cpu().numpy(), conf.cpu().numpy(), c["cost"], c["dv"], pix)
        ratios[form] = [round(rd, 4), round(rc, 4)]
        failures += [f"softargmin {form}: {p}" for p in problems]
    print(json.dumps({"case": "softargmin", "ratios": ratios}))
    return failures


def _chain_compare(tag, storage, cost, depth, conf, cost_o, depth_o, conf_o, allowed, failures, report):
    """R1 on logits, depth and confidence, R2 at test_gpu_parity's tolerances of the storage on every finite pixel (fp32:
    logits within 3e-4 of their range, depth relative L1 1e-5, confidence; 16-bit: depth relative L1 2e-4 / 1e-3 against
    the matched oracle), R3 as the carried extents, and the cap on the finite share."""
    nf_o, nf_g = ~np.isfinite(cost_o), ~np.isfinite(cost)
    pix_o, pix_g = nf_o.any(0), nf_g.any(0)
    for what, got, ref in (("logits", cost, cost_o), ("depth", depth, depth_o), ("confidence", conf, conf_o)):
        hidden = ~np.isfinite(ref) & np.isfinite(got)
        if hidden.any():
            i = tuple(int(v) for v in np.argwhere(hidden)[0])
            failures.append(f"chain {tag} {storage}: R1 {what} at {i}: got {float(got[i])!r}, oracle {float(ref[i])!r} "
                            f"({int(hidden.sum())} elements)")
    stray = (pix_g | ~np.isfinite(depth) | ~np.isfinite(conf)) & ~allowed
    if stray.any():
        i = tuple(int(v) for v in np.argwhere(stray)[0])
        failures.append(f"chain {tag} {storage}: R3 non-finite pixel {i} outside the carried extents "
                        f"({int(stray.sum())} pixels)")
    ok = ~nf_g & ~nf_o
    scale = max(float(np.abs(cost_o[~nf_o]).max()), 1.0)
    err = np.where(ok, np.abs(np.where(ok, cost, 0) - np.where(ok, cost_o, 0)), 0.0)
    tol = 2 * N.CHAIN_EPS[storage] * np.where(ok, np.abs(np.where(ok, cost_o, 0)), 0) + 3e-4 * scale
    fin = np.isfinite(depth) & np.isfinite(depth_o)
    l1 = float(np.abs(depth[fin] - depth_o[fin]).mean() / np.abs(depth_o[fin]).mean())
    share = float(np.isfinite(depth).mean())
    report[f"{tag}:{storage}"] = dict(logit_ratio=round(float((err / tol).max()), 4), depth_l1=l1,
                                      finite_got=round(share, 4), finite_oracle=round(float(np.isfinite(depth_o).mean()), 4),
                                      nonfinite_x_got=int(np.nonzero(pix_g.any(0))[0].max()) if pix_g.any() else -1,
                                      nonfinite_x_oracle=int(np.nonzero(pix_o.any(0))[0].max()) if pix_o.any() else -1)
    # 16-bit storage: test_gpu_parity holds the chain to the depth's relative L1 only (activations on a rounding boundary
    # flip with the summation order and the flip travels through the layers); the per-layer logit tolerance is reported
    if storage == "f32" and (err > tol).any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(err / tol)), err.shape))
        failures.append(f"chain {tag} {storage}: R2 logits {float((err / tol).max()):.3g} x tolerance at {i}")
    if not l1 < N.CHAIN_DEPTH_L1[storage]:
        failures.append(f"chain {tag} {storage}: R2 depth relative L1 {l1:.3e} on the finite pixels")
    if storage == "f32":
        bad = float((np.abs(conf[fin] - conf_o[fin]) > 5e-3).mean())
        if not bad < 0.01:
            failures.append(f"chain {tag} {storage}: R2 confidence differs by > 5e-3 on {bad:.4f} of the finite pixels")
    if share < N.MIN_FINITE_GOT:
        failures.append(f"chain {tag} {storage}: only {share:.3f} of the pixels stay finite")


def check_chain():
    failures, report = [], {}
    D, h, w = N.CHAIN_SHAPE
    sd = synthetic.random_costreg_state(seed=13)
    blob = _lib.pack_weights(sd).to(DEV)
    rig = N.chain_rig()
    dv_v = synthetic.depth_values(D)
    var = N.chain_voxel_volume()
    for storage in ("f32", "f16", "bf16"):
        code = _lib.dtype_code(storage)
        ws = _lib.alloc_workspace(3, 32, D, h, w, DEV, code)
        # one NaN voxel in the variance volume: mvs_costreg_forward + mvs_softargmin_conf
        vq = orc.round_storage(var, storage)
        cost = _lib.costreg_forward(_lib.to_c8(cu(vq)).to(_lib.TORCH_DTYPES[code]), blob, ws, code)
        depth, conf = _lib.softargmin_conf(cost, cu(dv_v))
        cost_o = orc.costreg_forward(vq, sd, storage, arith16=True)
        depth_o, conf_o, _ = orc.softargmin_conf(cost_o, dv_v)
        allowed = N.chain_allowed(~np.isfinite(vq).all(0), storage)
        _chain_compare("voxel", storage, cost.cpu().numpy(), depth.cpu().numpy(), conf.cpu().numpy(), cost_o, depth_o,
                       conf_o, allowed, failures, report)
        # the z0 rig: the warp writes the NaN itself; mvs_depth_infer, and the stages one by one for the logits
        feats, proj, dv = cu(rig["feats"]), torch.from_numpy(rig["proj"]).to(DEV), cu(rig["dv"])
        d_out, c_out = torch.empty((h, w), device=DEV), torch.empty((h, w), device=DEV)
        _lib.depth_infer(feats, proj, dv, blob, ws, d_out, c_out, dtype=code)
        vol = _lib.warp_variance(feats, _lib.relative_proj(proj), dv, ws, dtype=code)
        cost = _lib.costreg_forward(vol, blob, ws, code)
        var_o = orc.round_storage(orc.variance_volume(rig["feats"], rig["proj"], rig["dv"]), storage)
        cost_o = orc.costreg_forward(var_o, sd, storage, arith16=True)
        depth_o, conf_o = orc.depth_infer(rig["feats"], rig["proj"], rig["dv"], sd, storage=storage)
        allowed = N.chain_allowed(~np.isfinite(var_o).all(0), storage)
        _chain_compare("rig", storage, cost.cpu().numpy(), d_out.cpu().numpy(), c_out.cpu().numpy(), cost_o, depth_o,
                       conf_o, allowed, failures, report)
    print(json.dumps({"case": "chain", "report": report}))
    return failures


def main():
    mode = sys.argv[1]
    failures = check_layers(sys.argv[2]) if mode == "layers" else check_softargmin() if mode == "softargmin" \
        else check_chain()
    for f in failures:
        print("FAIL", f)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
