#!/usr/bin/env python3
"""Child-process helper: single-product probes and the dense fp64 bound (tests/probes.py) for every CostRegNet layer
and the fused conv11_prob tail, under ONE kernel-selection environment (read once per process by options() in
mvs_host.hip).  Usage: probe_check.py <case>; the parent (test_gpu_conv_probes.py) sets CASES[case]["env"].
After the probes, the smallest volumes the ABI admits (TINY_* below, keys "<layer>:tiny:<storage>": one figure per
environment and layer -- at these shapes several environments fall back to the generic tile kernels (persist below four
tiles per block, convz16 below 4 output planes, conv0z16 below D = 8), which the launchers decide, not this file).
Prints one JSON line with the measured max ratios (got - want over the bound, per layer / set / storage) and exits
non-zero after listing every violated bound.

Which kernel each case reaches at the probe shapes of probes.GEOM (the planner in launch_plan.h, the dispatch in
conv3d_direct.hip launch_conv_layer, conv3d_mfma16.hip launch_layer16_dt / launch_layer_split, conv3d_mfma.hip launch_convg_dt,
conv11_prob.hip launch_conv11_prob); "wino" names the layers held to a Winograd bound (probes.WINO).
  fp32 "default": conv0 conv0_w48t (split-operand F(4,3), D % 4 == 0); conv1 convg (run_convg_persist falls back to the
      one-tile-per-block kernel below 4 tiles per block, and conv1z needs columns that fill the chip); conv2-conv4
      convg16<OpSplit>; conv5 / conv6 convs, conv7 deconvs (split-K); conv9 deconvg16<OpSplit> (MVS_SPLIT_DECONV=2);
      conv11 deconvg; prob prob_lds; tail conv11_prob_split.
  MVS_CONV0_SPLIT=0: conv0_w43 (fp32 F(4,3));  MVS_CONV0_WINO=0: conv0_4x4 (direct).
  MVS_CONV1Z=1: conv1z;  MVS_PERSIST_CUS=1 with MVS_CONV1Z=0: convg_persist on a one-CU grid (MVS_PERSIST_CUS alone
      would also make conv1z's "columns fill the chip" test pass).
  MVS_SPLIT_LAYERS=0: conv2 / conv4 convwz (F(2,3)), conv3 convg, conv9 deconvg;  + MVS_CONV_WINO=0: conv2 / conv4 convg.
  MVS_SPLIT_DECONV=3: conv7 deconvg16<OpSplit>;  =0: conv9 deconvg.
  MVS_TAIL_SPLIT=0: tail conv11_prob_priv.  MVS_FUSE_PROB=0 only splits the tail of mvs_costreg_forward into the
      layer-9 and layer-10 launches, which every case probes on their own; it selects no other kernel.
  MVS_FORCE_DIRECT=1: conv3d_direct / deconv3d_direct / prob for every layer (fp32 only).
  16-bit "default16": conv0 conv0p16 (conv0z16 needs columns that fill the chip), conv1-conv3 convg16<Op16> (likewise
      convz16), conv4-conv9 the shallow block tiles (tile_fills_chip is false at these sizes), prob prob_lds<16-bit>,
      tail conv11_prob16.  MVS_CONV0Z16=1/0, MVS_CONVZ16=1/0, MVS_DEEP_TILES=1/0 force either side.
  16-bit "fp32arith16" (MVS_MFMA16=0: launch_conv_layer skips launch_layer_mfma16, and launch_layer_split and
      launch_conv0_wino43_split ask for dtype == MVS_F32): the DT = F16 / BF16 instantiations of the fp32-MFMA kernels --
      conv0 conv0_w43<DT> (F(4,3)), conv1 convg<DT> (convg_persist's fall-back; conv1z is `if constexpr (DT == MVS_F32)`),
      conv2 / conv4 convwz<DT> (F(2,3)), conv3 convg<DT>, conv5 / conv6 convs<DT>, conv7 deconvs<DT>, conv8 / conv9
      deconvg<DT>, prob prob_lds<16-bit>; conv11_prob_enabled() is false, so the tail is the layer-9 and layer-10 launches.
      + MVS_CONV0_WINO=0: conv0_4x4<DT>;  + MVS_CONV_WINO=0: conv2 / conv4 convg<DT>;  + MVS_PERSIST_CUS=1:
      convg_persist<DT>.  MVS_SPLIT_DECONV and MVS_CONV1Z change nothing for 16-bit storage (both are read behind a
      dtype == MVS_F32 test) and MVS_FORCE_DIRECT=1 refuses it: UNREACHABLE16 quotes the lines.

16-bit storage, layers 0..9 (probes.py: bound_st, err_st): every check is against the UNROUNDED fp64 value of the
operands as the kernel holds them, within e_max + half a storage ulp; on the lattice an output may differ from
rne_st(ref64) only where ref64 is within e_max of a rounding boundary ("inexact16": [differing, boundary cases] per key,
"unexplained16" must be empty); the rounding-boundary probes and fp16's range ends ("<layer>:boundary:", "<layer>:ends:")
are bit-equal to rne_st of the one exact product, except on a Winograd form, whose transforms are not exact: those keep
the Winograd e_max.  "e_ratios": worst (|got - ref64| - half ulp) / (2^-24 S) of the dense launches, the figure
probes.DENSE_C's rule is applied to.
"""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import guarded as G  # noqa: E402
import probes as P  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from scene_3dreconstruction_mvsnet_amd import _lib, synthetic  # noqa: E402

DEV = "cuda:0"
ALL = tuple(range(11)) + ("tail",)
F32, B16 = ("f32",), ("f16", "bf16")

# case -> environment, storages, layers probed, Winograd form per layer (absent: direct / MFMA / split)
CASES = {
    "default": dict(env={}, storages=F32, layers=ALL, wino={0: "F43"}),
    "conv0_split0": dict(env={"MVS_CONV0_SPLIT": "0"}, storages=F32, layers=(0,), wino={0: "F43"}),
    "conv0_wino0": dict(env={"MVS_CONV0_WINO": "0"}, storages=F32, layers=(0,), wino={}),
    "conv1z": dict(env={"MVS_CONV1Z": "1"}, storages=F32, layers=(1,), wino={}),
    "persist": dict(env={"MVS_PERSIST_CUS": "1", "MVS_CONV1Z": "0"}, storages=F32, layers=(1,), wino={}),
    "split0": dict(env={"MVS_SPLIT_LAYERS": "0"}, storages=F32, layers=(2, 3, 4, 8), wino={2: "F23", 4: "F23"}),
    "split0_wino0": dict(env={"MVS_SPLIT_LAYERS": "0", "MVS_CONV_WINO": "0"}, storages=F32, layers=(2, 4), wino={}),
    "split_deconv3": dict(env={"MVS_SPLIT_DECONV": "3"}, storages=F32, layers=(7, 8), wino={}),
    "split_deconv0": dict(env={"MVS_SPLIT_DECONV": "0"}, storages=F32, layers=(7, 8), wino={}),
    "tail_split0": dict(env={"MVS_TAIL_SPLIT": "0"}, storages=F32, layers=("tail",), wino={}),
    "force_direct": dict(env={"MVS_FORCE_DIRECT": "1"}, storages=F32, layers=tuple(range(11)), wino={}),
    "default16": dict(env={}, storages=B16, layers=ALL, wino={}),
    "conv0z16_1": dict(env={"MVS_CONV0Z16": "1"}, storages=B16, layers=(0,), wino={}),
    "conv0z16_0": dict(env={"MVS_CONV0Z16": "0"}, storages=B16, layers=(0,), wino={}),
    "convz16_1": dict(env={"MVS_CONVZ16": "1"}, storages=B16, layers=(1, 2, 3), wino={}),
    "convz16_0": dict(env={"MVS_CONVZ16": "0"}, storages=B16, layers=(1, 2, 3), wino={}),
    "deep1": dict(env={"MVS_DEEP_TILES": "1"}, storages=B16, layers=(4, 5, 6, 7, 8), wino={}),
    "deep0": dict(env={"MVS_DEEP_TILES": "0"}, storages=B16, layers=(4, 5, 6, 7, 8), wino={}),
    "fp32arith16": dict(env={"MVS_MFMA16": "0"}, storages=B16, layers=tuple(range(11)), arith="fp32",
                        wino={0: "F43", 2: "F23", 4: "F23"}),
    "fp32arith16_conv0_wino0": dict(env={"MVS_MFMA16": "0", "MVS_CONV0_WINO": "0"}, storages=B16, layers=(0,),
                                    arith="fp32", wino={}),
    "fp32arith16_wino0": dict(env={"MVS_MFMA16": "0", "MVS_CONV_WINO": "0"}, storages=B16, layers=(2, 4), arith="fp32",
                              wino={}),
    "fp32arith16_persist": dict(env={"MVS_MFMA16": "0", "MVS_PERSIST_CUS": "1"}, storages=B16, layers=(1,),
                                arith="fp32", wino={}),
}

# every templated launcher instantiation of the CostRegNet conv kernels (run_*<...> in csrc/conv*.hip, whitespace
# removed) and every kernel launched directly -> the case that reaches it.  test_conv_probes_host.py parses the
# sources: a new instantiation or kernel without an entry here fails the CPU suite.
INSTANTIATIONS = {
    "run_direct<32,8,8,1,false,true,false>": "force_direct",
    "run_direct<8,16,16,2,false,true,false>": "force_direct",
    "run_direct<16,16,16,1,false,true,false>": "force_direct",
    "run_direct<16,32,16,2,false,true,false>": "force_direct",
    "run_direct<32,32,8,1,false,true,false>": "force_direct",
    "run_direct<32,64,4,2,false,true,false>": "force_direct",
    "run_direct<64,64,4,1,false,true,false>": "force_direct",
    "run_direct<64,32,8,2,true,true,true>": "force_direct",
    "run_direct<32,16,16,2,true,true,true>": "force_direct",
    "run_deconv<16,8,8>": "force_direct",
    "run_conv0_4x4<DT>": "conv0_wino0",
    "run_conv0_w43<DT>": "conv0_split0",
    "run_convwz<DT,16,16,4,2>": "split0",
    "run_convwz<DT,32,32,2,2>": "split0",
    "run_convg_persist<DT,8,16,2,1,2,2>": "persist",
    "run_convg<DT,16,16,1,2,4,2>": "split0_wino0",
    "run_convg<DT,16,32,2,1,2,2>": "split0",
    "run_convg<DT,32,32,1,1,2,2>": "split0_wino0",
    "run_deconvg<DT,32,16,1,4,1>": "split_deconv0",
    "run_deconvg<DT,16,8,1,4,2>": "default",
    "run_convs<DT,32,64,2,1,2,1,4>": "default",
    "run_convs<DT,64,64,1,1,2,1,4>": "default",
    "run_deconvs<DT,64,32,1,2,1,4>": "default",
    "run_convg16<OpSplit,16,16,1,2,4,2>": "default",
    "run_convg16<OpSplit,16,32,2,2,2,1>": "default",
    "run_convg16<OpSplit,32,32,1,4,2,1>": "default",
    "run_deconvg16<OpSplit,64,32,1,1,1>": "split_deconv3",
    "run_deconvg16<OpSplit,32,16,2,4,1>": "default",
    "run_convg16<Op16<DT>,8,16,2,2,2,2>": "convz16_0",
    "run_convg16<Op16<DT>,16,16,1,2,4,2>": "convz16_0",
    "run_convg16<Op16<DT>,16,32,2,4,1,1>": "convz16_0",
    "run_convg16<Op16<DT>,32,32,1,4,2,1>": "deep1",
    "run_convg16<Op16<DT>,32,32,1,1,2,2>": "deep0",
    "run_convg16<Op16<DT>,32,64,2,2,1,1>": "deep1",
    "run_convg16<Op16<DT>,32,64,2,1,1,1>": "deep0",
    "run_convg16<Op16<DT>,64,64,1,4,1,1>": "deep1",
    "run_convg16<Op16<DT>,64,64,1,1,1,1>": "deep0",
    "run_deconvg16<Op16<DT>,64,32,2,1,1>": "deep1",
    "run_deconvg16<Op16<DT>,64,32,1,1,1>": "deep0",
    "run_deconvg16<Op16<DT>,32,16,4,2,1>": "deep1",
    "run_deconvg16<Op16<DT>,32,16,1,4,1>": "deep0",
    "run_deconvg16<Op16<DT>,16,8,1,4,2>": "default16",
    "run_convz16<DT,8,16,2>": "convz16_1",
    "run_convz16<DT,16,16,1>": "convz16_1",
    "run_convz16<DT,16,32,2>": "convz16_1",
}
# every launcher templated on the storage type DT -> the case that runs it with 16-BIT storage (its F32 case in the table
# above does not count: St<DT>::load4 / store4 are other loads, stores and casts).  test_conv_probes_host.py requires
# an entry for every instantiation whose arguments name DT.
INSTANTIATIONS16 = {
    "run_conv0_4x4<DT>": "fp32arith16_conv0_wino0",
    "run_conv0_w43<DT>": "fp32arith16",
    "run_convwz<DT,16,16,4,2>": "fp32arith16",
    "run_convwz<DT,32,32,2,2>": "fp32arith16",
    "run_convg_persist<DT,8,16,2,1,2,2>": "fp32arith16_persist",
    "run_convg<DT,16,16,1,2,4,2>": "fp32arith16_wino0",
    "run_convg<DT,16,32,2,1,2,2>": "fp32arith16",
    "run_convg<DT,32,32,1,1,2,2>": "fp32arith16_wino0",
    "run_deconvg<DT,32,16,1,4,1>": "fp32arith16",
    "run_deconvg<DT,16,8,1,4,2>": "fp32arith16",
    "run_convs<DT,32,64,2,1,2,1,4>": "fp32arith16",
    "run_convs<DT,64,64,1,1,2,1,4>": "fp32arith16",
    "run_deconvs<DT,64,32,1,2,1,4>": "fp32arith16",
    "run_convg16<Op16<DT>,8,16,2,2,2,2>": "convz16_0",
    "run_convg16<Op16<DT>,16,16,1,2,4,2>": "convz16_0",
    "run_convg16<Op16<DT>,16,32,2,4,1,1>": "convz16_0",
    "run_convg16<Op16<DT>,32,32,1,4,2,1>": "deep1",
    "run_convg16<Op16<DT>,32,32,1,1,2,2>": "deep0",
    "run_convg16<Op16<DT>,32,64,2,2,1,1>": "deep1",
    "run_convg16<Op16<DT>,32,64,2,1,1,1>": "deep0",
    "run_convg16<Op16<DT>,64,64,1,4,1,1>": "deep1",
    "run_convg16<Op16<DT>,64,64,1,1,1,1>": "deep0",
    "run_deconvg16<Op16<DT>,64,32,2,1,1>": "deep1",
    "run_deconvg16<Op16<DT>,64,32,1,1,1>": "deep0",
    "run_deconvg16<Op16<DT>,32,16,4,2,1>": "deep1",
    "run_deconvg16<Op16<DT>,32,16,1,4,1>": "deep0",
    "run_deconvg16<Op16<DT>,16,8,1,4,2>": "default16",
    "run_convz16<DT,8,16,2>": "convz16_1",
    "run_convz16<DT,16,16,1>": "convz16_1",
    "run_convz16<DT,16,32,2>": "convz16_1",
}
# what 16-bit storage cannot reach, and the line of the dispatch that excludes it (file, line as written)
UNREACHABLE16 = {
    "conv1z_mfma_kernel (run_conv1z)": ("launch_plan.h", "if (dtype == MVS_F32 && opt.conv1z != 0 &&"),
    "conv3d_direct_kernel / deconv3d_direct_kernel (MVS_FORCE_DIRECT=1)": (
        "conv3d_direct.hip",
        'return fail(MVS_ERR_BAD_DTYPE, "MVS_FORCE_DIRECT kernels are fp32-storage only (dtype %d)", dtype);'),
    "the split-operand tile kernels run_convg16<OpSplit,...> / run_deconvg16<OpSplit,...> (MVS_SPLIT_DECONV)": (
        "launch_plan.h", "if (opt.split_layers && dtype == MVS_F32) {"),
    "conv0_w48t_kernel (launch_conv0_wino43_split)": (
        "launch_plan.h", "return formed(opt.conv0_split && dtype == MVS_F32 ? kConv0WinoSplit : kConv0Wino);"),
    "the fused 16-bit tail conv11_prob16_kernel under MVS_MFMA16=0": (
        "launch_plan.h",
        "inline bool tail_fused(int dtype, const Options& opt) { return opt.fuse_prob && (dtype == MVS_F32 || opt.mfma16); }"),
}
KERNELS = {
    "conv0_w48t_kernel": "default",
    "conv0_w43_mfma_kernel": "conv0_split0",
    "conv0_4x4_mfma_kernel": "conv0_wino0",
    "conv1z_mfma_kernel": "conv1z",
    "convg_mfma_kernel": "default",
    "convg_persist_mfma_kernel": "persist",
    "convwz_mfma_kernel": "split0",
    "convs_mfma_kernel": "default",
    "deconvs_mfma_kernel": "default",
    "deconvg_mfma_kernel": "default",
    "convg16_mfma_kernel": "default",
    "deconvg16_mfma_kernel": "default",
    "convz16_mfma_kernel": "convz16_1",
    "conv0z16_mfma_kernel": "conv0z16_1",
    "conv0p16_mfma_kernel": "conv0z16_0",
    "conv3d_direct_kernel": "force_direct",
    "deconv3d_direct_kernel": "force_direct",
    "prob_lds_kernel": "default",
    "conv11_prob_split_kernel": "default",
    "conv11_prob_priv_kernel": "tail_split0",
    "conv11_prob16_kernel": "default16",
}


# The smallest volumes mvs_conv_layer / mvs_conv11_prob admit (include/mvs_abi.h: Di, Hi, Wi >= 1, even at the stride-2
# layers): no tile of any form is filled in any dimension -- one voxel, one row along each axis, odd D through the
# two-plane F(2,3) tiles, D below the z-marching pipelines' depth, D % 4 != 0 at conv0 (conv0_mfma instead of the
# F(4,3) forms) and its smallest D % 4 == 0.  Dense standard-normal input against the dense bound of the form the
# dispatch takes, every launch in a guarded arena under the three poisons (tests/guarded.py).
TINY_S1 = ((1, 1, 1), (3, 1, 1), (1, 3, 1), (1, 1, 3), (5, 2, 9))
TINY_S2 = ((2, 2, 2), (6, 2, 2), (2, 6, 2), (2, 2, 6), (4, 2, 10))
TINY_CONV0 = ((4, 1, 1), (8, 1, 1), (5, 1, 1))
TINY_TAIL = ((1, 1, 1), (3, 1, 1), (1, 3, 1), (1, 1, 3), (2, 3, 5))
TINY_TAIL_CASES = ("default", "tail_split0", "default16")
ARENA_BYTES = 32 << 20


def tiny_shapes(layer):
    if layer == "tail":
        return TINY_TAIL
    return (TINY_S2 if P.GEOM[layer][2] == 2 and not P.GEOM[layer][3] else TINY_S1) + (TINY_CONV0 if layer == 0 else ())


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class Checker:
    def __init__(self, case):
        self.case = case
        self.ratios, self.inexact, self.unexplained, self.eratios, self.failures = {}, {}, {}, {}, []

    def add(self, key, err, bound):
        r = float((err / bound).max()) if err.size else 0.0
        self.ratios[key] = max(self.ratios.get(key, 0.0), r)
        if r > 1.0:
            i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
            self.failures.append(f"{key}: {r:.3g} x bound at {tuple(int(v) for v in i)} (err {float(err[i]):.3e}, "
                                 f"bound {float(bound[i]):.3e})")


def run_layer(layer, x, skip, blob, storage):
    code = _lib.dtype_code(storage)
    tdt = _lib.TORCH_DTYPES[code]
    xt = _lib.to_c8(cu(x)).to(tdt)
    st = None if skip is None else _lib.to_c8(cu(skip)).to(tdt)
    y = _lib.conv_layer(layer, xt, st, blob, dtype=code).float()
    return (y if layer == 10 else _lib.from_c8(y)).cpu().numpy().astype(np.float64)


def run_tail(x, skip, blob, storage):
    code = _lib.dtype_code(storage)
    tdt = _lib.TORCH_DTYPES[code]
    return _lib.conv11_prob(_lib.to_c8(cu(x)).to(tdt), _lib.to_c8(cu(skip)).to(tdt), blob,
                            dtype=code).cpu().numpy().astype(np.float64)


def out_shape(layer):
    ci, co, s, tr, (D, H, W) = P.GEOM[layer]
    if tr:
        return (co, 2 * D, 2 * H, 2 * W)
    return (co, (D - 1) // s + 1, (H - 1) // s + 1, (W - 1) // s + 1)


def narrowed(layer, storage):
    return storage != "f32" and layer != 10


def check_single(chk, key, layer, got, x, skip, wf, sh, storage, wino, arith="mfma16"):
    if not narrowed(layer, storage):
        want, bound = P.probe_want_bound(layer, x, skip, wf, sh, storage, wino, arith)
        chk.add(key, np.abs(got - want), bound)
        return
    ref, emax = P.ref_emax(layer, x, skip, wf, sh, storage, wino, arith)
    diff = got != P.rne_st(ref, storage)
    near = P.near_boundary_st(ref, emax, storage)
    d, n = chk.inexact.get(key, (0, 0))
    chk.inexact[key] = (d + int(diff.sum()), n + int(near.sum()))
    bad = diff & ~near
    if bad.any():
        chk.unexplained[key] = chk.unexplained.get(key, 0) + int(bad.sum())
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        chk.failures.append(f"{key}: {int(bad.sum())} outputs differ from RNE(ref64) away from every rounding boundary, "
                            f"first at {i}: got {float(got[i])!r}, ref64 {float(ref[i])!r}, e_max {float(emax[i]):.3e}")
    chk.add(key, *P.err_st(got, ref, emax, storage))


def check_exact(chk, key, layer, got, x, skip, wf, sh, storage, wino, arith):
    """One exact product per output: bit-equal to rne_st(product).  A Winograd form's transforms are not exact (the
    1/6 and 1/24 of G, sums of neighbouring planes): it is held to err_st with its own e_max."""
    ref, emax = P.ref_emax(layer, x, skip, wf, sh, storage, wino, arith)
    if wino:
        chk.add(key, *P.err_st(got, ref, emax, storage))
        return
    bad = got != P.rne_st(ref, storage)
    chk.ratios[key] = max(chk.ratios.get(key, 0.0), 2.0 * int(bad.sum()))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        chk.failures.append(f"{key}: {int(bad.sum())} of {bad.size} outputs are not RNE of their one product, first at "
                            f"{i}: got {float(got[i])!r}, product {float(ref[i])!r}")


def check_dense(chk, key, layer, got, x, skip, wf, sh, storage, wino, arith="mfma16"):
    if not narrowed(layer, storage):
        ref, bound = P.dense_ref_bound(layer, x, skip, wf, sh, storage, wino, arith)
        chk.add(key, np.abs(got - ref), bound)
        return
    ref, emax = P.ref_emax(layer, x, skip, wf, sh, storage, wino, arith, dense=True)
    err, bound = P.err_st(got, ref, emax, storage)
    chk.add(key, err, bound)
    if not wino:     # e / (u S): what is left of the error once the half ulp of the cast is taken off
        e = np.where(np.isfinite(err), err - (bound - emax), 0.0) / (emax / P.DENSE_C)
        chk.eratios[key] = max(chk.eratios.get(key, 0.0), float(e.max()))


def probe_layer(chk, layer, storage, sd, blobs_crafted, wino, rng, arith="mfma16"):
    ci, co, _, tr, shape = P.GEOM[layer]
    blob = blobs_crafted["rand"]
    wf, sh = P.folded(sd, layer)
    oshape = out_shape(layer)
    sp = P.spacing(layer, wino)
    for ph in P.phases(sp):
        x = P.lattice(ci, shape, sp, ph, rng)
        skip = rng.standard_normal(oshape).astype(np.float32) if tr else None
        got = run_layer(layer, x, skip, blob, storage)
        check_single(chk, f"{layer}:lattice:{storage}", layer, got, x, skip, wf, sh, storage, wino, arith)
    if narrowed(layer, storage):
        probe_boundaries(chk, layer, storage, blobs_crafted, wino, arith)
    if storage == "f32":
        runs = 27 if layer == 10 else P.crafted_runs(layer)
        for r in range(runs):
            sdc, blob_c = blobs_crafted[r]
            wfc, shc = P.folded(sdc, layer)
            x = P.crafted((ci,) + shape, rng)
            skip = np.zeros(oshape, np.float32) if tr else None
            got = run_layer(layer, x, skip, blob_c, storage)
            check_single(chk, f"{layer}:crafted:{storage}", layer, got, x, skip, wfc, shc, storage, wino)
    vols = [rng.standard_normal((ci,) + shape).astype(np.float32)]
    if storage == "f32":   # heavy-tailed non-negative, as a variance volume (fp16 would overflow)
        vols.append(np.exp(3.0 * rng.standard_normal((ci,) + shape)).astype(np.float32))
    for x in vols:
        skip = rng.standard_normal(oshape).astype(np.float32) if tr else None
        got = run_layer(layer, x, skip, blob, storage)
        check_dense(chk, f"{layer}:dense:{storage}", layer, got, x, skip, wf, sh, storage, wino, arith)
    if narrowed(layer, storage):   # heavy-tailed, non-negative; fp16 in the largest octave that keeps the output finite
        x, skip = P.heavy_launch(layer, storage, wf, sh, arith)
        got = run_layer(layer, x, skip, blob, storage)
        check_dense(chk, f"{layer}:heavy:{storage}", layer, got, x, skip, wf, sh, storage, wino, arith)


def probe_boundaries(chk, layer, storage, blobs, wino, arith):
    """The rounding-boundary probes of probes.py (every run, every exponent set) and, for fp16, the ends of its range."""
    ci, _, _, tr, shape = P.GEOM[layer]
    skip = np.zeros(out_shape(layer), np.float32) if tr else None
    brng = np.random.default_rng(41 + layer)
    for r in range(P.boundary_runs(layer)):
        sdb, blob_b = blobs[("boundary", storage, r)]
        wfb, shb = P.folded(sdb, layer)
        for exps in P.BOUNDARY_EXPS[storage]:
            x = P.boundary_inputs((ci,) + shape, storage, exps, brng)
            got = run_layer(layer, x, skip, blob_b, storage)
            check_exact(chk, f"{layer}:boundary:{storage}", layer, got, x, skip, wfb, shb, storage, wino, arith)
    if storage == "f16":
        sde, blob_e = blobs[("ends",)]
        wfe, she = P.folded(sde, layer)
        x = P.ends_inputs(ci, shape, brng)
        got = run_layer(layer, x, skip, blob_e, storage)
        check_exact(chk, f"{layer}:ends:{storage}", layer, got, x, skip, wfe, she, storage, wino, arith)


def probe_tail(chk, storage, sd, blobs_crafted, rng):
    """conv11_prob: prob.weight with one nonzero entry (channel, tap) swept over the 27 taps (channel 3 r % 8), the
    input on the spacing-2 lattice of a transposed layer (phase r % 8): every logit is pw d11 + pb with d11 a single
    product + shift + skip."""
    q = lambda t: orc.round_storage(np.asarray(t, np.float32), storage)  # noqa: E731
    D, H, W = P.TAIL_SHAPE
    sshape = (8, 2 * D, 2 * H, 2 * W)
    w9, sh9 = P.folded(sd, 9)
    wq = w9 if storage == "f32" else q(w9)
    sp = (2, 2, 2)
    ph = P.phases(sp)
    key = f"tail:lattice:{storage}"
    for r in range(27):
        sdr = dict(sd)
        sdr["prob.weight"] = P.single_prob_weight((3 * r) % 8, r, np.float32(rng.standard_normal()))
        blob = _lib.pack_weights(sdr).to(DEV)
        x = q(P.lattice(16, (D, H, W), sp, ph[r % 8], rng))
        skip = q(rng.standard_normal(sshape).astype(np.float32))
        got = run_tail(x, skip, blob, storage)
        want, S = P.tail64(x, skip, wq, sh9, sdr["prob.weight"], sdr["prob.bias"])
        chk.add(key, np.abs(got - want), P.TAIL_ULPS * P.ulp32(S))
    if storage == "f32":
        for r in range(27):
            sdc, blob_c = blobs_crafted[r]
            w9c, sh9c = P.folded(sdc, 9)
            x = P.crafted((16, D, H, W), rng)
            skip = np.zeros(sshape, np.float32)
            got = run_tail(x, skip, blob_c, storage)
            want, S = P.tail64(x, skip, w9c, sh9c, sdc["prob.weight"], sdc["prob.bias"])
            chk.add(f"tail:crafted:{storage}", np.abs(got - want), P.TAIL_ULPS * P.ulp32(S))
    blob = blobs_crafted["rand"]
    for x in (rng.standard_normal((16, D, H, W)).astype(np.float32),):
        x = q(x)
        skip = q(rng.standard_normal(sshape).astype(np.float32))
        got = run_tail(x, skip, blob, storage)
        want, S = P.tail64(x, skip, wq, sh9, sd["prob.weight"], sd["prob.bias"])
        chk.add(f"tail:dense:{storage}", np.abs(got - want), P.DENSE_C * P.U * S)


def tiny_out_shape(layer, shape):
    _, co, s, tr, _ = P.GEOM[layer]
    return (co,) + tuple(2 * n if tr else (n - 1) // s + 1 for n in shape)


def guarded_call(arena, fn, oshape):
    """fn(A) -> one output tensor carved from A; the output as float64 numpy [C, D, H, W] ([D, H, W] for logits)"""
    code_out = {}

    def run(A):
        y = fn(A)
        code_out["dtype"], code_out["shape"] = y.dtype, tuple(y.shape)
        return y
    (raw,), _ = G.same_under_all_poisons(arena, run)
    y = raw.view(code_out["dtype"]).view(code_out["shape"]).float()
    y = _lib.from_c8(y) if y.dim() == 5 else y
    assert tuple(y.shape) == tuple(oshape), (tuple(y.shape), oshape)
    return y.numpy().astype(np.float64)


def probe_tiny(chk, arena, layer, storage, sd, blob, wino, rng, arith="mfma16"):
    code = _lib.dtype_code(storage)
    tdt = _lib.TORCH_DTYPES[code]
    if layer == "tail":
        q = lambda t: orc.round_storage(np.asarray(t, np.float32), storage)  # noqa: E731
        w9, sh9 = P.folded(sd, 9)
        wq = w9 if storage == "f32" else q(w9)
        for D, H, W in TINY_TAIL:
            x = q(rng.standard_normal((16, D, H, W)).astype(np.float32))
            skip = q(rng.standard_normal((8, 2 * D, 2 * H, 2 * W)).astype(np.float32))

            def run(A):
                xt, st = A.put(_lib.to_c8(cu(x)).to(tdt), "in", "x"), A.put(_lib.to_c8(cu(skip)).to(tdt), "in", "skip")
                b = A.put(blob, "in", "blob")
                with A.intercept(_lib):
                    return _lib.conv11_prob(xt, st, b, dtype=code)
            got = guarded_call(arena, run, (2 * D, 2 * H, 2 * W))
            want, S = P.tail64(x, skip, wq, sh9, sd["prob.weight"], sd["prob.bias"])
            chk.add(f"tail:tiny:{storage}", np.abs(got - want), P.DENSE_C * P.U * S)
        return
    ci, _, _, tr, _ = P.GEOM[layer]
    wf, sh = P.folded(sd, layer)
    for shape in tiny_shapes(layer):
        oshape = tiny_out_shape(layer, shape)
        x = rng.standard_normal((ci,) + shape).astype(np.float32)
        skip = rng.standard_normal(oshape).astype(np.float32) if tr else None

        def run(A):
            xt = A.put(_lib.to_c8(cu(x)).to(tdt), "in", "x")
            st = None if skip is None else A.put(_lib.to_c8(cu(skip)).to(tdt), "in", "skip")
            b = A.put(blob, "in", "blob")
            with A.intercept(_lib):
                return _lib.conv_layer(layer, xt, st, b, dtype=code)
        got = guarded_call(arena, run, oshape[1:] if layer == 10 else oshape)
        # conv0's F(4,3) forms need D % 4 == 0: any other D runs conv0_mfma and is held to the direct forms' bound
        form = None if layer == 0 and shape[0] % 4 else wino
        if narrowed(layer, storage):
            ref, emax = P.ref_emax(layer, x, skip, wf, sh, storage, form, arith, dense=True)
            chk.add(f"{layer}:tiny:{storage}", *P.err_st(got, ref, emax, storage))
            continue
        ref, bound = P.dense_ref_bound(layer, x, skip, wf, sh, storage, form, arith)
        if layer == 10:
            ref, bound = ref[0], bound[0]
        chk.add(f"{layer}:tiny:{storage}", np.abs(got - ref), bound)


class CraftedBlobs(dict):
    """run -> (crafted state, packed blob on the GPU), packed on first use; "rand" -> the random state's blob."""

    def __init__(self, sd):
        super().__init__(rand=_lib.pack_weights(sd).to(DEV))
        self.sd = sd

    def __missing__(self, r):
        if isinstance(r, tuple):     # ("boundary", storage, run) / ("ends",): the 16-bit rounding probes
            sdc = P.ends_state(self.sd) if r[0] == "ends" else P.boundary_state(self.sd, r[2], r[1])
            self[r] = (sdc, _lib.pack_weights(sdc).to(DEV))
            return self[r]
        sdc = P.crafted_state(self.sd, r, np.random.default_rng(1000 + r))
        self[r] = (sdc, _lib.pack_weights(sdc).to(DEV))
        return self[r]


def main():
    t0 = time.perf_counter()
    name = sys.argv[1]
    case = CASES[name]
    arith = case.get("arith", "mfma16")
    for k, v in case["env"].items():
        assert os.environ.get(k) == v, f"case {name} needs {k}={v} in the environment"
    sd = synthetic.random_costreg_state(seed=13)
    blobs = CraftedBlobs(sd)
    chk = Checker(name)
    arena = G.Arena(ARENA_BYTES, DEV)
    for storage in case["storages"]:
        rng = np.random.default_rng(17)
        for layer in case["layers"]:
            if layer == "tail":
                probe_tail(chk, storage, sd, blobs, rng)
            else:
                probe_layer(chk, layer, storage, sd, blobs, case["wino"].get(layer), rng, arith)
        trng = np.random.default_rng(29)     # a stream of their own: the probes above keep their inputs
        for layer in case["layers"]:
            if layer != "tail" or name in TINY_TAIL_CASES:
                probe_tiny(chk, arena, layer, storage, sd, blobs["rand"], case["wino"].get(layer), trng, arith)
    print(json.dumps({"case": name, "ratios": {k: round(v, 4) for k, v in chk.ratios.items()},
                      "inexact16": chk.inexact, "unexplained16": chk.unexplained,
                      "e_ratios": {k: round(v, 3) for k, v in chk.eratios.items()},
                      "seconds": round(time.perf_counter() - t0, 1)}))
    for f in chk.failures:
        print("FAIL", name, f)
    return 1 if chk.failures else 0


if __name__ == "__main__":
    sys.exit(main())
