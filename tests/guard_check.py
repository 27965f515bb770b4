#!/usr/bin/env python3
"""Child-process helper of tests/test_gpu_guarded.py: runs a list of poison-and-guard cases (tests/guarded.py) under
whatever kernel-selection environment the parent set (read once per process by options() in mvs_host.hip).

    guard_check.py CASES.json RESULTS.json

Every case is {"id", "entries": [mvs_* names], "env", "kind", "args"}.  A case runs its call three times in the arena,
once per poison, with every output, workspace and input between guards; the outputs must be the same bytes in the
three runs and equal to a plain call's, no guard byte and no input may change.  The results file maps each id to
{"ok", "msg", "shape", "guard_bytes", "exempt"} and is rewritten after every case.  The child stops at its first HIP
error, which is any RuntimeError but an argument refusal of the library (exit status 2): the cases after it have no
verdict.

STATIC_CASES lists the cases that do not depend on the device; the parent adds the run-time z-chunk splits, whose
shapes depend on the CU count (tests/zchunks.py).
"""
import json
import os
import sys
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import guarded as G  # noqa: E402
import probe_check  # noqa: E402
import probes as P  # noqa: E402
import warp_ref as W  # noqa: E402
import warp_ref_check  # noqa: E402

DEV = "cuda:0"
ARENA_BYTES = 1 << 30
STORAGES = ("f32", "f16", "bf16")
WARP_RIGS = ("dtu_n4", "dtu_n5", "borders")      # D = 8; D = 48 (slab 40 + 8); all four borders crossed
HOMO_RIGS = ("odd", "border")
COSTREG_SHAPE = (16, 24, 40)                     # ragged at every level: 24 x 40 -> 12 x 20 -> 6 x 10 -> 3 x 5
# softargmin: every instantiation of launch_softargmin at its smallest D, hw = 127 * 131 (odd, >= 16384) for the
# 32-pixel forms; D = 17 with odd h w for the ragged last block
SOFTARGMIN_SHAPES = ((8, 127, 131), (136, 127, 131), (200, 127, 131), (17, 3, 5), (136, 5, 7), (264, 5, 7))
DEPTH_INFER = dict(N=4, h=24, w=40, D=32, kw=dict(yaw_deg=2.0))   # of test_depth_infer_matches_oracle_random
FEAT_SIZES = ((2, 50, 70), (2, 64, 96))          # test_feature_net_ragged_size_matches_oracle's, and a 32-aligned one
METRIC_SHAPES = ((1, 1, 1), (3, 37, 53))
TRAIN_CONV = ("conv6_tiny", "conv4_tiny", "conv5_tiny", "conv3_tiny", "conv2_tiny", "prob_tiny",
              "layer0", "layer1", "layer7")      # TINY, and a stride-1, a stride-2 and a transposed geometry of CASES
BN_CASES = ((64, 2), (64, 12), (8, 1001))
GRAD_RIG = "dtu_n4"


def _case(cid, entries, env, kind, **args):
    return {"id": cid, "entries": list(entries), "env": dict(env), "kind": kind, "args": args}


def static_cases():
    out = []
    for name, c in probe_check.CASES.items():
        for st in c["storages"]:
            for layer in c["layers"]:
                if layer == "tail":
                    out.append(_case(f"conv-{name}-tail-{st}", ["mvs_conv11_prob"], c["env"], "tail", storage=st))
                else:
                    out.append(_case(f"conv-{name}-layer{layer}-{st}", ["mvs_conv_layer"], c["env"], "layer",
                                     layer=layer, storage=st))
            out.append(_case(f"conv-{name}-costreg-{st}", ["mvs_costreg_forward"], c["env"], "costreg", storage=st))
    for name, e in warp_ref_check.ENVS.items():
        for st in e["storages"]:
            for rig in WARP_RIGS:
                out.append(_case(f"warp-{name}-{rig}-{st}", ["mvs_warp_variance", "mvs_relative_proj"], e["env"], "warp",
                                 rig=rig, storage=st))
        for rig in HOMO_RIGS:
            out.append(_case(f"warp-{name}-homo-{rig}", ["mvs_homo_warp"], e["env"], "homo", rig=rig))
    d = {}
    for D, h, w in SOFTARGMIN_SHAPES:
        out.append(_case(f"softargmin-D{D}h{h}w{w}", ["mvs_softargmin_conf", "mvs_depth_regression",
                                                      "mvs_softargmin_backward"], d, "softargmin", shape=[D, h, w]))
    for st in STORAGES:
        out.append(_case(f"depth_infer-{st}", ["mvs_depth_infer", "mvs_depth_infer_views"], d, "depth_infer", storage=st))
    for N, H, Wd in FEAT_SIZES:
        for fmt in ("f32_chw", "u8_chw", "u8_hwc"):
            out.append(_case(f"feature_net-{fmt}-{H}x{Wd}", ["mvs_feature_net_fmt"], d, "feature_net",
                             shape=[N, H, Wd], fmt=fmt))
        out.append(_case(f"feature_net-plain-{H}x{Wd}", ["mvs_feature_net"], d, "feature_net_plain", shape=[N, H, Wd]))
        out.append(_case(f"feature_slot-{H}x{Wd}", ["mvs_feature_net_fmt"], d, "feature_slot", shape=[N, H, Wd]))
        out.append(_case(f"feature_layers-{H}x{Wd}", ["mvs_feature_layer", "mvs_feature_conv01_fmt"], d, "feature_layers",
                         shape=[N, H, Wd]))
    for st in STORAGES:
        for fmt in ("f32_chw", "u8_hwc"):
            out.append(_case(f"forward_images-{fmt}-{st}", ["mvs_forward_images_fmt"], d, "forward_images",
                             storage=st, fmt=fmt))
    out.append(_case("forward_images-plain", ["mvs_forward_images"], d, "forward_images_plain"))
    out.append(_case("filter_depth", ["mvs_filter_depth"], d, "filter"))
    for B, h, w in METRIC_SHAPES:
        for errmap in (True, False):
            out.append(_case(f"depth_metrics-B{B}h{h}w{w}-{'errmap' if errmap else 'null'}", ["mvs_depth_metrics"], d,
                             "metrics", shape=[B, h, w], errmap=errmap))
    for name in TRAIN_CONV:
        out.append(_case(f"train_conv-{name}", ["mvs_conv3d_train_forward", "mvs_conv3d_train_backward_data",
                                                "mvs_conv3d_train_backward_weight"], d, "train_conv", name=name))
    for C, M in BN_CASES:
        for relu in (True, False):
            for skip in (True, False):
                out.append(_case(f"bn3d-C{C}M{M}-relu{int(relu)}-skip{int(skip)}",
                                 ["mvs_bn3d_train_forward", "mvs_bn3d_train_backward"], d, "bn3d", C=C, M=M, relu=relu,
                                 skip=skip))
    out.append(_case("warp_variance_backward", ["mvs_warp_variance_backward"], d, "warp_backward"))
    for C, dims in ((32, (8, 8, 8)), (8, (16, 16, 24))):
        out.append(_case(f"volume_relayout-C{C}", ["mvs_volume_relayout"], d, "relayout", C=C, dims=list(dims)))
    out.append(_case("module-A-B-A", ["mvs_forward_images_fmt"], d, "module"))
    return out


STATIC_CASES = static_cases()


# ------------------------------------------------------------------------------------------------ the child
def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class Runner:
    def __init__(self):
        from conftest import load_fixture, load_weights
        from scene_3dreconstruction_mvsnet_amd import _lib, synthetic
        self.lib, self.syn, self.load_fixture = _lib, synthetic, load_fixture
        self.arena = G.Arena(ARENA_BYTES, DEV)
        self.load_weights = load_weights
        self._blob = self._weights = self._fblob = None     # made on first use: most children need only one of them
        self._model = None

    @property
    def blob(self):
        if self._blob is None:
            self._blob = self.lib.pack_weights(self.syn.random_costreg_state(seed=13)).to(DEV)
        return self._blob

    @property
    def weights(self):
        if self._weights is None:
            self._weights = self.load_weights()
        return self._weights

    @property
    def fblob(self):
        if self._fblob is None:
            st = {k[len("feature."):]: v for k, v in self.weights.items() if k.startswith("feature.")}
            self._fblob = self.lib.pack_feature_weights(st).to(DEV)
        return self._fblob

    def check(self, fn):
        return G.guarded_and_plain(self.arena, fn)

    def c8(self, x, storage):
        return self.lib.to_c8(cu(x)).to(self.lib.TORCH_DTYPES[self.lib.dtype_code(storage)])

    # ---------------------------------------------------------------- CostRegNet
    def conv_layer_at(self, layer, shape, storage, seed):
        L = self.lib
        ci, co = L._LAYER_CH[layer]
        rng = np.random.default_rng(seed)
        x = self.c8(rng.standard_normal((ci,) + tuple(shape)), storage)
        skip = None
        if 7 <= layer <= 9:
            skip = self.c8(rng.standard_normal((co,) + tuple(2 * s for s in shape)), storage)
        code = L.dtype_code(storage)

        def run(A):
            xt, st, blob = A.put(x, "in", "x"), None if skip is None else A.put(skip, "in", "skip"), A.put(self.blob, "in", "blob")
            with A.intercept(L):
                return L.conv_layer(layer, xt, st, blob, dtype=code)
        return self.check(run), [ci] + list(shape)

    def layer(self, layer, storage):
        return self.conv_layer_at(layer, P.GEOM[layer][4], storage, 100 + layer)

    def tail_at(self, shape, storage, seed):
        L = self.lib
        rng = np.random.default_rng(seed)
        x = self.c8(rng.standard_normal((16,) + tuple(shape)), storage)
        skip = self.c8(rng.standard_normal((8,) + tuple(2 * s for s in shape)), storage)
        code = L.dtype_code(storage)

        def run(A):
            xt, st, blob = A.put(x, "in", "x"), A.put(skip, "in", "skip"), A.put(self.blob, "in", "blob")
            with A.intercept(L):
                return L.conv11_prob(xt, st, blob, dtype=code)
        return self.check(run), [16] + list(shape)

    def tail(self, storage):
        return self.tail_at(P.TAIL_SHAPE, storage, 99)

    def zchunk(self, op, layer, storage, shape):
        D, h, w = shape
        if op == "conv11_prob":
            return self.tail_at((D // 2, h // 2, w // 2), storage, D + h + w)
        lvl = 0 if layer <= 1 else 1
        return self.conv_layer_at(layer, (D >> lvl, h >> lvl, w >> lvl), storage, D + h + w)

    def costreg(self, storage):
        L = self.lib
        D, h, w = COSTREG_SHAPE
        code = L.dtype_code(storage)
        var = self.c8(np.abs(np.random.default_rng(7).standard_normal((32, D, h, w))), storage)
        nbytes = L.query_workspace(2, 32, D, h, w, code)

        def run(A):
            v, blob = A.put(var, "in", "var"), A.put(self.blob, "in", "blob")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            with A.intercept(L):
                return L.costreg_forward(v, blob, ws, dtype=code)
        return self.check(run), [32, D, h, w]

    # ---------------------------------------------------------------- warp + variance
    def warp(self, rig, storage):
        L = self.lib
        c = W.CASES[rig][0]()
        N, Cn, h, w = c["feats"].shape
        D = len(c["dv"])
        code = L.dtype_code(storage)
        feats, proj, dv = cu(c["feats"]), cu(c["proj"]), cu(c["dv"])
        nbytes = L.query_workspace(N, Cn, D, h, w, code)

        def run(A):
            f, p, d = A.put(feats, "in", "feats"), A.put(proj, "in", "proj"), A.put(dv, "in", "depth_values")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            with A.intercept(L):
                rt = L.relative_proj(p)
                var = L.warp_variance(f, rt, d, ws, dtype=code)
            return rt, var
        gb = self.check(run)
        var = run(G.Plain(DEV))[1]
        assert bool(torch.isfinite(var.float()).all()), "the rig must have no non-finite coordinates"
        return gb, [N, Cn, D, h, w]

    def homo(self, rig):
        L = self.lib
        c = W.homo_cases()[rig]
        Cn, h, w = c["fea"].shape
        D = len(c["dv"])
        fea, proj, dv = cu(c["fea"]), cu(c["proj"]), cu(c["dv"])

        def run(A):
            f, p, d = A.put(fea, "in", "src_fea"), A.put(proj, "in", "proj"), A.put(dv, "in", "depth_values")
            out = A.carve((Cn, D, h, w), torch.float32, "out", "warped")
            with A.intercept(L):
                rt = L.relative_proj(p)
            L.check(L.load().mvs_homo_warp(f.data_ptr(), rt.data_ptr(), d.data_ptr(), out.data_ptr(), Cn, D, h, w,
                                           L._stream(out.device)))
            return out
        return self.check(run), [Cn, D, h, w]

    # ---------------------------------------------------------------- softargmin, depth regression
    def softargmin(self, shape):
        L = self.lib
        D, h, w = shape
        rng = np.random.default_rng(D * 7 + h)
        cost = cu(3.0 * rng.standard_normal((D, h, w)))
        dv = cu(self.syn.depth_values(D))
        prob = torch.softmax(cost, 0).contiguous()
        gd = cu(rng.standard_normal((h, w)))

        def run(A):
            c, d, p, g = A.put(cost, "in", "cost"), A.put(dv, "in", "depth_values"), A.put(prob, "in", "prob"), A.put(gd, "in", "grad_depth")
            reg = A.carve((h, w), torch.float32, "out", "depth_regression")
            with A.intercept(L):
                depth, conf = L.softargmin_conf(c, d)
                gc = L.softargmin_backward(c, d, g)
            L.check(L.load().mvs_depth_regression(p.data_ptr(), d.data_ptr(), reg.data_ptr(), D, h, w, L._stream(reg.device)))
            return depth, conf, gc, reg
        return self.check(run), [D, h, w]

    # ---------------------------------------------------------------- the whole depth path
    def depth_infer(self, storage):
        L = self.lib
        t = DEPTH_INFER
        N, h, w, D = t["N"], t["h"], t["w"], t["D"]
        code = L.dtype_code(storage)
        V = N + 2
        bank = self.syn.random_features(V, 32, h, w, seed=11)
        ids = np.array([4, 0, 5, 2][:N])
        feats, bank_d = cu(bank[ids]), cu(bank)
        proj, dv = cu(self.syn.cameras(N, h, w, **t["kw"])), cu(self.syn.depth_values(D))
        nbytes = L.query_workspace(N, 32, D, h, w, code)

        def run(A):
            f, b, p, d, blob = (A.put(feats, "in", "feats"), A.put(bank_d, "in", "bank"), A.put(proj, "in", "proj"),
                                A.put(dv, "in", "depth_values"), A.put(self.blob, "in", "blob"))
            outs = [A.carve((h, w), torch.float32, "out", n) for n in ("depth", "conf", "depth_views", "conf_views")]
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            L.depth_infer(f, p, d, blob, ws, outs[0], outs[1], dtype=code)
            ws2 = A.carve((nbytes,), torch.uint8, "scratch", "workspace_views")
            L.depth_infer_views(b, ids, p, d, blob, ws2, outs[2], outs[3], dtype=code)
            return outs
        gb = self.check(run)
        outs = run(G.Plain(DEV))
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
        return gb, [N, 32, D, h, w]

    # ---------------------------------------------------------------- FeatureNet
    def images(self, shape, fmt, seed=5):
        N, H, Wd = shape
        rng = np.random.default_rng(seed)
        if fmt == "f32_chw":
            return cu(rng.random((N, 3, H, Wd), dtype=np.float32))
        u8 = rng.integers(0, 256, (N, 3, H, Wd), dtype=np.uint8)
        return torch.from_numpy(u8 if fmt == "u8_chw" else np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(DEV)

    def feature_net(self, shape, fmt):
        L = self.lib
        imgs = self.images(shape, fmt)

        def run(A):
            i, fb = A.put(imgs, "in", "imgs"), A.put(self.fblob, "in", "feature_blob")
            with A.intercept(L):
                return L.feature_net(i, fb)
        return self.check(run), list(shape)

    def feature_net_plain(self, shape):
        L = self.lib
        N, H, Wd = shape
        imgs = self.images(shape, "f32_chw")
        h4, w4 = ((H - 1) // 2) // 2 + 1, ((Wd - 1) // 2) // 2 + 1
        nbytes = L.query_feature_workspace(N, H, Wd)

        def run(A):
            i, fb = A.put(imgs, "in", "imgs"), A.put(self.fblob, "in", "feature_blob")
            out = A.carve((N, 32, h4, w4), torch.float32, "out", "feats")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            L.check(L.load().mvs_feature_net(i.data_ptr(), fb.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, N, H, Wd,
                                             L._stream(out.device)))
            return out
        return self.check(run), list(shape)

    def feature_slot(self, shape):
        """What MVSNet.extract_features does per chunk: FeatureNet's output goes into one slot of a bank.  The bank is
        one carved [3, 32, h4, w4] tensor with known contents (`inout`: its neighbouring slots are data); the middle
        slot is filled with the poison byte by hand and written by the call, the slots before and after it must keep
        their bytes, and the guards stand around the bank.  At a 32-aligned size MVSNet.extract_features(chunk=1) runs
        as well, its own bank and cached workspace carved through the proxy."""
        L = self.lib
        N, H, Wd = shape
        imgs = self.images(shape, "u8_hwc")[:1]
        h4, w4 = ((H - 1) // 2) // 2 + 1, ((Wd - 1) // 2) // 2 + 1
        bank0 = cu(np.random.default_rng(3).standard_normal((3, 32, h4, w4)))
        nbytes = L.query_feature_workspace(1, H, Wd)
        aligned = H % 32 == 0 and Wd % 32 == 0
        if aligned:
            from scene_3dreconstruction_mvsnet_amd import mvsnet as M
            if self._model is None:
                m = M.MVSNet(refine=False)
                m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in self.weights.items()})
                self._model = m.to(DEV).eval()
            stack = self.images((3, H, Wd), "u8_hwc", seed=6)

        def run(A):
            i, fb = A.put(imgs, "in", "imgs"), A.put(self.fblob, "in", "feature_blob")
            bank = A.put(bank0, "inout", "bank")
            bank[1].view(torch.uint8).fill_(getattr(A, "poison", 0))
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            outs = [L.feature_net(i, fb, ws, out=bank[1:2])]
            torch.cuda.synchronize()
            for k in (0, 2):
                assert torch.equal(G.raw_bytes(bank[k]), G.raw_bytes(bank0[k])), f"bank slot {k}, beside the written one, changed"
            if aligned:
                st = A.put(stack, "in", "stack")
                self._model._workspace_cache.clear()      # a workspace of the previous run's arena must not be reused
                with A.intercept(M):
                    outs.append(self._model.extract_features(st, chunk=1))
                self._model._workspace_cache.clear()
            return outs
        return self.check(run), [1, H, Wd]

    def feature_layers(self, shape):
        L = self.lib
        N, H, Wd = shape
        imgs = self.images(shape, "f32_chw")
        u8 = self.images(shape, "u8_hwc")
        rng = np.random.default_rng(9)
        xs = {}
        hh, ww = H, Wd
        for l, (ci, co, k, s) in enumerate(L.FEATURE_LAYERS):
            if l:
                xs[l] = cu(rng.standard_normal((ci // 8, N, hh, ww, 8)))
            hh, ww = (hh - 1) // s + 1, (ww - 1) // s + 1

        def run(A):
            fb = A.put(self.fblob, "in", "feature_blob")
            i, u = A.put(imgs, "in", "imgs"), A.put(u8, "in", "imgs_u8")
            ins = {l: A.put(x, "in", f"x{l}") for l, x in xs.items()}
            with A.intercept(L):
                outs = [L.feature_layer(0, i, fb)] + [L.feature_layer(l, ins[l], fb) for l in sorted(ins)]
                outs += [L.feature_conv01(i, fb), L.feature_conv01(u, fb)]
            return outs
        return self.check(run), list(shape)

    def forward_problem(self, fmt, seed=0):
        N, H, Wd, D = 3, 64, 96, 8
        imgs = self.images((N, H, Wd), fmt, seed=seed + 20)
        return imgs, cu(self.syn.cameras(N, H // 4, Wd // 4)), cu(self.syn.depth_values(D)), (N, H, Wd, D)

    def forward_images(self, storage, fmt):
        L = self.lib
        imgs, proj, dv, (N, H, Wd, D) = self.forward_problem(fmt)
        code = L.dtype_code(storage)
        nbytes = L.query_forward_workspace(N, H, Wd, D, code)

        def run(A):
            i, p, d = A.put(imgs, "in", "imgs"), A.put(proj, "in", "proj"), A.put(dv, "in", "depth_values")
            fb, blob = A.put(self.fblob, "in", "feature_blob"), A.put(self.blob, "in", "blob")
            depth, conf = A.carve((H // 4, Wd // 4), torch.float32, "out", "depth"), A.carve((H // 4, Wd // 4), torch.float32, "out", "conf")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            L.forward_images(i, p, d, fb, blob, ws, depth, conf, dtype=code)
            return depth, conf
        return self.check(run), [N, H, Wd, D]

    def forward_images_plain(self):
        L = self.lib
        imgs, proj, dv, (N, H, Wd, D) = self.forward_problem("f32_chw")
        nbytes = L.query_forward_workspace(N, H, Wd, D, L.MVS_F32)

        def run(A):
            i, p, d = A.put(imgs, "in", "imgs"), A.put(proj, "in", "proj"), A.put(dv, "in", "depth_values")
            fb, blob = A.put(self.fblob, "in", "feature_blob"), A.put(self.blob, "in", "blob")
            depth, conf = A.carve((H // 4, Wd // 4), torch.float32, "out", "depth"), A.carve((H // 4, Wd // 4), torch.float32, "out", "conf")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            L.check(L.load().mvs_forward_images(i.data_ptr(), p.data_ptr(), d.data_ptr(), fb.data_ptr(), blob.data_ptr(),
                                                depth.data_ptr(), conf.data_ptr(), ws.data_ptr(), nbytes, N, H, Wd, D,
                                                L.MVS_F32, L._stream(depth.device)))
            return depth, conf
        return self.check(run), [N, H, Wd, D]

    def module(self):
        """MVSNet.forward on problem A, on B (same workspace key, other data), on A again, every cached workspace
        filled with 0xFF before each call (a warm-up forward of B creates it before the first): both A results are the
        same bits, and a fresh module's."""
        from scene_3dreconstruction_mvsnet_amd import MVSNet
        state = {k: torch.from_numpy(np.asarray(v)) for k, v in self.weights.items()}

        def model():
            m = MVSNet(refine=False)
            m.load_state_dict(state)
            return m.to(DEV).eval()

        def problem(seed):
            imgs, proj, dv, dims = self.forward_problem("f32_chw", seed=seed)
            if seed:
                dv = dv + 7.5
            return imgs[None], proj[None], dv[None]

        def call(m, args):
            if not m._workspace_cache:       # create the workspace first, so that no result is computed over fresh memory
                m(*B_)
                torch.cuda.synchronize()
            assert m._workspace_cache
            for ws in m._workspace_cache.values():
                ws.fill_(0xFF)
            out = m(*args)
            torch.cuda.synchronize()
            return G.raw_bytes(out["depth"]), G.raw_bytes(out["photometric_confidence"])
        A_, B_ = problem(0), problem(1)
        m = model()
        a1 = call(m, A_)
        assert len(m._workspace_cache) == 1
        b = call(m, B_)
        assert len(m._workspace_cache) == 1, "B must reuse A's workspace"
        a2 = call(m, A_)
        fresh = call(model(), A_)
        assert not torch.equal(a1[0], b[0]), "problem B must differ from A"
        for name, x, y in (("second A", a1, a2), ("a fresh module", a1, fresh)):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), f"A differs from {name}'s result"
        assert not bool(torch.isnan(a1[0].view(torch.float32)).any())
        return 0, list(A_[0].shape)

    # ---------------------------------------------------------------- filter, metrics
    def filter(self):
        import filter_ref as R
        L = self.lib
        fx = self.load_fixture("filter")
        sc = R.fixture_scene(fx, R.FIXTURE_SCENES[0])
        ref_idx, src_idx = R.abi_rows(sc)
        rm, pm = L.filter_compose(sc["Ks"], sc["Es"], ref_idx, src_idx)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
        ins = [t(sc["depths"]), t(sc["confs"]), t(rm), t(pm), t(ref_idx), t(src_idx)]
        th = sc["th"]

        def run(A):
            a = [A.put(x, "in", n) for x, n in zip(ins, ("depth", "conf", "ref_mats", "pair_mats", "ref_idx", "src_idx"))]
            with A.intercept(L):
                return L.filter_depth(*a, th["photomask"], th["geomask"], th["condmask_pixel"], th["condmask_depth"])
        return self.check(run), list(sc["depths"].shape)

    def metrics(self, shape, errmap):
        L = self.lib
        B, h, w = shape
        rng = np.random.default_rng(h * 1000 + w + B)
        gt = rng.uniform(425.0, 470.0, size=(B, h, w)).astype(np.float32)
        est = (gt + rng.normal(0.0, 4.0, size=(B, h, w))).astype(np.float32)
        mask = rng.choice(np.array([0.0, 0.5, 0.6, 1.0], np.float32), size=(B, h, w))
        # as test_gpu_depth_metrics._random: invalid pixels hold gt = 0 or inf, so the error map's inf * 0 = NaN path runs
        gt[mask <= 0.5] = np.where(rng.random(size=gt[mask <= 0.5].shape) < 0.1, np.inf, 0.0)
        ins = [cu(est), cu(gt), cu(mask)]
        K = 3 + 4
        nbytes = L.query_metrics_workspace(B, h, w)

        def run(A):
            e, g, m = (A.put(x, "in", n) for x, n in zip(ins, ("depth_est", "depth_gt", "mask")))
            # rows 1 .. B of a running accumulator (inout: never poisoned); its other rows must keep their values
            acc = A.put(torch.full((B + 2, K), -3.25 - getattr(A, "poison", 0), dtype=torch.float64, device=DEV), "inout", "sums")
            ws = A.carve((nbytes,), torch.uint8, "scratch", "workspace")
            with A.intercept(L):
                sums, err = L.depth_metrics(e, g, m, sums_out=acc[1:B + 1], errmap=errmap, workspace=ws)
            assert bool((acc[0] == acc[B + 1]).all()) and float(acc[0, 0]) == -3.25 - getattr(A, "poison", 0), \
                "rows of the accumulator outside sums_out changed"
            return sums, err
        return self.check(run), [B, h, w]

    # ---------------------------------------------------------------- training
    def train_conv(self, name):
        import test_gpu_train_conv as T
        L = self.lib
        _, cin, cout, s, shape = {c[0]: c for c in T.CASES + T.TINY}[name]
        gen = torch.Generator().manual_seed(61)
        x = T.cl(T.heavy((cin,) + shape, gen))
        gy = T.cl(T.heavy((cout,) + T.out_shape(shape, s), gen))
        wt = torch.randn((cout, cin, 3, 3, 3), generator=gen).to(DEV)
        bias = torch.randn((cout,), generator=gen).to(DEV)

        def run(A):
            xi, gi, wi, bi = A.put(x, "in", "x"), A.put(gy, "in", "gy"), A.put(wt, "in", "weight"), A.put(bias, "in", "bias")
            with A.intercept(L):
                outs = [L.conv3d_train_forward(xi, wi, bi, s), L.conv3d_train_forward(xi, wi, None, s),
                        L.conv3d_train_backward_data(gi, wi, s), L.conv3d_train_backward_weight(xi, gi, s)]
                outs += list(L.conv3d_train_backward_weight(xi, gi, s, with_bias=True))
            return outs
        return self.check(run), [cin, cout, s] + list(shape)

    def bn3d(self, C, M, relu, skip):
        L = self.lib
        rng = np.random.default_rng(C + M)
        y, go, sk = (cu(rng.standard_normal((M, C))) for _ in range(3))
        gamma, beta = cu(rng.standard_normal(C)), cu(rng.standard_normal(C))
        rm0, rv0 = cu(rng.standard_normal(C)), cu(rng.random(C) + 0.5)

        def run(A):
            yi, gi, ga, be = A.put(y, "in", "y"), A.put(go, "in", "grad_out"), A.put(gamma, "in", "gamma"), A.put(beta, "in", "beta")
            si = A.put(sk, "in", "skip") if skip else None
            rm, rv = A.put(rm0, "inout", "running_mean"), A.put(rv0, "inout", "running_var")
            with A.intercept(L):
                out, mean, invstd = L.bn3d_train_forward(yi, ga, be, si, rm, rv, relu=relu)
                out2 = L.bn3d_train_forward(yi, ga, be, si, relu=relu)[0]
                back = L.bn3d_train_backward(yi, gi, ga, be, mean, invstd, relu=relu)
            return (out, mean, invstd, out2, rm, rv) + tuple(back)
        return self.check(run), [M, C]

    def relayout(self, C, dims):
        L = self.lib
        rng = np.random.default_rng(C)
        c8 = cu(rng.standard_normal((C // 8,) + tuple(dims) + (8,)))
        cl = cu(rng.standard_normal(tuple(dims) + (C,)))

        def run(A):
            a, b = A.put(c8, "in", "c8_planar"), A.put(cl, "in", "channels_last")
            with A.intercept(L):
                return (L.volume_relayout(a, L.RELAYOUT_C8_TO_CHANNELS_LAST),
                        L.volume_relayout(b, L.RELAYOUT_CHANNELS_LAST_TO_PLANAR))
        return self.check(run), [C] + list(dims)

    def warp_backward(self):
        """Float atomics: not bit-reproducible.  Each of the three poisoned runs is held to the per-element fp64 bound
        of tests/cost_volume_grad_ref.py instead and must hold no NaN (0xFF would be NaN, 0x4B about 1e7 x the
        bound's scale); grad_feats is `out`: the launcher zeroes it itself."""
        import cost_volume_grad_ref as CG
        L = self.lib
        c = W.CASES[GRAD_RIG][0]()
        N, Cn, h, w = c["feats"].shape
        D = len(c["dv"])
        feats, proj, dv = cu(c["feats"]), cu(c["proj"]), cu(c["dv"])
        rt_dev = L.relative_proj(proj)
        adj = CG.Adjoint(c["feats"], rt_dev.cpu().numpy()[:N - 1], c["dv"])
        g = CG.dense_g(D, h, w, 11)
        res = adj.grad(g)
        gd = cu(g)
        guard_bytes = 0
        for p in G.POISONS:
            A = self.arena
            A.reset(poison=p)
            f, r, d, gi = A.put(feats, "in", "feats"), A.put(rt_dev, "in", "rt"), A.put(dv, "in", "depth_values"), A.put(gd, "in", "grad_var")
            with A.intercept(L):
                out = L.warp_variance_backward(f, r, d, gi)
            findings = A.check()
            assert not findings, f"poison 0x{p:02X}: " + "; ".join(findings)
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), f"poison 0x{p:02X}: NaN in grad_feats"
            ratio, problems = CG.compare(got, res, adj)
            assert not problems, f"poison 0x{p:02X}: " + "; ".join(problems)
            guard_bytes = A.guard_bytes
        return guard_bytes, [N, Cn, D, h, w]


def main():
    cases_path, out_path = sys.argv[1:3]
    with open(cases_path) as f:
        cases = json.load(f)
    env = {k: v for k, v in os.environ.items() if k.startswith("MVS_")}
    for case in cases:
        for k, v in case["env"].items():
            assert os.environ.get(k) == v, f"case {case['id']} needs {k}={v} in the environment"
    runner = Runner()
    results, status = {}, 0
    for case in cases:
        hip_error = False
        try:
            guard_bytes, shape = getattr(runner, case["kind"])(**case["args"])
            results[case["id"]] = {"ok": True, "msg": "", "shape": shape, "guard_bytes": guard_bytes, "exempt": 0.0}
        except Exception as e:      # one broken case does not take the others' verdicts with it
            msg = ("".join(traceback.format_exception_only(type(e), e)) if isinstance(e, AssertionError)
                   else traceback.format_exc())[-4000:]
            results[case["id"]] = {"ok": False, "msg": msg, "shape": None, "guard_bytes": 0, "exempt": 0.0}
            # fatal: the library's MVS_ERR_HIP, and every other RuntimeError (what torch raises at a synchronise or a
            # copy after a GPU fault, however it is worded); the library's argument refusals (codes 1, 2, 3, 5) enqueue
            # nothing and are an ordinary failure of the case
            refusal = isinstance(e, runner.lib.MvsError) and e.code != 4
            hip_error = isinstance(e, RuntimeError) and not refusal
        r = results[case["id"]]
        print(f"[guarded] {'+'.join(case['entries'])} env={env} shape={r['shape']} guard_bytes={r['guard_bytes']} "
              f"exempt={r['exempt']:.3f} {'ok' if r['ok'] else 'FAIL ' + r['msg'].strip()[-300:]}", flush=True)
        with open(out_path, "w") as f:
            json.dump(results, f)
        if hip_error:      # nothing more on the GPU after a HIP error
            status = 2
            break
    return status


if __name__ == "__main__":
    sys.exit(main())
