"""The shape domain include/mvs_abi.h states for every depth-path entry point, held to the library from the refused
side with made-up pointers (256-byte aligned addresses that are never dereferenced: every refusal is decided on the host
before anything is enqueued).  The whole sweep is run by tests/refusals.py in a child process that sees no device, so a
call the library fails to refuse cannot reach hardware: it comes back as MVS_ERR_HIP (4) and is reported as "reached a
HIP call".  The accepted side of a bound is asserted only through the mvs_query_* functions, which do no device work.  A
second child repeats the sweep under MVS_FORCE_DIRECT=1 (the environment is read once per process).

SPECS is keyed by entry point.  The completeness test reads the prototypes of every header of include/ and the tables
of every host module: an entry point with a `stream` parameter without cases in a no-device child, a pointer parameter
with neither a NULL case nor an `optional` entry, or, in mvs_abi.h, an int parameter without a below-range case or a
device pointer without an alignment case fails this file."""
import ctypes
import functools
import glob
import importlib
import json
import os
import re
import sys
import threading

import numpy as np
import pytest

import refusals
from refusals import BAD_DTYPE, BAD_SHAPE, HERE, NULL, OK, WORKSPACE
from scene_3dreconstruction_mvsnet_amd import _lib

# ---- Python restatements of the library's byte counts (csrc/mvs_internal.h) ---------------------------------------
_LEVEL_OUT = (0, 1, 1, 2, 2, 3, 3, 2, 1, 0)
_COUT = (8, 16, 16, 32, 32, 64, 64, 32, 16, 8)


def _up(n):
    return (n + 255) // 256 * 256


def feats_region_bytes(N, h, w):
    return _up(N * 32 * h * w * 4)


def workspace_bytes(N, D, h, w, dtype=0):
    es = 4 if dtype == 0 else 2
    n = feats_region_bytes(N, h, w) + _up(max(N - 1, 1) * 12 * 4) + _up(D * h * w * 32 * es)
    for lv, co in zip(_LEVEL_OUT, _COUT):
        n += _up((D >> lv) * (h >> lv) * (w >> lv) * co * es)
    return n + _up(D * h * w * 4)


def feature_workspace_bytes(N, H, W):
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h4, w4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    return 2 * max(_up(N * H * W * 8 * 4), _up(N * H2 * W2 * 16 * 4)) + _up(N * h4 * w4 * 32 * 4)


def forward_workspace_bytes(N, H, W, D, dtype=0):
    return workspace_bytes(N, D, H // 4, W // 4, dtype) + feature_workspace_bytes(N, H, W)


_COSTREG_CH = ((32, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 32), (32, 16), (16, 8), (8, 1))
_FEATURE_CH = ((3, 8, 3), (8, 8, 3), (8, 16, 5), (16, 16, 3), (16, 16, 3), (16, 32, 5), (32, 32, 3), (32, 32, 3))

# ---- the case table -------------------------------------------------------------------------------------------------
# good:     in-range value of every int argument (the base every case overrides one thing of)
# optional: pointer -> an out-of-range override that must give BAD_SHAPE with that pointer NULL (so NULL was not the
#           reason), optionally after `with_` puts the call where the pointer is optional
# below / above: int argument -> out-of-range values (-> `code`, BAD_SHAPE unless stated); an `above` value may be a
#           dict that moves other arguments too (a bound on a product)
# rules:    (override, code) for the rules that tie arguments together
# sizes:    `need` restates the smallest workspace of the call: one byte less and a pointer at +16 give WORKSPACE
# host:     arguments that are real host arrays, built in the child (tests/refusals.py)
VOL = dict(N=3, C=32, D=16, h=16, w=24, dtype=0)
VOL_BELOW = dict(N=[0, -8], C=[0, -8], D=[0, -8], h=[0, -8], w=[0, -8])
G30 = 1 << 30         # cubed it is 0 mod 2^64: a product formed in size_t would pass every "< 2^31" test
VOL_ABOVE = dict(N=[65], C=[33, 64], D=[dict(D=416, h=512, w=640), dict(D=G30, h=G30, w=G30)],
                 h=[dict(D=8, h=1 << 21, w=8)], w=[dict(D=8, h=8, w=1 << 21)])
VOL_RULES = [(dict(D=12), 1), (dict(h=20), 1), (dict(w=28), 1), (dict(C=16), 1)]
DTYPES = dict(dtype=[3, -1])
IMG = dict(N=2, H=64, W=96)
IMG_BELOW = dict(N=[0, -8], H=[0, -8, 3], W=[0, -8, 3])
IMG_ABOVE = dict(N=[65536], H=[dict(N=1, H=1 << 26, W=4), dict(N=2, H=G30, W=G30)], W=[dict(N=1, H=4, W=1 << 26)])
FWD = dict(N=3, H=64, W=96, D=16, dtype=0)
FWD_BELOW = dict(N=[0, -8], H=[0, -8], W=[0, -8], D=[0, -8])
FWD_ABOVE = dict(N=[65], H=[dict(D=8, H=1 << 23, W=32)], W=[dict(D=8, H=32, W=1 << 23)],
                 D=[dict(D=416, H=2048, W=2560)])
FWD_RULES = [(dict(H=68), 1), (dict(W=100), 1), (dict(H=80), 1), (dict(W=112), 1), (dict(D=12), 1)]   # 4 | H but not 32
BIG = 4096
PIX_MAX = (1 << 31) - 256



@functools.lru_cache(None)
def _pack_arrays(kind):
    """conv weights, BatchNorm vectors, bias and blob of a pack call: real host arrays, made once in the child"""
    if kind == "costreg":
        convs = [np.ones(27 * ci * co, np.float32) for ci, co in _COSTREG_CH]
        bns = [np.ones(_COSTREG_CH[k // 4][1], np.float32) for k in range(40)]
        return convs, bns, np.ones(1, np.float32), np.zeros(_lib.query_weights_blob(), np.uint8)
    convs = [np.ones(k * k * ci * co, np.float32) for ci, co, k in _FEATURE_CH]
    bns = [np.ones(_FEATURE_CH[k // 4][1], np.float32) for k in range(28)]
    return convs, bns, np.ones(32, np.float32), np.zeros(_lib.query_feature_blob(), np.uint8)


def _pack(kind):
    """The spec entries of a pack function: `null_conv` / `null_bn` name the array whose pointer is NULL."""
    def pointers(which, null):
        def build(a, ov):
            ptrs = [x.ctypes.data for x in _pack_arrays(kind)[which]]
            if null in ov:
                ptrs[ov[null]] = None
            return (ctypes.c_void_p * len(ptrs))(*ptrs)
        return build
    bias = "prob_bias" if kind == "costreg" else "feature_bias"
    return dict(good=dict(eps=1e-5, blob_bytes="blob"), pack=kind, extra=("null_conv", "null_bn"),
                sizes=dict(blob=lambda a: _pack_arrays(kind)[3].size),
                host={"conv_weights": pointers(0, "null_conv"), "bn_params": pointers(1, "null_bn"),
                      bias: lambda a, ov: ctypes.c_void_p(_pack_arrays(kind)[2].ctypes.data),
                      "blob_out": lambda a, ov: ctypes.c_void_p(_pack_arrays(kind)[3].ctypes.data)})


VIEWS = dict(view_idx=lambda a, ov: (ctypes.c_int * 64)(*a["view_idx"]))

SPECS = {
    "mvs_query_workspace": dict(good=VOL, below=VOL_BELOW, above=VOL_ABOVE, rules=VOL_RULES, dtypes=DTYPES),
    "mvs_query_weights_blob": dict(good={}),
    "mvs_pack_weights": _pack("costreg"),
    "mvs_relative_proj": dict(good=dict(N=3), below=dict(N=[0, -8]), above=dict(N=[65])),
    "mvs_warp_variance": dict(good=VOL, below=VOL_BELOW, above=VOL_ABOVE, rules=VOL_RULES + [(dict(rt=None), NULL)],
                              dtypes=DTYPES,
                              optional=dict(rt=dict(with_=dict(N=1), D=0)),
                              sizes=dict(need=lambda a: feats_region_bytes(a["N"], a["h"], a["w"]))),
    "mvs_costreg_forward": dict(good=dict(D=16, h=16, w=24, dtype=0),
                                below={k: VOL_BELOW[k] for k in "Dhw"}, above={k: VOL_ABOVE[k] for k in "Dhw"},
                                rules=VOL_RULES[:3], dtypes=DTYPES,
                                sizes=dict(need=lambda a: workspace_bytes(1, a["D"], a["h"], a["w"], a["dtype"]))),
    "mvs_conv_layer": dict(good=dict(layer=0, Di=8, Hi=8, Wi=8, dtype=0),
                           below=dict(layer=[-1], Di=[0, -8], Hi=[0, -8], Wi=[0, -8]),
                           above=dict(layer=[11], Di=[dict(Di=1 << 28, Hi=1, Wi=1)], Hi=[dict(Di=1, Hi=1 << 28, Wi=1)],
                                      Wi=[dict(Di=1, Hi=1, Wi=1 << 28), dict(Di=1 << 10, Hi=1 << 9, Wi=1 << 9),
                                          dict(Di=G30, Hi=G30, Wi=G30)]),
                           rules=[(dict(layer=l, **{k: 7}), 1) for l in (1, 3, 5) for k in ("Di", "Hi", "Wi")] +
                                 [(dict(layer=l, x=None), NULL) for l in range(11)] +
                                 [(dict(layer=l, skip=None), NULL) for l in (7, 8, 9)] +
                                 # 4096^3: beyond the int offsets of every kernel form, whichever one the layer and the environment select
                                 [(dict(layer=l, Di=BIG, Hi=BIG, Wi=BIG), 1) for l in range(11)] +
                                 [(dict(layer=l, Di=BIG, Hi=BIG, Wi=BIG, dtype=1), 1) for l in (7, 10)] +
                                 # layer 10: (5 Hi + 9) Wi + 33 < 2^28 (prob_lds' int offsets from the halo origin); both
                                 # shapes pass Di*Hi*Wi < 2^28; 19173960 is the first refused Wi at Hi = 1
                                 [(dict(layer=10, Di=4, Hi=8192, Wi=8191), 1), (dict(layer=10, Di=1, Hi=1, Wi=19173960), 1),
                                  (dict(layer=10, Di=4, Hi=8192, Wi=8191, dtype=2), 1)],
                           dtypes=DTYPES,
                           optional=dict(skip=[dict(with_=dict(layer=l), Di=0) for l in (0, 1, 2, 3, 4, 5, 6, 10)])),
    "mvs_conv11_prob": dict(good=dict(Di=8, Hi=8, Wi=8, dtype=0), below=dict(Di=[0, -8], Hi=[0, -8], Wi=[0, -8]),
                            above=dict(Di=[dict(Di=1 << 25, Hi=1, Wi=1)], Hi=[dict(Di=1, Hi=1 << 25, Wi=1)],
                                       Wi=[dict(Di=1, Hi=1, Wi=1 << 25), dict(Di=BIG, Hi=BIG, Wi=BIG),
                                           dict(Di=G30, Hi=G30, Wi=G30)]),
                            dtypes=DTYPES),
    "mvs_softargmin_conf": dict(good=dict(D=16, h=16, w=24), below=dict(D=[0, -8], h=[0, -8], w=[0, -8]),
                                above=dict(D=[(1 << 24) + 1, 1 << 30], h=[dict(h=PIX_MAX + 1, w=1)],
                                           w=[dict(h=1, w=PIX_MAX + 1)]),
                                rules=[(dict(D=8, h=65536, w=65536), 1), (dict(D=8, h=46341, w=46341), 1)]),
    "mvs_depth_infer": dict(good=VOL, below=VOL_BELOW, above=VOL_ABOVE, rules=VOL_RULES, dtypes=DTYPES,
                            sizes=dict(need=lambda a: workspace_bytes(a["N"], a["D"], a["h"], a["w"], a["dtype"]))),
    "mvs_depth_infer_views": dict(good=dict(VOL, V=5, view_idx=lambda a: list(range(max(a["N"], 0) % 64))), host=VIEWS,
                                  below=dict(VOL_BELOW, V=[0, -8]), above=VOL_ABOVE,
                                  rules=VOL_RULES + [(dict(view_idx=[0, -1, 2]), 1), (dict(view_idx=[0, 1, 5]), 1),
                                                     (dict(view_idx=[5, 1, 2]), 1)],
                                  dtypes=DTYPES,
                                  sizes=dict(need=lambda a: workspace_bytes(a["N"], a["D"], a["h"], a["w"], a["dtype"]))),
    "mvs_homo_warp": dict(good=dict(C=32, D=16, h=16, w=24),
                          below=dict(C=[0, -8], D=[0, -8], h=[0, -8, 1], w=[0, -8, 1]),
                          above=dict(C=[dict(C=(1 << 23) + 1, D=1 << 18, h=1 << 10, w=1 << 10)],
                                     D=[dict(C=1, D=1 << 19, h=1 << 10, w=1 << 10)],
                                     h=[dict(C=1, D=1, h=1 << 30, w=2)], w=[dict(C=1, D=1, h=2, w=1 << 30)]),
                          rules=[(dict(C=32, D=1 << 20, h=1 << 15, w=1 << 15), 1)]),
    "mvs_depth_regression": dict(good=dict(D=16, h=16, w=24), below=dict(D=[0, -8], h=[0, -8], w=[0, -8]),
                                 above=dict(h=[dict(h=PIX_MAX + 1, w=1)], w=[dict(h=1, w=PIX_MAX + 1)]),
                                 rules=[(dict(D=8, h=65536, w=65536), 1)]),
    "mvs_query_feature_blob": dict(good={}),
    "mvs_pack_feature_weights": _pack("feature"),
    "mvs_query_feature_workspace": dict(good=IMG, below=IMG_BELOW, above=IMG_ABOVE),
    "mvs_feature_layer": dict(good=dict(layer=0, N=2, Hi=64, Wi=96),
                              below=dict(layer=[-1], N=[0, -8], Hi=[0, -8, 3], Wi=[0, -8, 3]),
                              above=dict(layer=[8], N=[65536], Hi=[dict(N=1, Hi=1 << 26, Wi=4), dict(N=2, Hi=G30, Wi=G30)],
                                         Wi=[dict(N=1, Hi=4, Wi=1 << 26)])),
    "mvs_feature_conv01_fmt": dict(good=dict(IMG, image_format=0), below=IMG_BELOW, above=IMG_ABOVE,
                                   dtypes=dict(image_format=[3, -1])),
    "mvs_feature_net": dict(good=IMG, below=IMG_BELOW, above=IMG_ABOVE,
                            sizes=dict(need=lambda a: feature_workspace_bytes(a["N"], a["H"], a["W"]))),
    "mvs_feature_net_fmt": dict(good=dict(IMG, image_format=2), below=IMG_BELOW, above=IMG_ABOVE,
                                dtypes=dict(image_format=[3, -1]),
                                sizes=dict(need=lambda a: feature_workspace_bytes(a["N"], a["H"], a["W"]))),
    "mvs_query_forward_workspace": dict(good=FWD, below=FWD_BELOW, above=FWD_ABOVE, rules=FWD_RULES, dtypes=DTYPES),
    "mvs_forward_images": dict(good=FWD, below=FWD_BELOW, above=FWD_ABOVE, rules=FWD_RULES, dtypes=DTYPES,
                               sizes=dict(need=lambda a: forward_workspace_bytes(a["N"], a["H"], a["W"], a["D"], a["dtype"]))),
    "mvs_forward_images_fmt": dict(good=dict(FWD, image_format=1), below=FWD_BELOW, above=FWD_ABOVE, rules=FWD_RULES,
                                   dtypes=dict(DTYPES, image_format=[3, -1]),
                                   sizes=dict(need=lambda a: forward_workspace_bytes(a["N"], a["H"], a["W"], a["D"], a["dtype"]))),
    "mvs_warp_variance_backward": dict(good=dict(N=3, C=32, D=16, h=16, w=24),
                                       below=VOL_BELOW, above=VOL_ABOVE, rules=VOL_RULES + [(dict(rt=None), NULL)],
                                       optional=dict(rt=dict(with_=dict(N=1), D=0))),
    # also in tests/test_training_host.py, swept here for the one row of the oversized table it owns
    "mvs_softargmin_backward": dict(good=dict(D=16, h=16, w=24), below=dict(D=[0, -8], h=[0, -8], w=[0, -8]),
                                    above=dict(D=[(1 << 24) + 1], h=[dict(h=PIX_MAX + 1, w=1)],
                                               w=[dict(h=1, w=PIX_MAX + 1)]),
                                    rules=[(dict(D=1 << 30, h=1 << 15, w=1 << 15), 1)]),
}

# The alignment rule of include/mvs_abi.h: entry point -> (data pointers, blobs).  A data pointer at +4 of its good
# (256-byte aligned, fake) address gives BAD_SHAPE, a blob at +4 WORKSPACE, with every other argument good.  The workspace
# has its own "+16" case above (it is held to 256 bytes); HOST arrays (view_idx) are not device addresses.
ALIGN = {
    "mvs_relative_proj": (("proj", "rt_out"), ()),
    "mvs_warp_variance": (("rt", "depth_values", "var_out"), ()),
    "mvs_costreg_forward": (("var", "cost_out"), ("weights_blob",)),
    "mvs_conv_layer": (("x", "skip", "y"), ("weights_blob",)),
    "mvs_conv11_prob": (("x", "skip", "cost_out"), ("weights_blob",)),
    "mvs_depth_infer": (("proj", "depth_values"), ("weights_blob",)),
    "mvs_depth_infer_views": (("proj", "depth_values"), ("weights_blob",)),
    "mvs_homo_warp": (("rt",), ()),
    "mvs_feature_layer": (("x", "y"), ("feature_blob",)),
    "mvs_feature_conv01_fmt": (("imgs", "y"), ("feature_blob",)),
    "mvs_feature_net": (("imgs", "feats_out"), ("feature_blob",)),
    "mvs_feature_net_fmt": (("imgs", "feats_out"), ("feature_blob",)),
    "mvs_forward_images": (("imgs", "proj", "depth_values"), ("feature_blob", "weights_blob")),
    "mvs_forward_images_fmt": (("imgs", "proj", "depth_values"), ("feature_blob", "weights_blob")),
    "mvs_warp_variance_backward": (("feats", "rt", "depth_values", "grad_var", "grad_feats"), ()),
}
# the pointers the header states are per element, or asks nothing of: no refusal to sweep (the per-element ones run one
# element into a larger allocation in tests/test_gpu_wrapper_contract.py)
NOT_HELD = {
    "mvs_warp_variance": ("feats",),
    "mvs_depth_infer": ("feats", "depth_out", "conf_out"),
    "mvs_depth_infer_views": ("feats", "depth_out", "conf_out"),
    "mvs_homo_warp": ("src_fea", "depth_values", "out"),
    "mvs_forward_images": ("depth_out", "conf_out"),
    "mvs_forward_images_fmt": ("depth_out", "conf_out"),
    "mvs_softargmin_conf": ("cost", "depth_values", "depth_out", "conf_out"),
    "mvs_softargmin_backward": ("cost", "depth_values", "grad_depth", "grad_cost"),
    "mvs_depth_regression": ("p", "depth_values", "depth_out"),
}

NO_ARGUMENTS = ("mvs_abi_version", "mvs_last_error_string")
# `stream` may be NULL everywhere (the default stream): every case of the sweep passes NULL and still gets its code


def _as_list(v):
    return v if isinstance(v, list) else [v]


def cases_of(name, spec, protos):
    """[(label, overrides, expected code)] of one entry point."""
    out = []
    ptrs = [p for k, p in protos[name] if k == "ptr" and p != "stream"]
    optional = spec.get("optional", {})
    for p in ptrs:
        if p in optional:
            for ov in _as_list(optional[p]):
                ov = dict(ov)
                base = ov.pop("with_", {})
                out.append((f"optional {p}=NULL with {base} and {ov}", dict(base, **ov, **{p: None}), BAD_SHAPE))
        else:
            out.append((f"{p}=NULL", {p: None}, NULL))
    for side in ("below", "above"):
        for arg, vals in spec.get(side, {}).items():
            for v in vals:
                out.append((f"{side} {arg}: {v}", v if isinstance(v, dict) else {arg: v}, BAD_SHAPE))
    for arg, vals in spec.get("dtypes", {}).items():
        for v in vals:
            out.append((f"{arg}={v}", {arg: v}, BAD_DTYPE))
    for ov, code in spec.get("rules", []):
        out.append((f"rule {ov}", ov, code))
    if "need" in spec.get("sizes", {}):
        out.append(("workspace one byte short", {"workspace_bytes": "need-1"}, WORKSPACE))
        out.append(("workspace at +16", {"workspace": "plus16", "workspace_bytes": "need"}, WORKSPACE))
    data, blobs = ALIGN.get(name, ((), ()))
    out += [(f"{p} at +4", {p: "plus4"}, BAD_SHAPE) for p in data]
    out += [(f"blob {p} at +4", {p: "plus4"}, WORKSPACE) for p in blobs]
    if spec.get("pack"):
        nconv, nbn = (11, 40) if spec["pack"] == "costreg" else (8, 28)
        out += [(f"conv_weights[{l}]=NULL", {"null_conv": l}, NULL) for l in range(nconv)]
        out += [(f"bn_params[{k}]=NULL", {"null_bn": k}, NULL) for k in range(nbn)]
        out.append(("blob one byte short", {"blob_bytes": "blob-1"}, WORKSPACE))
    return out


# ---- the child --------------------------------------------------------------------------------------------------------
def REFUSALS(part):
    """The table tests/refusals.py runs.  "main" is every case but the ones whose plain size_t product wraps (two or more
    dims of 2^30), which run in a child of their own ("wrap"): a library that divides by the wrapped zero dies there and
    nowhere else."""
    protos = refusals.prototypes("mvs_abi.h")
    return {name: dict(spec, cases=[(label, ov, want, "") for label, ov, want in cases_of(name, spec, protos)
                                    if (label.count(str(G30)) >= 2) == (part == "wrap")]) for name, spec in SPECS.items()}


def error_string_of_two_threads(lib):
    """the error string is thread-local: a refusal on a second thread leaves this thread's string alone"""
    assert lib.mvs_query_workspace(0, 32, 16, 16, 24, 0, ctypes.byref(ctypes.c_size_t(0))) == BAD_SHAPE
    mine = lib.mvs_last_error_string()
    other = {}

    def refuse_elsewhere():
        other["status"] = lib.mvs_query_feature_workspace(1, 3, 3, ctypes.byref(ctypes.c_size_t(0)))
        other["err"] = (lib.mvs_last_error_string() or b"").decode()
    t = threading.Thread(target=refuse_elsewhere)
    t.start()
    t.join()
    return dict(mine_before=mine.decode(), mine_after=lib.mvs_last_error_string().decode(), other=other)


def refusals_epilogue(lib):
    """what the child prints after its sweep"""
    print("T " + json.dumps(dict(threads=error_string_of_two_threads(lib), force_direct=os.environ.get("MVS_FORCE_DIRECT", ""))),
          flush=True)


# ---- the tests --------------------------------------------------------------------------------------------------------
CHILDREN = {"default": (False, "main"), "MVS_FORCE_DIRECT=1": (True, "main"), "default/wrap": (False, "wrap")}       # (force_direct, part)


def sweep(child):
    force_direct, part = CHILDREN[child]
    env = {"MVS_FORCE_DIRECT": "1"} if force_direct else None
    r, records = refusals.run(__name__, part, env)
    tail = r.records("T ")
    if tail:
        assert tail[-1]["force_direct"] == ("1" if force_direct else "")
    return dict(records=list(records.values()), part=part, env=env, stderr=r.stderr[-2000:],
                threads=tail[-1]["threads"] if tail else None)


@pytest.mark.parametrize("child", list(CHILDREN))
def test_every_out_of_domain_call_is_refused_with_its_status(child):
    res = sweep(child)
    n = refusals.check(sys.modules[__name__], part=res["part"], env=res["env"])
    assert n == len(res["records"]) > (400 if res["part"] == "main" else 10)


@pytest.mark.parametrize("child", list(CHILDREN))
def test_every_refusal_explains_itself(child):
    """non-empty, and set by THIS refusal: the string the call left differs from the one a refusal before it set"""
    silent = [r for r in sweep(child)["records"] if r["got"] not in (OK, None) and (not r["err"].strip() or r["stale"])]
    assert not silent, silent[:5]


def test_a_refusal_on_another_thread_leaves_this_threads_error_string():
    t = sweep("default")["threads"]
    assert t is not None, sweep("default")["stderr"]
    assert t["other"]["status"] == BAD_SHAPE and t["other"]["err"]
    assert t["mine_before"] and t["mine_before"] == t["mine_after"] != t["other"]["err"]


def host_tables():
    """{entry point: [spec with its cases]} over the tables of every host module that has one"""
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "test_*_host.py"))):
        if re.search(r"^(def )?REFUSALS\b", open(path).read(), flags=re.M):
            module = importlib.import_module(os.path.basename(path)[:-3])
            parts = ("main", "wrap") if callable(module.REFUSALS) else (None,)
            for part in parts:
                for name, spec in refusals.table_of(module, part).items():
                    out.setdefault(name, []).append(spec)
    return out


# pointers the library takes as NULL without a refusal of their own and without a word in a header (none so far)
NOT_REFUSED = {}


def test_every_entry_point_pointer_and_integer_of_the_header_has_its_cases():
    protos = refusals.all_prototypes()
    assert set(refusals.prototypes("mvs_abi.h")) == set(_lib.SYMBOLS)
    tables = host_tables()
    missing = []
    # every header: a device entry point has its cases in a no-device child, and every pointer of an entry point with
    # cases has a NULL case or is stated optional
    for name, params in protos.items():
        specs = tables.get(name, [])
        if not specs:
            if any(p == "stream" for _, p in params):
                missing.append(f"{name}: takes a stream and has no cases in a no-device child")
            continue
        nulled = {k for spec in specs for _, ov, code, _ in spec["cases"] if code == NULL for k, v in ov.items() if v is None}
        optional = {p for spec in specs for p in spec.get("optional", ())} | set(NOT_REFUSED.get(name, ()))
        for kind, p in params:
            if kind == "ptr" and p != "stream" and p not in nulled | optional:
                missing.append(f"{name}: pointer {p} has neither a NULL case nor an optional entry")
    assert not set(tables) - set(protos) and not set(NOT_REFUSED) - set(protos)
    # mvs_abi.h: the below-range and the alignment rule
    for name, spec in SPECS.items():
        params = protos[name]
        for kind, p in params:
            if kind == "int":
                below = spec.get("dtypes", {}) if p in ("dtype", "image_format") else spec.get("below", {})
                if p not in below or not any(v < 0 or v == 0 for v in below[p]):
                    missing.append(f"{name}: int {p} has no below-range case")
        if any(kind == "ptr" and p == "stream" for kind, p in params):      # a device entry point: the alignment cases
            data, blobs = ALIGN.get(name, ((), ()))
            free = NOT_HELD.get(name, ())
            for kind, p in params:
                if kind == "ptr" and p not in ("stream", "workspace") + tuple(spec.get("host", ())) and p not in data + blobs + free:
                    missing.append(f"{name}: pointer {p} has neither an alignment case nor a NOT_HELD entry")
            assert not set(data + blobs + free) - {p for _, p in params} and not set(free) & set(data + blobs), name
        stale = [k for k in list(spec.get("below", {})) + list(spec.get("above", {})) + list(spec.get("optional", {}))
                 if k not in [p for _, p in params]]
        assert not stale, (name, stale)
    assert not missing, "\n".join(missing)
    assert not set(SPECS) - set(refusals.prototypes("mvs_abi.h"))
    for name in NO_ARGUMENTS:
        assert not protos[name]


def test_the_abi_version_is_still_2():
    """the library-wide fact the per-header declaration tests used to repeat"""
    assert _lib.load().mvs_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"^#define MVS_ABI_VERSION 2$", refusals.header_text("mvs_abi.h"), flags=re.M)


def _query(fn, *args):
    n = ctypes.c_size_t(0)
    return getattr(_lib.load(), fn)(*args, ctypes.byref(n)), int(n.value)


@pytest.mark.parametrize("args", [(64, 32, 8, 8, 8, 0), (1, 32, 408, 512, 640, 0), (3, 32, 408, 512, 640, 1),
                                  (1, 32, 8, (1 << 21) - 8, 8, 2), (1, 32, 8, 8, (1 << 21) - 8, 0)])
def test_the_largest_admitted_volume_is_admitted(args):
    N, C, D, h, w, dtype = args
    assert D * h * w * 32 < 2 ** 32
    assert _query("mvs_query_workspace", *args) == (0, workspace_bytes(N, D, h, w, dtype))
    for grow in ((0, 0, 8, 0, 0), (0, 0, 0, 8, 0), (0, 0, 0, 0, 8)) if D * h * w > 1 << 20 else ((1, 0, 0, 0, 0),):
        bigger = tuple(a + g for a, g in zip(args, grow + (0,)))
        assert _query("mvs_query_workspace", *bigger)[0] == BAD_SHAPE, bigger


@pytest.mark.parametrize("args", [(65535, 4, 4), (1, (1 << 26) - 1, 4), (1, 4, (1 << 26) - 1), (2, 4, 4), (1, 5, 7)])
def test_the_largest_admitted_images_are_admitted(args):
    N, H, W = args
    assert N * H * W * 8 < 2 ** 31
    assert _query("mvs_query_feature_workspace", *args) == (0, feature_workspace_bytes(*args))


@pytest.mark.parametrize("args", [(64, 32, 32, 8, 0), (1, 2048, 2560, 408, 0), (2, 2048, 2560, 408, 2),
                                  (1, (1 << 23) - 32, 32, 8, 1), (1, 32, (1 << 23) - 32, 8, 0)])
def test_the_largest_admitted_forward_problem_is_admitted(args):
    N, H, W, D, dtype = args
    assert _query("mvs_query_forward_workspace", *args) == (0, forward_workspace_bytes(*args))
    assert _query("mvs_query_forward_workspace", N, H + 32, W, D, dtype)[0] == (BAD_SHAPE if D * H * W > 1 << 22 else OK)
    assert _query("mvs_query_forward_workspace", N, H + 4, W, D, dtype)[0] == BAD_SHAPE     # 4 | H is not enough


def test_the_added_refusals_sit_above_the_largest_shape_of_the_limit_tests():
    """tests/test_gpu_limits.py runs D_MAX x 512 x 640, the largest volume check_dims admits: every stage of it is
    inside the bounds stated with this file (layer 0 sees the largest conv input, the soft-argmin h*w and D)."""
    src = open(os.path.join(HERE, "test_gpu_limits.py")).read()
    h, w = (int(v) for v in re.search(r"^H4, W4 = (\d+), (\d+)", src, re.M).groups())
    D = max(d for d in range(8, 1 << 13, 8) if d * h * w * 32 < 2 ** 32)
    assert (D, h, w) == (408, 512, 640) and "D_MAX = largest_d(abi_fits)" in src
    assert _query("mvs_query_workspace", 3, 32, D, h, w, 0)[0] == OK
    assert _query("mvs_query_forward_workspace", 3, 4 * h, 4 * w, D, 0)[0] == OK
    assert D * h * w < 2 ** 28 and (D // 2) * (h // 2) * (w // 2) * 64 < 2 ** 31       # mvs_conv_layer, mvs_conv11_prob
    assert h * w <= PIX_MAX and D <= 1 << 24                                            # mvs_softargmin_conf
