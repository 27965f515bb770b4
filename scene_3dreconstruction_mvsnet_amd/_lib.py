"""ctypes binding of libmvs_hip.so (the C ABI declared in include/mvs_abi.h).

There is no CPU fallback: if the shared library is missing or an entry point fails, a
RuntimeError is raised.  `import torch` must happen before the library is loaded so that the
HIP runtime torch ships (same soname, libamdhip64.so.7) is the one both sides share -- stream
handles and device pointers are only meaningful inside one runtime instance.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must be imported first, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVS_LIB_PATH") or os.path.join(_HERE, "csrc", "libmvs_hip.so")

MVS_F32, MVS_F16, MVS_BF16 = 0, 1, 2
DTYPE_CODES = {"f32": MVS_F32, "f16": MVS_F16, "bf16": MVS_BF16,
               "float32": MVS_F32, "float16": MVS_F16, "bfloat16": MVS_BF16}
TORCH_DTYPES = {MVS_F32: torch.float32, MVS_F16: torch.float16, MVS_BF16: torch.bfloat16}


def dtype_code(dtype) -> int:
    """'f32' | 'f16' | 'bf16' | torch dtype | mvs_dtype int -> mvs_dtype int (storage dtype of the
    private volumes; arithmetic stays fp32)."""
    if isinstance(dtype, int):
        if dtype in TORCH_DTYPES:
            return dtype
        raise ValueError(f"unknown mvs_dtype {dtype}")
    if isinstance(dtype, torch.dtype):
        for code, td in TORCH_DTYPES.items():
            if td == dtype:
                return code
        raise ValueError(f"unsupported storage dtype {dtype}")
    return DTYPE_CODES[str(dtype)]
NUM_LAYERS = 11
ABI_VERSION = 2

# mvs_image_format (include/mvs_abi.h)
MVS_IMG_F32_CHW, MVS_IMG_U8_CHW, MVS_IMG_U8_HWC = 0, 1, 2

_lock = threading.Lock()
_lib = None

_vp = ctypes.c_void_p
_i = ctypes.c_int
_sz = ctypes.c_size_t
_f, _d, _ll, _ull = ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_ulonglong
_szp = ctypes.POINTER(_sz)      # size_t* bytes
_vpp = ctypes.POINTER(_vp)      # const float* const*

# Every entry point, declared once on this side: header -> {name: argument types}, in the headers' order.  Any other
# pointer is a c_void_p (device and host addresses travel as integers).  load() applies the table; SYMBOLS and
# FUSE_SYMBOLS, CLOUD_SYMBOLS, NORMALS_SYMBOLS, OUTLIERS_SYMBOLS, DISTANCE_SYMBOLS, REDUCE_SYMBOLS and CLUSTER_SYMBOLS are its
# keys; tests/test_host_logic.py, tests/test_scan_fusion_host.py, tests/test_cloud_downsample_host.py,
# tests/test_cloud_normals_host.py, tests/test_cloud_outliers_host.py, tests/test_cloud_distance_host.py,
# tests/test_cloud_reduce_host.py and tests/test_cloud_cluster_host.py hold every argument list to its prototype.
# Everything returns int except mvs_last_error_string.
_ABI = {
    "mvs_abi.h": {
        "mvs_abi_version": [],
        "mvs_last_error_string": [],
        "mvs_query_workspace": [_i, _i, _i, _i, _i, _i, _szp],
        "mvs_query_weights_blob": [_szp],
        "mvs_pack_weights": [_vpp, _vpp, _vp, _f, _vp, _sz],
        "mvs_relative_proj": [_vp, _vp, _i, _vp],
        "mvs_warp_variance": [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_costreg_forward": [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _vp],
        "mvs_conv_layer": [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "mvs_conv11_prob": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "mvs_softargmin_conf": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
        "mvs_depth_infer": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_depth_infer_views": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_homo_warp": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "mvs_depth_regression": [_vp, _vp, _vp, _i, _i, _i, _vp],
        "mvs_filter_compose": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
        "mvs_filter_depth": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _d, _d, _vp, _vp, _vp, _vp, _vp],
        "mvs_query_feature_blob": [_szp],
        "mvs_pack_feature_weights": [_vpp, _vpp, _vp, _f, _vp, _sz],
        "mvs_query_feature_workspace": [_i, _i, _i, _szp],
        "mvs_feature_layer": [_i, _vp, _vp, _vp, _i, _i, _i, _vp],
        "mvs_feature_conv01_fmt": [_vp, _i, _vp, _vp, _i, _i, _i, _vp],
        "mvs_feature_net": [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp],
        "mvs_query_forward_workspace": [_i, _i, _i, _i, _i, _szp],
        "mvs_forward_images": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp],
        "mvs_feature_net_fmt": [_vp, _i, _vp, _vp, _vp, _sz, _i, _i, _i, _vp],
        "mvs_forward_images_fmt": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp],
        "mvs_query_metrics_workspace": [_i, _i, _i, _szp],
        "mvs_depth_metrics": [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp],
        "mvs_warp_variance_backward": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
        "mvs_softargmin_backward": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
        "mvs_query_conv3d_train_workspace": [_i, _i, _i, _i, _i, _i, _szp],
        "mvs_conv3d_train_forward": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_conv3d_train_backward_data": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_conv3d_train_backward_weight": [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
        "mvs_query_bn3d_train_workspace": [_i, _ll, _szp],
        "mvs_bn3d_train_forward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _ll, _vp, _sz, _vp],
        "mvs_bn3d_train_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _ll, _vp, _sz, _vp],
        "mvs_volume_relayout": [_vp, _vp, _i, _ll, _i, _vp],
    },
    # kept apart: SYMBOLS is exactly mvs_abi.h
    "mvs_fuse_abi.h": {
        "mvs_query_fuse_workspace": [_i, _i, _i, _szp],
        "mvs_fuse_points": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _ll, _vp, _vp, _vp, _vp, _sz, _vp],
    },
    "mvs_cloud_abi.h": {
        "mvs_query_cloud_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_downsample": [_vp, _i, _vp, _ll, _vp, _vp, _d, _d, _ll, _vp, _vp, _vp, _vp, _sz, _vp],
    },
    "mvs_normals_abi.h": {
        "mvs_query_normals_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_normals": [_vp, _i, _ll, _vp, _vp, _d, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp],
        "mvs_query_cloud_normals_downsample_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_downsample_normals": [_vp, _i, _vp, _vp, _ll, _vp, _vp, _d, _d, _ll, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    },
    "mvs_outliers_abi.h": {
        "mvs_query_outliers_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_outliers": [_vp, _i, _ll, _vp, _vp, _d, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    },
    "mvs_distance_abi.h": {
        "mvs_query_distance_workspace": [_ll, _ll, _vp, _vp, _d, _szp],
        "mvs_cloud_distance": [_vp, _i, _ll, _vp, _i, _ll, _vp, _vp, _d, _d, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    },
    "mvs_reduce_abi.h": {
        "mvs_query_reduce_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_reduce": [_vp, _i, _ll, _vp, _vp, _d, _d, _ull, _i, _vp, _vp, _vp, _sz, _vp],
        "mvs_cloud_select": [_vp, _i, _ll, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp],
    },
    "mvs_cluster_abi.h": {
        "mvs_query_cluster_workspace": [_ll, _vp, _vp, _d, _szp],
        "mvs_cloud_cluster": [_vp, _i, _ll, _vp, _vp, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    },
}
SYMBOLS = tuple(_ABI["mvs_abi.h"])
FUSE_SYMBOLS = tuple(_ABI["mvs_fuse_abi.h"])
CLOUD_SYMBOLS = tuple(_ABI["mvs_cloud_abi.h"])
NORMALS_SYMBOLS = tuple(_ABI["mvs_normals_abi.h"])
OUTLIERS_SYMBOLS = tuple(_ABI["mvs_outliers_abi.h"])
DISTANCE_SYMBOLS = tuple(_ABI["mvs_distance_abi.h"])
REDUCE_SYMBOLS = tuple(_ABI["mvs_reduce_abi.h"])
CLUSTER_SYMBOLS = tuple(_ABI["mvs_cluster_abi.h"])

# The headers under include/ext/, kept in a table of their own: `_ABI` is exactly the headers of include/*.h.  load()
# applies both; tests/test_cloud_register_host.py and tests/test_cloud_planes_host.py hold this one to its prototypes.
_ABI_EXT = {
    "ext/mvs_register_abi.h": {
        "mvs_query_register_workspace": [_ll, _ll, _vp, _vp, _d, _i, _szp],
        "mvs_cloud_register": [_vp, _i, _ll, _vp, _vp, _i, _ll, _vp, _vp, _d, _d, _vp, _i, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _sz, _vp],
    },
    "ext/mvs_planes_abi.h": {
        "mvs_query_planes_workspace": [_ll, _i, _i, _szp],
        "mvs_cloud_planes": [_vp, _i, _ll, _vp, _vp, _d, _i, _i, _ll, _ull, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    },
}
REGISTER_SYMBOLS = tuple(_ABI_EXT["ext/mvs_register_abi.h"])
PLANES_SYMBOLS = tuple(_ABI_EXT["ext/mvs_planes_abi.h"])


class MvsError(RuntimeError):
    """Non-zero status from libmvs_hip.so (decoded with mvs_last_error_string)."""

    def __init__(self, code, msg):
        super().__init__(f"libmvs_hip status {code}: {msg}")
        self.code = code


def load():
    """Load libmvs_hip.so once; raises RuntimeError if it is missing (no fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or make -C scene_3dreconstruction_mvsnet_amd/csrc). "
                "There is no CPU/PyTorch fallback for the MVSNet depth path.")
        lib = ctypes.CDLL(LIB_PATH)
        for name in (SYMBOLS + FUSE_SYMBOLS + CLOUD_SYMBOLS + NORMALS_SYMBOLS + OUTLIERS_SYMBOLS + DISTANCE_SYMBOLS
                     + REDUCE_SYMBOLS + CLUSTER_SYMBOLS + REGISTER_SYMBOLS + PLANES_SYMBOLS):
            if not hasattr(lib, name):
                raise RuntimeError(f"{LIB_PATH} does not export {name}")
        for prototypes in list(_ABI.values()) + list(_ABI_EXT.values()):
            for name, argtypes in prototypes.items():
                fn = getattr(lib, name)
                fn.argtypes = argtypes
                fn.restype = ctypes.c_char_p if name == "mvs_last_error_string" else _i
        if lib.mvs_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libmvs_hip ABI {lib.mvs_abi_version()} != expected {ABI_VERSION}")
        _lib = lib
        return _lib


def check(status: int) -> None:
    if status != 0:
        raise MvsError(status, load().mvs_last_error_string().decode("utf-8", "replace"))


def _query(name, *args) -> int:
    """The byte count an mvs_query_* entry point writes through its last argument (`size_t* bytes`)."""
    n = _sz(0)
    check(getattr(load(), name)(*args, ctypes.byref(n)))
    return int(n.value)


def query_workspace(N, C, D, h, w, dtype=MVS_F32) -> int:
    return _query("mvs_query_workspace", N, C, D, h, w, dtype)


def query_weights_blob() -> int:
    return _query("mvs_query_weights_blob")


def _stream(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def _check_out(t, shape, dtype, device, who, what):
    """The refusal of a caller's output tensor that is not contiguous, of `dtype`, shaped `shape` and on `device`."""
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != device:
        raise RuntimeError(f"{who} must be a contiguous {what}")


def _dev_in(t, name, dtype=torch.float32, shape=None, device=None):
    """The refusal of a device input that is on the host, not of `dtype`, empty, or (where given) not shaped `shape` or
    not on `device`; otherwise the tensor, contiguous (a non-contiguous view is copied)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device if isinstance(t, torch.Tensor) else type(t).__name__}); "
                           "the MVSNet depth path has no CPU implementation")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype)[6:]} (got {t.dtype})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, not on {device}: the tensors of one call must be on one device")
    if t.numel() == 0:
        raise RuntimeError(f"{name} is empty: {list(t.shape)}")
    return t.contiguous()


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    return _dev_in(t, name)


def _aligned16(who, **tensors):
    """The library's alignment rule (include/mvs_abi.h), before the call: the pointers its kernels touch wider than an
    element, and the blobs, are refused unless 16-byte aligned, which a contiguous view at an offset of a larger tensor
    need not be.  The tensors the header states are per element are not passed here."""
    for name, t in tensors.items():
        if t is not None and t.data_ptr() & 15:
            raise RuntimeError(f"{who}: {name} starts at 0x{t.data_ptr():x}: the library reads and writes 16 bytes at a time "
                               "and refuses an address that is not 16-byte aligned (a view at an offset of a larger tensor)")


_BLOB_QUERY = {"weights": "mvs_query_weights_blob", "feature": "mvs_query_feature_blob"}
_blob_bytes = {}


def _check_blob(blob, which, device, who):
    """The refusal of a packed blob ("weights": pack_weights, "feature": pack_feature_weights) that is not a contiguous
    1-D uint8 tensor on `device` of at least its query's bytes: the library gets an address and no size to check."""
    need = _blob_bytes.get(which)
    if need is None:
        need = _blob_bytes[which] = _query(_BLOB_QUERY[which])
    if not isinstance(blob, torch.Tensor) or not blob.is_cuda or blob.device != device or blob.dtype != torch.uint8 \
            or blob.dim() != 1 or blob.numel() < need or not blob.is_contiguous() or blob.data_ptr() & 15:
        got = f"{blob.dtype} {list(blob.shape)} on {blob.device}" if isinstance(blob, torch.Tensor) else type(blob).__name__
        raise RuntimeError(f"{who}: the {which} blob must be a contiguous, 16-byte aligned uint8 [{need}] tensor on {device} (pack_"
                           f"{'feature_' if which == 'feature' else ''}weights(...).to(device)), got {got}")


def _check_workspace(ws, device, who, align=256):
    """The refusal of a workspace that is not a contiguous 1-D uint8 tensor on `device`, aligned as its entry point asks:
    its numel() travels as its size in bytes.  Whether it is large enough is the library's check."""
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != device or ws.dtype != torch.uint8 \
            or ws.dim() != 1 or not ws.is_contiguous() or ws.data_ptr() & (align - 1):
        got = f"{ws.dtype} {list(ws.shape)} on {ws.device}" if isinstance(ws, torch.Tensor) else type(ws).__name__
        raise RuntimeError(f"{who}: workspace must be a contiguous, {align}-byte aligned 1-D uint8 tensor on {device}, got {got}")


def _rt_arg(rt, N, device, who):
    """rt [(N-1),12] of relative_proj on `device`; with one view there is nothing to read and None may stand for it."""
    if N == 1 and rt is None:
        return None
    if N == 1 and isinstance(rt, torch.Tensor) and rt.dim() == 2:
        return _dev_in(rt, f"{who}: rt", shape=(rt.shape[0], 12), device=device)
    return _dev_in(rt, f"{who}: rt", shape=(N - 1, 12), device=device)


# reference parameter names, relative to `cost_regularization.` (models/mvsnet.py:35-62)
CONV_WEIGHT_KEYS = tuple([f"conv{i}.conv.weight" for i in range(7)] +
                         ["conv7.0.weight", "conv9.0.weight", "conv11.0.weight", "prob.weight"])
BN_PREFIXES = tuple([f"conv{i}.bn" for i in range(7)] + ["conv7.1", "conv9.1", "conv11.1"])
_LAYER_CH = ((32, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64),
             (64, 32), (32, 16), (16, 8), (8, 1))


_BN_SUFFIXES = ("weight", "bias", "running_mean", "running_var")


def _host_f32(state, entries):
    """Named state entries -> (array of their addresses, the arrays): entries = [(key, shape)], each taken from `state`
    as a contiguous float32 host array of exactly that shape.  The addresses hold while the arrays are alive."""
    import numpy as np
    arrays = []
    for key, shape in entries:
        a = state[key]
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise RuntimeError(f"{key}: shape {tuple(a.shape)} != expected {tuple(shape)}")
        arrays.append(a)
    return (_vp * len(arrays))(*[a.ctypes.data for a in arrays]), arrays


def _pack(pack, nbytes, state, convs, bns, bias, eps):
    """One mvs_pack_* call: the conv weights, the BatchNorm parameters and the bias of `state` -> host blob (uint8)."""
    conv_ptrs, conv_arrays = _host_f32(state, convs)      # the arrays are locals: they outlive the call below
    bn_ptrs, bn_arrays = _host_f32(state, bns)
    bias_ptr, bias_array = _host_f32(state, [bias])
    blob = torch.empty(nbytes, dtype=torch.uint8)
    check(pack(conv_ptrs, bn_ptrs, bias_ptr[0], ctypes.c_float(eps), blob.data_ptr(), nbytes))
    return blob


def pack_weights(state: dict, eps: float = 1e-5) -> torch.Tensor:
    """BN-fold + re-layout the CostRegNet parameters into the kernels' blob (host, uint8).

    `state` maps names relative to `cost_regularization.` to CPU float32 tensors/arrays.
    """
    convs = [(key, (ci, co, 3, 3, 3) if 7 <= l <= 9 else (co, ci, 3, 3, 3))
             for l, (key, (ci, co)) in enumerate(zip(CONV_WEIGHT_KEYS, _LAYER_CH))]
    bns = [(f"{pre}.{suffix}", (_LAYER_CH[l][1],)) for l, pre in enumerate(BN_PREFIXES) for suffix in _BN_SUFFIXES]
    return _pack(load().mvs_pack_weights, query_weights_blob(), state, convs, bns, ("prob.bias", (1,)), eps)


def relative_proj(proj: torch.Tensor) -> torch.Tensor:
    """proj [N,4,4] cuda -> rt [(N-1),12] cuda (models/module.py:107-109)."""
    proj = _dev_f32(proj, "proj_matrices")
    if proj.dim() != 3 or tuple(proj.shape[1:]) != (4, 4):
        raise RuntimeError(f"proj_matrices must be [N,4,4], got {list(proj.shape)}")
    N = proj.shape[0]
    _aligned16("relative_proj", proj_matrices=proj)
    with torch.cuda.device(proj.device):
        rt = torch.empty((max(N - 1, 1), 12), dtype=torch.float32, device=proj.device)
        check(load().mvs_relative_proj(proj.data_ptr(), rt.data_ptr(), N, _stream(proj.device)))
    return rt


def _depth_values_arg(depth_values, device, who, D=None):
    """depth_values [D] on `device` (D given: exactly that many)."""
    if isinstance(depth_values, torch.Tensor) and depth_values.dim() != 1:
        raise RuntimeError(f"{who}: depth_values must be [D], got {list(depth_values.shape)}")
    return _dev_in(depth_values, f"{who}: depth_values", shape=None if D is None else (D,), device=device)


def warp_variance(feats, rt, depth_values, workspace, dtype=MVS_F32):
    """feats [N,32,h,w], rt [(N-1),12], depth_values [D] -> C8-planar volume [4,D,h,w,8]."""
    feats = _dev_f32(feats, "features")
    if feats.dim() != 4 or feats.shape[1] % 8:
        raise RuntimeError(f"warp_variance: features must be [N,C,h,w] with 8 | C, got {list(feats.shape)}")
    N, C, h, w = feats.shape
    dev = feats.device
    rt = _rt_arg(rt, N, dev, "warp_variance")
    depth_values = _depth_values_arg(depth_values, dev, "warp_variance")
    D = depth_values.shape[0]
    _check_workspace(workspace, dev, "warp_variance")
    _aligned16("warp_variance", rt=rt, depth_values=depth_values)
    with torch.cuda.device(dev):
        var = torch.empty((C // 8, D, h, w, 8), dtype=TORCH_DTYPES[dtype], device=dev)
        check(load().mvs_warp_variance(feats.data_ptr(), None if rt is None else rt.data_ptr(), depth_values.data_ptr(),
                                       var.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       N, C, D, h, w, dtype, _stream(dev)))
    return var


def costreg_forward(var, blob, workspace, dtype=MVS_F32):
    """var [4,D,h,w,8] (C8-planar) -> cost logits [D,h,w] fp32."""
    if var.dtype != TORCH_DTYPES[dtype] or not var.is_cuda or not var.is_contiguous():
        raise RuntimeError(f"variance volume must be a contiguous CUDA tensor of {TORCH_DTYPES[dtype]}")
    if var.dim() != 5 or var.shape[0] != 4 or var.shape[4] != 8 or var.numel() == 0:
        raise RuntimeError(f"costreg_forward: the variance volume must be C8-planar [4,D,h,w,8], got {list(var.shape)}")
    _, D, h, w, _ = var.shape
    _check_blob(blob, "weights", var.device, "costreg_forward")
    _check_workspace(workspace, var.device, "costreg_forward")
    _aligned16("costreg_forward", var=var)
    with torch.cuda.device(var.device):
        cost = torch.empty((D, h, w), dtype=torch.float32, device=var.device)
        check(load().mvs_costreg_forward(var.data_ptr(), blob.data_ptr(), cost.data_ptr(),
                                         workspace.data_ptr(), workspace.numel(), D, h, w, dtype,
                                         _stream(var.device)))
    return cost


def conv_layer(layer, x, skip, blob, dtype=MVS_F32):
    """One CostRegNet layer on C8-planar tensors [Cin/8,D,h,w,8] -> [Cout/8,D',h',w',8]."""
    ci, co = _LAYER_CH[layer]
    if not isinstance(x, torch.Tensor) or x.dim() != 5 or x.numel() == 0:
        raise RuntimeError(f"layer {layer}: input must be a C8-planar [Cin/8,D,h,w,8] tensor")
    planes, Di, Hi, Wi, c8 = x.shape
    if planes * c8 != ci or c8 != 8:
        raise RuntimeError(f"layer {layer}: input has {planes}x{c8} channels, expected {ci}")
    if x.dtype != TORCH_DTYPES[dtype] or (skip is not None and skip.dtype != TORCH_DTYPES[dtype]):
        raise RuntimeError(f"layer {layer}: tensors are {x.dtype}, storage dtype says {TORCH_DTYPES[dtype]}")
    if not x.is_cuda or not x.is_contiguous() or (skip is not None and not (skip.is_cuda and skip.is_contiguous())):
        raise RuntimeError(f"layer {layer}: needs contiguous CUDA(ROCm) tensors")
    if skip is not None and skip.device != x.device:
        raise RuntimeError(f"layer {layer}: x and skip must be on one device")
    _check_blob(blob, "weights", x.device, f"layer {layer}")
    _aligned16(f"layer {layer}", x=x, skip=skip)
    if 7 <= layer <= 9:
        odims = (2 * Di, 2 * Hi, 2 * Wi)
    elif layer in (1, 3, 5):
        odims = ((Di - 1) // 2 + 1, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    else:
        odims = (Di, Hi, Wi)
    oshape = odims if layer == 10 else (co // 8,) + odims + (8,)
    if skip is not None and tuple(skip.shape) != tuple(oshape):
        raise RuntimeError(f"layer {layer}: skip shape {tuple(skip.shape)} != {oshape}")
    with torch.cuda.device(x.device):
        y = torch.empty(oshape, dtype=torch.float32 if layer == 10 else TORCH_DTYPES[dtype], device=x.device)
        check(load().mvs_conv_layer(layer, x.data_ptr(), 0 if skip is None else skip.data_ptr(),
                                    y.data_ptr(), blob.data_ptr(), Di, Hi, Wi, dtype,
                                    _stream(x.device)))
    return y


def conv11_prob(x, skip, blob, dtype=MVS_F32):
    """Layers 9 + 10 in one kernel: x [2,Di,Hi,Wi,8], skip [1,2Di,2Hi,2Wi,8] (storage dtype) -> fp32 cost logits
    [2Di,2Hi,2Wi]."""
    if not isinstance(x, torch.Tensor) or not isinstance(skip, torch.Tensor) or x.dim() != 5 or x.numel() == 0:
        raise RuntimeError("conv11_prob: x and skip must be C8-planar tensors")
    planes, Di, Hi, Wi, c8 = x.shape
    if planes != 2 or c8 != 8 or tuple(skip.shape) != (1, 2 * Di, 2 * Hi, 2 * Wi, 8):
        raise RuntimeError(f"conv11_prob: shapes {tuple(x.shape)} / {tuple(skip.shape)}")
    if x.dtype != TORCH_DTYPES[dtype] or skip.dtype != TORCH_DTYPES[dtype]:
        raise RuntimeError(f"conv11_prob: tensors must be {TORCH_DTYPES[dtype]}")
    if not (x.is_cuda and skip.is_cuda and x.is_contiguous() and skip.is_contiguous()):
        raise RuntimeError("conv11_prob: needs contiguous CUDA(ROCm) tensors")
    if skip.device != x.device:
        raise RuntimeError("conv11_prob: x and skip must be on one device")
    _check_blob(blob, "weights", x.device, "conv11_prob")
    _aligned16("conv11_prob", x=x, skip=skip)
    with torch.cuda.device(x.device):
        cost = torch.empty((2 * Di, 2 * Hi, 2 * Wi), dtype=torch.float32, device=x.device)
        check(load().mvs_conv11_prob(x.data_ptr(), skip.data_ptr(), cost.data_ptr(), blob.data_ptr(), Di, Hi, Wi,
                                     dtype, _stream(x.device)))
    return cost


def _cost_arg(cost, who):
    cost = _dev_f32(cost, "cost")
    if cost.dim() != 3:
        raise RuntimeError(f"{who}: cost must be [D,h,w], got {list(cost.shape)}")
    return cost


def softargmin_conf(cost, depth_values):
    cost = _cost_arg(cost, "softargmin_conf")
    D, h, w = cost.shape
    depth_values = _depth_values_arg(depth_values, cost.device, "softargmin_conf", D)
    with torch.cuda.device(cost.device):
        depth = torch.empty((h, w), dtype=torch.float32, device=cost.device)
        conf = torch.empty_like(depth)
        check(load().mvs_softargmin_conf(cost.data_ptr(), depth_values.data_ptr(), depth.data_ptr(), conf.data_ptr(),
                                         D, h, w, _stream(cost.device)))
    return depth, conf


def warp_variance_backward(feats, rt, depth_values, grad_var, out=None):
    """Adjoint of warp_variance (fp32): feats [N,32,h,w], rt [(N-1),12], depth_values [D], grad_var [32,D,h,w]
    (NCDHW) -> grad_feats [N,32,h,w] (into `out` when given).  Enqueued on the current stream."""
    feats = _dev_f32(feats, "features")
    if feats.dim() != 4:
        raise RuntimeError(f"warp_variance_backward: features must be [N,C,h,w], got {list(feats.shape)}")
    N, C, h, w = feats.shape
    dev = feats.device
    depth_values = _depth_values_arg(depth_values, dev, "warp_variance_backward")
    D = depth_values.shape[0]
    grad_var = _dev_in(grad_var, "grad_var", shape=(C, D, h, w), device=dev)
    rt = _rt_arg(rt, N, dev, "warp_variance_backward")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(feats)
        else:
            _check_out(out, feats.shape, torch.float32, dev, "warp_variance_backward: out",
                       "float32 tensor shaped like feats")
        _aligned16("warp_variance_backward", features=feats, rt=rt, depth_values=depth_values, grad_var=grad_var, out=out)
        check(load().mvs_warp_variance_backward(feats.data_ptr(), None if rt is None else rt.data_ptr(),
                                                depth_values.data_ptr(), grad_var.data_ptr(), out.data_ptr(),
                                                N, C, D, h, w, _stream(dev)))
    return out


def softargmin_backward(cost, depth_values, grad_depth):
    """Adjoint of softargmin_conf's depth: cost [D,h,w], depth_values [D], grad_depth [h,w] -> grad_cost [D,h,w]."""
    cost = _cost_arg(cost, "softargmin_backward")
    D, h, w = cost.shape
    grad_depth = _dev_in(grad_depth, "grad_depth", shape=(h, w), device=cost.device)
    depth_values = _depth_values_arg(depth_values, cost.device, "softargmin_backward", D)
    with torch.cuda.device(cost.device):
        gc = torch.empty_like(cost)
        check(load().mvs_softargmin_backward(cost.data_ptr(), depth_values.data_ptr(), grad_depth.data_ptr(),
                                             gc.data_ptr(), D, h, w, _stream(cost.device)))
    return gc


# ---- training convolutions (csrc/train_conv3d.hip).  Volumes are channels-last [D,H,W,C] float32 tensors of one batch
# item; Cin, Cout, D, H, W, stride describe the convolution (x [D,H,W,Cin] -> y [D/s,H/s,W/s,Cout]).
def conv3d_train_workspace_bytes(Cin, Cout, D, H, W, stride) -> int:
    return _query("mvs_query_conv3d_train_workspace", Cin, Cout, D, H, W, stride)


def _cl_volume(t, name):
    t = _dev_f32(t, name)
    if t.dim() != 4:
        raise RuntimeError(f"{name} must be a channels-last volume [D,H,W,C], got {tuple(t.shape)}")
    return t


def _check_stride(dims, stride, who):
    """The library takes D, H, W of the full-resolution side and an int stride: dims the stride does not divide would be
    floored here and the kernel would then read or write a volume the caller does not have."""
    if stride not in (1, 2):
        raise RuntimeError(f"{who}: stride {stride!r} (1 or 2)")
    if any(d % stride for d in dims):      # the library's words for it
        raise RuntimeError(f"{who}: stride 2 needs even D,H,W (got {','.join(str(d) for d in dims)})")


def conv3d_train_forward(x, w, bias, stride, flip_transpose=False):
    """x [D,H,W,Cin], w [Cout,Cin,3,3,3] ([Cin,Cout,3,3,3] with flip_transpose) -> y [D/s,H/s,W/s,Cout]."""
    x = _cl_volume(x, "x")
    w = _dev_in(w, "weight", device=x.device)
    D, H, W, Cin = x.shape
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or (w.shape[0] if flip_transpose else w.shape[1]) != Cin:
        raise RuntimeError(f"weight {tuple(w.shape)} does not fit a 3x3x3 convolution of {Cin} channels")
    Cout = w.shape[1] if flip_transpose else w.shape[0]
    _check_stride((D, H, W), stride, "conv3d_train_forward")
    if bias is not None:
        bias = _dev_in(bias, "bias", shape=(Cout,), device=x.device)
    with torch.cuda.device(x.device):
        y = torch.empty((D // stride, H // stride, W // stride, Cout), dtype=torch.float32, device=x.device)
        check(load().mvs_conv3d_train_forward(x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(),
                                              y.data_ptr(), Cin, Cout, D, H, W, stride, int(bool(flip_transpose)),
                                              _stream(x.device)))
    return y


def conv3d_train_backward_data(gy, w, stride):
    """gy [D/s,H/s,W/s,Cout], w [Cout,Cin,3,3,3] -> gx [D,H,W,Cin] (every voxel written)."""
    gy = _cl_volume(gy, "gy")
    w = _dev_in(w, "weight", device=gy.device)
    Do, Ho, Wo, Cout = gy.shape
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or w.shape[0] != Cout:
        raise RuntimeError(f"weight {tuple(w.shape)} does not fit a gradient of {Cout} channels")
    Cin = w.shape[1]
    _check_stride((), stride, "conv3d_train_backward_data")
    D, H, W = Do * stride, Ho * stride, Wo * stride
    with torch.cuda.device(gy.device):
        gx = torch.empty((D, H, W, Cin), dtype=torch.float32, device=gy.device)
        check(load().mvs_conv3d_train_backward_data(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), Cin, Cout, D, H, W,
                                                    stride, _stream(gy.device)))
    return gx


def conv3d_train_backward_weight(x, gy, stride, with_bias=False):
    """x [D,H,W,Cin], gy [D/s,H/s,W/s,Cout] -> gw [Cout,Cin,3,3,3] (and gbias [Cout] with with_bias)."""
    x, gy = _cl_volume(x, "x"), _cl_volume(gy, "gy")
    D, H, W, Cin = x.shape
    Cout = gy.shape[3]
    _check_stride((D, H, W), stride, "conv3d_train_backward_weight")
    if tuple(gy.shape[:3]) != (D // stride, H // stride, W // stride):
        raise RuntimeError(f"gy {tuple(gy.shape)} does not fit x {tuple(x.shape)} at stride {stride}")
    if gy.device != x.device:
        raise RuntimeError("conv3d_train_backward_weight: x and gy must be on one device")
    nbytes = conv3d_train_workspace_bytes(Cin, Cout, D, H, W, stride)
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        gw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
        gb = torch.empty((Cout,), dtype=torch.float32, device=x.device) if with_bias else None
        check(load().mvs_conv3d_train_backward_weight(x.data_ptr(), gy.data_ptr(), gw.data_ptr(),
                                                      None if gb is None else gb.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      Cin, Cout, D, H, W, stride, _stream(x.device)))
    return (gw, gb) if with_bias else gw


# ---- training batch-norm (csrc/train_bn3d.hip).  Data is channels-last [M, C] float32: M voxels pooled over the batch.
def bn3d_train_workspace_bytes(C, M) -> int:
    return _query("mvs_query_bn3d_train_workspace", C, M)


def _cl_rows(t, name):
    t = _dev_f32(t, name)
    if t.dim() != 2:
        raise RuntimeError(f"{name} must be channels-last rows [M,C], got {tuple(t.shape)}")
    return t


def _channel_vector(t, C, name, device=None):
    t = _dev_f32(t, name)
    if tuple(t.shape) != (C,):
        raise RuntimeError(f"{name} {tuple(t.shape)} must be [{C}]")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, not on {device}: the tensors of one call must be on one device")
    return t


def bn3d_train_forward(y, gamma, beta, skip=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                       relu=True):
    """y [M,C], gamma, beta [C], skip [M,C] or None -> (out [M,C], save_mean [C], save_invstd [C]); out = relu(bn(y)) +
    skip with batch statistics.  running_mean / running_var [C] (both or neither) are updated in place."""
    y = _cl_rows(y, "y")
    M, C = y.shape
    dev = y.device
    gamma, beta = _channel_vector(gamma, C, "gamma", dev), _channel_vector(beta, C, "beta", dev)
    if skip is not None:
        skip = _cl_rows(skip, "skip")
        if skip.shape != y.shape or skip.device != dev:
            raise RuntimeError(f"skip {tuple(skip.shape)} must be shaped like y {tuple(y.shape)} and on its device")
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("running_mean and running_var must both be given or both be None")
    if running_mean is not None:
        for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (C,) \
                    or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"{name} must be a contiguous float32 CUDA tensor [{C}] on y's device (it is updated in "
                                   "place)")
    nbytes = bn3d_train_workspace_bytes(C, M)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty_like(y)
        mean = torch.empty((C,), dtype=torch.float32, device=dev)
        invstd = torch.empty_like(mean)
        check(load().mvs_bn3d_train_forward(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                            None if skip is None else skip.data_ptr(), out.data_ptr(), mean.data_ptr(),
                                            invstd.data_ptr(), None if running_mean is None else running_mean.data_ptr(),
                                            None if running_var is None else running_var.data_ptr(), float(momentum),
                                            float(eps), int(bool(relu)), C, M, ws.data_ptr(), ws.numel(),
                                            _stream(dev)))
    return out, mean, invstd


def bn3d_train_backward(y, grad_out, gamma, beta, save_mean, save_invstd, relu=True):
    """y, grad_out [M,C]; gamma, beta, save_mean, save_invstd [C] -> (grad_y [M,C], grad_gamma [C], grad_beta [C]).
    grad_out is the gradient of relu(bn(y)) (+ skip: the skip's own gradient is grad_out itself)."""
    y, grad_out = _cl_rows(y, "y"), _cl_rows(grad_out, "grad_out")
    M, C = y.shape
    dev = y.device
    if grad_out.shape != y.shape or grad_out.device != dev:
        raise RuntimeError(f"grad_out {tuple(grad_out.shape)} must be shaped like y {tuple(y.shape)} and on its device")
    vec = [_channel_vector(t, C, n, dev) for t, n in ((gamma, "gamma"), (beta, "beta"), (save_mean, "save_mean"),
                                                      (save_invstd, "save_invstd"))]
    nbytes = bn3d_train_workspace_bytes(C, M)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gy = torch.empty_like(y)
        gg = torch.empty((C,), dtype=torch.float32, device=dev)
        gb = torch.empty_like(gg)
        check(load().mvs_bn3d_train_backward(y.data_ptr(), grad_out.data_ptr(), *[t.data_ptr() for t in vec],
                                             gy.data_ptr(), gg.data_ptr(), gb.data_ptr(), int(bool(relu)), C, M,
                                             ws.data_ptr(), ws.numel(), _stream(dev)))
    return gy, gg, gb


RELAYOUT_C8_TO_CHANNELS_LAST, RELAYOUT_CHANNELS_LAST_TO_PLANAR = 0, 1


def volume_relayout(src, direction, out=None):
    """direction RELAYOUT_C8_TO_CHANNELS_LAST: C8-planar [C/8,D,h,w,8] -> channels-last [D,h,w,C];
    RELAYOUT_CHANNELS_LAST_TO_PLANAR: channels-last [D,h,w,C] -> planar [C,D,h,w].  A pure copy (into `out` when given)."""
    src = _dev_f32(src, "volume")
    if direction == RELAYOUT_C8_TO_CHANNELS_LAST:
        if src.dim() != 5 or src.shape[4] != 8:
            raise RuntimeError(f"volume must be C8-planar [C/8,D,h,w,8], got {tuple(src.shape)}")
        C, dims = src.shape[0] * 8, tuple(src.shape[1:4])
        oshape = dims + (C,)
    elif direction == RELAYOUT_CHANNELS_LAST_TO_PLANAR:
        if src.dim() != 4:
            raise RuntimeError(f"volume must be channels-last [D,h,w,C], got {tuple(src.shape)}")
        C, dims = src.shape[3], tuple(src.shape[:3])
        oshape = (C,) + dims
    else:
        raise RuntimeError(f"volume_relayout: direction {direction!r} (0 or 1)")
    with torch.cuda.device(src.device):
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=src.device)
        else:
            _check_out(out, oshape, torch.float32, src.device, "volume_relayout: out", f"float32 tensor {oshape}")
        check(load().mvs_volume_relayout(src.data_ptr(), out.data_ptr(), C, dims[0] * dims[1] * dims[2], direction,
                                         _stream(src.device)))
    return out


def _depth_call_args(who, dev, N, h, w, proj, depth_values, blob, workspace, depth_out, conf_out, fblob=None):
    """What depth_infer, depth_infer_views and forward_images check alike, on the device `dev` of their first tensor:
    proj [N,4,4] and depth_values [D] (returned contiguous), the blob(s), the workspace and the two [h,w] outputs."""
    proj = _dev_in(proj, f"{who}: proj_matrices", shape=(N, 4, 4), device=dev)
    depth_values = _depth_values_arg(depth_values, dev, who)
    if fblob is not None:
        _check_blob(fblob, "feature", dev, who)
    _check_blob(blob, "weights", dev, who)
    _check_workspace(workspace, dev, who)
    _check_out(depth_out, (h, w), torch.float32, dev, f"{who}: depth_out", f"float32 [{h},{w}] tensor on {dev}")
    _check_out(conf_out, (h, w), torch.float32, dev, f"{who}: conf_out", f"float32 [{h},{w}] tensor on {dev}")
    _aligned16(who, proj_matrices=proj, depth_values=depth_values)
    return proj, depth_values


_workspace_bytes = {}      # (N, C, D, h, w, dtype) -> mvs_query_workspace's answer


def depth_infer(feats, proj, depth_values, blob, workspace, depth_out, conf_out, dtype=MVS_F32):
    """Whole path for one batch item; outputs are written into depth_out / conf_out [h,w]."""
    feats = _dev_f32(feats, "features")
    if feats.dim() != 4:
        raise RuntimeError(f"depth_infer: feats must be [N,C,h,w], got {list(feats.shape)}")
    N, C, h, w = feats.shape
    dev = feats.device
    depth_values = _depth_values_arg(depth_values, dev, "depth_infer")
    D = depth_values.shape[0]
    # the library's own answers first, with its status: the shape domain (1, 2), then a workspace that is too small (3)
    key = (N, C, D, h, w, dtype)
    need = _workspace_bytes.get(key)
    if need is None:      # a refusal raises and is asked again next time; an answer is kept: one dict lookup per map
        need = _workspace_bytes[key] = query_workspace(*key)
    _check_workspace(workspace, dev, "depth_infer")
    if workspace.numel() < need:
        raise MvsError(3, f"workspace needs >= {need} bytes, got {workspace.numel()}")
    proj, depth_values = _depth_call_args("depth_infer", dev, N, h, w, proj, depth_values, blob, workspace, depth_out,
                                          conf_out)
    with torch.cuda.device(dev):
        check(load().mvs_depth_infer(feats.data_ptr(), proj.data_ptr(), depth_values.data_ptr(),
                                     blob.data_ptr(), depth_out.data_ptr(), conf_out.data_ptr(),
                                     workspace.data_ptr(), workspace.numel(), N, C, D, h, w, dtype,
                                     _stream(dev)))


def _view_ids_arg(view_ids):
    """view_ids (a sequence of ints or a CPU integer tensor) -> contiguous host int32 array [N].  A tensor
    on another device is refused: reading it here would synchronise with that device."""
    import numpy as np
    if isinstance(view_ids, torch.Tensor):
        if view_ids.device.type != "cpu":
            raise RuntimeError(f"view_ids must be a host sequence or a CPU tensor (got a tensor on {view_ids.device}): "
                               "the view table travels in the kernel arguments, reading device memory would sync")
        if view_ids.is_floating_point() or view_ids.is_complex():
            raise RuntimeError(f"view_ids must be integers, got {view_ids.dtype}")
        view_ids = view_ids.numpy()
    ids = np.asarray(view_ids)
    if ids.ndim != 1 or ids.size < 1 or ids.dtype.kind not in "iu":
        raise RuntimeError(f"view_ids must be a non-empty 1-D sequence of integers, got shape {ids.shape} "
                           f"dtype {ids.dtype}")
    if ids.min() < np.iinfo(np.int32).min or ids.max() > np.iinfo(np.int32).max:
        raise RuntimeError("view_ids do not fit int32")
    return np.ascontiguousarray(ids, dtype=np.int32)


def depth_infer_views(feats, view_ids, proj, depth_values, blob, workspace, depth_out, conf_out, dtype=MVS_F32):
    """depth_infer with the N views picked from a bank: feats [V,32,h,w] fp32 (any V), view_ids [N] host ints
    (entry 0 = reference view; repeats allowed; the library rejects any outside [0, V)), proj [N,4,4] in
    view_ids order, depth_values [D]; outputs are written into depth_out / conf_out [h,w]."""
    ids = _view_ids_arg(view_ids)
    N = ids.shape[0]
    if feats.dim() != 4 or feats.shape[1] != 32:
        raise RuntimeError(f"depth_infer_views: feats must be [V,32,h,w], got {tuple(feats.shape)}")
    V, C, h, w = feats.shape
    if tuple(proj.shape) != (N, 4, 4):
        raise RuntimeError(f"depth_infer_views: proj must be [N,4,4] = [{N},4,4] for {N} view ids, got {tuple(proj.shape)}")
    if depth_values.dim() != 1:
        raise RuntimeError(f"depth_infer_views: depth_values must be [D], got {tuple(depth_values.shape)}")
    for name, t in (("depth_out", depth_out), ("conf_out", conf_out)):
        if tuple(t.shape) != (h, w) or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"depth_infer_views: {name} must be a contiguous float32 [{h},{w}] tensor, "
                               f"got {t.dtype} {tuple(t.shape)}")
    feats = _dev_f32(feats, "features")
    dev = feats.device
    proj, depth_values = _depth_call_args("depth_infer_views", dev, N, h, w, proj, depth_values, blob, workspace,
                                          depth_out, conf_out)
    D = depth_values.shape[0]
    with torch.cuda.device(dev):
        check(load().mvs_depth_infer_views(feats.data_ptr(), V, ids.ctypes.data, proj.data_ptr(), depth_values.data_ptr(),
                                           blob.data_ptr(), depth_out.data_ptr(), conf_out.data_ptr(),
                                           workspace.data_ptr(), workspace.numel(), N, C, D, h, w, dtype,
                                           _stream(dev)))


def alloc_workspace(N, C, D, h, w, device, dtype=MVS_F32) -> torch.Tensor:
    nbytes = query_workspace(N, C, D, h, w, dtype)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def to_c8(t: torch.Tensor) -> torch.Tensor:
    """[C,D,h,w] (reference layout, one batch item) -> C8-planar [C/8,D,h,w,8]."""
    C = t.shape[0]
    return t.reshape(C // 8, 8, *t.shape[1:]).permute(0, 2, 3, 4, 1).contiguous()


def from_c8(t: torch.Tensor) -> torch.Tensor:
    """C8-planar [C/8,D,h,w,8] -> [C,D,h,w]."""
    P, D, h, w, _ = t.shape
    return t.permute(0, 4, 1, 2, 3).reshape(P * 8, D, h, w).contiguous()


FILTER_REF_FLOATS, FILTER_PAIR_FLOATS = 30, 42


def filter_compose(intrinsics, extrinsics, ref_idx, src_idx):
    """Host-side float32 camera products for mvs_filter_depth (numpy arrays in / out).

    intrinsics [V,3,3], extrinsics [V,4,4] float32; ref_idx [R] int32; src_idx [R,S] int32 (-1 pad).
    """
    import numpy as np
    K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 9)
    E = np.ascontiguousarray(extrinsics, np.float32).reshape(-1, 16)
    ref = np.ascontiguousarray(ref_idx, np.int32)
    src = np.ascontiguousarray(src_idx, np.int32)
    if K.shape[0] != E.shape[0] or src.ndim != 2 or src.shape[0] != ref.shape[0]:
        raise RuntimeError(f"filter_compose: inconsistent shapes K{K.shape} E{E.shape} ref{ref.shape} src{src.shape}")
    V, R, S = K.shape[0], ref.shape[0], src.shape[1]
    ref_mats = np.empty((R, FILTER_REF_FLOATS), np.float32)
    pair_mats = np.empty((R, S, FILTER_PAIR_FLOATS), np.float32)
    check(load().mvs_filter_compose(K.ctypes.data, E.ctypes.data, ref.ctypes.data, src.ctypes.data,
                                    V, R, S, ref_mats.ctypes.data, pair_mats.ctypes.data))
    return ref_mats, pair_mats


def filter_depth(depth, conf, ref_mats, pair_mats, ref_idx, src_idx, photomask=0.8, geomask=3,
                 condmask_pixel=1.0, condmask_depth=0.01):
    """Device tensors in, device tensors out: geo_sum int32 [R,h,w], depth_avg float64 [R,h,w],
    masks uint8 [R,3,h,w] (photo, geo, final), xyz_world float64 [R,h*w,3]."""
    depth = _dev_f32(depth, "depth")
    conf = _dev_f32(conf, "conf")
    dev = depth.device
    if depth.dim() != 3 or conf.shape != depth.shape:
        raise RuntimeError(f"filter_depth: depth {tuple(depth.shape)} / conf {tuple(conf.shape)} must both be [V,h,w]")
    V, h, w = depth.shape
    ref_mats = _dev_f32(ref_mats, "ref_mats")
    pair_mats = _dev_f32(pair_mats, "pair_mats")
    if ref_idx.dtype != torch.int32 or src_idx.dtype != torch.int32 or not ref_idx.is_cuda or not src_idx.is_cuda:
        raise RuntimeError("filter_depth: ref_idx / src_idx must be int32 tensors on the GPU")
    if any(t.device != dev for t in (conf, ref_mats, pair_mats, ref_idx, src_idx)):
        raise RuntimeError("filter_depth: depth, conf, ref_mats, pair_mats, ref_idx and src_idx must be on one device")
    if src_idx.dim() != 2:
        raise RuntimeError(f"filter_depth: src_idx must be [R,S], got {list(src_idx.shape)}")
    R, S = src_idx.shape
    if tuple(ref_mats.shape) != (R, FILTER_REF_FLOATS) or tuple(pair_mats.shape) != (R, S, FILTER_PAIR_FLOATS) \
            or ref_idx.numel() != R:
        raise RuntimeError("filter_depth: ref_mats / pair_mats / ref_idx do not match src_idx's [R,S]")
    ref_idx, src_idx = ref_idx.contiguous(), src_idx.contiguous()
    with torch.cuda.device(dev):
        geo = torch.empty((R, h, w), dtype=torch.int32, device=dev)
        avg = torch.empty((R, h, w), dtype=torch.float64, device=dev)
        masks = torch.empty((R, 3, h, w), dtype=torch.uint8, device=dev)
        xyz = torch.empty((R, h * w, 3), dtype=torch.float64, device=dev)
        check(load().mvs_filter_depth(depth.data_ptr(), conf.data_ptr(), ref_mats.data_ptr(),
                                      pair_mats.data_ptr(), ref_idx.data_ptr(), src_idx.data_ptr(),
                                      V, R, S, h, w, float(photomask), int(geomask), float(condmask_pixel),
                                      float(condmask_depth), geo.data_ptr(), avg.data_ptr(), masks.data_ptr(),
                                      xyz.data_ptr(), _stream(dev)))
    return geo, avg, masks, xyz


# ---- the cloud path: what its wrappers share ---------------------------------------------------
MVS_CLOUD_F32, MVS_CLOUD_F64 = 0, 1


def _outputs(who, dev, specs, out):
    """The tensors a wrapper's results go to, one per entry of `specs` = [(name, shape, dtype, wanted)], in the order of
    its `out` tuple.  Without `out` they are allocated here (None where not wanted); otherwise `out` is unpacked and each
    tensor that is present is checked against its entry.  Called inside `with torch.cuda.device(dev)`, before the
    workspace is allocated."""
    if out is None:
        return [torch.empty(shape, dtype=dtype, device=dev) if wanted else None for _, shape, dtype, wanted in specs]
    out = list(out)
    if len(out) != len(specs):
        raise ValueError(f"{who}: out must hold ({', '.join(s[0] for s in specs)}), got {len(out)} entries")
    for t, (name, shape, dtype, _) in zip(out, specs):
        if t is not None:
            _check_out(t, shape, dtype, dev, f"{who}: out {name}", f"{dtype} {shape} tensor on {dev}")
    return out


def _cloud_xyz(xyz, who):
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError(f"{who}: xyz must be a CUDA(ROCm) tensor; there is no CPU implementation")
    if xyz.dtype not in (torch.float32, torch.float64) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError(f"{who}: xyz must be float32 or float64 [P,3], got {xyz.dtype} {tuple(xyz.shape)}")
    return xyz.contiguous()


def _cloud_rows(t, name, dtype, P, dev, who):
    """What travels with xyz, one row per point (rgb, normals): a `dtype` [P,3] tensor on xyz's device."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA(ROCm) tensor; there is no CPU implementation")
    if t.device != dev:
        raise RuntimeError(f"{who}: xyz and {name} must be on one device")
    if t.dtype != dtype or tuple(t.shape) != (P, 3):
        raise RuntimeError(f"{who}: {name} must be {str(dtype)[6:]} [P,3] = [{P},3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _xyz_code(t):
    return MVS_CLOUD_F64 if t.dtype == torch.float64 else MVS_CLOUD_F32


def _box_arg(box_min, box_max, who):
    """Two host triples -> two ctypes double[3] (the library reads them before it returns)."""
    out = []
    for name, b in (("box_min", box_min), ("box_max", box_max)):
        if isinstance(b, torch.Tensor):
            if b.device.type != "cpu":
                raise RuntimeError(f"{who}: {name} must be host numbers (got a tensor on {b.device}): the box travels in "
                                   "the kernel arguments, reading device memory would sync")
            b = b.tolist()
        b = [float(x) for x in b]
        if len(b) != 3:
            raise RuntimeError(f"{who}: {name} must hold 3 numbers, got {len(b)}")
        out.append((_d * 3)(*b))
    return out


def _box_query(symbol, who, *counts, box_min, box_max, edge) -> int:
    """The bytes `symbol` asks for: a workspace query over the grid of a box, after its point counts."""
    lo, hi = _box_arg(box_min, box_max, who)
    return _query(symbol, *(int(c) for c in counts), lo, hi, float(edge))


# ---- fused point cloud (include/mvs_fuse_abi.h, csrc/fuse_points.hip) -------------------------
FUSE_TILE, FUSE_SCAN_WIDTH = 1024, 1024     # MVS_FUSE_TILE, MVS_FUSE_SCAN_WIDTH


def query_fuse_workspace(R, h, w) -> int:
    return _query("mvs_query_fuse_workspace", R, h, w)


def fuse_points(xyz_world, masks, images, ref_idx, capacity=None, out=None):
    """The selected points of every reference view, in order, with their colours (eval.py:745-758), on the device.

    xyz_world float64 [R,h*w,3] and masks uint8 or bool [R,3,h,w] as filter_depth returns them (plane 2 selects);
    images uint8 [V,3,4h,4w] or [V,4h,4w,3]; ref_idx int32 [R], the image of each reference view.  Returns
    (xyz float32 [capacity,3], rgb uint8 [capacity,3], counts int32 [R+1]: per view, then the total), all on the
    device; rows at and beyond the total are not written.  capacity defaults to R*h*w, which always suffices; with
    less, the first `capacity` points are written and counts stays exact.  `out` = (xyz, rgb, counts) receives the
    results.  Enqueued on the current stream; nothing synchronises."""
    for name, t in (("xyz_world", xyz_world), ("masks", masks), ("images", images), ("ref_idx", ref_idx)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"fuse_points: {name} must be a CUDA(ROCm) tensor; there is no CPU implementation")
    dev = xyz_world.device
    if any(t.device != dev for t in (masks, images, ref_idx)):
        raise RuntimeError("fuse_points: xyz_world, masks, images and ref_idx must be on one device")
    if masks.dtype == torch.bool:
        masks = masks.contiguous().view(torch.uint8)      # one byte each, 0 / 1
    if masks.dtype != torch.uint8 or masks.dim() != 4 or masks.shape[1] != 3:
        raise RuntimeError(f"fuse_points: masks must be uint8 or bool [R,3,h,w], got {masks.dtype} {tuple(masks.shape)}")
    R, _, h, w = masks.shape
    if xyz_world.dtype != torch.float64 or tuple(xyz_world.shape) != (R, h * w, 3):
        raise RuntimeError(f"fuse_points: xyz_world must be float64 [R,h*w,3] = [{R},{h * w},3], got {xyz_world.dtype} "
                           f"{tuple(xyz_world.shape)}")
    if images.dtype != torch.uint8:
        raise RuntimeError(f"fuse_points: images must be uint8 (the colours are copied bytes), got {images.dtype}")
    images, fmt, V, H, W = _image_arg(images, "fuse_points")
    if (H, W) != (4 * h, 4 * w):
        raise RuntimeError(f"fuse_points: images are {H}x{W}, the maps {h}x{w}: incompatible depth and image dimensions.")
    if ref_idx.dtype != torch.int32 or tuple(ref_idx.shape) != (R,):
        raise RuntimeError(f"fuse_points: ref_idx must be int32 [{R}], got {ref_idx.dtype} {tuple(ref_idx.shape)}")
    capacity = R * h * w if capacity is None else int(capacity)
    if capacity < 0:
        raise RuntimeError(f"fuse_points: capacity {capacity} is negative")
    xyz_world, masks, ref_idx = xyz_world.contiguous(), masks.contiguous(), ref_idx.contiguous()
    with torch.cuda.device(dev):
        xyz, rgb, counts = _outputs("fuse_points", dev, [("xyz", (capacity, 3), torch.float32, True),
                                                         ("rgb", (capacity, 3), torch.uint8, True),
                                                         ("counts", (R + 1,), torch.int32, True)], out)
        ws = torch.empty(query_fuse_workspace(R, h, w), dtype=torch.uint8, device=dev)
        check(load().mvs_fuse_points(xyz_world.data_ptr(), masks.data_ptr(), images.data_ptr(), fmt, ref_idx.data_ptr(),
                                     V, R, h, w, capacity, xyz.data_ptr() if capacity else None,
                                     rgb.data_ptr() if capacity else None, counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream(dev)))
    return xyz, rgb, counts


# ---- crop + voxel downsample of a cloud (include/mvs_cloud_abi.h, csrc/cloud_downsample.hip), and the one that also
# ---- carries the points' normals (include/mvs_normals_abi.h) ----
CLOUD_CHUNK, CLOUD_TILE, CLOUD_SCAN_WIDTH, CLOUD_RECORD = 1024, 1024, 1024, 64     # the header's MVS_CLOUD_* sizes


def query_cloud_workspace(P, box_min, box_max, voxel_size) -> int:
    return _box_query("mvs_query_cloud_workspace", "query_cloud_workspace", P, box_min=box_min, box_max=box_max,
                      edge=voxel_size)


def query_cloud_normals_downsample_workspace(P, box_min, box_max, voxel_size) -> int:
    return _box_query("mvs_query_cloud_normals_downsample_workspace", "query_cloud_normals_downsample_workspace", P,
                      box_min=box_min, box_max=box_max, edge=voxel_size)


def _downsample(who, xyz, rgb, normals, box_min, box_max, voxel_size, scale, capacity, out):
    """Both downsamples: `normals` is None for the plain one, whose entry point, `out` and result lack the normals."""
    xyz = _cloud_xyz(xyz, who)
    dev, P = xyz.device, xyz.shape[0]
    carried = [_cloud_rows(rgb, "rgb", torch.uint8, P, dev, who)]
    if normals is not None:
        carried.append(_cloud_rows(normals, "normals", torch.float32, P, dev, who))
    lo, hi = _box_arg(box_min, box_max, who)
    capacity = P if capacity is None else int(capacity)
    if capacity < 0:
        raise RuntimeError(f"{who}: capacity {capacity} is negative")
    symbol = "mvs_cloud_downsample" if normals is None else "mvs_cloud_downsample_normals"
    nbytes = _box_query("mvs_query_cloud_workspace" if normals is None else "mvs_query_cloud_normals_downsample_workspace",
                        who, P, box_min=lo, box_max=hi, edge=voxel_size)
    with torch.cuda.device(dev):
        specs = [("xyz", (capacity, 3), torch.float32, True), ("rgb", (capacity, 3), torch.uint8, True),
                 ("normals", (capacity, 3), torch.float32, True)][:1 + len(carried)]
        *means, counts = _outputs(who, dev, specs + [("counts", (2,), torch.int64, True)], out)
        if P == 0:          # an empty tensor has no address to hand over: the two zero counts of the header's P == 0
            counts.zero_()
            return (*means, counts)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(getattr(load(), symbol)(xyz.data_ptr(), _xyz_code(xyz), *(t.data_ptr() for t in carried), P, lo, hi,
                                      float(voxel_size), float(scale), capacity,
                                      *(t.data_ptr() if capacity else None for t in means), counts.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream(dev)))
    return (*means, counts)


def cloud_downsample(xyz, rgb, box_min, box_max, voxel_size, scale=1.0, capacity=None, out=None):
    """Crop a coloured cloud to a box and keep the mean point and colour of every occupied voxel (the reference's
    pcd.crop / voxel_down_sample / scale, eval.py:831-840, as include/mvs_cloud_abi.h defines them), on the device.

    xyz float32 or float64 [P,3] and rgb uint8 [P,3] on one device; box_min, box_max: 3 host numbers each.  Returns
    (xyz float32 [capacity,3], rgb uint8 [capacity,3], counts int64 [2]: kept points, occupied voxels), all on the
    device, voxels in ascending (iz, iy, ix); rows at and beyond counts[1] are not written.  capacity defaults to P,
    which always suffices; with less, the first `capacity` voxels are written and counts stays exact.  `out` =
    (xyz, rgb, counts) receives the results.  Enqueued on the current stream; nothing synchronises."""
    return _downsample("cloud_downsample", xyz, rgb, None, box_min, box_max, voxel_size, scale, capacity, out)


def cloud_downsample_normals(xyz, rgb, normals, box_min, box_max, voxel_size, scale=1.0, capacity=None, out=None):
    """cloud_downsample that also carries the points' normals: returns (xyz float32 [capacity,3], rgb uint8 [capacity,3],
    normals float32 [capacity,3]: the mean of each voxel's normals, not renormalised, counts int64 [2]).  The first, second
    and last are byte for byte what cloud_downsample returns.  normals float32 [P,3] on xyz's device.  `out` = (xyz, rgb,
    normals, counts).  Enqueued on the current stream; nothing synchronises."""
    if normals is None:
        raise RuntimeError("cloud_downsample_normals: normals must be a CUDA(ROCm) tensor; there is no CPU implementation")
    return _downsample("cloud_downsample_normals", xyz, rgb, normals, box_min, box_max, voxel_size, scale, capacity, out)


# ---- point normals (include/mvs_normals_abi.h, csrc/cloud_normals.hip) ----
NORMALS_KNN_MAX, NORMALS_TILE = 64, 1024     # MVS_NORMALS_KNN_MAX, MVS_NORMALS_TILE


def query_normals_workspace(P, box_min, box_max, cell) -> int:
    return _box_query("mvs_query_normals_workspace", "query_normals_workspace", P, box_min=box_min, box_max=box_max, edge=cell)


def cloud_normals(xyz, box_min, box_max, cell=5.0, knn=30, view_starts=None, centres=None, neighbours=False, out=None):
    """A normal for every point of the cloud inside the box from its `knn` nearest neighbours there (the reference's
    pcd.estimate_normals(), eval.py:817, as include/mvs_normals_abi.h defines it), on the device.

    xyz float32 or float64 [P,3]; box_min, box_max: 3 host numbers each; cell: the search grid's cell edge (it changes the
    time, never the result).  view_starts int64 [R+1] and centres float64 [R,3], both on the device or both None: the
    normals of points view_starts[r] .. view_starts[r+1]-1 are turned towards centres[r].  Returns (normals float32 [P,3],
    neighbours int32 [P,knn] or None, counts int64 [3]: members, members with an estimated normal, members an outside
    point could have served better), all on the device.  `out` = (normals, neighbours or None, counts) receives the
    results.  Enqueued on the current stream; nothing synchronises."""
    xyz = _cloud_xyz(xyz, "cloud_normals")
    dev = xyz.device
    P, knn = xyz.shape[0], int(knn)
    lo, hi = _box_arg(box_min, box_max, "cloud_normals")
    if (view_starts is None) != (centres is None):
        raise RuntimeError("cloud_normals: view_starts and centres must both be given or both be None")
    R = 0
    if view_starts is not None:
        R = view_starts.shape[0] - 1 if isinstance(view_starts, torch.Tensor) and view_starts.dim() == 1 else -1
        if R < 1 or view_starts.dtype != torch.int64 or view_starts.device != dev:
            raise RuntimeError("cloud_normals: view_starts must be an int64 [R+1] tensor, R >= 1, on xyz's device")
        if not isinstance(centres, torch.Tensor) or centres.dtype != torch.float64 or tuple(centres.shape) != (R, 3) \
                or centres.device != dev:
            raise RuntimeError(f"cloud_normals: centres must be a float64 [R,3] = [{R},3] tensor on xyz's device")
        view_starts, centres = view_starts.contiguous(), centres.contiguous()
    nbytes = _box_query("mvs_query_normals_workspace", "cloud_normals", P, box_min=lo, box_max=hi, edge=cell)
    with torch.cuda.device(dev):
        normals, nbr, counts = _outputs("cloud_normals", dev, [("normals", (P, 3), torch.float32, True),
                                                               ("neighbours", (P, knn), torch.int32, neighbours),
                                                               ("counts", (3,), torch.int64, True)], out)
        if P == 0:          # an empty tensor has no address to hand over: the three zero counts of the header's P == 0
            if not 3 <= knn <= NORMALS_KNN_MAX:
                raise RuntimeError(f"cloud_normals: knn = {knn} (need 3 <= knn <= {NORMALS_KNN_MAX})")
            counts.zero_()
            return normals, nbr, counts
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(load().mvs_cloud_normals(xyz.data_ptr(), _xyz_code(xyz), P, lo, hi, float(cell), knn,
                                       view_starts.data_ptr() if R else None, centres.data_ptr() if R else None, R,
                                       normals.data_ptr(), None if nbr is None else nbr.data_ptr(), counts.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _stream(dev)))
    return normals, nbr, counts


# ---- statistical outlier removal (include/mvs_outliers_abi.h, csrc/cloud_outliers.hip) ----
OUTLIERS_BLOCK, OUTLIERS_SCALARS = 1024, 64     # MVS_OUTLIERS_BLOCK, MVS_OUTLIERS_SCALARS


def query_outliers_workspace(P, box_min, box_max, cell) -> int:
    return _box_query("mvs_query_outliers_workspace", "query_outliers_workspace", P, box_min=box_min, box_max=box_max,
                      edge=cell)


def cloud_outliers(xyz, box_min, box_max, cell=5.0, nb_neighbors=20, std_ratio=2.0, masked=False, out=None):
    """Statistical outlier removal among the points of the cloud inside the box (the reference's
    pcd.remove_statistical_outlier(), eval.py:495, as include/mvs_outliers_abi.h defines it), on the device.

    xyz float32 or float64 [P,3]; box_min, box_max: 3 host numbers each; cell: the search grid's cell edge (it changes the
    time, never the result).  Returns (dist float64 [P]: the mean distance to the nb_neighbors nearest points inside the box,
    -1 outside it, keep bool [P]: True where dist is positive and below mean + std_ratio * std, xyz_masked of xyz's dtype
    [P,3] or None: the kept points, NaN elsewhere, counts int64 [3]: points inside the box, valid ones, kept ones, stats
    float64 [3]: mean, std, threshold), all on the device.  `out` = (dist, keep, xyz_masked or None, counts, stats)
    receives the results.  Enqueued on the current stream; nothing synchronises."""
    xyz = _cloud_xyz(xyz, "cloud_outliers")
    dev = xyz.device
    P, nb, ratio = xyz.shape[0], int(nb_neighbors), float(std_ratio)
    lo, hi = _box_arg(box_min, box_max, "cloud_outliers")
    nbytes = _box_query("mvs_query_outliers_workspace", "cloud_outliers", P, box_min=lo, box_max=hi, edge=cell)
    with torch.cuda.device(dev):
        dist, keep, xyz_masked, counts, stats = _outputs("cloud_outliers", dev, [
            ("dist", (P,), torch.float64, True), ("keep", (P,), torch.bool, True),      # the library writes bytes 0 and 1
            ("xyz_masked", (P, 3), xyz.dtype, masked), ("counts", (3,), torch.int64, True),
            ("stats", (3,), torch.float64, True)], out)
        if out is not None and xyz_masked is not None and P and xyz_masked.data_ptr() == xyz.data_ptr():
            raise RuntimeError("cloud_outliers: out xyz_masked must not alias xyz")
        if P == 0:          # an empty tensor has no address to hand over: the zeros of the header's P == 0
            if not 2 <= nb <= NORMALS_KNN_MAX:
                raise RuntimeError(f"cloud_outliers: nb_neighbors = {nb} (need 2 <= nb_neighbors <= {NORMALS_KNN_MAX})")
            if not (0.0 < ratio < float("inf")):
                raise RuntimeError(f"cloud_outliers: std_ratio = {ratio} (need a finite ratio > 0)")
            counts.zero_()
            stats.zero_()
            return dist, keep, xyz_masked, counts, stats
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(load().mvs_cloud_outliers(xyz.data_ptr(), _xyz_code(xyz), P, lo, hi, float(cell), nb, ratio, dist.data_ptr(),
                                        keep.data_ptr(), None if xyz_masked is None else xyz_masked.data_ptr(),
                                        counts.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return dist, keep, xyz_masked, counts, stats


# ---- cloud-to-cloud distance (include/mvs_distance_abi.h, csrc/cloud_distance.hip) ----
DISTANCE_THRESHOLDS_MAX, DISTANCE_SCALARS = 8, 64     # MVS_DISTANCE_THRESHOLDS_MAX, MVS_DISTANCE_SCALARS


def query_distance_workspace(P, N, box_min, box_max, cell) -> int:
    return _box_query("mvs_query_distance_workspace", "query_distance_workspace", P, N, box_min=box_min, box_max=box_max,
                      edge=cell)


def cloud_distance(ref, query, box_min, box_max, cell, max_dist, thresholds, indices=False, out=None):
    """The distance from every point of `query` to the nearest point of `ref` inside the box, its counts and its mean
    (one direction of accuracy / completeness, as include/mvs_distance_abi.h defines it), on the device.

    ref float32 or float64 [P,3] and query float32 or float64 [N,3] on one device (they may be the same tensor); box_min,
    box_max: 3 host numbers each, the box of `ref`; cell: the search grid's cell edge (it changes the time, never the
    result); max_dist >= 0, +inf allowed; thresholds: up to 8 finite host numbers >= 0.  Returns (dist float64 [N]: the
    distance, +inf where no point of `ref` in the box lies within max_dist, -1 for a query with a non-finite coordinate,
    idx int32 [N] or None: the nearest point's row in `ref`, -1 where there is none, counts int64 [2 + T]: queries with
    finite coordinates, those within max_dist, those below each threshold, stats float64 [2]: the sum of the distances
    within max_dist and their mean), all on the device.  `out` = (dist, idx or None, counts, stats) receives the results.
    Enqueued on the current stream; nothing synchronises."""
    import numpy as np
    ref, query = _cloud_xyz(ref, "cloud_distance"), _cloud_xyz(query, "cloud_distance")
    dev = ref.device
    if query.device != dev:
        raise RuntimeError("cloud_distance: ref and query must be on one device")
    P, N, cap = ref.shape[0], query.shape[0], float(max_dist)
    th = np.ascontiguousarray([float(t) for t in thresholds], dtype=np.float64)
    T = int(th.size)
    if T > DISTANCE_THRESHOLDS_MAX:
        raise RuntimeError(f"cloud_distance: {T} thresholds (at most {DISTANCE_THRESHOLDS_MAX})")
    if not cap >= 0.0:
        raise RuntimeError(f"cloud_distance: max_dist = {cap} (need max_dist >= 0; +inf is allowed)")
    if T and not (np.isfinite(th).all() and (th >= 0).all()):
        raise RuntimeError(f"cloud_distance: thresholds {th.tolist()} (need finite thresholds >= 0)")
    lo, hi = _box_arg(box_min, box_max, "cloud_distance")
    nbytes = _box_query("mvs_query_distance_workspace", "cloud_distance", P, N, box_min=lo, box_max=hi, edge=cell)
    with torch.cuda.device(dev):
        dist, idx, counts, stats = _outputs("cloud_distance", dev, [
            ("dist", (N,), torch.float64, True), ("idx", (N,), torch.int32, indices),
            ("counts", (2 + T,), torch.int64, True), ("stats", (2,), torch.float64, True)], out)
        if N == 0:          # an empty tensor has no address to hand over: the zeros of the header's N == 0
            counts.zero_()
            stats.zero_()
            return dist, idx, counts, stats
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # P == 0: the library does not read ref; it gets the workspace's address in place of an empty tensor's
        check(load().mvs_cloud_distance(ref.data_ptr() if P else ws.data_ptr(), _xyz_code(ref), P, query.data_ptr(),
                                        _xyz_code(query), N, lo, hi, float(cell), cap, th.ctypes.data if T else None, T,
                                        dist.data_ptr(), None if idx is None else idx.data_ptr(), counts.data_ptr(),
                                        stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return dist, idx, counts, stats


# ---- DTU's point reduction, observability mask and plane (include/mvs_reduce_abi.h, csrc/cloud_reduce.hip) ----
REDUCE_ROUNDS_MAX = 256     # MVS_REDUCE_ROUNDS_MAX


def query_reduce_workspace(P, box_min, box_max, cell) -> int:
    return _box_query("mvs_query_reduce_workspace", "query_reduce_workspace", P, box_min=box_min, box_max=box_max, edge=cell)


def cloud_reduce(xyz, box_min, box_max, cell, min_dist, seed=0, max_rounds=64, out=None):
    """Thin the points of the cloud inside the box so that no two kept points lie within min_dist of each other: the
    greedy pass of DTU's reducePts in the order of a hash of (seed, index), as include/mvs_reduce_abi.h defines it, on the
    device.

    xyz float32 or float64 [P,3]; box_min, box_max: 3 host numbers each; cell: the search grid's cell edge (it changes the
    time, never the result); min_dist finite and >= 0; seed an integer modulo 2^64; max_rounds in [1, 256].  Returns
    (keep bool [P], counts int64 [4]: members, kept, undecided after max_rounds, rounds), both on the device; the mask is
    the greedy result iff undecided == 0.  `out` = (keep, counts) receives the results.  Enqueued on the current stream;
    nothing synchronises."""
    xyz = _cloud_xyz(xyz, "cloud_reduce")
    dev = xyz.device
    P, dist, rounds = xyz.shape[0], float(min_dist), int(max_rounds)
    if not (0.0 <= dist < float("inf")):
        raise RuntimeError(f"cloud_reduce: min_dist = {dist} (need a finite min_dist >= 0)")
    if not 1 <= rounds <= REDUCE_ROUNDS_MAX:
        raise RuntimeError(f"cloud_reduce: max_rounds = {rounds} (need 1 <= max_rounds <= {REDUCE_ROUNDS_MAX})")
    lo, hi = _box_arg(box_min, box_max, "cloud_reduce")
    nbytes = _box_query("mvs_query_reduce_workspace", "cloud_reduce", P, box_min=lo, box_max=hi, edge=cell)
    with torch.cuda.device(dev):
        keep, counts = _outputs("cloud_reduce", dev, [("keep", (P,), torch.bool, True),      # the library writes bytes 0 and 1
                                                      ("counts", (4,), torch.int64, True)], out)
        if P == 0:          # an empty tensor has no address to hand over: the four zero counts of the header's P == 0
            counts.zero_()
            return keep, counts
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(load().mvs_cloud_reduce(xyz.data_ptr(), _xyz_code(xyz), P, lo, hi, float(cell), dist,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, rounds, keep.data_ptr(), counts.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream(dev)))
    return keep, counts


def cloud_select(xyz, mask=None, origin=None, res=1.0, plane=None, out=None):
    """DTU's two per-point filters (include/mvs_reduce_abi.h), on the device: is the voxel of the point -- the one whose
    centre origin + g * res is nearest, halves away from zero -- set in `mask` (uint8 or bool [n0,n1,n2] on xyz's device,
    or None: no test), and is ((plane[0] x + plane[1] y) + plane[2] z) + plane[3] > 0 (4 host numbers, or None: no test).

    Returns (keep bool [P]: the conjunction of the tests asked for, False for a non-finite point, counts int64 [3]: finite
    points, observed ones, kept ones), both on the device.  `out` = (keep, counts).  Enqueued on the current stream;
    nothing synchronises."""
    xyz = _cloud_xyz(xyz, "cloud_select")
    dev, P = xyz.device, xyz.shape[0]
    n = org = pl = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dim() != 3 \
                or mask.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError("cloud_select: mask must be a uint8 or bool [n0,n1,n2] tensor on xyz's device")
        if origin is None or len(origin) != 3:
            raise RuntimeError("cloud_select: a mask needs origin, 3 host numbers")
        mask = mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)      # one byte each, 0 / 1
        if mask.numel() == 0:
            raise RuntimeError(f"cloud_select: the mask is empty: {tuple(mask.shape)}")
        n = (_i * 3)(*mask.shape)
        org = (_d * 3)(*(float(v) for v in origin))
    if plane is not None:
        if len(plane) != 4:
            raise RuntimeError(f"cloud_select: plane must hold 4 numbers, got {len(plane)}")
        pl = (_d * 4)(*(float(v) for v in plane))
    with torch.cuda.device(dev):
        keep, counts = _outputs("cloud_select", dev, [("keep", (P,), torch.bool, True),      # the library writes bytes 0 and 1
                                                      ("counts", (3,), torch.int64, True)], out)
        if P == 0:          # an empty tensor has no address to hand over: the three zero counts of the header's P == 0
            counts.zero_()
            return keep, counts
        check(load().mvs_cloud_select(xyz.data_ptr(), _xyz_code(xyz), P, None if mask is None else mask.data_ptr(),
                                      None if n is None else ctypes.addressof(n),
                                      None if org is None else ctypes.addressof(org), float(res),
                                      None if pl is None else ctypes.addressof(pl), keep.data_ptr(), counts.data_ptr(),
                                      _stream(dev)))
    return keep, counts


# ---- density-connected components (include/mvs_cluster_abi.h, csrc/cloud_cluster.hip) ----
def query_cluster_workspace(P, box_min, box_max, cell) -> int:
    return _box_query("mvs_query_cluster_workspace", "query_cluster_workspace", P, box_min=box_min, box_max=box_max, edge=cell)


def cloud_cluster(xyz, box_min, box_max, cell, eps, min_points=10, min_size=1, out=None):
    """The density-connected components (DBSCAN) of the points of the cloud inside the box, numbered as the libraries'
    traversal in index order numbers them, and the mask of the clusters of at least min_size points, as
    include/mvs_cluster_abi.h defines them, on the device.

    xyz float32 or float64 [P,3]; box_min, box_max: 3 host numbers each; cell: the search grid's cell edge (it changes the
    time, never the result); eps finite and >= 0; min_points >= 1: the neighbours within eps, itself counted, of a core
    point; min_size >= 1.  Returns (labels int32 [P]: the cluster number, -1 noise, -2 outside the box, keep bool [P],
    counts int64 [7]: points inside the box, core, border, noise, clusters, kept points, size of the largest cluster), all
    on the device.  `out` = (labels, keep, counts) receives the results.  Enqueued on the current stream; nothing
    synchronises."""
    xyz = _cloud_xyz(xyz, "cloud_cluster")
    dev = xyz.device
    P, radius, min_points, min_size = xyz.shape[0], float(eps), int(min_points), int(min_size)
    if not (0.0 <= radius < float("inf")):
        raise RuntimeError(f"cloud_cluster: eps = {radius} (need a finite eps >= 0)")
    if not 1 <= min_points < 1 << 31:
        raise RuntimeError(f"cloud_cluster: min_points = {min_points} (need 1 <= min_points < 2^31)")
    if not 1 <= min_size < 1 << 31:
        raise RuntimeError(f"cloud_cluster: min_size = {min_size} (need 1 <= min_size < 2^31)")
    lo, hi = _box_arg(box_min, box_max, "cloud_cluster")
    nbytes = _box_query("mvs_query_cluster_workspace", "cloud_cluster", P, box_min=lo, box_max=hi, edge=cell)
    with torch.cuda.device(dev):
        labels, keep, counts = _outputs("cloud_cluster", dev, [
            ("labels", (P,), torch.int32, True), ("keep", (P,), torch.bool, True),      # the library writes bytes 0 and 1
            ("counts", (7,), torch.int64, True)], out)
        if P == 0:          # an empty tensor has no address to hand over: the seven zero counts of the header's P == 0
            counts.zero_()
            return labels, keep, counts
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(load().mvs_cloud_cluster(xyz.data_ptr(), _xyz_code(xyz), P, lo, hi, float(cell), radius, min_points, min_size,
                                       labels.data_ptr(), keep.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(dev)))
    return labels, keep, counts


# ---- rigid registration, ICP (include/ext/mvs_register_abi.h, csrc/cloud_register.hip) ----
# MVS_REGISTER_ITERATIONS_MAX, _TERMS, _HISTORY, _GROUP, _FANIN, _SCALARS
REGISTER_ITERATIONS_MAX, REGISTER_TERMS, REGISTER_HISTORY, REGISTER_GROUP, REGISTER_FANIN, REGISTER_SCALARS = 1000, 31, 19, 32, 256, 512
REGISTER_STOPS = {1: "converged", 2: "max_iterations", 3: "degenerate"}     # MVS_REGISTER_STOP_*


def query_register_workspace(P, N, box_min, box_max, cell, max_iterations=30) -> int:
    lo, hi = _box_arg(box_min, box_max, "query_register_workspace")
    return _query("mvs_query_register_workspace", int(P), int(N), lo, hi, float(cell), int(max_iterations))


def cloud_register(target, source, box_min, box_max, cell, max_dist, target_normals=None, init=None, max_iterations=30,
                   rel_fitness=1e-6, rel_rmse=1e-6, history=False, systems=False, indices=False, out=None):
    """The rigid transform that lays `source` onto `target` by iterative closest point, with the semantics of Open3D's
    registration_icp (include/ext/mvs_register_abi.h), on the device.

    target float32 or float64 [P,3] and source float32 or float64 [N,3] on one device (they may be the same tensor);
    target_normals: [P,3] of target's dtype -> point-to-plane, None -> point-to-point; box_min, box_max: 3 host numbers
    each, the box of `target`; cell: the search grid's cell edge (it changes the time, never the result); max_dist >= 0,
    +inf allowed; init: 16 host numbers (4 x 4, row-major, last row 0 0 0 1) or None for the identity; rel_fitness,
    rel_rmse >= 0: the changes of fitness and rmse below which the loop stops.  Returns (transformation float64 [4,4],
    counts int64 [4]: counted sources, inliers, iterations run, stop reason (REGISTER_STOPS), stats float64 [2]: fitness
    and inlier rmse, history float64 [max_iterations + 1, 19] or None: T_k, fitness, rmse, inliers of every evaluation
    (NaN after the stop), systems float64 [max_iterations, 31] or None: the reduced sums of every step, idx int32 [N] or
    None: the target row of every source in the last evaluation, -1 for none), all on the device.  `out` = (the same six,
    None where not wanted) receives the results.  Enqueued on the current stream; nothing synchronises."""
    import math
    import numpy as np
    target, source = _cloud_xyz(target, "cloud_register"), _cloud_xyz(source, "cloud_register")
    dev = target.device
    if source.device != dev:
        raise RuntimeError("cloud_register: target and source must be on one device")
    P, N, cap, its = target.shape[0], source.shape[0], float(max_dist), int(max_iterations)
    if target_normals is not None:
        if P == 0:
            raise RuntimeError("cloud_register: target_normals of an empty target (pass None)")
        target_normals = _cloud_rows(target_normals, "target_normals", target.dtype, P, dev, "cloud_register")
    if not 0 <= its <= REGISTER_ITERATIONS_MAX:
        raise RuntimeError(f"cloud_register: max_iterations = {its} (need 0 <= max_iterations <= {REGISTER_ITERATIONS_MAX})")
    if not cap >= 0.0:
        raise RuntimeError(f"cloud_register: max_dist = {cap} (need max_dist >= 0; +inf is allowed)")
    rel_fitness, rel_rmse = float(rel_fitness), float(rel_rmse)
    if not (rel_fitness >= 0.0 and rel_rmse >= 0.0):
        raise RuntimeError(f"cloud_register: rel_fitness = {rel_fitness}, rel_rmse = {rel_rmse} (need both >= 0)")
    T0 = None
    if init is not None:
        if isinstance(init, torch.Tensor):
            if init.device.type != "cpu":
                raise RuntimeError(f"cloud_register: init must be host numbers (got a tensor on {init.device}): it travels "
                                   "in the kernel arguments, reading device memory would sync")
        flat = np.asarray(init, dtype=np.float64).reshape(-1).tolist()
        if len(flat) != 16 or not all(math.isfinite(x) for x in flat) or flat[12:] != [0.0, 0.0, 0.0, 1.0]:
            raise RuntimeError("cloud_register: init must be 16 finite numbers, a 4 x 4 matrix whose last row is 0 0 0 1")
        T0 = (_d * 16)(*flat)
    lo, hi = _box_arg(box_min, box_max, "cloud_register")
    nbytes = _query("mvs_query_register_workspace", P, N, lo, hi, float(cell), its)
    with torch.cuda.device(dev):
        T, counts, stats, hist, system, idx = _outputs("cloud_register", dev, [
            ("transformation", (4, 4), torch.float64, True), ("counts", (4,), torch.int64, True),
            ("stats", (2,), torch.float64, True), ("history", (its + 1, REGISTER_HISTORY), torch.float64, history),
            ("systems", (its, REGISTER_TERMS), torch.float64, systems), ("idx", (N,), torch.int32, indices)], out)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # P == 0, N == 0: the library does not read the empty cloud; it gets the workspace's address in place of an empty
        # tensor's.  An empty systems or idx tensor is not written either
        check(load().mvs_cloud_register(
            target.data_ptr() if P else ws.data_ptr(), _xyz_code(target), P,
            None if target_normals is None else target_normals.data_ptr(),
            source.data_ptr() if N else ws.data_ptr(), _xyz_code(source), N, lo, hi, float(cell), cap, T0, its, rel_fitness,
            rel_rmse, T.data_ptr(), counts.data_ptr(), stats.data_ptr(), None if hist is None else hist.data_ptr(),
            None if system is None or its == 0 else system.data_ptr(), None if idx is None or N == 0 else idx.data_ptr(),
            ws.data_ptr(), ws.numel(), _stream(dev)))
    return T, counts, stats, hist, system, idx


# ---- plane segmentation, RANSAC (include/ext/mvs_planes_abi.h, csrc/cloud_planes.hip) ----
# MVS_PLANES_CANDIDATES_MAX, _MAX, _SUMS, _TILE, _GROUP, _FANIN, _SCALARS
PLANES_CANDIDATES_MAX, PLANES_MAX, PLANES_SUMS, PLANES_TILE, PLANES_GROUP, PLANES_FANIN, PLANES_SCALARS = 8192, 64, 9, 1024, 256, 256, 512
PLANES_STOPS = {1: "max_planes", 2: "no_plane", 3: "exhausted"}     # MVS_PLANES_STOP_*


def query_planes_workspace(P, num_candidates, max_planes=1) -> int:
    return _query("mvs_query_planes_workspace", int(P), int(num_candidates), int(max_planes))


def cloud_planes(xyz, box_min, box_max, dist, num_candidates=1000, max_planes=1, min_inliers=3, seed=0, toward=None,
                 cand_counts=False, sums=False, out=None):
    """The dominant planes of the points of the cloud inside the box, one RANSAC round per plane over the points that have
    no plane yet (Open3D's segment_plane applied repeatedly, as include/ext/mvs_planes_abi.h defines it), on the device.

    xyz float32 or float64 [P,3]; box_min, box_max: 3 host numbers each; dist finite and >= 0: how far from a plane its
    points may lie; num_candidates in [1, 8192]: the planes through three points tried per round; max_planes in [1, 64];
    min_inliers >= 3: a round whose best candidate counts fewer ends the call; seed an integer modulo 2^64; toward: 3 host
    numbers, the side every normal is turned to, or None.  Returns (planes float64 [max_planes,4]: (n, d) with
    n . x + d = 0, NaN for the rounds that gave none, rounds int64 [max_planes,4]: active members, winning candidate, its
    count, final inliers, counts int64 [4]: points inside the box, planes found, points on planes, stop reason
    (PLANES_STOPS), labels int32 [P]: the plane's number, -1 on no plane, -2 outside the box, cand_counts int32
    [max_planes,num_candidates] or None, sums float64 [max_planes,9] or None), all on the device.  `out` = (the same six,
    None where not wanted) receives the results.  Enqueued on the current stream; nothing synchronises."""
    import math
    xyz = _cloud_xyz(xyz, "cloud_planes")
    dev = xyz.device
    P, t, K, rounds, least = xyz.shape[0], float(dist), int(num_candidates), int(max_planes), int(min_inliers)
    if not (0.0 <= t < float("inf")):
        raise RuntimeError(f"cloud_planes: dist = {t} (need a finite dist >= 0)")
    if not 1 <= K <= PLANES_CANDIDATES_MAX:
        raise RuntimeError(f"cloud_planes: num_candidates = {K} (need 1 <= num_candidates <= {PLANES_CANDIDATES_MAX})")
    if not 1 <= rounds <= PLANES_MAX:
        raise RuntimeError(f"cloud_planes: max_planes = {rounds} (need 1 <= max_planes <= {PLANES_MAX})")
    if not 3 <= least < 1 << 62:
        raise RuntimeError(f"cloud_planes: min_inliers = {least} (need min_inliers >= 3)")
    side = None
    if toward is not None:
        if isinstance(toward, torch.Tensor):
            if toward.device.type != "cpu":
                raise RuntimeError(f"cloud_planes: toward must be host numbers (got a tensor on {toward.device}): it travels "
                                   "in the kernel arguments, reading device memory would sync")
            toward = toward.tolist()
        flat = [float(v) for v in toward]
        if len(flat) != 3 or not all(math.isfinite(v) for v in flat):
            raise RuntimeError("cloud_planes: toward must be 3 finite numbers")
        side = (_d * 3)(*flat)
    lo, hi = _box_arg(box_min, box_max, "cloud_planes")
    nbytes = _query("mvs_query_planes_workspace", P, K, rounds)
    with torch.cuda.device(dev):
        planes, rnds, counts, labels, cand, sm = _outputs("cloud_planes", dev, [
            ("planes", (rounds, 4), torch.float64, True), ("rounds", (rounds, 4), torch.int64, True),
            ("counts", (4,), torch.int64, True), ("labels", (P,), torch.int32, True),
            ("cand_counts", (rounds, K), torch.int32, cand_counts), ("sums", (rounds, PLANES_SUMS), torch.float64, sums)], out)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # P == 0: the library reads no point and writes no label; it gets the workspace's address in place of the empty
        # tensors'
        check(load().mvs_cloud_planes(
            xyz.data_ptr() if P else ws.data_ptr(), _xyz_code(xyz), P, lo, hi, t, K, rounds, least,
            int(seed) & 0xFFFFFFFFFFFFFFFF, side, planes.data_ptr(), rnds.data_ptr(), counts.data_ptr(),
            labels.data_ptr() if P else ws.data_ptr(), None if cand is None else cand.data_ptr(),
            None if sm is None else sm.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return planes, rnds, counts, labels, cand, sm


# ---- FeatureNet (reference models/mvsnet.py:10-30) -------------------------------------------
# (cin, cout, k, stride) of conv0..conv6 and the final `feature` Conv2d
FEATURE_LAYERS = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1),
                  (16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 3, 1))
FEATURE_WEIGHT_KEYS = tuple([f"conv{i}.conv.weight" for i in range(7)] + ["feature.weight"])


def query_feature_blob() -> int:
    return _query("mvs_query_feature_blob")


def pack_feature_weights(state: dict, eps: float = 1e-5) -> torch.Tensor:
    """BN-fold + re-layout FeatureNet's parameters into MFMA panels (host, uint8).
    `state` maps names relative to `feature.` to CPU float32 tensors/arrays."""
    convs = [(key, (co, ci, k, k)) for key, (ci, co, k, _) in zip(FEATURE_WEIGHT_KEYS, FEATURE_LAYERS)]
    bns = [(f"conv{l}.bn.{suffix}", (FEATURE_LAYERS[l][1],)) for l in range(7) for suffix in _BN_SUFFIXES]
    return _pack(load().mvs_pack_feature_weights, query_feature_blob(), state, convs, bns, ("feature.bias", (32,)), eps)


def query_feature_workspace(N, H, W) -> int:
    return _query("mvs_query_feature_workspace", N, H, W)


def query_forward_workspace(N, H, W, D, dtype=MVS_F32) -> int:
    return _query("mvs_query_forward_workspace", N, H, W, D, dtype)


def feature_layer(layer, x, fblob):
    """One FeatureNet layer on the GPU.  x: NCHW images [N,3,H,W] for layer 0, otherwise C8-planar
    [Cin/8,N,H,W,8]; returns C8-planar [Cout/8,N,Ho,Wo,8]."""
    x = _dev_f32(x, "x")
    ci, co, k, s = FEATURE_LAYERS[layer]
    if layer == 0:
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"feature layer 0 wants [N,3,H,W] images, got {tuple(x.shape)}")
        N, c, H, W = x.shape
    else:
        if x.dim() != 5:
            raise RuntimeError(f"feature layer {layer} wants C8-planar input with {ci} channels, got {tuple(x.shape)}")
        pl, N, H, W, e = x.shape
        if pl * e != ci or e != 8:
            raise RuntimeError(f"feature layer {layer} wants C8-planar input with {ci} channels, got {tuple(x.shape)}")
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    _check_blob(fblob, "feature", x.device, f"feature layer {layer}")
    _aligned16(f"feature layer {layer}", x=x)
    with torch.cuda.device(x.device):
        y = torch.empty((co // 8, N, Ho, Wo, 8), dtype=torch.float32, device=x.device)
        check(load().mvs_feature_layer(layer, x.data_ptr(), y.data_ptr(), fblob.data_ptr(), N, H, W,
                                       _stream(x.device)))
    return y


def _image_arg(imgs, what):
    """Device images in one of the ABI's pixel formats -> (tensor, mvs_image_format, N, H, W):
    float32 [N,3,H,W]; uint8 [N,3,H,W]; uint8 [N,H,W,3] (as PIL yields a decoded image).  The uint8 forms are
    divided by 255 inside FeatureNet's first kernel -- the reference's host-side conversion
    (datasets/data_io.py:143), bit for bit -- so the caller copies a quarter of the bytes."""
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise RuntimeError(f"{what}: images must be a CUDA(ROCm) tensor")
    if imgs.dim() != 4:
        raise RuntimeError(f"{what} wants [N,3,H,W] (float32 / uint8) or [N,H,W,3] (uint8) images, got {tuple(imgs.shape)}")
    if imgs.numel() == 0:
        raise RuntimeError(f"{what}: images are empty: {list(imgs.shape)}")
    if imgs.dtype == torch.uint8:
        imgs = imgs.contiguous()
        if imgs.shape[1] == 3:
            return imgs, MVS_IMG_U8_CHW, imgs.shape[0], imgs.shape[2], imgs.shape[3]
        if imgs.shape[3] == 3:
            return imgs, MVS_IMG_U8_HWC, imgs.shape[0], imgs.shape[1], imgs.shape[2]
        raise RuntimeError(f"{what}: uint8 images must be [N,3,H,W] or [N,H,W,3], got {tuple(imgs.shape)}")
    imgs = _dev_f32(imgs, "imgs")
    if imgs.shape[1] != 3:
        raise RuntimeError(f"{what} wants [N,3,H,W] images, got {tuple(imgs.shape)}")
    return imgs, MVS_IMG_F32_CHW, imgs.shape[0], imgs.shape[2], imgs.shape[3]


def feature_conv01(imgs, fblob):
    """conv0 + conv1 of FeatureNet as the one fused kernel the net runs: imgs [N,3,H,W] fp32 (or uint8, see
    _image_arg) -> C8-planar [1,N,H,W,8].  For parity tests and per-kernel timing."""
    imgs, fmt, N, H, W = _image_arg(imgs, "feature_conv01")
    _check_blob(fblob, "feature", imgs.device, "feature_conv01")
    _aligned16("feature_conv01", imgs=imgs)
    with torch.cuda.device(imgs.device):
        y = torch.empty((1, N, H, W, 8), dtype=torch.float32, device=imgs.device)
        check(load().mvs_feature_conv01_fmt(imgs.data_ptr(), fmt, y.data_ptr(), fblob.data_ptr(), N, H, W,
                                            _stream(imgs.device)))
    return y


def feature_net(imgs, fblob, workspace=None, out=None):
    """FeatureNet.forward on the GPU: imgs [N,3,H,W] fp32 (or uint8, see _image_arg) -> [N,32,H/4,W/4] fp32 (NCHW),
    written into `out` when given (a contiguous tensor of that shape)."""
    imgs, fmt, N, H, W = _image_arg(imgs, "feature_net")
    dev = imgs.device
    _check_blob(fblob, "feature", dev, "feature_net")
    h4, w4 = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(query_feature_workspace(N, H, W), dtype=torch.uint8, device=dev)
        else:
            _check_workspace(workspace, dev, "feature_net")
        if out is None:
            out = torch.empty((N, 32, h4, w4), dtype=torch.float32, device=dev)
        else:
            _check_out(out, (N, 32, h4, w4), torch.float32, dev, "feature_net: out",
                       f"float32 [{N},32,{h4},{w4}] tensor on {dev}")
        _aligned16("feature_net", imgs=imgs, out=out)
        check(load().mvs_feature_net_fmt(imgs.data_ptr(), fmt, fblob.data_ptr(), out.data_ptr(), workspace.data_ptr(),
                                         workspace.numel(), N, H, W, _stream(dev)))
    return out


def forward_images(imgs, proj, depth_values, fblob, blob, workspace, depth_out, conf_out, dtype=MVS_F32):
    """MVSNet.forward of one batch item from images: imgs [N,3,H,W] fp32 (or uint8, see _image_arg), proj [N,4,4],
    depth_values [D]."""
    imgs, fmt, N, H, W = _image_arg(imgs, "forward_images")
    dev = imgs.device
    _aligned16("forward_images", imgs=imgs)
    proj, depth_values = _depth_call_args("forward_images", dev, N, H // 4, W // 4, proj, depth_values, blob, workspace,
                                          depth_out, conf_out, fblob=fblob)
    D = depth_values.shape[0]
    with torch.cuda.device(dev):
        check(load().mvs_forward_images_fmt(imgs.data_ptr(), fmt, proj.data_ptr(), depth_values.data_ptr(),
                                            fblob.data_ptr(), blob.data_ptr(), depth_out.data_ptr(),
                                            conf_out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                            N, H, W, D, dtype, _stream(dev)))


# ---- depth error against ground truth (reference train.py:302-358) ---------------------------
METRICS_MAX_THRES = 8


def query_metrics_workspace(B, h, w) -> int:
    return _query("mvs_query_metrics_workspace", B, h, w)


def depth_metrics(depth_est, depth_gt, mask, thresholds=(1.0, 2.0, 4.0, 8.0), sums_out=None, errmap=False,
                  workspace=None):
    """Per-image masked error sums of depth maps [B,h,w] (or [h,w]) against ground truth, on the GPU.

    mask is float32 as the loaders produce it (PNG / 255) or bool (converted on the device); valid = mask > 0.5.
    Returns (sums float64 [B, 3 + len(thresholds)] on the device -- rows [n_valid, sum |e|, sum smooth_l1(e),
    count(|e| > t) ...] -- and the error map |est - gt| * mask float32 [B,h,w] or None).  `sums_out` (a
    contiguous float64 CUDA tensor of that shape, e.g. rows of a larger buffer) receives the sums when given.
    Enqueued on the current stream; nothing synchronises."""
    import numpy as np
    if not isinstance(mask, torch.Tensor):
        raise RuntimeError("depth_metrics: mask must be a tensor")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.float32)
    est = _dev_f32(depth_est, "depth_est")
    gt = _dev_f32(depth_gt, "depth_gt")
    mask = _dev_f32(mask, "mask")
    if est.dim() == 2:
        est, gt, mask = est[None], gt[None], mask[None]
    if est.dim() != 3 or gt.shape != est.shape or mask.shape != est.shape:
        raise RuntimeError(f"depth_metrics: depth_est {tuple(depth_est.shape)}, depth_gt {tuple(depth_gt.shape)} and "
                           f"mask {tuple(mask.shape)} must all be [B,h,w]")
    if gt.device != est.device or mask.device != est.device:
        raise RuntimeError("depth_metrics: depth_est, depth_gt and mask must be on one device")
    B, h, w = est.shape
    th = np.ascontiguousarray([float(t) for t in thresholds], dtype=np.float32)
    K = 3 + th.size
    dev = est.device
    if sums_out is None:
        sums_out = torch.empty((B, K), dtype=torch.float64, device=dev)
    else:
        _check_out(sums_out, (B, K), torch.float64, dev, "depth_metrics: sums_out", f"float64 [{B},{K}] tensor on {dev}")
    err = torch.empty((B, h, w), dtype=torch.float32, device=dev) if errmap else None
    with torch.cuda.device(dev):
        nbytes = query_metrics_workspace(B, h, w)
        if workspace is not None and isinstance(workspace, torch.Tensor) and workspace.device == dev:
            _check_workspace(workspace, dev, "depth_metrics", align=8)
        if workspace is None or workspace.numel() < nbytes or workspace.device != dev:      # replaced, not refused
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(load().mvs_depth_metrics(est.data_ptr(), gt.data_ptr(), mask.data_ptr(), B, h, w,
                                       th.ctypes.data if th.size else None, int(th.size), sums_out.data_ptr(),
                                       err.data_ptr() if err is not None else None, workspace.data_ptr(),
                                       workspace.numel(), _stream(dev)))
    return sums_out, err
