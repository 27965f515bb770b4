"""Host side of the training convolutions (csrc/train_conv3d.hip, training.conv3d / conv_transpose3d): the C ABI's
refusals, which happen before anything is enqueued (the pointers below are never dereferenced), the workspace formula,
and the Python layer's refusals."""
import ctypes

import pytest
import torch

from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, training

_FAKE = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(5)]   # 256-byte aligned, never dereferenced
GOOD = dict(Cin=32, Cout=8, D=16, H=12, W=20, stride=1)
LAYERS = [(32, 8, 1), (8, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (8, 1, 1)]


def _dims(a):
    return a["Cin"], a["Cout"], a["D"], a["H"], a["W"], a["stride"]


def _forward(null=None, flip=0, **kw):
    a = dict(GOOD, **kw)
    p = list(_FAKE)
    if null is not None:
        p[null] = None
    return _lib.load().mvs_conv3d_train_forward(p[0], p[1], p[2], p[3], *_dims(a), flip, None)


def _backward_data(null=None, **kw):
    a = dict(GOOD, **kw)
    p = list(_FAKE)
    if null is not None:
        p[null] = None
    return _lib.load().mvs_conv3d_train_backward_data(p[0], p[1], p[2], *_dims(a), None)


def _backward_weight(null=None, ws_bytes=None, ws_ptr=None, **kw):
    a = dict(GOOD, **kw)
    p = list(_FAKE)
    if null is not None:
        p[null] = None
    if ws_ptr is not None:
        p[4] = ctypes.c_void_p(ws_ptr)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return _lib.load().mvs_conv3d_train_backward_weight(p[0], p[1], p[2], p[3], p[4], ws_bytes, *_dims(a), None)


def _query(**kw):
    a = dict(GOOD, **kw)
    n = ctypes.c_size_t(0)
    return _lib.load().mvs_query_conv3d_train_workspace(*_dims(a), ctypes.byref(n)), int(n.value)


ENTRY_POINTS = [_forward, _backward_data, _backward_weight, lambda **kw: _query(**kw)[0]]

BAD_SHAPES = [dict(D=0), dict(H=0), dict(W=-4), dict(D=-1),                       # zero / negative dims
              dict(Cin=8, Cout=16, stride=2, D=15), dict(Cin=8, Cout=16, stride=2, H=13),
              dict(Cin=8, Cout=16, stride=2, W=21),                               # odd dims at stride 2
              dict(stride=0), dict(stride=3),                                     # stride not 1 or 2
              dict(Cin=32, Cout=16), dict(Cin=3, Cout=5), dict(Cin=8, Cout=32),   # a pair no kernel exists for
              dict(Cin=32, Cout=8, stride=2), dict(Cin=8, Cout=16, stride=1),     # ... at this stride
              dict(D=1024, H=1024, W=2048), dict(D=512, H=512, W=512),            # D*H*W*32 >= 2^31
              dict(Cin=64, Cout=64, D=512, H=256, W=256)]


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_bad_shapes_are_refused_by_every_entry_point(shape):
    for f in ENTRY_POINTS:
        assert f(**shape) == 1                                # MVS_ERR_BAD_SHAPE


def test_the_flipped_forward_takes_the_transposed_stride_1_pairs_only():
    assert _forward(Cin=32, Cout=8, flip=1) == 1              # (32, 8) flipped would need a conv (8, 32)
    assert _forward(Cin=16, Cout=8, stride=2, flip=1) == 1    # stride 2 has no flipped form
    assert _forward(Cin=8, Cout=32, flip=2) == 1


def test_null_pointers_are_refused():
    for k in (0, 1, 3):                                       # x, w, y; the bias (2) may be NULL
        assert _forward(null=k) == 5
    for k in (0, 1, 2):
        assert _backward_data(null=k) == 5
    for k in (0, 1, 2, 4):                                    # x, gy, gw, workspace; gbias (3) may be NULL
        assert _backward_weight(null=k) == 5
    assert b"NULL" in _lib.load().mvs_last_error_string()
    assert _lib.load().mvs_query_conv3d_train_workspace(32, 8, 16, 12, 20, 1, None) == 5


def workspace_formula(Cin, Cout, D, H, W, stride):
    """Restatement of csrc/train_conv3d.hip's split: a block owns `rpc` output (z, y) rows and TW taps; the partial
    [Cout][Cin][27] slabs and the partial bias rows are each rounded up to 256 bytes."""
    tiles = -(-Cout // 16) * (Cin // 16 if Cin >= 16 else 1)
    tw = 9 if 9 * tiles <= 24 else 3 if 3 * tiles <= 24 else 1
    rows = (D // stride) * (H // stride)
    target = 1024 * tw // 27
    rpc = -(-rows // target)
    chunks = -(-rows // rpc)
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    return up(chunks * Cout * Cin * 27 * 4) + up(chunks * Cout * 4)


@pytest.mark.parametrize("dims", [(2, 2, 4), (16, 12, 20), (192, 128, 160), (48, 296, 400), (8, 14, 26)])
def test_workspace_query_agrees_with_its_formula_and_one_byte_less_is_refused(dims):
    D, H, W = dims
    for cin, cout, s in LAYERS:
        st, n = _query(Cin=cin, Cout=cout, D=D, H=H, W=W, stride=s)
        assert st == 0 and n == workspace_formula(cin, cout, D, H, W, s), (cin, cout, s, n)
        assert n == _lib.conv3d_train_workspace_bytes(cin, cout, D, H, W, s)
        kw = dict(Cin=cin, Cout=cout, D=D, H=H, W=W, stride=s)
        assert _backward_weight(ws_bytes=n - 1, **kw) == 3               # MVS_ERR_WORKSPACE
        assert _backward_weight(ws_bytes=n, ws_ptr=0x500010, **kw) == 3  # misaligned
    assert b"aligned" in _lib.load().mvs_last_error_string()


def test_python_functions_refuse_cpu_and_non_fp32_tensors():
    x, w = torch.zeros(1, 32, 4, 4, 4), torch.zeros(8, 32, 3, 3, 3)
    with pytest.raises(RuntimeError, match="CPU"):
        training.conv3d(x, w)
    with pytest.raises(RuntimeError, match="CPU"):
        training.conv_transpose3d(torch.zeros(1, 16, 2, 2, 2), torch.zeros(16, 8, 3, 3, 3))
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="float32"):
            training.conv3d(x.cuda().half(), w.cuda().half())
        with pytest.raises(RuntimeError, match="float32"):
            training.conv_transpose3d(torch.zeros(1, 16, 2, 2, 2).cuda().double(),
                                      torch.zeros(16, 8, 3, 3, 3).cuda().double())


def test_costreg_impl_is_validated_and_leaves_the_state_dict_alone():
    m = training.TrainableMVSNet(refine=False)
    assert m.costreg_impl == "torch"
    keys = list(m.state_dict().keys())
    m.costreg_impl = "hip"
    assert list(m.state_dict().keys()) == keys == list(MVSNet(refine=False).state_dict().keys())
    m.costreg_impl = "nope"
    imgs, proj, dv = torch.zeros(1, 3, 3, 32, 32), torch.eye(4).repeat(1, 3, 1, 1), torch.linspace(425, 500, 8)[None]
    with pytest.raises(RuntimeError, match="costreg_impl"):
        m.train()(imgs, proj, dv)
    with pytest.raises(RuntimeError, match="costreg_impl"):
        training._costreg(m.cost_regularization, torch.zeros(1, 32, 8, 8, 8), "nope")
