"""The training path's host side (scene_3dreconstruction_mvsnet_amd/training.py, csrc/train_backward.hip): refusals
of the Python layer and of the C ABI, which happen before anything is enqueued, and the model's parameter names."""
import ctypes

import pytest
import torch

from scene_3dreconstruction_mvsnet_amd import MVSNet, _lib, training


def _inputs(N=3, H=32, W=32, D=8):
    return torch.zeros(1, N, 3, H, W), torch.eye(4).repeat(1, N, 1, 1), torch.linspace(425, 500, D)[None]


def test_state_dict_keys_and_shapes_equal_mvsnet():
    a = training.TrainableMVSNet(refine=False).state_dict()
    b = MVSNet(refine=False).state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(a[k].shape == b[k].shape for k in a)
    a = training.TrainableMVSNet(refine=True).state_dict()
    assert list(a.keys()) == list(MVSNet(refine=True).state_dict().keys())


def test_train_mode_refuses_cpu_refine_and_16_bit_storage():
    imgs, proj, dv = _inputs()
    with pytest.raises(RuntimeError, match="no CPU"):
        training.TrainableMVSNet(refine=False).train()(imgs, proj, dv)
    with pytest.raises(NotImplementedError, match="refine=True"):
        training.TrainableMVSNet(refine=True).train()(imgs, proj, dv)
    m = training.TrainableMVSNet(refine=False).train()
    for dt in ("f16", "bf16"):
        m.storage_dtype = dt
        with pytest.raises(RuntimeError, match="f32"):
            m(imgs, proj, dv)
    with pytest.raises(AssertionError, match="Different number"):
        training.TrainableMVSNet(refine=False).train()(imgs, proj[:, :2], dv)


def test_eval_mode_is_mvsnet_forward_and_mvsnet_still_refuses_training():
    imgs, proj, dv = _inputs()
    with pytest.raises(RuntimeError, match="no CPU"):
        training.TrainableMVSNet(refine=False).eval()(imgs, proj, dv)
    with pytest.raises(RuntimeError, match="eval"):
        MVSNet(refine=False).train()(imgs, proj, dv)


def test_autograd_functions_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="CPU"):
        training.cost_volume(torch.zeros(1, 3, 32, 8, 8), torch.eye(4).repeat(1, 3, 1, 1), torch.ones(1, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        training.soft_argmin(torch.zeros(1, 8, 8, 8), torch.ones(1, 8))


def test_loss_is_the_masked_mean_smooth_l1_with_gradients():
    est = torch.tensor([[[1.0, 2.0, 5.0, float("nan")]]], requires_grad=True)
    gt = torch.tensor([[[1.5, 4.0, 5.0, 3.0]]])
    mask = torch.tensor([[[1.0, 0.75, 0.5, 0.0]]])       # 0.5 is not valid (mask > 0.5), NaN is masked out
    loss = training.mvsnet_loss(est, gt, mask)
    want = torch.nn.functional.smooth_l1_loss(est[mask > 0.5], gt[mask > 0.5])
    assert torch.allclose(loss, want)
    loss.backward()
    assert torch.equal(est.grad, torch.tensor([[[-0.25, -0.5, 0.0, 0.0]]]))
    assert torch.isnan(training.mvsnet_loss(est.detach(), gt, torch.zeros_like(gt)))


# ---- the C ABI refuses bad arguments and enqueues nothing --------------------------------------------------------
_FAKE = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(5)]   # never dereferenced: refused first


def _wvb(N=3, C=32, D=16, h=16, w=24, null=None):
    p = list(_FAKE)
    if null is not None:
        p[null] = None
    return _lib.load().mvs_warp_variance_backward(p[0], p[1], p[2], p[3], p[4], N, C, D, h, w, None)


@pytest.mark.parametrize("shape", [dict(N=0), dict(N=65), dict(C=16), dict(D=12), dict(h=4), dict(w=20),
                                   dict(D=0), dict(D=512, h=512, w=512), dict(D=8, h=4096, w=16384)])
def test_warp_variance_backward_bad_shape_is_refused(shape):
    assert _wvb(**shape) == 1                                    # MVS_ERR_BAD_SHAPE


def test_warp_variance_backward_refuses_beyond_the_forward_limit_and_nulls():
    # D = 408 is the largest the forward accepts at 512 x 640 (D*h*w*32 < 2^32, test_gpu_limits.py); 416 is refused
    assert _wvb(D=416, h=512, w=640) == 1
    for k in (0, 2, 3, 4):
        assert _wvb(null=k) == 5                                 # MVS_ERR_NULL
    assert b"NULL" in _lib.load().mvs_last_error_string()


def test_softargmin_backward_refusals():
    lib = _lib.load()
    f = _FAKE
    for D, h, w in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (8, 65536, 32768)):
        assert lib.mvs_softargmin_backward(f[0], f[1], f[2], f[3], D, h, w, None) == 1
    assert lib.mvs_softargmin_backward(None, f[1], f[2], f[3], 8, 8, 8, None) == 5


@pytest.mark.parametrize("N,D,h,w", [(2, 8, 8, 8), (3, 192, 128, 160), (7, 16, 24, 40), (5, 48, 296, 400)])
def test_cost_volume_workspace_is_what_warp_variance_requires(N, D, h, w):
    """training.cost_volume sizes mvs_warp_variance's workspace itself (the feature-transpose region only): one byte
    less is refused with MVS_ERR_WORKSPACE before anything is enqueued.  That the size suffices is pinned on the GPU
    (test_gpu_training.py::test_cost_volume_workspace_size_suffices)."""
    nbytes = training.feature_workspace_bytes(N, h, w)
    f = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(5)]      # 256-byte aligned, never dereferenced
    st = _lib.load().mvs_warp_variance(f[0], f[1], f[2], f[3], f[4], nbytes - 1, N, 32, D, h, w, _lib.MVS_F32, None)
    assert st == 3, st                                                # MVS_ERR_WORKSPACE
