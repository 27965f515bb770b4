"""The training path's host side (scene_3dreconstruction_mvsnet_amd/training.py, csrc/train_backward.hip): refusals
of the Python layer and of the C ABI, which happen before anything is enqueued (tests/refusals.py makes the C calls in a
child process that sees no device), and the model's parameter names."""
import sys

import pytest
import torch

import refusals
from refusals import BAD_SHAPE, NULL, WORKSPACE
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
# every refusal below is run by tests/refusals.py in a child that sees no device; the tests look their record up
WVB_SHAPES = [dict(N=0), dict(N=65), dict(C=16), dict(D=12), dict(h=4), dict(w=20), dict(D=0), dict(D=512, h=512, w=512),
              dict(D=8, h=4096, w=16384)]
WVB_NULLS = ("feats", "depth_values", "grad_var", "grad_feats")
SAB_SHAPES = [dict(D=0, h=8, w=8), dict(D=8, h=0, w=8), dict(D=8, h=8, w=0), dict(D=8, h=65536, w=32768)]
COST_VOLUMES = [(2, 8, 8, 8), (3, 192, 128, 160), (7, 16, 24, 40), (5, 48, 296, 400)]
REFUSALS = {
    "mvs_warp_variance_backward": dict(
        good=dict(N=3, C=32, D=16, h=16, w=24),
        # D = 408 is the largest the forward accepts at 512 x 640 (D*h*w*32 < 2^32, test_gpu_limits.py); 416 is refused
        cases=refusals.cases(*[(bad, BAD_SHAPE, "") for bad in WVB_SHAPES + [dict(D=416, h=512, w=640)]],
                             *[({p: None}, NULL, "NULL") for p in WVB_NULLS])),
    "mvs_softargmin_backward": dict(
        good=dict(D=8, h=8, w=8),
        cases=refusals.cases(*[(bad, BAD_SHAPE, "") for bad in SAB_SHAPES], (dict(cost=None), NULL, ""))),
    "mvs_warp_variance": dict(
        good=dict(C=32, dtype=_lib.MVS_F32), sizes=dict(need=lambda a: training.feature_workspace_bytes(a["N"], a["h"], a["w"])),
        cases=refusals.cases(*[(dict(N=N, D=D, h=h, w=w, workspace_bytes="need-1"), WORKSPACE, "")
                               for N, D, h, w in COST_VOLUMES])),
}


def _refused(name, **ov):
    return refusals.expect(sys.modules[__name__], name, ov)


@pytest.mark.parametrize("shape", WVB_SHAPES)
def test_warp_variance_backward_bad_shape_is_refused(shape):
    assert _refused("mvs_warp_variance_backward", **shape) == BAD_SHAPE


def test_warp_variance_backward_refuses_beyond_the_forward_limit_and_nulls():
    assert _refused("mvs_warp_variance_backward", D=416, h=512, w=640) == BAD_SHAPE
    for p in WVB_NULLS:
        assert _refused("mvs_warp_variance_backward", **{p: None}) == NULL


def test_softargmin_backward_refusals():
    for shape in SAB_SHAPES:
        assert _refused("mvs_softargmin_backward", **shape) == BAD_SHAPE
    assert _refused("mvs_softargmin_backward", cost=None) == NULL


@pytest.mark.parametrize("N,D,h,w", COST_VOLUMES)
def test_cost_volume_workspace_is_what_warp_variance_requires(N, D, h, w):
    """training.cost_volume sizes mvs_warp_variance's workspace itself (the feature-transpose region only): one byte
    less is refused with MVS_ERR_WORKSPACE before anything is enqueued.  That the size suffices is pinned on the GPU
    (test_gpu_training.py::test_cost_volume_workspace_size_suffices)."""
    assert _refused("mvs_warp_variance", N=N, D=D, h=h, w=w, workspace_bytes="need-1") == WORKSPACE
