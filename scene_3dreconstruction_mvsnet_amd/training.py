"""Training path: the reference's `train.py --mode train` step on the MI355X (models/mvsnet.py:91-244, train.py:241-298).

The cost volume and the soft-argmin -- the parts of a training step whose torch autograd graph is largest -- run as
HIP kernels with hand-written adjoints (csrc/train_backward.hip); FeatureNet runs in torch (MIOpen) with autograd,
and so does CostRegNet unless `costreg_impl = "hip"` puts its convolutions on csrc/train_conv3d.hip
(`"hip_fused"`: its batch-norms, ReLUs and skip additions on csrc/train_bn3d.hip as well):

  cost_volume(feats, proj_matrices, depth_values)   mvs_relative_proj + mvs_warp_variance (fp32) forward,
                                                    mvs_warp_variance_backward; saves only its inputs, rt and the
                                                    depth values (no volume)
  soft_argmin(cost, depth_values)                   mvs_softargmin_conf forward, mvs_softargmin_backward; only the
                                                    depth is differentiable (the confidence is no_grad, mvsnet.py:213)
  conv3d(x, weight, bias, stride)                   mvs_conv3d_train_forward / _backward_data / _backward_weight: CostRegNet's
  conv_transpose3d(x, weight)                       3x3x3 convolutions, raw (BatchNorm3d and ReLU stay in torch)
  batch_norm_relu(x, bn, relu, skip)                mvs_bn3d_train_forward / _backward: train-mode BatchNorm3d + ReLU +
                                                    skip addition as one forward and one backward call
                                                    (csrc/train_bn3d.hip; `costreg_impl = "hip_fused"`)
  mvsnet_loss(depth_est, depth_gt, mask)            masked-mean smooth-L1 (mvsnet.py:242-244) without boolean
                                                    indexing, so it never synchronises
  TrainableMVSNet                                   MVSNet whose train-mode forward builds an autograd graph
  train_sample(model, optimizer, sample)            one optimisation step, train.py:241-298

Everything is enqueued on torch's current stream; nothing here synchronises except train_sample's one copy of its
scalars to the host at the end, where the reference's tensor2float makes one copy per scalar.
"""
import torch
import torch.nn.functional as F

from . import _lib, metrics
from .mvsnet import MVSNet


def feature_workspace_bytes(N, h, w):
    """Workspace bytes mvs_warp_variance needs on its own: the feature-transpose region only (include/mvs_abi.h),
    N*32*h*w fp32 rounded to 256 bytes -- not mvs_query_workspace's whole depth-path workspace, whose volume and
    activation regions make it 0.90 GB instead of 7.9 MB at the training shape (512 x 640, D = 192).
    tests/test_training_host.py and tests/test_gpu_training.py pin this size against the library from both sides."""
    return (N * 32 * h * w * 4 + 255) // 256 * 256


def _feature_workspace(N, h, w, device):
    return torch.empty(feature_workspace_bytes(N, h, w), dtype=torch.uint8, device=device)


class _CostVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, proj_matrices, depth_values, channels_last=False):
        B, N, C, h, w = feats.shape
        D = depth_values.shape[1]
        device = feats.device
        with torch.cuda.device(device):
            feats = _lib._dev_f32(feats.detach(), "features")
            proj = _lib._dev_f32(proj_matrices.detach().to(device), "proj_matrices")
            dv = _lib._dev_f32(depth_values.detach().to(device), "depth_values")
            ws = _feature_workspace(N, h, w, device)
            oshape = (B, D, h, w, C) if channels_last else (B, C, D, h, w)
            out = torch.empty(oshape, dtype=torch.float32, device=device)
            rts = []
            for b in range(B):
                rt = _lib.relative_proj(proj[b])
                var = _lib.warp_variance(feats[b], rt, dv[b], ws, _lib.MVS_F32)   # C8-planar [4,D,h,w,8]
                if channels_last:
                    _lib.volume_relayout(var, _lib.RELAYOUT_C8_TO_CHANNELS_LAST, out=out[b])
                else:
                    out[b].view(C // 8, 8, D, h, w).copy_(var.permute(0, 4, 1, 2, 3))
                rts.append(rt)
        ctx.save_for_backward(feats, torch.stack(rts), dv)
        ctx.channels_last = channels_last
        return _logical(out) if channels_last else out

    @staticmethod
    def backward(ctx, grad_var):
        feats, rts, dv = ctx.saved_tensors
        if grad_var is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        with torch.cuda.device(feats.device):
            grad = torch.empty_like(feats)
            if ctx.channels_last:
                g = _channels_last(grad_var, "cost volume gradient")   # no copy when it comes from conv3d's backward
                planar = torch.empty((g.shape[4],) + tuple(g.shape[1:4]), dtype=torch.float32, device=g.device)
                for b in range(feats.shape[0]):
                    _lib.volume_relayout(g[b], _lib.RELAYOUT_CHANNELS_LAST_TO_PLANAR, out=planar)
                    _lib.warp_variance_backward(feats[b], rts[b], dv[b], planar, out=grad[b])
            else:
                grad_var = grad_var.contiguous()
                for b in range(feats.shape[0]):
                    _lib.warp_variance_backward(feats[b], rts[b], dv[b], grad_var[b], out=grad[b])
        return grad, None, None, None


def cost_volume(feats, proj_matrices, depth_values, channels_last=False):
    """Variance cost volume with autograd (models/module.py:96-139 + models/mvsnet.py:145-177, training branch).

    feats [B,N,32,h,w] float32 CUDA (view 0 = reference view), proj_matrices [B,N,4,4], depth_values [B,D]
    -> variance [B,32,D,h,w] float32, NCDHW as CostRegNet's Conv3d takes it.  Gradients flow to feats only.
    channels_last=True: the same logical tensor in torch's channels_last_3d memory format, as conv3d above takes it
    without a copy -- one mvs_volume_relayout of the kernel's C8-planar output instead of a permute to NCDHW and a
    second one to channels-last, and one relayout of the incoming gradient on the way back."""
    if not feats.is_cuda:
        raise RuntimeError(f"cost_volume needs CUDA(ROCm) tensors: the depth path has no CPU implementation "
                           f"(got feats on {feats.device})")
    if feats.dim() != 5 or feats.shape[2] != 32:
        raise RuntimeError(f"cost_volume: feats must be [B,N,32,h,w], got {tuple(feats.shape)}")
    if proj_matrices.shape[:2] != feats.shape[:2] or depth_values.dim() != 2 \
            or depth_values.shape[0] != feats.shape[0]:
        raise RuntimeError(f"cost_volume: proj_matrices {tuple(proj_matrices.shape)} must be [B,N,4,4] and "
                           f"depth_values {tuple(depth_values.shape)} [B,D] for feats {tuple(feats.shape)}")
    return _CostVolume.apply(feats, proj_matrices, depth_values, bool(channels_last))


class _SoftArgmin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, depth_values):
        B, D, h, w = cost.shape
        device = cost.device
        with torch.cuda.device(device):
            cost = _lib._dev_f32(cost.detach(), "cost")
            dv = _lib._dev_f32(depth_values.detach().to(device), "depth_values")
            depth = torch.empty((B, h, w), dtype=torch.float32, device=device)
            conf = torch.empty_like(depth)
            for b in range(B):
                d, c = _lib.softargmin_conf(cost[b], dv[b])
                depth[b].copy_(d)
                conf[b].copy_(c)
        ctx.save_for_backward(cost, dv)
        ctx.mark_non_differentiable(conf)
        return depth, conf

    @staticmethod
    def backward(ctx, grad_depth, grad_conf):
        cost, dv = ctx.saved_tensors
        if grad_depth is None or not ctx.needs_input_grad[0]:
            return None, None
        with torch.cuda.device(cost.device):
            grad_depth = grad_depth.contiguous()
            grad = torch.empty_like(cost)
            for b in range(cost.shape[0]):
                grad[b].copy_(_lib.softargmin_backward(cost[b], dv[b], grad_depth[b]))
        return grad, None


def soft_argmin(cost, depth_values):
    """cost logits [B,D,h,w], depth_values [B,D] -> (depth [B,h,w], photometric_confidence [B,h,w])
    (models/mvsnet.py:192-218).  Only depth carries a gradient."""
    if not cost.is_cuda:
        raise RuntimeError(f"soft_argmin needs CUDA(ROCm) tensors (got cost on {cost.device})")
    if cost.dim() != 4 or depth_values.shape != cost.shape[:2]:
        raise RuntimeError(f"soft_argmin: cost {tuple(cost.shape)} must be [B,D,h,w] and depth_values "
                           f"{tuple(depth_values.shape)} [B,D]")
    return _SoftArgmin.apply(cost, depth_values)


def mvsnet_loss(depth_est, depth_gt, mask):
    """smooth_l1_loss(depth_est[mask > 0.5], depth_gt[mask > 0.5]) averaged over the selected pixels
    (models/mvsnet.py:242-244), differentiable and without boolean indexing.  No valid pixel gives NaN, as the
    reference's mean over an empty selection does."""
    valid = mask > 0.5
    est = torch.where(valid, depth_est, torch.zeros_like(depth_est))
    gt = torch.where(valid, depth_gt, torch.zeros_like(depth_gt))
    return F.smooth_l1_loss(est, gt, reduction="sum") / valid.sum().to(depth_est.dtype)


def _channels_last(t, name):
    """Logical [B,C,D,H,W] -> the kernels' [B,D,H,W,C] (no copy when t already is channels_last_3d)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} needs CUDA(ROCm) tensors: the training convolutions have no CPU implementation "
                           f"(got {t.device})")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != 5:
        raise RuntimeError(f"{name} must be [B,C,D,H,W], got {tuple(t.shape)}")
    return t.detach().permute(0, 2, 3, 4, 1).contiguous()


def _logical(t):
    """The kernels' [B,D,H,W,C] -> logical [B,C,D,H,W] in torch's channels_last_3d memory format (a view)."""
    return t.permute(0, 4, 1, 2, 3)


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        with torch.cuda.device(x.device):
            xc = _channels_last(x, "conv3d input")
            w = _lib._dev_f32(weight.detach(), "weight")
            b = None if bias is None else _lib._dev_f32(bias.detach(), "bias")
            y = torch.stack([_lib.conv3d_train_forward(xc[i], w, b, stride) for i in range(xc.shape[0])])
        ctx.save_for_backward(xc, w)
        ctx.stride, ctx.has_bias = stride, bias is not None
        return _logical(y)

    @staticmethod
    def backward(ctx, grad_y):
        xc, w = ctx.saved_tensors
        gx = gw = gb = None
        with torch.cuda.device(xc.device):
            g = _channels_last(grad_y, "conv3d output gradient")
            B = xc.shape[0]
            if ctx.needs_input_grad[0]:
                gx = _logical(torch.stack([_lib.conv3d_train_backward_data(g[i], w, ctx.stride) for i in range(B)]))
            if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
                for i in range(B):
                    r = _lib.conv3d_train_backward_weight(xc[i], g[i], ctx.stride, with_bias=ctx.has_bias)
                    gwi, gbi = r if ctx.has_bias else (r, None)
                    gw = gwi if gw is None else gw + gwi
                    gb = gbi if gb is None or gbi is None else gb + gbi
        return gx, gw, gb, None


class _ConvTranspose3d(torch.autograd.Function):
    """ConvTranspose3d(k=3, s=2, p=1, output_padding=1, bias=False): the adjoint of the stride-2 conv that has the same
    weight tensor, so its forward is that conv's data gradient and its data gradient that conv's forward."""

    @staticmethod
    def forward(ctx, x, weight):
        with torch.cuda.device(x.device):
            xc = _channels_last(x, "conv_transpose3d input")
            w = _lib._dev_f32(weight.detach(), "weight")
            y = torch.stack([_lib.conv3d_train_backward_data(xc[i], w, 2) for i in range(xc.shape[0])])
        ctx.save_for_backward(xc, w)
        return _logical(y)

    @staticmethod
    def backward(ctx, grad_y):
        xc, w = ctx.saved_tensors
        gx = gw = None
        with torch.cuda.device(xc.device):
            g = _channels_last(grad_y, "conv_transpose3d output gradient")
            B = xc.shape[0]
            if ctx.needs_input_grad[0]:
                gx = _logical(torch.stack([_lib.conv3d_train_forward(g[i], w, None, 2) for i in range(B)]))
            if ctx.needs_input_grad[1]:
                for i in range(B):
                    gwi = _lib.conv3d_train_backward_weight(g[i], xc[i], 2)
                    gw = gwi if gw is None else gw + gwi
        return gx, gw


def conv3d(x, weight, bias=None, stride=1):
    """nn.Conv3d(kernel_size=3, padding=1, stride=stride) with autograd on the HIP training kernels
    (csrc/train_conv3d.hip; models/module.py:26-33, models/mvsnet.py:36-62).  x [B,Cin,D,H,W] float32 CUDA, weight
    [Cout,Cin,3,3,3], bias [Cout] or None -> [B,Cout,D/stride,H/stride,W/stride] in channels_last_3d memory format.
    Only CostRegNet's (Cin, Cout, stride) combinations exist; anything else raises with the library's message."""
    _channels_last_check(x, weight, "conv3d")
    return _Conv3d.apply(x, weight, bias, int(stride))


def conv_transpose3d(x, weight):
    """nn.ConvTranspose3d(kernel_size=3, stride=2, padding=1, output_padding=1, bias=False) with autograd on the HIP
    training kernels.  x [B,Cin,D,H,W], weight [Cin,Cout,3,3,3] -> [B,Cout,2D,2H,2W] (channels_last_3d)."""
    _channels_last_check(x, weight, "conv_transpose3d")
    return _ConvTranspose3d.apply(x, weight)


def _check_cuda_f32(who, no_cpu, tensors):
    """`who` refuses those of `tensors` = [(tensor or None, its name)] that are not on the GPU or not float32;
    `no_cpu` is the clause that says what has no CPU implementation."""
    for t, name in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{who} needs CUDA(ROCm) tensors: {no_cpu} "
                               f"(got {name} on {t.device})")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32 (got {t.dtype})")


def _channels_last_check(x, weight, who):
    _check_cuda_f32(who, "the training convolutions have no CPU implementation", ((x, "input"), (weight, "weight")))
    if x.dim() != 5 or weight.dim() != 5:
        raise RuntimeError(f"{who}: input {tuple(x.shape)} must be [B,C,D,H,W] and weight {tuple(weight.shape)} 5-d")


class _BatchNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, skip, running_mean, running_var, momentum, eps, relu):
        with torch.cuda.device(x.device):
            xc = _channels_last(x, "batch_norm_relu input")
            C = xc.shape[4]
            g, b = _lib._dev_f32(gamma.detach(), "weight"), _lib._dev_f32(beta.detach(), "bias")
            sc = None if skip is None else _channels_last(skip, "batch_norm_relu skip").view(-1, C)
            out, mean, invstd = _lib.bn3d_train_forward(xc.view(-1, C), g, b, sc, running_mean, running_var, momentum,
                                                        eps, relu)
        ctx.save_for_backward(xc, g, b, mean, invstd)
        ctx.relu = relu
        return _logical(out.view(xc.shape))

    @staticmethod
    def backward(ctx, grad_out):
        xc, g, b, mean, invstd = ctx.saved_tensors
        C = xc.shape[4]
        with torch.cuda.device(xc.device):
            go = _channels_last(grad_out, "batch_norm_relu output gradient")
            gy, gg, gb = _lib.bn3d_train_backward(xc.view(-1, C), go.view(-1, C), g, b, mean, invstd, ctx.relu)
        # the skip joins after the ReLU: its gradient is the incoming one, the same tensor
        return (_logical(gy.view(xc.shape)), gg, gb, grad_out if ctx.needs_input_grad[3] else None,
                None, None, None, None, None)


def batch_norm_relu(x, bn, relu=True, skip=None):
    """relu(bn(x)) + skip with bn (an nn.BatchNorm3d) in training mode: batch statistics pooled over [B,D,H,W], the
    running buffers and num_batches_tracked updated as nn.BatchNorm3d updates them (models/module.py:32-33,
    models/mvsnet.py:47-60, 66-70), with autograd, on csrc/train_bn3d.hip.  x [B,C,D,H,W] float32 CUDA in
    channels_last_3d memory format (conv3d's output; anything else is copied), C in {8,16,32,64}, B*D*H*W >= 2;
    skip None or shaped like x -> [B,C,D,H,W] in channels_last_3d memory format."""
    _check_cuda_f32("batch_norm_relu", "the training batch-norm has no CPU implementation",
                    ((x, "input"), (skip, "skip")))
    if x.dim() != 5 or (skip is not None and skip.shape != x.shape):
        raise RuntimeError(f"batch_norm_relu: input {tuple(x.shape)} must be [B,C,D,H,W] and skip "
                           f"{None if skip is None else tuple(skip.shape)} shaped like it")
    if not isinstance(bn, torch.nn.BatchNorm3d) or not bn.affine or bn.num_features != x.shape[1]:
        raise RuntimeError(f"batch_norm_relu: bn must be an affine nn.BatchNorm3d of {x.shape[1]} features, got {bn!r}")
    if not bn.training:
        raise RuntimeError("batch_norm_relu computes batch statistics: bn must be in training mode")
    rm = rv = None
    momentum = 0.0
    if bn.track_running_stats and bn.running_mean is not None:
        rm, rv = bn.running_mean, bn.running_var
        # momentum None is nn.BatchNorm3d's cumulative average, 1 / num_batches_tracked (one host read, as torch's own)
        momentum = 1.0 / (float(bn.num_batches_tracked) + 1.0) if bn.momentum is None else bn.momentum
    out = _BatchNormReLU.apply(x, bn.weight, bn.bias, skip, rm, rv, momentum, bn.eps, bool(relu))
    if rm is not None:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)   # after the call: a refusal leaves the module as it was
    return out


def _conv_bn_relu(block, x):
    return F.relu(block.bn(block.conv(x)), inplace=True)   # models/module.py:32-33


def _deconv_bn_relu(seq, x, skip):
    return skip + seq(x)   # models/mvsnet.py:66-70


def _conv_bn_relu_hip(block, x):
    return F.relu(block.bn(conv3d(x, block.conv.weight, None, block.conv.stride[0])), inplace=True)


def _deconv_bn_relu_hip(seq, x, skip):
    return skip + F.relu(seq[1](conv_transpose3d(x, seq[0].weight)), inplace=True)   # models/mvsnet.py:47-60


def _conv_bn_relu_fused(block, x):
    return batch_norm_relu(conv3d(x, block.conv.weight, None, block.conv.stride[0]), block.bn)


def _deconv_bn_relu_fused(seq, x, skip):
    return batch_norm_relu(conv_transpose3d(x, seq[0].weight), seq[1], skip=skip)   # models/mvsnet.py:47-60, 66-70


def _prob(prob, x):
    return prob(x)


def _prob_hip(prob, x):
    return conv3d(x, prob.weight, prob.bias, 1)


# impl -> (ConvBnReLU3D block, deconvolution block with its skip, the prob convolution):
#   "torch"      through the blocks' .conv / .bn modules;
#   "hip"        every convolution on the HIP training kernels; BatchNorm3d (train-mode statistics and their backward),
#                ReLU and the skip additions stay in torch, on channels_last_3d tensors;
#   "hip_fused"  nothing left to torch: the convolutions as "hip" runs them, and after each of the ten normalised
#                layers one batch_norm_relu (the three deconvolution layers with their skip).
_COSTREG_BLOCKS = {"torch": (_conv_bn_relu, _deconv_bn_relu, _prob),
                   "hip": (_conv_bn_relu_hip, _deconv_bn_relu_hip, _prob_hip),
                   "hip_fused": (_conv_bn_relu_fused, _deconv_bn_relu_fused, _prob_hip)}
COSTREG_IMPLS = tuple(_COSTREG_BLOCKS)


def _costreg(cr, x, impl="torch"):
    """CostRegNet.forward (models/mvsnet.py:64-73): impl "torch" through the blocks' .conv / .bn modules, "hip" with
    the convolutions on csrc/train_conv3d.hip, "hip_fused" with BatchNorm3d, ReLU and the skip additions on
    csrc/train_bn3d.hip as well."""
    if impl not in COSTREG_IMPLS:
        raise RuntimeError(f"costreg_impl must be 'torch', 'hip' or 'hip_fused', got {impl!r}")
    conv, deconv, prob = _COSTREG_BLOCKS[impl]
    conv0 = conv(cr.conv0, x)
    conv2 = conv(cr.conv2, conv(cr.conv1, conv0))
    conv4 = conv(cr.conv4, conv(cr.conv3, conv2))
    x = conv(cr.conv6, conv(cr.conv5, conv4))
    x = deconv(cr.conv7, x, conv4)
    x = deconv(cr.conv9, x, conv2)
    x = deconv(cr.conv11, x, conv0)
    return prob(cr.prob, x)


class TrainableMVSNet(MVSNet):
    """MVSNet with a training-mode forward.  Same constructor, parameters and state_dict keys as MVSNet.

    eval(): MVSNet.forward unchanged (all HIP).  train(): the reference's forward with an autograd graph --
    FeatureNet in torch once per view (models/mvsnet.py:125: per-view BN batch statistics, running statistics
    updated N times), cost_volume, CostRegNet in torch, soft_argmin.  The HIP inference blobs are re-packed from
    the parameters after every train-mode forward (BN statistics) and whenever a parameter's `_version` changes
    (optimizer steps, MVSNet._param_versions).

    costreg_impl: "torch" (default) runs CostRegNet's convolutions on torch's backend; "hip" on the library's training
    kernels (conv3d / conv_transpose3d above), with BatchNorm3d and ReLU still in torch; "hip_fused" adds
    batch_norm_relu after every normalised layer and takes the cost volume channels-last, so that nothing between the
    cost volume and the soft-argmin runs in torch.  Parameters, state_dict keys and the eval path do not depend on it."""

    costreg_impl = "torch"

    def forward(self, imgs, proj_matrices, depth_values):
        if not self.training:
            return super().forward(imgs, proj_matrices, depth_values)
        n_imgs, n_proj = imgs.shape[1], proj_matrices.shape[1]
        assert n_imgs == n_proj, "Different number of images and projection matrices"
        if self.refine:
            raise NotImplementedError("refine=True: the reference's RefineNet path is broken "
                                      "(F.cat at models/mvsnet.py:85); every working caller passes "
                                      "refine=False (eval.py:308)")
        if _lib.dtype_code(self.storage_dtype) != _lib.MVS_F32:
            raise RuntimeError(f"training needs storage_dtype 'f32' (got {self.storage_dtype!r}): 16-bit training "
                               "is not implemented")
        if self.costreg_impl not in COSTREG_IMPLS:
            raise RuntimeError(f"costreg_impl must be 'torch', 'hip' or 'hip_fused', got {self.costreg_impl!r}")
        if not imgs.is_cuda:
            raise RuntimeError("MVSNet.forward needs CUDA(ROCm) tensors: the depth path has no CPU "
                               "implementation (got imgs on {})".format(imgs.device))
        # BatchNorm updates its running statistics inside the backend's kernel, which need not bump the `_version`
        # that MVSNet._param_versions compares; drop the packed inference blobs, the next eval forward re-packs them
        # (parameter updates by the optimizer are in-place ops and are seen through `_version`)
        with self._cache_lock:
            self._blob_cache.clear()
        device = imgs.device
        if imgs.dtype == torch.uint8:   # the loader's conversion, on the device (as forward does)
            if imgs.shape[2] != 3 and imgs.shape[-1] == 3:
                imgs = imgs.permute(0, 1, 4, 2, 3)
            imgs = imgs.to(torch.float32) / 255.0
        with torch.cuda.device(device):
            # step 1. feature extraction, one call per view (models/mvsnet.py:125)
            feats = torch.stack([self.feature(imgs[:, v]) for v in range(imgs.shape[1])], dim=1)
            # step 2. cost volume (models/mvsnet.py:145-177)
            proj = proj_matrices.to(device=device, dtype=torch.float32)
            dv = depth_values.to(device=device, dtype=torch.float32)
            volume = cost_volume(feats, proj, dv, channels_last=self.costreg_impl == "hip_fused")
            # step 3. cost regularisation (models/mvsnet.py:180, 192)
            cost = _costreg(self.cost_regularization, volume, self.costreg_impl).squeeze(1)
            # step 4. soft-argmin and photometric confidence (models/mvsnet.py:193-218)
            depth, conf = soft_argmin(cost, dv)
        return {"depth": depth, "photometric_confidence": conf}


def train_sample(model, optimizer, sample):
    """One training step as train.py:241-298: model.train(), zero_grad, forward, mvsnet_loss, backward, step.

    sample: the reference loader's dict (imgs [B,N,3,H,W], proj_matrices [B,N,4,4], depth_values [B,D],
    depth [B,h,w], mask [B,h,w]).  Returns (loss, scalar_outputs) as Python floats with the reference's keys:
    loss, abs_depth_error, thres1mm_error .. thres8mm_error (the metrics.py drop-ins)."""
    model.train()
    optimizer.zero_grad()
    device = next(model.parameters()).device
    sc = {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in sample.items()}
    depth_gt, mask = sc["depth"], sc["mask"]
    outputs = model(sc["imgs"], sc["proj_matrices"], sc["depth_values"])
    depth_est = outputs["depth"]
    loss = mvsnet_loss(depth_est, depth_gt, mask)
    with torch.no_grad():
        est = depth_est.detach()
        scalars = {"loss": loss.detach(),
                   "abs_depth_error": metrics.AbsDepthError_metrics(est, depth_gt, mask)}
        for t in metrics.THRESHOLDS:
            scalars[f"thres{t}mm_error"] = metrics.Thres_metrics(est, depth_gt, mask, t)
    loss.backward()
    optimizer.step()
    values = torch.stack([v.to(torch.float32) for v in scalars.values()]).tolist()   # one device-to-host copy
    out = dict(zip(scalars.keys(), values))
    return out["loss"], out
