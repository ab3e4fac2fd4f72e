"""``JointsKLLoss`` (reference ``uda/model/loss.py:115-158``) as one fused row kernel: log-softmax,
target normalisation, KL sum, weighting and the gradient w.r.t. the prediction in a single pass; ``mt_loss`` (reference
``uda/model/loss.py:265-297``), the mean-teacher consistency term, as one masked squared-difference row kernel; ``MMD_loss3``,
``MMD_loss`` and ``mmd_rbf`` (reference ``uda/model/loss.py:1061-1196``), the multi-kernel MMD between a source and a target
batch, as three launches that never form the reference's n x n x HW temporaries; ``loss1`` and ``loss3`` (reference
``uda/model/loss.py:331-378``), the per-joint feature alignment term, as a pooling kernel, a KL row kernel and a gather for the
pooling's backward instead of a Python loop over B x 21 windows."""
import torch
import torch.nn as nn

from mi355 import ops
import mi355 as _rt


class _KLFn(torch.autograd.Function):
    """loss = coeff * mean(rows).  The kernel already writes d loss / d pred; the backward multiplies it by the incoming
    gradient unless that is the shared unit scalar of ``mi355.unit_grad`` (``loss.backward(mi355.unit_grad(loss))``: the
    training step's way of saying "the gradient of the total is 1"), in which case it is handed on as it is."""

    @staticmethod
    def forward(ctx, pred, target, weight, eps, coeff):
        ctx.set_materialize_grads(False)      # `rows` is rarely differentiated: no zero tensor per call for its absent gradient
        rows, g = ops.kl_heatmap(pred, target, weight, eps, ctx.needs_input_grad[0], coeff)
        ctx.save_for_backward(g)
        return ops.reduce_sum(rows.view(-1), float(coeff) / rows.numel()), rows

    @staticmethod
    def backward(ctx, gout, grows):
        g, = ctx.saved_tensors
        if g is None or gout is None:
            return None, None, None, None, None
        if _rt.is_unit_grad(gout):
            return g, None, None, None, None
        return ops.scale_by_dev(g, gout.contiguous().float()), None, None, None, None


class JointsKLLoss(nn.Module):
    """KL Divergence for keypoint detection (RegDA).  ``reduction``: 'mean' | 'none'."""

    def __init__(self, reduction='mean', epsilon=0.):
        super().__init__()
        self.reduction = reduction
        self.epsilon = epsilon

    def forward(self, output, target, target_weight=None, scale=1.0):
        """``scale`` (extension, default 1 = reference): coefficient of this term in the total loss, folded into the kernel
        (the training step passes its 2 / 4 / trade-off factors here instead of multiplying 0-dim tensors)."""
        loss, rows = _KLFn.apply(output, target.detach(), target_weight, float(self.epsilon), float(scale))
        if self.reduction == 'mean':
            return loss
        elif self.reduction == 'none':
            return rows.detach().mean(dim=-1) * float(scale)     # forward-only, as no caller differentiates it


# ---------------------------------------------------------------- mean-teacher consistency (reference uda/model/loss.py:265-297)
# the joint curriculum of mt_loss: k < 100 the wrist, then one more joint per finger every 100, all joints from 400 on
MT_SUBSETS = ((100, (0,)),
              (200, (0, 1, 5, 9, 13, 17)),
              (300, (0, 1, 2, 5, 6, 9, 10, 13, 14, 17, 18)),
              (400, (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 18, 19)))


def mt_subset(k, num_joints):
    """The joints mt_loss(k) compares, as a tuple of channel indices."""
    for bound, joints in MT_SUBSETS:
        if k < bound:
            if joints[-1] >= num_joints:
                raise IndexError('mt_loss: joint %d of the k = %d subset, heat-maps have %d channels' % (joints[-1], k, num_joints))
            return joints
    return tuple(range(num_joints))


class _MSEFn(torch.autograd.Function):
    """loss = (*scale_dev) * sum(rows).  As _KLFn: the kernel writes d loss / d pred in the forward (its factor rides in the
    device record), the backward hands it on when the incoming gradient is the unit scalar."""

    @staticmethod
    def forward(ctx, pred, target, rec, scale_dev):
        rows, g = ops.mse_heatmap(pred, target, rec, ctx.needs_input_grad[0])
        ctx.save_for_backward(g)
        return ops.scale_by_dev(ops.reduce_sum(rows.view(-1)), scale_dev)

    @staticmethod
    def backward(ctx, gout):
        g, = ctx.saved_tensors
        if g is None or gout is None:
            return None, None, None, None
        if _rt.is_unit_grad(gout):
            return g, None, None, None
        return ops.scale_by_dev(g, gout.contiguous().float()), None, None, None


class MeanTeacherLoss:
    """``m * mt_loss(pre, label, weight, k)`` with everything that changes per epoch -- the joint mask, m / n and 2 m / n, n = B *
    |subset| * H * W -- in device memory: ``set()`` rewrites it (outside graph capture), a captured graph that contains the
    loss replays with the new values.  Both quotients are computed in double and rounded once to fp32."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.rec = torch.zeros(2, dtype=torch.int32, device=self.device)         # {int32 joint_mask, float grad_scale}
        self.scale = torch.zeros((), dtype=torch.float32, device=self.device)    # m / n
        self.state = None

    def set(self, m, k, shape):
        B, K, H, W = shape
        if K > 32:
            raise ValueError('mt_loss: at most 32 joints, got %d' % K)
        joints = mt_subset(k, K)
        mask = sum(1 << j for j in joints)
        n = B * len(joints) * H * W
        state = (float(m), mask, n)
        if state != self.state:
            ops.mse_record(mask, 2.0 * float(m) / n, out=self.rec)
            self.scale.copy_(torch.tensor(float(m) / n, dtype=torch.float64).to(torch.float32))
            self.state = state
        return self

    def __call__(self, pre, label):
        if self.state is None:
            raise RuntimeError('MeanTeacherLoss: set(m, k, shape) first')
        return _MSEFn.apply(pre, label.detach(), self.rec, self.scale)


_mt_cache = {}


def mt_loss(pre, label, weight, k):
    """The reference's ``mt_loss(pre, label, weight, k)``: ``MSELoss()`` (mean over every element) of the joints k selects;
    ``weight`` is accepted and ignored, as there.  Differentiable w.r.t. ``pre``."""
    B, K, H, W = pre.shape
    key = (pre.device, K, mt_subset(k, K), B * H * W)
    crit = _mt_cache.get(key)
    if crit is None:
        crit = _mt_cache[key] = MeanTeacherLoss(pre.device).set(1.0, k, (B, K, H, W))
    return crit(pre, label)


# ---------------------------------------------------------------- MMD alignment (reference uda/model/loss.py:1061-1196)
class _MMDFn(torch.autograd.Function):
    """loss = scale * mean over joints of the multi-kernel MMD between source and target (B, K, HW).  As _KLFn: the kernels
    write d loss / d source and / d target in the forward, for whichever of the two needs a gradient (the other side is
    neither allocated nor written); the backward hands them on when the incoming gradient is the unit scalar.  The bandwidth
    is a constant for the gradient, as the reference's ``.data`` makes it."""

    @staticmethod
    def forward(ctx, source, target, kernel_mul, kernel_num, fix_sigma, scale):
        rows, gs, gt = ops.mmd_heatmap(source, target, ctx.needs_input_grad[0], ctx.needs_input_grad[1], kernel_mul, kernel_num,
                                       fix_sigma, scale)
        ctx.save_for_backward(gs, gt)
        return ops.reduce_sum(rows, float(scale) / rows.numel())

    @staticmethod
    def backward(ctx, gout):
        gs, gt = ctx.saved_tensors
        if gout is None or (gs is None and gt is None):
            return None, None, None, None, None, None
        if not _rt.is_unit_grad(gout):
            gout = gout.contiguous().float()
            gs, gt = (None if g is None else ops.scale_by_dev(g, gout) for g in (gs, gt))
        return gs, gt, None, None, None, None


def _mmd_operand(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _mmd(source, target, kernel_mul, kernel_num, fix_sigma, scale):
    if tuple(source.shape) != tuple(target.shape):
        raise ValueError('MMD: source %s and target %s must have the same shape (the kernel matrix is sliced by one batch size)'
                         % (tuple(source.shape), tuple(target.shape)))
    return _MMDFn.apply(_mmd_operand(source), _mmd_operand(target), float(kernel_mul), int(kernel_num), fix_sigma, float(scale))


class MMD_loss3(nn.Module):
    """Per joint, the multi-Gaussian-kernel MMD between the batch of source heat-maps and the batch of target heat-maps
    (B, K, H, W), averaged over the joints (reference ``uda/model/loss.py:1061-1104``).

    ``scale`` (extension, default 1 = reference): coefficient of this term in the total loss, folded into the kernels.
    Extension: a joint whose 2 B maps are all identical has bandwidth 0, for which the reference returns NaN (0 / 0); here it
    contributes loss 0 and zero gradients -- the rule ``guard_empty_maps`` (regda_7.py) applies to empty pseudo-label maps."""

    def __init__(self, kernel_mul=2.0, kernel_num=5):
        super().__init__()
        self.kernel_num = kernel_num
        self.kernel_mul = kernel_mul
        self.fix_sigma = None

    def forward(self, source, target, scale=1.0):
        if source.dim() != 4:
            raise ValueError('MMD_loss3: (B, K, H, W) heat-maps, got %s' % (tuple(source.shape),))
        return _mmd(source, target, self.kernel_mul, self.kernel_num, self.fix_sigma, scale)


def mmd_rbf(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None, scale=1.0):
    """The reference's ``mmd_rbf`` (``uda/model/loss.py:1140-1161``) on (n, D) features: the same kernels with K = 1."""
    if source.dim() != 2:
        raise ValueError('mmd_rbf: (n, D) features, got %s' % (tuple(source.shape),))
    return _mmd(source.unsqueeze(1), target.unsqueeze(1), kernel_mul, kernel_num, fix_sigma, scale)


class MMD_loss(nn.Module):
    """Multi-kernel MMD between (n, D) source and target features (reference ``uda/model/loss.py:1164-1196``)."""

    def __init__(self, kernel_mul=2.0, kernel_num=5):
        super().__init__()
        self.kernel_num = kernel_num
        self.kernel_mul = kernel_mul
        self.fix_sigma = None

    def forward(self, source, target, scale=1.0):
        return mmd_rbf(source, target, self.kernel_mul, self.kernel_num, self.fix_sigma, scale)


# ---------------------------------------------------------------- joint feature alignment (reference uda/model/loss.py:331-378)
def _jfa_feature(feature):
    """The channels_last bf16 / fp32 tensor the kernels read: `feature` itself when it already is one (the neck output, whose
    GradFanIn then stays reachable), else its fp32 channels_last copy."""
    if feature.dim() != 4:
        raise ValueError('loss1: (B, C, H, W) features, got %s' % (tuple(feature.shape),))
    if ops.is_nhwc(feature) and feature.dtype in (torch.bfloat16, torch.float32):
        return feature
    if feature.dtype not in (torch.bfloat16, torch.float32):
        feature = feature.float()
    return feature.contiguous(memory_format=torch.channels_last)


def _jfa_points(pre, B):
    if pre.dim() != 3 or pre.shape[0] != B or pre.shape[2] != 2:
        raise ValueError('loss1: key points (B, K, 2) for %d images, got %s' % (B, tuple(pre.shape)))
    pre = pre.detach()
    return pre if (pre.dtype == torch.float32 and pre.is_contiguous()) else pre.float().contiguous()


class _JointPoolFn(torch.autograd.Function):
    """desc = joint_pool(feature, xy).  The backward is the gather ``jfa_scatter``.  A feature tensor that carries a
    ``mi355.nn.GradFanIn`` (the neck output, which the heads consume as well) gets its gradient through that protocol: when the
    fan-in buffer exists, this gradient is accumulated onto it in place and autograd is handed None; otherwise the buffer is
    written here, registered, and returned -- the convs that run later accumulate onto it.  Returning a dense tensor beside an
    existing buffer would make autograd add the two into a NEW tensor and lose every later in-place addition."""

    @staticmethod
    def forward(ctx, feature, xy, radius, axes, divisor, fan):
        ctx.args, ctx.fan = (radius, axes, divisor), fan
        ctx.like = (tuple(feature.shape), feature.dtype, feature.device)      # (the feature map itself is not kept)
        ctx.save_for_backward(xy)
        return ops.joint_pool(feature, xy, radius, axes, divisor)

    @staticmethod
    def backward(ctx, gdesc):
        xy, = ctx.saved_tensors
        shape, dtype, device = ctx.like
        if gdesc is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        radius, axes, divisor = ctx.args
        if gdesc.dtype != torch.float32 or not gdesc.is_contiguous():
            gdesc = gdesc.float().contiguous()
        fan = ctx.fan
        if fan is not None and fan.buf is not None and tuple(fan.buf.shape) == shape and fan.buf.dtype == dtype and ops.is_nhwc(fan.buf):
            ops.joint_scatter(gdesc, xy, fan.buf, True, radius, axes, divisor)
            return None, None, None, None, None, None
        B, C, H, W = shape
        dx = ops.joint_scatter(gdesc, xy, ops.nhwc_empty(B, C, H, W, dtype, device), False, radius, axes, divisor)
        if fan is not None:
            fan.buf = dx
        return dx, None, None, None, None, None


class _JointKLFn(torch.autograd.Function):
    """loss = scale * mean over (b, j) of KL(q(b) || softmax(a)) on descriptors a, b (B, K, C).  As _KLFn: the kernel writes
    d loss / d a and / d b in the forward, for whichever needs a gradient; the backward hands them on when the incoming gradient
    is the unit scalar."""

    @staticmethod
    def forward(ctx, a, b, scale):
        rows, ga, gb = ops.joint_kl(a, b, ctx.needs_input_grad[0], ctx.needs_input_grad[1], scale)
        ctx.save_for_backward(ga, gb)
        return ops.reduce_sum(rows.view(-1), float(scale) / rows.numel())

    @staticmethod
    def backward(ctx, gout):
        ga, gb = ctx.saved_tensors
        if gout is None or (ga is None and gb is None):
            return None, None, None
        if not _rt.is_unit_grad(gout):
            gout = gout.contiguous().float()
            ga, gb = (None if g is None else ops.scale_by_dev(g, gout) for g in (ga, gb))
        return ga, gb, None


def loss1(feature, pre, radius=6, axes='ref', scale=1.0):
    """The reference's ``loss1(feature, pre)`` (``uda/model/loss.py:331-365``): for every key point ``pre[b, j] = (x, y)`` in pixels
    of the map, the sum of ``feature[b]`` over the window ``int(max(. - radius, 0)) : int(min(. + radius, side - 1))`` on both axes,
    divided by ``(2 radius + 1)^2``; returns the descriptors (B, K, C) in fp32.  Differentiable w.r.t. ``feature``.

    ``axes='ref'`` slices the row axis by x and the column axis by y, as the reference does (transposed); ``axes='xy'`` is the
    geometric indexing (y selects the rows).  ``scale`` (extension) folds into the division: the kernels divide by
    ``(2 radius + 1)^2 / scale``.  Deviations from the reference: a coordinate outside the map gives an empty window and a zero
    descriptor (the reference falls into Python's negative-index slicing there); at sides other than 64 the upper clamp is
    ``side - 1`` instead of the constant 63; any K up to 32 instead of the constant 21."""
    f = _jfa_feature(feature)
    fan = getattr(feature, '_mi_fan', None) if (f is feature and torch.is_grad_enabled() and feature.requires_grad) else None
    return _JointPoolFn.apply(f, _jfa_points(pre, f.shape[0]), int(radius), axes, ops.joint_divisor(radius, scale), fan)


def joint_kl_loss(desc1, desc2, scale=1.0):
    """The part of ``loss3`` behind its two ``loss1`` calls, on ready descriptors (B, K, C): ``desc1`` goes through log_softmax (the
    prediction slot of KLDivLoss), ``desc2`` is normalised to a distribution after adding 1e-6."""
    if desc1.dim() != 3 or tuple(desc1.shape) != tuple(desc2.shape):
        raise ValueError('loss3: descriptors (B, K, C) of one shape, got %s and %s' % (tuple(desc1.shape), tuple(desc2.shape)))
    d1, d2 = (d if (d.dtype == torch.float32 and d.is_contiguous()) else d.float().contiguous() for d in (desc1, desc2))
    return _JointKLFn.apply(d1, d2, float(scale))


def loss3(f1, f2, pre1, pre2, radius=6, axes='ref', scale=1.0):
    """The reference's ``loss3(f1, f2, pre1, pre2)`` (``uda/model/loss.py:367-378``): the mean over (b, j) of the KL divergence
    between the channel distributions of ``loss1(f2, pre2)`` (plus 1e-6, normalised to sum 1) and ``softmax(loss1(f1, pre1))``.
    Both feature arguments may require a gradient.  ``radius``, ``axes``: as ``loss1``; ``scale`` (extension, default 1 =
    reference): coefficient of this term in the total loss, folded into the kernels.  ``loss1(f2, pre2) + 1e-6`` must be positive
    (the post-ReLU neck output always is); anything else is outside the contract."""
    for f, pre in ((f1, pre1), (f2, pre2)):                  # (both sides are checked before anything is launched)
        if f.dim() != 4:
            raise ValueError('loss3: (B, C, H, W) features, got %s' % (tuple(f.shape),))
        _jfa_points(pre, f.shape[0])
    if tuple(pre1.shape) != tuple(pre2.shape) or f1.shape[:2] != f2.shape[:2]:
        raise ValueError('loss3: the two sides must have one batch size, channel count and joint count, got features %s / %s, key points %s / %s'
                         % (tuple(f1.shape), tuple(f2.shape), tuple(pre1.shape), tuple(pre2.shape)))
    return joint_kl_loss(loss1(f1, pre1, radius, axes), loss1(f2, pre2, radius, axes), scale)
