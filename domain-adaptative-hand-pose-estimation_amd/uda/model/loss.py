"""``JointsKLLoss`` (reference ``uda/model/loss.py:115-158``) as one fused row kernel: log-softmax,
target normalisation, KL sum, weighting and the gradient w.r.t. the prediction in a single pass; ``mt_loss`` (reference
``uda/model/loss.py:265-297``), the mean-teacher consistency term, as one masked squared-difference row kernel; ``MMD_loss3``,
``MMD_loss`` and ``mmd_rbf`` (reference ``uda/model/loss.py:1061-1196``), the multi-kernel MMD between a source and a target
batch, as three launches that never form the reference's n x n x HW temporaries."""
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
