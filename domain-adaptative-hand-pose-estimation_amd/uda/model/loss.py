"""``JointsKLLoss`` (reference ``uda/model/loss.py:115-158``) as one fused row kernel: log-softmax,
target normalisation, KL sum, weighting and the gradient w.r.t. the prediction in a single pass; ``mt_loss`` (reference
``uda/model/loss.py:265-297``), the mean-teacher consistency term, as one masked squared-difference row kernel; ``MMD_loss3``,
``MMD_loss`` and ``mmd_rbf`` (reference ``uda/model/loss.py:1061-1196``), the multi-kernel MMD between a source and a target
batch, as three launches that never form the reference's n x n x HW temporaries; ``loss1`` and ``loss3`` (reference
``uda/model/loss.py:331-378``), the per-joint feature alignment term, as a pooling kernel, a KL row kernel and a gather for the
pooling's backward instead of a Python loop over B x 21 windows; ``lossx`` and ``lossx3`` (reference ``uda/model/loss.py:381-466``,
``560-652``), the alignment of per-joint class prototypes blended with a running memory, as four launches whose memory lives at
fixed device addresses."""
import torch
import torch.nn as nn

from mi355 import ops
import mi355 as _rt


# ---------------------------------------------------------------- cross-domain mixup (reference uda/model/loss.py:13-24)
def draw_mixup_coefficients(batch, beta):
    """The B coefficients of the reference's mixup, drawn as it draws them (uda/model/loss.py:14-17): Beta(beta, beta) with
    float32 concentrations, ``rsample((B, 1, 1, 1))`` on the CPU from the global RNG, then ``max(mix, 1 - mix)``.  (B,) fp32."""
    check_positive('mixup: beta', beta)
    m = torch.distributions.beta.Beta(torch.tensor(float(beta)), torch.tensor(float(beta)))
    mix = m.rsample(sample_shape=(int(batch), 1, 1, 1))
    return torch.max(mix, 1 - mix).reshape(-1)


def mixup(img_src, hm_src, weights_src, img_trg, hm_trg, weights_trg, beta, mix=None):
    """The reference's ``mixup`` (name, positional signature and 6-tuple), as one ``mi355_mixup_pairs`` launch: returns
    ``(img_src_mix, hm_src_mix, weights, img_trg_mix, hm_trg_mix, weights)`` with the source-dominant blends ``a_src * mix + a_trg *
    (1 - mix)``, the target-dominant ones ``a_trg * mix + a_src * (1 - mix)`` and ``weights = max(weights_src, weights_trg)``, the
    same object twice.  The six results are views into the kernel's three outputs.  ``mix=None`` draws the coefficients as the
    reference does (``draw_mixup_coefficients``: the same ``torch.manual_seed`` gives the same blends); ``mix=`` B values (any
    device) are taken as they are -- the reference's ``mix`` behind its ``max(mix, 1 - mix)`` -- and nothing is drawn.  All inputs
    are data: no autograd graph is built."""
    B = img_src.size(0)
    if mix is None:
        mix = draw_mixup_coefficients(B, beta)
    lam = torch.as_tensor(mix, dtype=torch.float32).detach().reshape(-1).to(img_src.device).contiguous()
    if lam.numel() != B:
        raise ValueError('mixup: %d coefficients for a batch of %d' % (lam.numel(), B))
    dense = lambda t: t.detach().float().contiguous()
    x, hm, w = ops.mixup_pairs(dense(img_src), dense(hm_src), dense(weights_src), dense(img_trg), dense(hm_trg), dense(weights_trg), lam)
    weights = w[:B]
    return x[:B], hm[:B], weights, x[B:], hm[B:], weights


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


# ---------------------------------------------------------------- coordinate loss on the soft-arg-max (not in the reference)
class _CoordFn(torch.autograd.Function):
    """loss = coeff * mean(rows) of the coordinate loss; built like _KLFn: the kernel writes d loss / d pred in the forward, the
    backward hands it on under the unit scalar of ``mi355.unit_grad`` and multiplies it by the incoming gradient otherwise."""

    @staticmethod
    def forward(ctx, pred, coord, weight, beta, delta, coeff):
        ctx.set_materialize_grads(False)
        rows, g, uv = ops.coord_heatmap(pred, coord, weight, beta, delta, coeff, ctx.needs_input_grad[0])
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(uv)
        return ops.reduce_sum(rows.view(-1), float(coeff) / rows.numel()), rows, uv

    @staticmethod
    def backward(ctx, gout, grows, guv):
        g, = ctx.saved_tensors
        if g is None or gout is None:
            return None, None, None, None, None, None
        if _rt.is_unit_grad(gout):
            return g, None, None, None, None, None
        return ops.scale_by_dev(g, gout.contiguous().float()), None, None, None, None, None


class JointsCoordLoss(nn.Module):
    """Integral-regression loss (Sun et al., ECCV 2018; not in the reference): the expectation of ``softmax(beta * output)`` over
    the pixel grid is a differentiable key point (u, v) in heat-map pixels, compared with the continuous annotation ``coords``
    (B, K, 2) = (x, y) under smooth-L1 with threshold ``delta`` (``delta=0``: L1), summed over the two axes, times
    ``target_weight`` (B, K[, 1]), averaged over the B*K maps.  A joint of weight 0 is left out whatever its coordinates hold.
    One launch computes the loss and its gradient w.r.t. ``output``.  ``uv`` holds the soft-arg-max of the last call, detached."""

    def __init__(self, beta=1.0, delta=1.0):
        super().__init__()
        check_positive('JointsCoordLoss: beta', beta)
        if not 0.0 <= float(delta) < float('inf'):
            raise ValueError('JointsCoordLoss: delta must be finite and not negative, got %r' % (delta,))
        self.beta, self.delta = float(beta), float(delta)
        self.uv = None

    def forward(self, output, coords, target_weight=None, scale=1.0):
        """``scale``: coefficient of this term in the total loss, folded into the kernel as ``JointsKLLoss``'s."""
        w = None if target_weight is None else target_weight.detach()
        loss, _, self.uv = _CoordFn.apply(output, coords.detach(), w, self.beta, self.delta, float(scale))
        return loss


def soft_argmax(output, beta=1.0):
    """(B, K, 2) soft-arg-max of ``softmax(beta * output)`` in heat-map pixels, (x, y), detached."""
    return ops.softargmax(output.detach(), beta, 1.0)


def peak_confidence(y, beta=1.0):
    """(xy, p) of heat-maps ``y`` (B, K, H, W), detached: the arg-max (B, K, 2) in heat-map pixels, (x, y), and the peak (B, K) of
    ``softmax(beta * y)`` over each map (``mi355_peak_prob``) -- the confidence ``DAStep(teacher_conf=...)`` thresholds.  The raw
    maximum of a map is an unbounded logit; the peak of the softmax lies in (0, 1], and a perfect sigma = 2 label has 1 / (8 pi).
    A map that holds a NaN or an inf has p = NaN, which passes no threshold."""
    y = y.detach()
    y = y if (y.dtype == torch.float32 and y.is_contiguous()) else y.float().contiguous()
    _, xy, p = ops.peak_prob(y, beta)
    return xy, p


# ---------------------------------------------------------------- bone-ratio skeleton prior (not in the reference)
# (parent, child) pairs of the 21-joint hand of uda/dataset/keypoint_dataset.py:47-57: the wrist and five chains of four joints
HAND_BONES = tuple((0 if j % 4 == 1 else j - 1, j) for j in range(1, 21))


def _check_bones(bones):
    bones = tuple((int(p), int(c)) for p, c in bones)
    if not 1 <= len(bones) <= 32:
        raise ValueError('the bone table needs 1 .. 32 (parent, child) pairs, got %d' % len(bones))
    for p, c in bones:
        if p == c or not (0 <= p < 32 and 0 <= c < 32):
            raise ValueError('a bone joins two different joints in 0 .. 31, got %r' % ((p, c),))
    return bones


class BoneStatistics:
    """Running mean and variance of the bone-length ratios of the source annotations (mi355_bone_stats_update), per bone of the
    table ``bones``, and which bones have been seen at all.  ``table`` (E, 2) int32, ``mean`` / ``var`` (E,) fp32 and ``seen``
    (E,) int32 live at fixed device addresses from the first ``update`` (or ``to``) on, so a captured launch carries them from
    replay to replay and handles the first batch like any other.  ``momentum``: the weight of a batch in the blend."""

    def __init__(self, bones=HAND_BONES, momentum=0.01, device=None):
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError('BoneStatistics: the momentum must be in [0, 1], got %r' % (momentum,))
        self.bones, self.momentum = _check_bones(bones), float(momentum)
        self.num_joints = 1 + max(max(b) for b in self.bones)
        self.table = self.mean = self.var = self.seen = None
        self._pending = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Allocate the device buffers (outside graph capture); a state loaded earlier is copied in."""
        if self.table is None:
            if torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise _rt.Mi355Error('bone statistics would be allocated during graph capture: warm up first')
            E = len(self.bones)
            self.table = torch.tensor(self.bones, dtype=torch.int32).to(device)
            self.mean = torch.zeros(E, dtype=torch.float32, device=device)
            self.var = torch.zeros(E, dtype=torch.float32, device=device)
            self.seen = torch.zeros(E, dtype=torch.int32, device=device)
            if self._pending is not None:
                state, self._pending = self._pending, None
                self.load_state_dict(state)
        return self

    def update(self, kp, w=None):
        """Blend the batch ``kp`` (B, K, 2) with joint weights ``w`` (B, K[, 1]) into the statistics: one launch."""
        self.to(kp.device)
        if kp.shape[1] < self.num_joints:
            raise ValueError('BoneStatistics: the table names joint %d, the batch has %d joints' % (self.num_joints - 1, kp.shape[1]))
        ops.bone_stats_update(kp.detach(), None if w is None else w.detach(), self.table, self.mean, self.var, self.seen, self.momentum)

    def reset(self):
        self._pending = None
        if self.table is not None:
            self.mean.zero_(); self.var.zero_(); self.seen.zero_()

    def state_dict(self):
        """CPU copies of mean, var and seen (None before first use): what the epoch checkpoint keeps as ``bone_state``."""
        if self.table is None:
            return dict(self._pending) if self._pending is not None else {'mean': None, 'var': None, 'seen': None}
        return {k: getattr(self, k).detach().cpu().clone() for k in ('mean', 'var', 'seen')}

    def load_state_dict(self, state):
        if state.get('mean') is None:
            self.reset()
            return
        E = len(self.bones)
        for k in ('mean', 'var', 'seen'):
            if tuple(state[k].shape) != (E,):
                raise ValueError('BoneStatistics: %s of the state is %s, the table has %d bones' % (k, tuple(state[k].shape), E))
        if self.table is None:
            self._pending = {k: state[k].detach().cpu().clone() for k in ('mean', 'var', 'seen')}
            return
        self.mean.copy_(state['mean'].float()); self.var.copy_(state['var'].float())      # (in place: a captured graph keeps the addresses)
        self.seen.copy_(state['seen'].to(torch.int32))


def _bone_check(stats, K):
    if stats.table is None:
        raise _rt.Mi355Error('bone_prior: the statistics have no device buffers yet (BoneStatistics.update or .to first)')
    if K < stats.num_joints:
        raise ValueError('bone_prior: the table names joint %d, the prediction has %d joints' % (stats.num_joints - 1, K))


def _bone_backward(ctx, gout, n_in):
    g, = ctx.saved_tensors
    rest = (None,) * (n_in - 1)
    if g is None or gout is None:
        return (None,) + rest
    if _rt.is_unit_grad(gout):
        return (g,) + rest
    return (ops.scale_by_dev(g, gout.contiguous().float()),) + rest


class _BoneFn(torch.autograd.Function):
    """loss = coeff * mean(rows) of the bone-ratio prior on coordinates; the kernel writes d loss / d uv in the forward (_KLFn's
    scheme)."""

    @staticmethod
    def forward(ctx, uv, weight, stats, margin, eps, coeff):
        ctx.set_materialize_grads(False)
        rows, g = ops.bone_prior(uv, weight, stats.table, stats.mean, stats.var, stats.seen, margin, eps, coeff, ctx.needs_input_grad[0])
        ctx.save_for_backward(g)
        return ops.reduce_sum(rows, float(coeff) / rows.numel()), rows

    @staticmethod
    def backward(ctx, gout, grows):
        return _bone_backward(ctx, gout, 6)


def bone_prior(uv, weight, stats, margin=1.0, eps=1e-4, scale=1.0):
    """The bone-ratio prior of the points ``uv`` (B, K, 2) against ``stats`` (a ``BoneStatistics``), differentiable w.r.t. ``uv``:
    per sample, the lengths of the present bones (both joints of weight > 0, bone seen in the statistics) divided by their mean
    are standardised by the running mean and variance, and what exceeds ``margin`` standard deviations is penalised
    quadratically; the mean over the batch, times ``scale``.  Invariant to rotation, scale and shift of a sample."""
    _bone_check(stats, uv.shape[1])
    w = None if weight is None else weight.detach()
    return _BoneFn.apply(uv, w, stats, float(margin), float(eps), float(scale))[0]


class _BoneHeatmapFn(torch.autograd.Function):
    """The same loss on heat-maps: soft-arg-max -> bone prior -> backward of the soft-arg-max, three launches in the forward."""

    @staticmethod
    def forward(ctx, pred, weight, stats, beta, margin, eps, coeff):
        ctx.set_materialize_grads(False)
        uv = ops.softargmax(pred, beta, 1.0)
        want = ctx.needs_input_grad[0]
        rows, g_uv = ops.bone_prior(uv, weight, stats.table, stats.mean, stats.var, stats.seen, margin, eps, coeff, want)
        ctx.save_for_backward(ops.softargmax_backward(pred, g_uv, beta) if want else None)
        ctx.mark_non_differentiable(uv)
        return ops.reduce_sum(rows, float(coeff) / rows.numel()), rows, uv

    @staticmethod
    def backward(ctx, gout, grows, guv):
        return _bone_backward(ctx, gout, 7)


class BonePriorLoss(nn.Module):
    """``bone_prior`` on the soft-arg-max of ``softmax(beta * output)`` (B, K, H, W), with its gradient w.r.t. the heat-maps.
    ``uv`` holds the soft-arg-max of the last call, detached."""

    def __init__(self, beta=1.0, margin=1.0, eps=1e-4):
        super().__init__()
        check_positive('BonePriorLoss: beta', beta)
        check_positive('BonePriorLoss: eps', eps)
        if not 0.0 <= float(margin) < float('inf'):
            raise ValueError('BonePriorLoss: the margin must be finite and not negative, got %r' % (margin,))
        self.beta, self.margin, self.eps = float(beta), float(margin), float(eps)
        self.uv = None

    def forward(self, output, weight, stats, scale=1.0):
        _bone_check(stats, output.shape[1])
        w = None if weight is None else weight.detach()
        loss, _, self.uv = _BoneHeatmapFn.apply(output, w, stats, self.beta, self.margin, self.eps, float(scale))
        return loss


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


class _MSEWFn(torch.autograd.Function):
    """_MSEFn with a per-map weight in device memory (mi355_mse_heatmap_w): loss = (*scale_dev) * sum_r w_r * rows_r; maps with
    weight 0 are neither read nor given a gradient other than zeros."""

    @staticmethod
    def forward(ctx, pred, target, rec, scale_dev, wmap):
        pred, target = ops._hm(pred), ops._hm(target)            # (as mse_heatmap takes them)
        B, K = pred.shape[:2]
        rows = torch.empty((B, K), dtype=torch.float32, device=pred.device)
        g = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        ops.mse_heatmap_w(pred, target, rec, wmap, g is not None, rows=rows, grad=g)
        ctx.save_for_backward(g)
        return ops.scale_by_dev(ops.reduce_sum(rows.view(-1)), scale_dev)

    @staticmethod
    def backward(ctx, gout):
        g, = ctx.saved_tensors
        if g is None or gout is None:
            return None, None, None, None, None
        if _rt.is_unit_grad(gout):
            return g, None, None, None, None
        return ops.scale_by_dev(g, gout.contiguous().float()), None, None, None, None


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

    def __call__(self, pre, label, wmap=None):
        """wmap: optional (B, K) fp32 per-map weights on the device (the flags of a geometric teacher view); n stays B * |subset| * H * W."""
        if self.state is None:
            raise RuntimeError('MeanTeacherLoss: set(m, k, shape) first')
        if wmap is None:
            return _MSEFn.apply(pre, label.detach(), self.rec, self.scale)
        return _MSEWFn.apply(pre, label.detach(), self.rec, self.scale, wmap.detach())


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


def _fan_in_scatter(fan, like, scatter):
    """The gradient of a pooled feature map, through the ``mi355.nn.GradFanIn`` protocol: ``scatter(out, accumulate)`` runs the
    gather into ``out``.  When the fan-in buffer exists, the gradient is accumulated onto it in place and None is returned (for
    autograd); otherwise a new map is written, registered as the buffer when there is a fan-in, and returned -- the convs that
    run later accumulate onto it.  Returning a dense tensor beside an existing buffer would make autograd add the two into a NEW
    tensor and lose every later in-place addition."""
    shape, dtype, device = like
    if fan is not None and fan.buf is not None and tuple(fan.buf.shape) == shape and fan.buf.dtype == dtype and ops.is_nhwc(fan.buf):
        scatter(fan.buf, True)
        return None
    B, C, H, W = shape
    dx = scatter(ops.nhwc_empty(B, C, H, W, dtype, device), False)
    if fan is not None:
        fan.buf = dx
    return dx


def _keep_for_scatter(ctx, feature, fan, args, *tensors):
    """What the backward of a pooling function needs: the feature map's shape, dtype and device (the map itself is not kept), its
    fan-in, the window arguments and the small tensors."""
    ctx.args, ctx.fan = args, fan
    ctx.like = (tuple(feature.shape), feature.dtype, feature.device)
    ctx.save_for_backward(*tensors)


def _scatter_backward(ctx, g, scatter):
    """The feature gradient of a pooling function, or None: ``scatter(g, out, accumulate)`` gathers the fp32 contiguous incoming
    gradient ``g`` into ``out`` (``_fan_in_scatter``)."""
    if g is None or not ctx.needs_input_grad[0]:
        return None
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.float().contiguous()
    return _fan_in_scatter(ctx.fan, ctx.like, lambda out, acc: scatter(g, out, acc))


def _kl_backward(ctx, gout):
    """The two gradients a KL function's forward saved (either may be None), times the incoming gradient unless it is the unit
    scalar."""
    ga, gb = ctx.saved_tensors
    if gout is None or (ga is None and gb is None):
        return None, None
    if not _rt.is_unit_grad(gout):
        gout = gout.contiguous().float()
        ga, gb = (None if g is None else ops.scale_by_dev(g, gout) for g in (ga, gb))
    return ga, gb


class _JointPoolFn(torch.autograd.Function):
    """desc = joint_pool(feature, xy).  The backward is the gather ``jfa_scatter``.  A feature tensor that carries a
    ``mi355.nn.GradFanIn`` (the neck output, which the heads consume as well) gets its gradient through that protocol: when the
    fan-in buffer exists, this gradient is accumulated onto it in place and autograd is handed None; otherwise the buffer is
    written here, registered, and returned (``_fan_in_scatter``)."""

    @staticmethod
    def forward(ctx, feature, xy, radius, axes, divisor, fan):
        _keep_for_scatter(ctx, feature, fan, (radius, axes, divisor), xy)
        return ops.joint_pool(feature, xy, radius, axes, divisor)

    @staticmethod
    def backward(ctx, gdesc):
        xy, = ctx.saved_tensors
        return (_scatter_backward(ctx, gdesc, lambda g, out, acc: ops.joint_scatter(g, xy, out, acc, *ctx.args)),) + (None,) * 5


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
        return _kl_backward(ctx, gout) + (None,)


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


# ---------------------------------------------------------------- prototype alignment (reference uda/model/loss.py:381-466, 560-652)
class _ProtoFn(torch.autograd.Function):
    """P = m * mean_b pool(feature, xy)[b] + (1 - m) * memory, and memory <- P in place: ``proto_pool`` and ``proto_update``.  The
    backward is the gather ``proto_scatter``, which reads the (K, C) gradient broadcast over the batch; the feature gradient goes
    through ``_fan_in_scatter`` as ``_JointPoolFn``'s does."""

    @staticmethod
    def forward(ctx, feature, xy, memory, blend, radius, axes, fan):
        _keep_for_scatter(ctx, feature, fan, (radius, axes), xy, blend)
        return ops.proto_update(ops.proto_pool(feature, xy, radius, axes), memory, blend)

    @staticmethod
    def backward(ctx, gp):
        xy, blend = ctx.saved_tensors
        return (_scatter_backward(ctx, gp, lambda g, out, acc: ops.proto_scatter(g, xy, blend, out, acc, *ctx.args)),) + (None,) * 6


class _ProtoKLFn(torch.autograd.Function):
    """loss = scale * mean_j rows ('kl') or scale * sum_j rows ('softkl') on prototypes pt, ps (K, C).  Gradients as _JointKLFn's."""

    @staticmethod
    def forward(ctx, pt, ps, mode, scale):
        rows, gt, gs = ops.proto_kl(pt, ps, ctx.needs_input_grad[0], ctx.needs_input_grad[1], mode, scale)
        ctx.save_for_backward(gt, gs)
        return ops.reduce_sum(rows, float(scale) / rows.numel() if mode == 'kl' else float(scale))

    @staticmethod
    def backward(ctx, gout):
        return _kl_backward(ctx, gout) + (None, None)


def prototype(feature, pre, memory, blend, radius=6, axes='ref'):
    """The reference's ``lossx.loss1(feature, pre, fea)`` (``uda/model/loss.py:394-449``): per joint, the window mean of
    ``feature[b]`` around ``pre[b, j] = (x, y)`` -- the sum over ``int(max(. - radius, 0)) : int(min(. + radius, side - 1))`` on
    both axes divided by the window's own ``s1 * s2``, ``s = hi - lo + 1`` -- averaged over the batch and blended with ``memory``
    (K, C): ``P = m * mean + (1 - m) * memory``.  Returns P (K, C) fp32 and overwrites ``memory`` with it in place (the reference's
    ``self.val1 = fea_c1.detach()``).  ``blend = ops.proto_blend(m)`` holds m on the device.  Differentiable w.r.t. ``feature``.
    ``axes`` and the deviations from the reference (empty windows outside the map and for NaN, the clamp ``side - 1``, any K up
    to 32) are ``loss1``'s."""
    f = _jfa_feature(feature)
    fan = getattr(feature, '_mi_fan', None) if (f is feature and torch.is_grad_enabled() and feature.requires_grad) else None
    return _ProtoFn.apply(f, _jfa_points(pre, f.shape[0]), memory, blend, int(radius), axes, fan)


def prototype_kl_loss(proto_t, proto_s, criterion='kl', scale=1.0):
    """The part of ``lossx`` (``criterion='kl'``, ``uda/model/loss.py:455-466``) or ``lossx3`` (``'softkl'``, ``:645``) behind the
    two prototypes (K, C): ``proto_t`` goes through log_softmax; ``proto_s`` is normalised to sum 1 ('kl', mean over the joints)
    or goes through softmax ('softkl', sum over the joints).  Deviation: under 'kl' a joint whose source prototype sums to 0 or
    less contributes 0 and gets zero gradients (the reference returns NaN)."""
    if proto_t.dim() != 2 or tuple(proto_t.shape) != tuple(proto_s.shape):
        raise ValueError('prototype_kl_loss: prototypes (K, C) of one shape, got %s and %s' % (tuple(proto_t.shape), tuple(proto_s.shape)))
    if criterion not in ops.PROTO_MODES:
        raise ValueError("prototype_kl_loss: criterion must be 'kl' or 'softkl', got %r" % (criterion,))
    pt, ps = (p if (p.dtype == torch.float32 and p.is_contiguous()) else p.float().contiguous() for p in (proto_t, proto_s))
    return _ProtoKLFn.apply(pt, ps, criterion, float(scale))


class PrototypeMemory:
    """The running memory of one side, (K, C) fp32 at a fixed device address once first used, and the device record of m."""

    def __init__(self):
        self.val = 0.

    def tensor(self, K, C, device):
        """The memory as a tensor: allocated as zeros (the reference's scalar 0., bit for bit) the first time it is asked for."""
        if not torch.is_tensor(self.val):
            if torch.cuda.is_current_stream_capturing():
                raise _rt.Mi355Error('prototype memory (%d, %d) would be allocated during graph capture: warm up first' % (K, C))
            self.val = torch.full((K, C), float(self.val), dtype=torch.float32, device=device)
        if tuple(self.val.shape) != (K, C) or self.val.device != torch.device(device):
            raise ValueError('prototype memory is %s on %s, the prototypes are (%d, %d) on %s: reset() belongs to one shape'
                             % (tuple(self.val.shape), self.val.device, K, C, device))
        return self.val

    def reset(self):
        if torch.is_tensor(self.val):
            self.val.zero_()
        else:
            self.val = 0.

    def set(self, val):
        if torch.is_tensor(self.val) and torch.is_tensor(val):
            self.val.copy_(val)                 # (in place: a captured graph keeps the address)
        elif torch.is_tensor(val):
            self.val = val.detach().to(torch.float32).contiguous().clone()
        elif torch.is_tensor(self.val):
            self.val.fill_(float(val))
        else:
            self.val = float(val)


# The range checks of the alignment terms' options: one text each, under the name `what` of whoever asks (a class's argument or a
# command-line flag).
def check_positive(what, v):
    if not v > 0:
        raise ValueError('%s must be positive, got %r' % (what, v))


def check_whole(what, n, most=None):
    """A whole number from 1 on (to `most`): a radius, a kernel count."""
    if not 1 <= int(n) <= (most or int(n)) or int(n) != n:
        raise ValueError('%s must be %s, got %r' % (what, '1 .. %d' % most if most else 'an integer of at least 1', n))


def check_axes(what, axes):
    if axes not in ops.JFA_AXES:
        raise ValueError("%s must be 'xy' or 'ref', got %r" % (what, axes))


def check_blend_weight(what, m):
    if not 0.0 < float(m) <= 1.0:
        raise ValueError('%s must be in (0, 1], got %r' % (what, m))


class PrototypeState:
    """What a prototype term carries from call to call: the running memory of either side (``mems``), the window arguments, m and
    its device record.  ``who`` names the owner in messages; ``max_radius``: the owner's bound on the radius, if it has one."""

    def __init__(self, who, radius, axes, m, max_radius=None):
        check_whole(who + ': the radius', radius, max_radius)
        check_axes(who + ': axes', axes)
        check_blend_weight(who + ': m', m)
        self.who, self.radius, self.axes, self.m = who, int(radius), axes, float(m)
        self.mems, self.blend = (PrototypeMemory(), PrototypeMemory()), None

    def set_m(self, m):
        """Change m (outside graph capture): the device record is rewritten in place, so a captured graph that contains the loss
        follows."""
        check_blend_weight(self.who + ': m', m)
        self.m = float(m)
        if self.blend is not None:
            ops.proto_blend(self.m, out=self.blend)

    def reset(self):
        for mem in self.mems:
            mem.reset()

    def prototype(self, side, f, pre):
        """``prototype(f, pre, .)`` against the memory of ``side`` (0 or 1), which it updates."""
        if self.blend is None or self.blend.device != f.device:
            self.blend = ops.proto_blend(self.m, device=f.device)
        return prototype(f, pre, self.mems[side].tensor(pre.shape[1], f.shape[1], f.device), self.blend, self.radius, self.axes)


class _ProtoLoss(nn.Module):
    criterion = None

    def __init__(self, reduction='mean', epsilon=0., radius=6, axes='ref', m=0.999, scale=1.0):
        super().__init__()
        self.reduction, self.epsilon = reduction, epsilon            # (kept for the signature; the reference ignores both)
        self.state, self.scale = PrototypeState(type(self).__name__, radius, axes, m), float(scale)
        self.reset, self.set_m = self.state.reset, self.state.set_m

    val1 = property(lambda self: self.state.mems[0].val)
    val2 = property(lambda self: self.state.mems[1].val)
    m = property(lambda self: self.state.m)

    def updata(self, val1, val2):
        self.state.mems[0].set(val1)
        self.state.mems[1].set(val2)

    def forward(self, f1, f2, pre1, pre2):
        for f, pre in ((f1, pre1), (f2, pre2)):                  # (both sides are checked before anything is launched)
            if f.dim() != 4:
                raise ValueError('%s: (B, C, H, W) features, got %s' % (type(self).__name__, tuple(f.shape)))
            _jfa_points(pre, f.shape[0])
        if pre1.shape[1] != pre2.shape[1] or f1.shape[1] != f2.shape[1]:
            raise ValueError('%s: the two sides must have one channel count and joint count, got features %s / %s, key points %s / %s'
                             % (type(self).__name__, tuple(f1.shape), tuple(f2.shape), tuple(pre1.shape), tuple(pre2.shape)))
        return prototype_kl_loss(self.state.prototype(0, f1, pre1), self.state.prototype(1, f2, pre2), self.criterion, self.scale)


class lossx(_ProtoLoss):
    """The reference's ``lossx`` (``uda/model/loss.py:381-466``): ``forward(f1, f2, pre1, pre2)`` is the mean over the joints of the
    KL divergence between the source prototype ``P2[j]`` normalised to sum 1 and ``softmax(P1[j])``, where ``P = m * (batch mean
    of the window means) + (1 - m) * memory`` (``prototype``) and the memories ``val1`` / ``val2`` are overwritten with the
    prototypes at every call.  ``reset()`` zeroes them, ``updata(val1, val2)`` (sic) copies into them; they are the float ``0.``
    until first used and (K, C) fp32 device tensors at fixed addresses from then on.  Either feature argument may require a
    gradient.  ``reduction`` and ``epsilon`` are accepted and ignored, as there.

    Extensions: ``radius`` (6 there), ``axes`` ('ref': x selects the rows, as there; 'xy': y does), ``m`` (0.999 there, the weight
    of the current batch), ``scale`` (coefficient of the term, folded into the kernels).  Deviations from the reference: a
    coordinate outside the map, or NaN, gives an empty window and a zero descriptor; at sides other than 64 the upper clamp is
    ``side - 1``; any K up to 32; a joint whose source prototype sums to 0 or less contributes 0 to the loss and gets zero
    gradients (the reference returns NaN for an all-zero source); the source gradient of an element whose prototype is exactly
    0 is 0 (the reference's autograd gives -inf there)."""
    criterion = 'kl'


class lossx3(_ProtoLoss):
    """The reference's ``lossx3`` (``uda/model/loss.py:560-652``): as ``lossx`` with the softmax of both prototypes and the sum
    over joints and channels (``F.kl_div(P1.softmax(-1).log(), P2.softmax(-1), reduction='sum')``).  Extensions and deviations
    as ``lossx``'s, without the zero-sum rule (a softmax has no zero sum)."""
    criterion = 'softkl'
