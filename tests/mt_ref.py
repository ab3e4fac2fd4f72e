"""Numpy restatement of the mean-teacher kernels (csrc/teacher.hip), rounding for rounding.

`fold`: mi355/nn.py's `_fold_scale_shift` followed by the multiply -- every operation a single fp32 rounding, numpy's float32
divide and square root being correctly rounded like torch's.  `mt_loss` / `mt_grad`: the reference's `mt_loss`
(uda/model/loss.py:265-297; equal to its live function through tests/golden/g12_mt.npz) in float64 and the fp32 gradient
expression of mi355_mse_heatmap."""
import numpy as np

SUBSETS = ((100, (0,)),
           (200, (0, 1, 5, 9, 13, 17)),
           (300, (0, 1, 2, 5, 6, 9, 10, 13, 14, 17, 18)),
           (400, (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 18, 19)))
GOLDEN_KS = (0, 99, 100, 199, 200, 299, 300, 399, 400, 1000)


def subset(k, K=21):
    for bound, joints in SUBSETS:
        if k < bound:
            return joints
    return tuple(range(K))


def mask(k, K=21):
    return sum(1 << j for j in subset(k, K))


def fold(w, gamma, beta, mean, var, conv_bias, eps, axis):
    """w: fp32 [O][T][I] -> (out_w, out_bias); axis 0: the scale runs along O, axis 1: along I."""
    f = np.float32
    w, gamma, beta, mean, var = (np.asarray(a, dtype=f) for a in (w, gamma, beta, mean, var))
    with np.errstate(all='ignore'):
        scale = gamma / np.sqrt(var + f(eps))
        shift = beta - mean * scale
        if conv_bias is not None:
            shift = shift + np.asarray(conv_bias, dtype=f) * scale
        out = w * (scale.reshape(-1, 1, 1) if axis == 0 else scale.reshape(1, 1, -1))
    assert out.dtype == f and shift.dtype == f
    return out, shift


def mt_loss64(pre, label, k):
    """float64 value of MSELoss over the joints k selects."""
    j = list(subset(k, pre.shape[1]))
    d = pre[:, j].astype(np.float64) - label[:, j].astype(np.float64)
    return float((d * d).mean())


def mt_grad64(pre, label, k):
    j = list(subset(k, pre.shape[1]))
    g = np.zeros(pre.shape, dtype=np.float64)
    d = pre[:, j].astype(np.float64) - label[:, j].astype(np.float64)
    g[:, j] = 2.0 * d / d.size
    return g


def unit_grad(pre, label, joint_mask, grad_scale):
    """fp32 expression of mi355_mse_heatmap: fl(fl(p - t) * grad_scale), exact zeros outside the mask."""
    f = np.float32
    d = pre.astype(f) - label.astype(f)
    g = d * f(grad_scale)
    on = np.array([(joint_mask >> j) & 1 for j in range(pre.shape[1])], dtype=bool)
    g[:, ~on] = 0
    return g


def grad_scale(m, pre_shape, k):
    """float32(2 m / n), n = B * |subset| * H * W, the quotient in double."""
    B, K, H, W = pre_shape
    return np.float32(2.0 * m / (B * len(subset(k, K)) * H * W))


def loss_scale(m, pre_shape, k):
    B, K, H, W = pre_shape
    return np.float32(float(m) / (B * len(subset(k, K)) * H * W))


def golden_grad(g, case, k):
    """The reference's full gradient (B, K, H, W) from tests/golden/g12_mt.npz, which stores the channels that are not zero
    throughout and their indices; returns (gradient, those indices)."""
    joints = [int(j) for j in g['%s/joints_%d' % (case, k)]]
    as_k = '%s/grad_as_%d' % (case, k)                    # stored once where two k give the same gradient bit for bit
    part = g['%s/grad_%d' % (case, int(g[as_k]) if as_k in g.files else k)]
    full = np.zeros(g[case + '/pre'].shape, dtype=part.dtype)
    full[:, joints] = part
    return full, tuple(joints)
