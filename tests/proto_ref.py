"""Prototype alignment in numpy: a restatement of the reference's lossx / lossx3 (uda/model/loss.py:381-466, 560-652) with the
options the kernels add (radius, axes, sides other than 64, m, scale), its closed-form gradients, the exact-order fp32 models of
the proto_pool / proto_update / proto_scatter kernels, and the tolerance rule of the GPU tests.  Test infrastructure only."""
import numpy as np

import jfa_ref
from jfa_ref import windows, bf16_round, errors            # noqa: F401  (the windows are loss1's)


def divisors(win):
    """(B, K) int: s_row * s_col, s = hi - lo + 1 -- ONE MORE than the pixels the half-open slice sums (the reference's s1 * s2);
    1 for an empty window, where nothing is divided."""
    r0, r1, q0, q1 = (win[..., i] for i in range(4))
    empty = (r1 <= r0) | (q1 <= q0)
    return np.where(empty, 1, (r1 - r0 + 1) * (q1 - q0 + 1))


def pool(feature, pre, radius=6, axes='ref', dtype=np.float64):
    """lossx.loss1 up to its stack: desc (B, K, C) from feature (B, C, H, W) and pre (B, K, 2); an empty window gives zeros."""
    feature = np.asarray(feature, dtype)
    B, C, H, W = feature.shape
    win = windows(pre, H, W, radius, axes)
    div = divisors(win)
    desc = np.zeros((B, win.shape[1], C), dtype)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):
            if r1 > r0 and q1 > q0:
                desc[b, j] = feature[b, :, r0:r1, q0:q1].sum(axis=(1, 2), dtype=dtype) / dtype(div[b, j])
    return desc


def blend(desc, memory, m=0.999, dtype=np.float64):
    """P (K, C) = m * mean_b desc + (1 - m) * memory; (1 - m) is formed in double, as the reference's Python floats are."""
    desc = np.asarray(desc, dtype)
    pbar = desc.sum(0, dtype=dtype) / dtype(desc.shape[0])
    return dtype(m) * pbar + dtype(1.0 - m) * np.asarray(memory, dtype)


def criterion(pt, ps, mode='kl', scale=1.0, dtype=np.float64):
    """(loss, rows (K,), d loss / d pt, d loss / d ps).  'kl' (lossx): q = ps / sum ps, loss = scale * mean rows; a joint with
    sum ps <= 0 has row 0 and zero gradients; an element with q = 0 adds 0 and has source gradient 0.  'softkl' (lossx3): q =
    softmax(ps), loss = scale * sum rows."""
    pt, ps = np.asarray(pt, dtype), np.asarray(ps, dtype)
    K = pt.shape[0]
    mt = pt.max(-1, keepdims=True)
    lp = (pt - mt) - np.log(np.exp(pt - mt).sum(-1, keepdims=True, dtype=dtype))
    with np.errstate(divide='ignore', invalid='ignore'):
        if mode == 'kl':
            S = ps.sum(-1, keepdims=True, dtype=dtype)
            dead = ~(S > 0)
            Ssafe = np.where(dead, 1, S)
            q = ps / Ssafe
            lq = np.log(q)
            coef = dtype(scale / K)
        else:
            ms = ps.max(-1, keepdims=True)
            lq = (ps - ms) - np.log(np.exp(ps - ms).sum(-1, keepdims=True, dtype=dtype))
            q = np.exp(lq)
            dead = np.zeros((K, 1), bool)
            coef = dtype(scale)
        zero = q == 0
        d = np.where(zero, 0, lq - lp)
        rows = np.where(dead[:, 0], 0, (q * d).sum(-1, dtype=dtype))
        gt = np.where(dead, 0, coef * (np.exp(lp) - q))
        if mode == 'kl':
            gs = np.where(dead | zero, 0, coef * ((d - rows[:, None]) / Ssafe))
        else:
            gs = np.where(zero, 0, coef * q * (d - rows[:, None]))
    loss = dtype(rows.sum(dtype=dtype) * coef)
    return loss, rows.astype(dtype), gt.astype(dtype), gs.astype(dtype)


def scatter(gproto, pre, shape, m=0.999, radius=6, axes='ref', dtype=np.float64):
    """The backward of pool + blend: (B, C, H, W) with sum_j gproto[j] * (m / B) / divisor(b, j) on every pixel of joint j's window."""
    B, C, H, W = shape
    win = windows(pre, H, W, radius, axes)
    div = divisors(win)
    g = np.zeros(shape, dtype)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):
            if r1 > r0 and q1 > q0:
                g[b, :, r0:r1, q0:q1] += (np.asarray(gproto[j], dtype) * dtype(m / B) / dtype(div[b, j]))[:, None, None]
    return g


class Loss:
    """lossx (mode 'kl') / lossx3 ('softkl') with its two memories: call(f1, f2, pre1, pre2) -> dict loss, grad_f1, grad_f2, val1,
    val2, proto1, proto2 (gradients per `want`)."""

    def __init__(self, mode='kl', radius=6, axes='ref', m=0.999, scale=1.0, dtype=np.float64):
        self.mode, self.radius, self.axes, self.m, self.scale, self.dtype = mode, radius, axes, m, scale, dtype
        self.reset()

    def reset(self):
        self.val1, self.val2 = 0., 0.

    def updata(self, val1, val2):
        self.val1, self.val2 = val1, val2

    def __call__(self, f1, f2, pre1, pre2, want=(True, True)):
        dt = self.dtype
        p1 = blend(pool(f1, pre1, self.radius, self.axes, dt), self.val1, self.m, dt)
        p2 = blend(pool(f2, pre2, self.radius, self.axes, dt), self.val2, self.m, dt)
        self.val1, self.val2 = p1.copy(), p2.copy()
        loss, rows, gt, gs = criterion(p1, p2, self.mode, self.scale, dt)
        g1 = scatter(gt, pre1, np.shape(f1), self.m, self.radius, self.axes, dt) if want[0] else None
        g2 = scatter(gs, pre2, np.shape(f2), self.m, self.radius, self.axes, dt) if want[1] else None
        return dict(loss=loss, rows=rows, grad_f1=g1, grad_f2=g2, val1=p1, val2=p2, grad_p1=gt, grad_p2=gs)


# ---------------------------------------------------------------- exact-order fp32 models of the kernels
def blend_record(m):
    """{m, 1 - m} as the two fp32 the kernels read: each formed in double and rounded once."""
    return np.float32(m), np.float32(1.0 - float(m))


def pool_model(feature_nhwc, pre, radius=6, axes='ref'):
    """fp32 model of proto_pool for operands whose window sums are exact in fp32 (small integers): the sum in any order, then
    one fp32 division by the window's divisor; zeros for an empty window.  feature_nhwc: (B, H, W, C)."""
    f = np.asarray(feature_nhwc, np.float32)
    B, H, W, C = f.shape
    win = windows(pre, H, W, radius, axes)
    div = divisors(win)
    desc = np.zeros((B, win.shape[1], C), np.float32)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):
            if r1 > r0 and q1 > q0:
                s = f[b, r0:r1, q0:q1].sum(axis=(0, 1), dtype=np.float64).astype(np.float32)
                desc[b, j] = s / np.float32(div[b, j])
    return desc


def update_model(desc, memory, m):
    """fp32 model of proto_update: b ascending, one division by B, two products and one sum."""
    desc = np.asarray(desc, np.float32)
    s = desc[0].copy()
    for b in range(1, desc.shape[0]):
        s = s + desc[b]
    mm, om = blend_record(m)
    return (mm * (s / np.float32(desc.shape[0])) + om * np.asarray(memory, np.float32)).astype(np.float32)


def scatter_model(gproto, pre, shape, m, radius=6, axes='ref', onto=None, round_to=None):
    """The exact-order fp32 model of the proto_scatter kernel, on NHWC arrays (B, H, W, C): gd = fp32(fp32(gproto * fp32(m / B)) /
    divisor) once per (b, j, c); per pixel the fp32 sum of gd[b, j] over the covering joints in ascending j; write mode
    (onto=None): that sum, +0 where no window covers; accumulate mode: fp32(onto) + sum on the covered pixels, `onto` untouched
    elsewhere.  `round_to` rounds an fp32 array to the storage type (None: fp32 storage)."""
    B, H, W, C = shape
    win = windows(pre, H, W, radius, axes)
    div = divisors(win)
    fac = np.float32(blend_record(m)[0] / np.float32(B))
    gp = (np.asarray(gproto, np.float32) * fac).astype(np.float32)
    s = np.zeros(shape, np.float32)
    cov = np.zeros((B, H, W), bool)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):           # ascending j: every pixel's sum runs in the kernel's order
            if r1 > r0 and q1 > q0:
                s[b, r0:r1, q0:q1] = s[b, r0:r1, q0:q1] + (gp[j] / np.float32(div[b, j])).astype(np.float32)
                cov[b, r0:r1, q0:q1] = True
    rnd = (lambda v: v) if round_to is None else round_to
    if onto is None:
        return rnd(s), cov
    out = np.array(onto, copy=True)
    tot = (np.asarray(onto, np.float32) + s).astype(np.float32)
    out[cov] = rnd(tot)[cov]
    return out, cov


# ---------------------------------------------------------------- fixture access and the tolerance rule
def fixture_calls(g, case):
    """[(f1, f2, pre1, pre2)] fp32 for the three calls of a case of tests/golden/g16_proto.npz (features stored as uint8 codes f * 4)."""
    return [tuple(g['%s/%d/%s_q4' % (case, i, n)].astype(np.float32) / np.float32(4) for n in ('f1', 'f2')) +
            (g['%s/%d/pre1' % (case, i)], g['%s/%d/pre2' % (case, i)]) for i in range(3)]


KEYS = ('loss', 'grad_f1', 'grad_f2', 'val1', 'val2')


def fixture_results(g, case, cls, i, suffix=''):
    return {k: g['%s/%d/%s/%s%s' % (case, i, cls, k, suffix)] for k in KEYS}


# The floors of the tolerance, as fractions of |loss|, of max |grad| and of max |prototype|: jfa_ref's, which rest on the same kind
# of arithmetic (a KL row that is a small difference of large logarithms, a box mean, a piecewise constant gradient).  Over the
# fixture (tests/golden/g16_proto.npz) the reference's own float32 run is at most 1.9e-5 (relative) from its float64 run on the
# loss; on the gradients and the memories it is at or above the floors, so there 4 times its own distance is what binds
# (tests/test_proto_cpu.py prints the figures).  None of them comes from a kernel run.
LOSS_FLOOR, GRAD_FLOOR, PROTO_FLOOR = jfa_ref.LOSS_FLOOR, jfa_ref.GRAD_FLOOR, jfa_ref.DESC_FLOOR


def bounds(ref32, ref64):
    """The tolerance rule, as jfa_ref.bounds: a kernel result may be as far from the float64 reference as 4 times the
    reference's own float32 run is from it, with the floors above.  ref32, ref64: dicts under the keys 'loss', 'grad_f1', 'grad_f2',
    'val1', 'val2' (any subset; None values skipped).  Returns (own, bound): the float32 run's own distances and the bounds."""
    return jfa_ref.bounds(ref32, ref64, floors=dict(val1=PROTO_FLOOR, val2=PROTO_FLOOR))
