"""Joint feature alignment in numpy: a restatement of the reference's loss1 / loss3 (uda/model/loss.py:331-378) with the options
the kernels add (radius, axes, sides other than 64, scale), its closed-form gradients, the exact-order fp32 model of the
jfa_scatter kernel, and the tolerance rule of the GPU tests.  Test infrastructure only."""
import numpy as np


def windows(pre, H, W, radius=6, axes='ref'):
    """(B, K, 4) int: rows [r0, r1) x columns [q0, q1) of every joint's window.  fp32 arithmetic and truncation towards zero as
    the reference's clamp(...).int(); axes='ref': x selects the rows (the reference), 'xy': y selects the rows.  A window with
    r1 <= r0 or q1 <= q0 is empty; a NaN coordinate gives the empty window (0, 0, 0, 0)."""
    pre = np.asarray(pre, np.float32)
    nan = np.isnan(pre).any(-1)
    pre = np.where(nan[..., None], np.float32(0), pre)
    rad = np.float32(radius)
    x, y = pre[..., 0], pre[..., 1]
    cr, cc = (x, y) if axes == 'ref' else (y, x)
    r0 = np.trunc(np.maximum(cr - rad, np.float32(0))).clip(-2.0 ** 40, 2.0 ** 40).astype(np.int64)
    r1 = np.trunc(np.minimum(cr + rad, np.float32(H - 1))).clip(-2.0 ** 40, 2.0 ** 40).astype(np.int64)
    q0 = np.trunc(np.maximum(cc - rad, np.float32(0))).clip(-2.0 ** 40, 2.0 ** 40).astype(np.int64)
    q1 = np.trunc(np.minimum(cc + rad, np.float32(W - 1))).clip(-2.0 ** 40, 2.0 ** 40).astype(np.int64)
    win = np.stack([r0, r1, q0, q1], -1)              # (the clip keeps an infinity a finite integer: the window stays empty)
    win[nan] = 0
    return win


def pool(feature, pre, radius=6, axes='ref', dtype=np.float64, divisor=None):
    """loss1: desc (B, K, C) from feature (B, C, H, W) and pre (B, K, 2)."""
    feature = np.asarray(feature, dtype)
    B, C, H, W = feature.shape
    win = windows(pre, H, W, radius, axes)
    div = dtype((2 * radius + 1) ** 2 if divisor is None else divisor)
    desc = np.zeros((B, win.shape[1], C), dtype)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):
            if r1 > r0 and q1 > q0:
                desc[b, j] = feature[b, :, r0:r1, q0:q1].sum(axis=(1, 2), dtype=dtype) / div
    return desc


def kl(a, b, scale=1.0, dtype=np.float64):
    """(loss, rows (B, K), d loss / d a, d loss / d b) of loss3 behind its two loss1 calls, loss = scale * mean(rows)."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    m = a.max(-1, keepdims=True)
    lp = (a - m) - np.log(np.exp(a - m).sum(-1, keepdims=True, dtype=dtype))
    be = b + dtype(1e-6)
    S = be.sum(-1, keepdims=True, dtype=dtype)
    q = be / S
    d = np.log(q) - lp
    rows = (q * d).sum(-1, dtype=dtype)
    coef = dtype(scale / rows.size)
    ga = coef * (np.exp(lp) - q)
    gb = coef * ((d - rows[..., None]) / S)
    loss = dtype(rows.mean(dtype=dtype) * dtype(scale))
    return loss, rows, ga.astype(dtype), gb.astype(dtype)


def scatter(gdesc, pre, shape, radius=6, axes='ref', dtype=np.float64, divisor=None):
    """The backward of pool: (B, C, H, W) with sum_j gdesc[b, j, :] / divisor on every pixel of joint j's window."""
    B, C, H, W = shape
    win = windows(pre, H, W, radius, axes)
    div = dtype((2 * radius + 1) ** 2 if divisor is None else divisor)
    g = np.zeros(shape, dtype)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):
            if r1 > r0 and q1 > q0:
                g[b, :, r0:r1, q0:q1] += (np.asarray(gdesc[b, j], dtype) / div)[:, None, None]
    return g


def loss3(f1, f2, pre1, pre2, radius=6, axes='ref', scale=1.0, dtype=np.float64, want=(True, True)):
    """(loss, grad_f1, grad_f2, desc1, desc2): the whole of the reference's loss3 with both feature gradients."""
    d1, d2 = pool(f1, pre1, radius, axes, dtype), pool(f2, pre2, radius, axes, dtype)
    loss, rows, ga, gb = kl(d1, d2, scale, dtype)
    g1 = scatter(ga, pre1, np.shape(f1), radius, axes, dtype) if want[0] else None
    g2 = scatter(gb, pre2, np.shape(f2), radius, axes, dtype) if want[1] else None
    return loss, g1, g2, d1, d2


def covered(pre, H, W, radius=6, axes='ref'):
    """(B, H, W) bool: the pixels at least one window holds."""
    win = windows(pre, H, W, radius, axes)
    m = np.zeros((win.shape[0], H, W), bool)
    for b in range(win.shape[0]):
        for r0, r1, q0, q1 in win[b]:
            if r1 > r0 and q1 > q0:
                m[b, r0:r1, q0:q1] = True
    return m


def scatter_model(gdesc, pre, shape, radius=6, axes='ref', divisor=None, onto=None, round_to=None):
    """The exact-order fp32 model of the jfa_scatter kernel, on NHWC arrays (B, H, W, C): gd = fp32(gdesc / divisor) once per
    (b, j, c); per pixel the fp32 sum of gd[b, j] over the covering joints in ascending j; write mode (onto=None): that sum,
    +0 where no window covers; accumulate mode: fp32(onto) + sum on the covered pixels, `onto` untouched elsewhere.  `round_to`
    rounds an fp32 array to the storage type (None: fp32 storage)."""
    B, H, W, C = shape
    win = windows(pre, H, W, radius, axes)
    div = np.float32((2 * radius + 1) ** 2 if divisor is None else divisor)
    gd = (np.asarray(gdesc, np.float32) / div).astype(np.float32)
    s = np.zeros(shape, np.float32)
    cov = np.zeros((B, H, W), bool)
    for b in range(B):
        for j, (r0, r1, q0, q1) in enumerate(win[b]):           # ascending j: every pixel's sum runs in the kernel's order
            if r1 > r0 and q1 > q0:
                s[b, r0:r1, q0:q1] = s[b, r0:r1, q0:q1] + gd[b, j]
                cov[b, r0:r1, q0:q1] = True
    rnd = (lambda v: v) if round_to is None else round_to
    if onto is None:
        return rnd(s), cov
    out = np.array(onto, copy=True)
    tot = (np.asarray(onto, np.float32) + s).astype(np.float32)
    out[cov] = rnd(tot)[cov]
    return out, cov


# The floors of the tolerance, as fractions of |loss|, of max |grad| and of max |desc|.  Over the fixture cases
# (tests/golden/g15_jfa.npz) the reference's own float32 run is at most 1.15e-5 (relative) from its float64 run on the loss -- a
# small difference of large terms: sum q log q and sum q lp are each near -log C while the loss is 1e-3 .. 1e-2 -- 1.72e-6 of
# max |grad| on the feature gradients and 4.2e-8 of max |desc| on the descriptors (tests/test_jfa_cpu.py prints and checks them);
# each floor is the next 1-2-5 step above that.  None of them comes from a kernel run.
LOSS_FLOOR, GRAD_FLOOR, DESC_FLOOR = 2e-5, 2e-6, 5e-8


def bounds(ref32, ref64, floors=None):
    """The tolerance rule: a kernel result may be as far from the float64 reference as 4 times the reference's own float32 run
    is from it, with the floors above.  ref32, ref64: dicts of the float32 and float64 results under the keys 'loss', 'grad_f1',
    'grad_f2', 'desc1', 'desc2' (any subset; None values skipped).  Returns (own, bound): dicts of the float32 run's own distances
    and of the bounds (max abs)."""
    fl = dict(loss=LOSS_FLOOR, grad_f1=GRAD_FLOOR, grad_f2=GRAD_FLOOR, desc1=DESC_FLOOR, desc2=DESC_FLOOR)
    fl.update(floors or {})
    own, bound = {}, {}
    for k, r64 in ref64.items():
        if r64 is None or ref32.get(k) is None:
            continue
        r64 = np.asarray(r64, np.float64)
        own[k] = float(np.abs(np.asarray(ref32[k], np.float64) - r64).max())
        bound[k] = max(4 * own[k], fl[k] * float(np.abs(r64).max()))
    return own, bound


def errors(got, ref64):
    return {k: float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref64[k], np.float64)).max()) for k in ref64
            if ref64[k] is not None and got.get(k) is not None}


def bf16_round(a):
    """fp32 array rounded to the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))
