"""numpy restatements of the Adam / AdamW update of include/mi355pose.h (mi355_adam_step_batched):

  adam_step64: the oracle -- torch.optim.Adam / AdamW (`_single_tensor_adam`) in float64 with the hyper-parameters as given;
  adam_step32: the kernel's arithmetic operation for operation -- float32 in torch's order, every operation rounded on its own,
               square root and division correctly rounded, with the scalars the kernel derives per block (lr, eps and the weight
               decay are float32 values; the betas and the bias corrections are float64, beta^t by squaring as ipow64 does) --
               so the kernel is compared with it bit for bit.

Both return new (p, m, v, step) and leave their arguments alone.  `coef` / `skip` are the fields of a mi355_clip_rec (None: no
record): the step is taken on fl32(g * coef), or not at all.
"""
import numpy as np


def adam_step64(p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled, coef=None, skip=0):
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    if skip:
        return p.copy(), m.copy(), v.copy(), step
    t = step + 1
    gc = g * np.float64(coef) if coef is not None else g
    if wd != 0:
        if decoupled:
            p = p * (1 - lr * wd)
        else:
            gc = gc + wd * p
    m = m + (1 - beta1) * (gc - m)
    v = beta2 * v + (1 - beta2) * gc * gc
    bc1 = 1 - beta1 ** t
    bc2s = (1 - beta2 ** t) ** 0.5
    p = p - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))
    return p, m, v, t


def ipow(x, t):
    """x ** t for a whole t >= 0 by squaring, in the order of the kernel's ipow64."""
    r, x, t = 1.0, float(x), int(t)
    while t:
        if t & 1:
            r *= x
        x *= x
        t >>= 1
    return r


def adam_step32(p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled, coef=None, skip=0):
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    if skip:
        return p.copy(), m.copy(), v.copy(), step
    t = int(step) + 1
    lr, eps, wd = f(lr), f(eps), f(wd)
    bc1 = 1.0 - ipow(beta1, t)
    bc2s = float(np.sqrt(np.float64(1.0 - ipow(beta2, t))))
    step_size, bc2s_f = f(float(lr) / bc1), f(bc2s)
    decay = f(1.0 - float(lr) * float(wd))
    omb1, omb2, beta2 = f(1.0 - float(beta1)), f(1.0 - float(beta2)), f(beta2)
    gc = g * f(coef) if coef is not None else g
    if decoupled:
        p = p * decay
    elif wd != 0:
        gc = gc + wd * p
    m = m + omb1 * (gc - m)
    v = beta2 * v + (omb2 * gc) * gc
    p = p - step_size * (m / (np.sqrt(v) / bc2s_f + eps))
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v, t


def bound(torch32, oracle64, largest=None):
    """The distance allowed from the float64 oracle: twice that of torch's float32 result, or 4 float32 ulps of the tensor's largest
    magnitude, whichever is larger."""
    oracle64 = np.asarray(oracle64, dtype=np.float64)
    d_torch = float(np.abs(np.asarray(torch32, dtype=np.float64) - oracle64).max())
    big = float(np.abs(oracle64).max()) if largest is None else largest
    return max(2.0 * d_torch, 4.0 * float(np.spacing(np.float32(big)))), d_torch


def distance(x, oracle64):
    return float(np.abs(np.asarray(x, dtype=np.float64) - np.asarray(oracle64, dtype=np.float64)).max())
