"""numpy reference of the gradient-norm clipping entry points (include/mi355pose.h: mi355_grad_sumsq_batched,
mi355_grad_clip_coef, mi355_sgd_nesterov_clipped):

    sumsq = sum (double)g * (double)g                    float64 (the square of an fp32 value is exact in float64)
    norm  = (float)sqrt(sumsq)                           float64 root, rounded once to float32
    coef  = fminf(1.0f, max_norm / (norm + 1e-6f))       float32 -- torch: max_norm / (total_norm + 1e-6), clamp(max=1.0)
    sumsq not finite:  skip = 1, coef = 0
    step:  g_c = fl(g * coef); d = g_c + wd * p; buf = mu * buf + d; p -= lr * (nesterov ? d + mu * buf : buf)

`dtype` selects the precision of the step (float32: what the kernel computes, every operation rounded on its own; float64: the
comparison with torch in double precision)."""
import numpy as np

F32 = np.float32


def sumsq(ranges):
    """float64 sum of squares over every element of every range (pairwise inside numpy: for exact operands any order agrees)."""
    return float(sum(np.sum(np.asarray(r, dtype=np.float64) ** 2) for r in ranges))


def norm_coef_skip(ss, max_norm, dtype=np.float32):
    """(norm, coef, skip) from the float64 sum of squares and max_norm; norm and coef in `dtype` (float32: the kernel's)."""
    T = np.dtype(dtype).type
    ss = np.float64(ss)
    with np.errstate(all='ignore'):
        if not np.isfinite(ss):
            return T(ss), T(0.0), 1
        norm = T(np.sqrt(ss))
        coef = np.fmin(T(1.0), T(max_norm) / (norm + T(1e-6)))     # fmin: fminf's NaN rule
    return norm, T(coef), 0


def clip_record(ranges, max_norm, dtype=np.float32):
    ss = sumsq(ranges)
    return (ss,) + norm_coef_skip(ss, max_norm, dtype)


def sgd_step(p, g, buf, lr, coef, skip, momentum, wd, nesterov, dtype=np.float32):
    """One clipped Nesterov step; returns (p, buf) as new arrays of `dtype` (the inputs when skip is set)."""
    T = np.dtype(dtype).type
    p, g, buf = (np.asarray(a, dtype=dtype) for a in (p, g, buf))
    if skip:
        return p.copy(), buf.copy()
    gc = (g * T(coef)).astype(dtype)
    d = (gc + (T(wd) * p).astype(dtype)).astype(dtype)
    nb = ((T(momentum) * buf).astype(dtype) + d).astype(dtype)
    upd = (d + (T(momentum) * nb).astype(dtype)).astype(dtype) if nesterov else nb
    return (p - (T(lr) * upd).astype(dtype)).astype(dtype), nb
