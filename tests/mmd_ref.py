"""The multi-kernel MMD of uda.model.loss.MMD_loss3 / MMD_loss / mmd_rbf and its gradient in closed form, in numpy, in the
precision asked for (float64: the yardstick of the tests; float32: the restatement whose own distance from float64 sizes
the tolerance of the GPU tests).

Per joint k, rows x_0 .. x_{n-1} = the B source rows, then the B target rows (n = 2 B):
    D_ij    = sum_p (x_i[p] - x_j[p])^2                                   (difference form, summed in chunks of HW)
    bw      = sum_ij D_ij / (n^2 - n)   or fix_sigma;   bw /= kernel_mul^(kernel_num // 2);   bw_m = bw * kernel_mul^m
    Kmat_ij = sum_m exp(-D_ij / bw_m)
    loss_k  = mean over a, b < B of Kmat[a, b] + Kmat[B+a, B+b] - Kmat[a, B+b] - Kmat[B+a, b]
    loss    = scale * mean_k loss_k
    c_ij    = s_ij * scale / (B^2 K) * sum_m (-1 / bw_m) exp(-D_ij / bw_m),   s_ij = +1 inside a domain, -1 across
    d loss / d x_i = 4 (x_i sum_j c_ij - sum_j c_ij x_j)                   (the bandwidth is a constant)
A joint whose distances are all zero (bw = 0) contributes loss_k = 0 and zero gradient rows.
"""
import numpy as np


def distances(X, chunk=256):
    """(n, HW) -> (n, n) squared distances in X's dtype, accumulated over chunks of HW."""
    n, HW = X.shape
    D = np.zeros((n, n), X.dtype)
    for p in range(0, HW, chunk):
        d = X[:, None, p:p + chunk] - X[None, :, p:p + chunk]
        D += (d * d).sum(-1)
    return D


def mmd(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None, scale=1.0, dtype=np.float64, chunk=256):
    """source, target: (B, K, ...) arrays.  Returns (loss, loss_rows (K,), grad_source, grad_target), all in `dtype`."""
    src = np.asarray(source).astype(dtype)
    tgt = np.asarray(target).astype(dtype)
    assert src.shape == tgt.shape
    B, K = src.shape[:2]
    s3, t3 = src.reshape(B, K, -1), tgt.reshape(B, K, -1)
    n = 2 * B
    f = dtype
    sign = np.ones((n, n), dtype)
    sign[:B, B:] = -1
    sign[B:, :B] = -1
    rows = np.zeros(K, dtype)
    gs, gt = np.zeros_like(s3), np.zeros_like(t3)
    for k in range(K):
        X = np.concatenate([s3[:, k], t3[:, k]], 0)
        D = distances(X, chunk)
        if fix_sigma:
            bw = f(fix_sigma)
        else:
            bw = f(D.sum() / f(n * n - n))
        if bw == 0:
            continue
        bw = f(bw / f(kernel_mul ** (kernel_num // 2)))
        Kmat, cc = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
        for m in range(kernel_num):
            bwm = f(bw * f(kernel_mul ** m))
            e = np.exp(-D / bwm)
            Kmat += e
            cc += (f(-1) / bwm) * e
        rows[k] = (Kmat[:B, :B] + Kmat[B:, B:] - Kmat[:B, B:] - Kmat[B:, :B]).mean(dtype=dtype)
        c = sign * f(scale / (B * B * K)) * cc
        G = f(4) * (X * c.sum(1, keepdims=True) - c @ X)
        gs[:, k], gt[:, k] = G[:B], G[B:]
    loss = f(rows.mean(dtype=dtype) * f(scale))
    return loss, rows, gs.reshape(src.shape), gt.reshape(tgt.shape)


# the floors of the tolerance, as fractions of |loss| and of max |grad|: test_mmd_cpu.py shows the reference's own float32 run to
# stay below them
LOSS_FLOOR, GRAD_FLOOR = 5e-7, 1e-6


def bounds(loss32, gs32, gt32, loss64, gs64, gt64):
    """The tolerance of the GPU tests for one case, from a float32 run of the reference expression and its float64 run: a kernel
    may be 4 times as far from float64 as the float32 run is, with floors of 5e-7 relative on the loss and 1e-6 of max |grad|
    on each gradient.  Returns ((the float32 run's own distances), (the three bounds)): loss, grad_source, grad_target."""
    own = (abs(float(loss32) - float(loss64)),
           float(np.abs(np.asarray(gs32, np.float64) - gs64).max()), float(np.abs(np.asarray(gt32, np.float64) - gt64).max()))
    floor = (LOSS_FLOOR * abs(float(loss64)), GRAD_FLOOR * float(np.abs(gs64).max()), GRAD_FLOOR * float(np.abs(gt64).max()))
    return own, tuple(max(4 * o, fl) for o, fl in zip(own, floor))
