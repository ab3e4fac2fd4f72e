"""Float64 restatement of mi355_coord_heatmap (include/mi355pose.h): the coordinate loss on the soft-arg-max, its gradient by
the closed formula, the soft-arg-max itself, and the input builders of tests/test_coord_cpu.py and tests/test_gpu_coord.py.
No GPU-only code."""
import numpy as np
import torch
import torch.nn.functional as F

OFFSETS = (0.25, -0.25, 0.5, -0.5, 2.5, -2.5, 7.0, -7.0)      # coord = uv_ref + offset: both branches of the smooth-L1
KINK_GAP = 0.05                                               # | |d| - delta | and |d| stay at least this far from a kink


def f32(x):
    """The float32 value the C ABI receives for a Python float argument."""
    return float(np.float32(x))


def _h(d, delta):
    a = d.abs()
    if delta > 0:
        return torch.where(a < delta, 0.5 * d * d / delta, a - 0.5 * delta)
    return a


def _dh(d, delta):
    s = torch.sign(d)
    if delta > 0:
        return torch.where(d.abs() < delta, d / delta, s)
    return s


def coord(pred, coords, weight, beta, delta, coef, dtype=torch.float64):
    """(loss_rows [rows], unit_grad [rows, H, W], uv [rows, 2]) of section 1 of the specification, evaluated in `dtype` with
    torch expressions: pred [rows, H, W], coords [rows, 2], weight [rows] or None.  A row of weight 0 is selected out."""
    rows, H, W = pred.shape
    z = pred.to(dtype) * beta
    p = F.softmax(z.reshape(rows, H * W), dim=1)
    i = torch.arange(H * W)
    x, y = (i % W).to(dtype), (i // W).to(dtype)
    u, v = (p * x).sum(1), (p * y).sum(1)
    c = coords.to(dtype)
    dx, dy = u - c[:, 0], v - c[:, 1]
    w = torch.ones(rows, dtype=dtype) if weight is None else weight.to(dtype).reshape(rows)
    skip = w == 0
    loss = torch.where(skip, torch.zeros_like(w), w * (_h(dx, delta) + _h(dy, delta)))
    t = (x[None] - u[:, None]) * _dh(dx, delta)[:, None] + (y[None] - v[:, None]) * _dh(dy, delta)[:, None]
    g = coef * w[:, None] * beta * p * t
    g = torch.where(skip[:, None], torch.zeros_like(g), g)
    return loss, g.reshape(rows, H, W), torch.stack([u, v], 1)


def coord_autograd(pred, coords, weight, beta, delta, coef):
    """The same rows and gradient from torch.autograd in float64: softmax -> expectation -> F.smooth_l1_loss(beta=delta)
    (delta = 0: abs().sum())."""
    rows, H, W = pred.shape
    z = pred.double().clone().requires_grad_(True)
    p = F.softmax((z * beta).reshape(rows, H * W), dim=1)
    i = torch.arange(H * W)
    uv = torch.stack([(p * (i % W).double()).sum(1), (p * (i // W).double()).sum(1)], 1)
    c = coords.double()
    if delta > 0:
        per = F.smooth_l1_loss(uv, c, reduction='none', beta=delta).sum(1)
    else:
        per = (uv - c).abs().sum(1)
    w = torch.ones(rows, dtype=torch.float64) if weight is None else weight.double().reshape(rows)
    loss = w * per
    (coef * loss.sum()).backward()
    return loss.detach(), z.grad, uv.detach()


def maps(H, W, rows, beta, seed=0):
    """[rows, H, W] float32 maps spread so that beta * z has a standard deviation of about 3 (gradients that do not vanish)."""
    g = torch.Generator().manual_seed(7700 + 131 * H + 17 * W + rows + seed)
    return (torch.randn(rows, H, W, generator=g, dtype=torch.float64) * (3.0 / beta)).float()


def weights(rows, seed=0):
    """[rows] float32 weights: 1, 0.5, 0 (a skipped row) and 2 in turn, never all zero."""
    w = torch.tensor([1.0, 0.5, 0.0, 2.0])[torch.arange(rows) % 4]
    return w.float()


def coords_for(uv_ref, delta, shift=0):
    """[rows, 2] float32 coordinates uv_ref + offset from OFFSETS (x and y take different entries); checked afterwards by
    `kink_clear`."""
    rows = uv_ref.shape[0]
    off = torch.tensor(OFFSETS, dtype=torch.float64)
    ox = off[(torch.arange(rows) + shift) % len(OFFSETS)]
    oy = off[(torch.arange(rows) * 3 + 1 + shift) % len(OFFSETS)]
    return (uv_ref + torch.stack([ox, oy], 1)).float()


def kink_clear(uv_ref, coords, delta):
    """True when every |d| and every | |d| - delta | of the float64 reference is at least KINK_GAP: the float32 and the float64
    side then sit on the same branch."""
    d = (uv_ref - coords.double()).abs()
    ok = bool((d >= KINK_GAP).all())
    if delta > 0:
        ok = ok and bool(((d - delta).abs() >= KINK_GAP).all())
    return ok


def exact_case(name, H=4, W=8, oy=0, ox=0):
    """The exact cases of the specification, optionally embedded at (oy, ox) of a larger H x W map: dict(pred [1, H, W], coord
    [1, 2], beta, delta, uv, loss, grad [1, H, W]) -- every value exactly representable, to be met bit for bit in float32."""
    pred = torch.full((1, H, W), -1.0e4)
    grad = torch.zeros(1, H, W)
    if name == 'two':                  # two pixels of 0 at (x, y) = (2, 1), (3, 1); quadratic branch, dx = 0.25
        pred[0, oy + 1, ox + 2] = pred[0, oy + 1, ox + 3] = 0.0
        uv, c, delta, loss = (ox + 2.5, oy + 1.0), (ox + 2.25, oy + 1.0), 1.0, 0.03125
        grad[0, oy + 1, ox + 2], grad[0, oy + 1, ox + 3] = -0.0625, 0.0625
    elif name == 'onehot':             # a one-hot map: p (x - u) = 0 everywhere, whatever the distance
        pred[0, oy + 2, ox + 5] = 0.0
        uv, c, delta, loss = (ox + 5.0, oy + 2.0), (ox + 1.0, oy + 2.5), 1.0, 3.5 + 0.125
    elif name == 'linear':             # two pixels, dx = 2.5: linear branch, h = 2.0, h' = 1
        pred[0, oy + 1, ox + 2] = pred[0, oy + 1, ox + 3] = 0.0
        uv, c, delta, loss = (ox + 2.5, oy + 1.0), (ox + 0.0, oy + 1.0), 1.0, 2.0
        grad[0, oy + 1, ox + 2], grad[0, oy + 1, ox + 3] = -0.25, 0.25
    elif name == 'l1':                 # delta = 0: |dx| + |dy| = 0.25 + 1, h' = (1, -1)
        pred[0, oy + 1, ox + 2] = pred[0, oy + 1, ox + 3] = 0.0
        uv, c, delta, loss = (ox + 2.5, oy + 1.0), (ox + 2.25, oy + 2.0), 0.0, 1.25
        grad[0, oy + 1, ox + 2], grad[0, oy + 1, ox + 3] = -0.25, 0.25
    else:
        raise KeyError(name)
    return dict(pred=pred, coord=torch.tensor([c], dtype=torch.float32), beta=1.0, delta=delta, coef=1.0,
                uv=torch.tensor([uv], dtype=torch.float32), loss=torch.tensor([loss], dtype=torch.float32), grad=grad)


EXACT = ('two', 'onehot', 'linear', 'l1')
