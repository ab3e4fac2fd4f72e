"""Plain float64 references of the heat-map kernels of csrc/heatmap.hip, and the inputs the tests feed them.

numpy / torch on the CPU only.  Every reference is the CPU oracle's own expression (oracle/losses.py) evaluated in float64
(`dtype=torch.float32` gives the oracle's float32 arithmetic back: tests/test_heatmap_ref_cpu.py pins both ends), generalised
where the kernel's ABI is more general than the oracle's call (beta / out_scale, non-square maps, per-map loss rows, one
label centre at a time instead of the oracle's S^4 table).

The input generators at the end are shared by the CPU module (which measures what float32 arithmetic costs on each input)
and the GPU module (which runs the kernels on the same inputs): one row of a case = one pattern, patterns cycle over the rows
with an offset that depends on the row count, so that the small row counts see different patterns."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as ol

# H x W: register forms 1 / 2 / 3; register forms with W != sqrt(H*W); loop forms of the shipped configurations; ragged
SIZES = [(64, 64), (32, 32), (16, 16), (32, 128), (128, 32), (16, 64), (8, 32), (128, 128), (8, 8),
         (5, 7), (10, 12), (1, 1), (1, 3), (63, 65)]
ROWS = [1, 2, 3, 5, 42, 63, 64 * 21]          # every rows % 4; first and last workgroup differ


def size_id(hw):
    return '%dx%d' % hw


# ---------------------------------------------------------------------------------------------------------------- references
def argmax(hm):
    """hm: numpy float32 [B, K, H, W] -> (idx int32 [B, K], preds float32 [B, K, 2], maxvals float32 [B, K, 1]): numpy's
    first-maximum and NaN rules are the specification (oracle.losses.get_max_preds as it stands)."""
    B, K = hm.shape[:2]
    with np.errstate(invalid='ignore'):
        preds, maxvals = ol.get_max_preds(hm)
    return np.argmax(hm.reshape(B, K, -1), 2).astype(np.int32), preds, maxvals


def soft_argmax(hm, beta=100.0, out_scale=4.0, dtype=torch.float64):
    """oracle.losses.soft_argmax with its two constants as arguments; [B, K, 2] = (u = column, v = row) * out_scale."""
    hm = hm.to(dtype).mul(beta)
    B, K, H, W = hm.size()
    sm = F.softmax(hm.view(B, K, H * W), dim=2).view(B, K, H, W)
    xx, yy = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    ax = sm.mul(xx.to(dtype)).view(B, K, H * W).sum(2).unsqueeze(2)
    ay = sm.mul(yy.to(dtype)).view(B, K, H * W).sum(2).unsqueeze(2)
    return torch.cat([ay, ax], 2) * out_scale


def f32(x):
    """The float32 value the C ABI receives for a Python float argument."""
    return float(np.float32(x))


def kl(pred, target, weight, eps, coeff=1.0, dtype=torch.float64):
    """(loss rows [B, K], d(coeff * mean over B*K of the rows) / d pred [B, K, H, W]) from oracle.losses.JointsKLLoss under
    autograd.  Every map is its own 'image' with one key point, so that the oracle's mean over the key points is the row.
    NaN where the oracle gives NaN (an all-zero target map with eps = 0: 0 / 0; a target map with a +inf pixel)."""
    B, K, H, W = pred.shape
    p = pred.to(dtype).reshape(B * K, 1, H, W).clone().requires_grad_(True)
    t = target.to(dtype).reshape(B * K, 1, H, W)
    w = None if weight is None else weight.to(dtype).reshape(B * K, 1)
    rows = ol.JointsKLLoss(reduction='none', epsilon=f32(eps))(p, t, w)
    (rows.mean() * coeff).backward()
    return rows.detach().reshape(B, K), p.grad.reshape(B, K, H, W)


def patch(tmp_size, sigma=2):
    """Patch values in float32 exactly as uda.model.regda_4.gaussian_patch makes them (the kernel's host table)."""
    from uda.model.regda_4 import gaussian_patch
    return gaussian_patch(tmp_size, sigma)


def centre_map(mx, my, S, tmp_size, g):
    """One entry hm[mx][my] of oracle.losses._table(S, S, tmp_size, sigma), by its slice arithmetic."""
    hm = np.zeros((S, S), dtype=np.float32)
    ul = [int(mx - tmp_size), int(my - tmp_size)]
    br = [int(mx + tmp_size + 1), int(my + tmp_size + 1)]
    gx = max(0, -ul[0]), min(br[0], S) - ul[0]
    gy = max(0, -ul[1]), min(br[1], S) - ul[1]
    ix = max(0, ul[0]), min(br[0], S)
    iy = max(0, ul[1]), min(br[1], S)
    hm[iy[0]:iy[1], ix[0]:ix[1]] = g[gy[0]:gy[1], gx[0]:gx[1]]
    return hm


def labels(xy, tmp_size, sigma, div, S, kind, extra=None, normalise=0):
    """xy: numpy float32 [B, K, 2] arg-max coordinates -> (gt float32 [B, K, S, S], gf float64 [B, K, S, S]).
    gt: the clipped Gaussian at centre = trunc(xy / div); gf by `kind` as include/mi355pose.h documents it
    (0: clip(sum of the OTHER key points' gt), 1: clip(1 - 10 gt), 2: clip(clip(sum of all gt) - 10 gt)), then
    clip(gf + extra - 100 gt) when `extra` is given, then per-map division by the maximum (normalise 1: 0 / 0 = NaN as the
    oracle's _max_normalise; 2: a map whose maximum is not positive is left alone)."""
    B, K, _ = xy.shape
    g = patch(tmp_size, sigma)
    c = (xy.reshape(-1, 2).astype(np.float32) / div).astype(int)
    cache = {}
    gt = np.empty((B * K, S, S), dtype=np.float32)
    for i, (mx, my) in enumerate(c):
        key = (int(mx), int(my))
        if key not in cache:
            cache[key] = centre_map(key[0], key[1], S, tmp_size, g)
        gt[i] = cache[key]
    gt = gt.reshape(B, K, S, S)
    g64 = gt.astype(np.float64)
    tot = g64.sum(1, keepdims=True)
    if kind == 0:
        gf = (tot - g64).clip(0., 1.)              # (in float64 the sum without map k, to 1e-16)
    elif kind == 1:
        gf = (1. - g64 * 10).clip(0., 1.)
    else:
        gf = (tot.clip(0., 1.) - g64 * 10).clip(0., 1.)
    if extra is not None:
        gf = (gf + np.asarray(extra, dtype=np.float64).reshape(B, K, S, S) - g64 * 100).clip(0., 1.)
    if normalise:
        mx = gf.reshape(B, K, -1).max(2).reshape(B, K, 1, 1)
        with np.errstate(invalid='ignore', divide='ignore'):
            q = gf / mx
        gf = q if normalise == 1 else np.where(mx > 0, q, gf)
    return gt, gf


def bilinear(x, size, alpha=1.0, out=None):
    """alpha * interpolate(x, size, 'bilinear', align_corners=False) (+ out) in float64; size: int or (H, W)."""
    size = (size, size) if isinstance(size, int) else tuple(size)
    y = F.interpolate(x.double(), size=size, mode='bilinear', align_corners=False) * f32(alpha)
    return y if out is None else y + out.double()


def pck(pred, tgt, nx, ny):
    """oracle.losses.calc_dists with every image normalised by (nx, ny), transposed to [B, K] (float64)."""
    B = pred.shape[0]
    norm = np.ones((B, 2)) * np.array([f32(nx), f32(ny)])
    return ol.calc_dists(np.asarray(pred), np.asarray(tgt), norm).T.copy()


# -------------------------------------------------------------------------------------------------------------------- inputs
def _rng(tag, H, W, rows):
    return np.random.default_rng([tag, H, W, rows])


SOFT_PATTERNS = 8


def softargmax_maps(H, W, rows):
    """float32 tensor [rows, 1, H, W].  Patterns: 0 the golden's scale (N(0, 0.05) + one peak of 1), 1-4 a dominant peak at
    each corner, 5 a flat map (centroid = map centre), 6 N(0, 3): beta * x spans far more than the float32 exp range below
    the maximum, 7 diffuse noise without a peak."""
    rng = _rng(11, H, W, rows)
    hm = (rng.standard_normal((rows, H, W)) * 0.05).astype(np.float32)
    pat = (np.arange(rows) + rows) % SOFT_PATTERNS
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for r in range(rows):
        p = pat[r]
        if p == 0:
            hm[r, rng.integers(0, H), rng.integers(0, W)] += 1.0
        elif p <= 4:
            hm[r][corners[p - 1]] += 5.0
        elif p == 5:
            hm[r] = 0.3
        elif p == 6:
            hm[r] *= 60.0
    return torch.from_numpy(hm).view(rows, 1, H, W)


KL_TARGETS = 5


def kl_inputs(H, W, rows):
    """(pred, target) float32 [rows, 1, H, W].  Logits N(0, 1) on even rows, N(0, 30) on odd ones; targets cycle through
    sparse (uniform values on a tenth of the pixels: the recipe of the golden losses), dense, one-hot, all-zero, and dense with
    one +inf pixel (its normalised target is NaN there and 0 elsewhere: loss and the WHOLE gradient row are NaN in the oracle,
    the softmax term of every pixel being scaled by the sum of the normalised target)."""
    rng = _rng(13, H, W, rows)
    pred = rng.standard_normal((rows, H, W)).astype(np.float32)
    pred[1::2] *= 30.0
    tgt = rng.random((rows, H, W)).astype(np.float32)
    mask = rng.random((rows, H, W)) > 0.9
    pat = (np.arange(rows) // 2 + rows) % KL_TARGETS
    for r in range(rows):
        p = pat[r]
        if p == 0:
            tgt[r] *= mask[r]
        elif p == 2:
            tgt[r] = 0
            tgt[r].reshape(-1)[int(np.argmin(pred[r]))] = 1.0     # at the smallest logit: the largest |log p| the row has
        elif p == 3:
            tgt[r] = 0
        elif p == 4:
            tgt[r, rng.integers(0, H), rng.integers(0, W)] = np.inf
    return torch.from_numpy(pred).view(rows, 1, H, W), torch.from_numpy(tgt).view(rows, 1, H, W)


def kl_weight(mode, rows):
    """None, all ones, or ones with some zeros ([rows, 1])."""
    if mode is None:
        return None
    w = torch.ones(rows, 1)
    if mode == 'zeros':
        w[::3] = 0
    return w


# (eps, weight mode, coeff): both eps, the three weight modes and both coefficients, each against each other value at least once
KL_CONFIGS = [(0.0, None, 1.0), (1e-7, 'ones', 0.25), (1e-7, 'zeros', 1.0), (0.0, 'zeros', 0.25), (1e-7, None, 0.25), (0.0, 'ones', 1.0)]
SOFT_CONFIGS = [(100.0, 4.0), (1.0, 4.0), (100.0, 1.0), (1.0, 2.5)]            # (beta, out_scale); the caller's is the first


def configs_for(configs, rows):
    """The largest row count is there for the grid, not for the values: it runs the first and the third configuration only."""
    return configs if rows < 1000 else [configs[0], configs[2]]
