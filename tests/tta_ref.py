"""CPU reference of the flip test and the sub-pixel decodes (csrc/eval.hip: mi355_mirror_batch, mi355_flip_decode), a numpy
restatement of the specification in include/mi355pose.h:
  * the mirror of a batch, the flip back with its optional one-column shift, and the fp32 average (sum and product rounded
    separately);
  * the first-index arg-max (eval_ref.first_argmax) and the quarter-pixel offset;
  * the taylor step: the separable smoothing in fp32 in the kernel's fixed order (numpy float32 arrays: one rounding per
    operation, no contraction), then float64 from the logarithm on.
Nothing here touches the GPU or the library."""
import math

import numpy as np

from eval_ref import first_argmax

MODES = {'argmax': 0, 'quarter': 1, 'taylor': 2}
# (dx, dy) of the thirteen points, in the order the differences below index them
POINTS = np.array([(0, 0), (1, 0), (-1, 0), (2, 0), (-2, 0), (0, 1), (0, -1), (0, 2), (0, -2), (1, 1), (-1, 1), (1, -1), (-1, -1)])
DET_MIN = 0.01            # below this the float64 part of the taylor step is not compared to the last place (1/64 for sigma 2 labels)


def gaussian_taps(sigma):
    """(fp32 taps [2 r + 1], r): r = ceil(2.5 sigma), exp(-i^2 / (2 sigma^2)) in float64, normalised, rounded to fp32."""
    r = int(math.ceil(2.5 * float(sigma)))
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32), r


def mirror_batch(x):
    """(2B,C,H,W): x followed by x mirrored along W."""
    x = np.asarray(x, np.float32)
    return np.concatenate([x, x[..., ::-1]], 0)


def flip_back(hm_flip, shift):
    """The heat-maps of the mirrored image in the frame of the image: mirrored along w, then with `shift` = 1 moved one column to
    the right, column 0 keeping its unshifted value (Simple Baselines' SHIFT_HEATMAP)."""
    f = np.ascontiguousarray(np.asarray(hm_flip, np.float32)[..., ::-1])
    if shift:
        g = f.copy()
        g[..., 1:] = f[..., :-1]
        f = g
    return f


def working_map(hm, hm_flip=None, shift=1):
    hm = np.asarray(hm, np.float32)
    if hm_flip is None:
        return hm
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.float32(0.5) * (hm + flip_back(hm_flip, shift))
    assert m.dtype == np.float32
    return m


def smoothed_points(m, px, py, taps, r):
    """(n, 13) fp32: the maps m (n,h,w) smoothed by the separable taps, zero padded, at POINTS around (px, py) -- for each dy
    ascending: row = sum over dx ascending of taps[dx + r] * m, tot = tot + taps[dy + r] * row."""
    n, h, w = m.shape
    pad = np.zeros((n, h + 2 * r + 4, w + 2 * r + 4), np.float32)
    o = r + 2
    pad[:, o:o + h, o:o + w] = m
    X = px[:, None] + POINTS[None, :, 0] + o
    Y = py[:, None] + POINTS[None, :, 1] + o
    rows = np.arange(n)[:, None]
    tot = np.zeros((n, len(POINTS)), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for dy in range(-r, r + 1):
            row = np.zeros_like(tot)
            for dx in range(-r, r + 1):
                row = row + taps[dx + r] * pad[rows, Y + dy, X + dx]
            tot = tot + taps[dy + r] * row
    assert tot.dtype == np.float32
    return tot


def taylor_offsets(S, with_bound=False):
    """(ox, oy, det) in float64 from the (n, 13) smoothed values.  `with_bound` appends (n, 2) bounds on how far another correct
    float64 evaluation of the same formulas can be from (ox, oy): two logarithms that are each within an ulp of the true value
    differ by at most e = 2^-51 max|L|; the halved / quartered differences gx, gy, dxx, dyy, dxy then by at most e each, the
    numerator dyy gx - dxy gy by e (|gx| + |gy| + |dyy| + |dxy|) and det by e (|dxx| + |dyy| + 2 |dxy|) to first order, so
    |d ox| <= e ((|gx| + |gy| + |dyy| + |dxy|) + |ox| (|dxx| + |dyy| + 2 |dxy|)) / |det|, doubled for the higher orders and the
    roundings of the arithmetic itself (oy likewise with dxx for dyy)."""
    t = S.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        L = np.log(np.where(t > 1e-10, t, 1e-10))
        gx, gy = .5 * (L[:, 1] - L[:, 2]), .5 * (L[:, 5] - L[:, 6])
        dxx = .25 * (L[:, 3] - 2. * L[:, 0] + L[:, 4])
        dyy = .25 * (L[:, 7] - 2. * L[:, 0] + L[:, 8])
        dxy = .25 * (L[:, 9] - L[:, 10] - L[:, 11] + L[:, 12])
        det = dxx * dyy - dxy * dxy
        ox, oy = -(dyy * gx - dxy * gy) / det, -(dxx * gy - dxy * gx) / det
        ok = (det != 0) & np.isfinite(ox) & np.isfinite(oy)
        ox, oy = np.where(ok, ox, 0.0), np.where(ok, oy, 0.0)
        if not with_bound:
            return ox, oy, det
        e = 2.0 ** -51 * np.abs(L).max(1)
        g, dd = np.abs(gx) + np.abs(gy) + np.abs(dxy), np.abs(dxx) + np.abs(dyy) + 2 * np.abs(dxy)
        bx = 2 * e * (g + np.abs(dyy) + np.abs(ox) * dd) / np.abs(det)
        by = 2 * e * (g + np.abs(dxx) + np.abs(oy) * dd) / np.abs(det)
    return ox, oy, det, np.where(ok[:, None], np.stack([bx, by], 1), 0.0)


def decode(m, mode='argmax', sigma=2.0, scale=(1., 1.), with_bound=False):
    """(idx int32, xy float32 (n,2), maxval, det) of the working maps m (n,h,w).  det: float64, the determinant of the taylor
    step where it was applied (mode 'taylor', arg-max at least two pixels inside, positive maximum), nan elsewhere.
    `with_bound` appends taylor_offsets' (n, 2) bound, in heat-map pixels (zero where the step was not applied)."""
    m = np.asarray(m, np.float32)
    n, h, w = m.shape
    idx, _, mv = first_argmax(m)
    px, py = (idx % w).astype(np.int64), (idx // w).astype(np.int64)
    pos = mv > 0
    ox, oy, det, bound = np.zeros(n), np.zeros(n), np.full(n, np.nan), np.zeros((n, 2))
    if MODES[mode] == 1:
        with np.errstate(invalid='ignore', over='ignore'):
            for i in range(n):
                if 1 <= px[i] <= w - 2:
                    d = m[i, py[i], px[i] + 1] - m[i, py[i], px[i] - 1]
                    ox[i] = .25 if d > 0 else (-.25 if d < 0 else 0.)
                if 1 <= py[i] <= h - 2:
                    d = m[i, py[i] + 1, px[i]] - m[i, py[i] - 1, px[i]]
                    oy[i] = .25 if d > 0 else (-.25 if d < 0 else 0.)
    elif MODES[mode] == 2:
        taps, r = gaussian_taps(sigma)
        sel = np.flatnonzero(pos & (px >= 2) & (px <= w - 3) & (py >= 2) & (py <= h - 3))
        if len(sel):
            ox[sel], oy[sel], det[sel], bound[sel] = taylor_offsets(smoothed_points(m[sel], px[sel], py[sel], taps, r), True)
    x = (px + ox).astype(np.float32) * np.float32(scale[0])
    y = (py + oy).astype(np.float32) * np.float32(scale[1])
    xy = np.stack([np.where(pos, x, np.float32(0)), np.where(pos, y, np.float32(0))], 1).astype(np.float32)
    return (idx, xy, mv, det, bound) if with_bound else (idx, xy, mv, det)


def flip_decode(hm, hm_flip=None, shift=1, mode='argmax', sigma=2.0, scale=(1., 1.), with_bound=False):
    """The reference of mi355_flip_decode on (rows, h, w) maps: (idx, xy, maxval, det, [bound,] working map)."""
    m = working_map(hm, hm_flip, shift)
    return decode(m, mode, sigma, scale, with_bound) + (m,)


# ---------------------------------------------------------------- the inputs the CPU and GPU tests share
def gaussians(n, size=64, sigma=2.0, seed=5, lo=8.0, hi=55.0, noise=0.0):
    """(maps (n,size,size) fp32, centres (n,2) float64 [x, y]): unit Gaussians exp(-d^2 / (2 sigma^2)) at centres uniform in
    [lo, hi]^2, plus N(0, noise^2) where asked."""
    rng = np.random.default_rng([2209, n, size, seed])
    c = rng.uniform(lo, hi, (n, 2))
    g = np.arange(size, dtype=np.float64)
    d2 = (g[None, None, :] - c[:, 0, None, None]) ** 2 + (g[None, :, None] - c[:, 1, None, None]) ** 2
    maps = np.exp(-d2 / (2.0 * sigma * sigma))
    if noise:
        maps = maps + rng.normal(0.0, noise, maps.shape)
    return maps.astype(np.float32), c


def random_normal_maps():
    """The 64 x 64 standard-normal maps of test_gpu_eval.py's inexact case."""
    return np.random.default_rng([9, 64, 256]).standard_normal((8, 64, 64)).astype(np.float32)


def taylor_cases():
    """{name: (n,size,size) maps} of the mode-2 comparisons: Gaussians at sub-pixel centres without and with noise and random
    maps at 64 x 64, and Gaussians on maps of 64 KB (the 1024-thread form) and beyond (read through the caches)."""
    return {'clean': gaussians(48)[0], 'noisy': gaussians(48, seed=6, noise=0.02)[0], 'normal': random_normal_maps(),
            'map64k': gaussians(2, size=128, hi=119.0)[0], 'beyond_lds': gaussians(2, size=130, hi=121.0, noise=0.02)[0]}


def border_maps(h=12, w=16):
    """((n,h,w) integer-valued maps, [(x, y)]): a single maximum in columns 0, 1, 2, w-3, w-2, w-1 and rows likewise, on a
    background that rises towards +x and +y (so every quarter-pixel sign is defined and positive where it applies)."""
    spots = [(0, 5), (1, 5), (2, 5), (w - 3, 5), (w - 2, 5), (w - 1, 5), (7, 0), (7, 1), (7, 2), (7, h - 3), (7, h - 2), (7, h - 1),
             (0, 0), (w - 1, h - 1), (1, 1), (w - 2, h - 2), (2, 2), (w - 3, h - 3)]
    base = (np.arange(w, dtype=np.float32)[None, :] + np.float32(2) * np.arange(h, dtype=np.float32)[:, None]) + np.float32(1)
    maps = np.repeat(base[None], len(spots), 0)
    for i, (x, y) in enumerate(spots):
        maps[i, y, x] = 512.0
    return maps, spots


def faint_maps():
    """Two 40 x 40 maps of zeros with one pixel of 1e-20 at (20, 13) and (2, 37): a positive maximum whose smoothed
    neighbourhood lies below the 1e-10 clamp everywhere, so every log is equal, det == 0 and the taylor step adds nothing."""
    m = np.zeros((2, 40, 40), np.float32)
    m[0, 13, 20] = 1e-20
    m[1, 37, 2] = 1e-20
    return m
