"""numpy restatement of the Pillow operations behind the training augmentation chain, one stage at a time, in the
integer / float32 / float64 arithmetic Pillow's C code uses (Geometry.c affine NEAREST, Resample.c BILINEAR, Blend.c,
Convert.c RGB->L, BoxBlur.c).  Test code only: tests/test_augment_cpu.py checks every stage against PIL bit for bit,
and the device kernels (csrc/augment.hip) follow the same arithmetic."""
import math

import numpy as np


# ------------------------------------------------------------------ rotate (Image.rotate, NEAREST, same canvas, fill 0)
def rotate(arr, angle):
    h, w = arr.shape[:2]
    angle = angle % 360.0
    if angle == 0:
        return arr.copy()
    if angle == 180:
        return arr[::-1, ::-1].copy()
    if angle in (90, 270) and w == h:
        return np.ascontiguousarray(np.rot90(arr, 1 if angle == 90 else 3))
    rad = -math.radians(angle)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    a0, a1, a3, a4 = fix(m[0]), fix(m[1]), fix(m[3]), fix(m[4])
    a2, a5 = fix(m[0] * 0.5 + m[1] * 0.5 + m[2]), fix(m[3] * 0.5 + m[4] * 0.5 + m[5])
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xx = (a2 + y * a1 + x * a0) >> 16
    yy = (a5 + y * a4 + x * a3) >> 16
    inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
    out = np.zeros_like(arr)
    out[inside] = arr[yy[inside], xx[inside]]
    return out


# ------------------------------------------------------------------ resize (Image.resize, BILINEAR, no box)
PRECISION_BITS = 32 - 8 - 2


def bilinear_coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc: per output index (xmin, n, int32 coefficients)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((out_size, 2), np.int64), np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            ws.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in ws:
            ww += v
        for x, v in enumerate(ws):
            v = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = xmin, xmax
    return bounds, kk


def _pass(arr, bounds, kk):
    """One 1-D pass along axis 1 of an (H, W, C) uint8 array."""
    out = np.empty((arr.shape[0], len(bounds), arr.shape[2]), np.uint8)
    src = arr.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.einsum('hkc,k->hc', src[:, xmin:xmin + n], kk[xx, :n])
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(arr, size):
    h, w = arr.shape[:2]
    if (w, h) == (size, size):
        return arr.copy()
    bh, kh = bilinear_coeffs(w, size)
    bv, kv = bilinear_coeffs(h, size)
    y0, y1 = bv[0, 0], bv[-1, 0] + bv[-1, 1]
    tmp = _pass(arr[y0:y1], bh, kh) if w != size else arr[y0:y1]
    bv = bv.copy()
    bv[:, 0] -= y0
    if h == size:
        return tmp.copy()
    return _pass(tmp.transpose(1, 0, 2), bv, kv).transpose(1, 0, 2).copy()


# ------------------------------------------------------------------ colour jitter (ImageEnhance + Image.blend)
def luminance(arr):
    a = arr.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, arr, factor):
    """Blend.c: out = in1 + alpha * (in2 - in1) in float32, truncated; clipped only when alpha leaves [0, 1]."""
    f = np.float32(factor)
    v = degenerate.astype(np.float32) + f * (arr.astype(np.float32) - degenerate.astype(np.float32))
    if 0 <= factor <= 1:
        return v.astype(np.uint8)
    return np.where(v <= 0, 0, np.where(v >= 255, 255, np.clip(v, 0, 255).astype(np.uint8))).astype(np.uint8)


def brightness(arr, f):
    return blend(np.zeros_like(arr), arr, f)


def contrast(arr, f):
    L = luminance(arr)
    mean = int(float(L.astype(np.int64).sum()) / L.size + 0.5)
    return blend(np.full_like(arr, mean), arr, f)


def saturation(arr, f):
    return blend(np.repeat(luminance(arr)[..., None], 3, axis=2), arr, f)


OPS = (brightness, contrast, saturation)


def jitter(arr, factors, order):
    """factors (brightness, contrast, saturation); order: op indices (0, 1, 2 as above) in application order."""
    for k in order:
        arr = OPS[k](arr, factors[k])
    return arr


# ------------------------------------------------------------------ Gaussian blur (ImagingGaussianBlur: 3 box passes per axis)
def box_radius(radius, passes=3):
    """BoxBlur.c _gaussian_blur_radius in float32 (sqrt and floor in double, as C promotes them)."""
    f32 = np.float32
    sigma2 = f32(radius) * f32(radius) / f32(passes)
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * sigma2)
    a = a / (f32(6) * (sigma2 - (l + f32(1)) * (l + f32(1))))
    return f32(l + a)


def box_weights(fr):
    """ImagingHorizontalBoxBlur: integer radius, centre weight ww and far weight fw (24-bit fixed point)."""
    r = int(fr)
    ww = int(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1)))
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww, fw


def _box_line(a, r, ww, fw):
    """One box pass along axis 1 with edge clamp: (ww * window sum + fw * (far left + far right) + 2^23) >> 24."""
    n = a.shape[1]
    src = a.astype(np.int64)
    idx = lambda k: np.clip(np.arange(n) + k, 0, n - 1)
    acc = sum(src[:, idx(k)] for k in range(-r, r + 1))
    bulk = (acc * ww + (src[:, idx(-r - 1)] + src[:, idx(r + 1)]) * fw) & 0xffffffff
    return ((bulk + (1 << 23)) >> 24).astype(np.uint8)


def blur(arr, radius, passes=3):
    if radius == 0:
        return arr.copy()
    fr = box_radius(radius, passes)
    out = arr
    if fr != 0:
        r, ww, fw = box_weights(fr)
        for _ in range(passes):
            out = _box_line(out, r, ww, fw)
        out = out.transpose(1, 0, 2)
        for _ in range(passes):
            out = _box_line(out, r, ww, fw)
        out = out.transpose(1, 0, 2)
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------ normalisation (to_tensor + Normalize)
def normalise(arr, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    x = arr.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return (x - np.array(mean, np.float32)[:, None, None]) / np.array(std, np.float32)[:, None, None]
