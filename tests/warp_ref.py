"""Numpy restatement of the geometric teacher view (csrc/warp.hip), rounding for rounding, a float64 oracle of the same sampler
and the composition of the per-sample records.

The view of sample b maps a point p = (x, y) of the loader's frame to q = s R(a) (p - c) + c + t, c = ((W-1)/2, (H-1)/2).  A record
holds three row-major 2 x 3 fp32 matrices, each composed in float64 and rounded once:

    img     output pixel of the warped image -> input pixel:                A^-1
    hm      A written in heat-map pixels (image = stride * heat-map):       [L | (c + t - L c) / stride],  L = s R(a)
    hm_inv  the inverse of hm

Arithmetic of both warps, fp32, nothing contracted into an FMA, for the output pixel (row i, column j) and the matrix m:

    xs = fl(fl(fl(m00 * j) + fl(m01 * i)) + m02),  ys likewise with m10, m11, m12
    the sample is +0 unless xs > -1 and xs < W and ys > -1 and ys < H     (false for NaN: nothing is converted out of range)
    x0 = floor(xs), fx = fl(xs - x0);  a tap outside the plane has the value +0
    horizontally  r = v0 if fx == 0 else fl(fl(v0 * fl(1 - fx)) + fl(v1 * fx)); vertically the same form on the two row results
    with fy.  A tap with weight exactly 0 (fx == 0: v1; fy == 0: the whole lower row) is not read.

So the identity record, integer shifts and exact quarter turns copy their taps bit for bit, -0, inf and NaN included.

The flag of a map: u* = the arg-max of the teacher's map by mi355_argmax2d's rules (first index on ties; a NaN counts as the
maximum, the first NaN wins); valid iff margin <= u*_x <= (w-1) - margin and margin <= u*_y <= (h-1) - margin in fp32, and
p* = hm_inv u* (the order above) lies in [0, w-1] x [0, h-1].  The location decides, not the peak's value.

The weighted MSE: mi355_mse_heatmap's row sum s in its fixed order, rows[r] = fl(s * w), grad = fl(fl(d * gs) * w); a row
with w == 0 or outside the joint mask is exact zeros."""
import numpy as np

F = np.float32
IDENTITY = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float64)


# ---------------------------------------------------------------- records
def _hw(size):
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


def compose64(angle_deg, scale, shift, image_size, heatmap_size):
    """The three float64 2 x 3 matrices (img, hm, hm_inv) of one sample.  shift = (tx, ty) in image pixels."""
    H, W = _hw(image_size)
    h, w = _hw(heatmap_size)
    if H * w != W * h or W % w != 0:
        raise ValueError('the strides in x and y must be equal whole numbers: image %dx%d, heat-map %dx%d' % (H, W, h, w))
    stride = W // w
    a = np.deg2rad(np.float64(angle_deg))
    L = np.float64(scale) * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], dtype=np.float64)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0], dtype=np.float64)
    T = c + np.asarray(shift, dtype=np.float64) - L @ c
    Li = np.linalg.inv(L)
    img = np.concatenate([Li, (-Li @ T)[:, None]], axis=1)
    hm = np.concatenate([L, (T / stride)[:, None]], axis=1)
    hm_inv = np.concatenate([Li, (-Li @ T / stride)[:, None]], axis=1)
    return img, hm, hm_inv


def records(angle_deg, scale, shift, image_size, heatmap_size):
    """(B, 18) fp32: img, hm, hm_inv of every sample, each rounded once from float64."""
    angle_deg, scale = np.atleast_1d(angle_deg), np.atleast_1d(scale)
    shift = np.asarray(shift, dtype=np.float64).reshape(len(angle_deg), 2)
    out = np.zeros((len(angle_deg), 18), dtype=F)
    for b in range(len(angle_deg)):
        out[b] = np.concatenate([m.reshape(-1) for m in compose64(angle_deg[b], scale[b], shift[b], image_size, heatmap_size)]).astype(F)
    return out


def from_matrices(img=IDENTITY, hm=IDENTITY, hm_inv=None):
    """One record (18,) from matrices given as such (no cos / sin); hm_inv defaults to the float64 inverse of hm."""
    hm = np.asarray(hm, dtype=np.float64)
    if hm_inv is None:
        Li = np.linalg.inv(hm[:, :2])
        hm_inv = np.concatenate([Li, (-Li @ hm[:, 2])[:, None]], axis=1)
    return np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1) for m in (img, hm, hm_inv)]).astype(F)


def shift_matrix(dx, dy):
    """Output pixel (x, y) samples the input at (x + dx, y + dy)."""
    return np.array([[1, 0, dx], [0, 1, dy]], dtype=np.float64)


def quarter_matrix(side):
    """An exact quarter turn of a square plane of `side` pixels: output (x, y) samples the input at (side - 1 - y, x)."""
    return np.array([[0, -1, side - 1], [1, 0, 0]], dtype=np.float64)


# ---------------------------------------------------------------- the sampler
def _coords32(m, H, W):
    m = np.asarray(m, dtype=F).reshape(2, 3)
    j = np.arange(W, dtype=F)[None, :]
    i = np.arange(H, dtype=F)[:, None]
    with np.errstate(all='ignore'):
        xs = ((m[0, 0] * j) + (m[0, 1] * i)) + m[0, 2]
        ys = ((m[1, 0] * j) + (m[1, 1] * i)) + m[1, 2]
    assert xs.dtype == F and ys.dtype == F
    return np.broadcast_to(xs, (H, W)), np.broadcast_to(ys, (H, W))


def _blend32(v0, v1, f):
    with np.errstate(all='ignore'):
        om = F(1) - f
        r = (v0 * om) + (v1 * f)
    assert r.dtype == F
    return np.where(f == 0, v0, r)


def sample32(plane, m, out_hw=None):
    """One fp32 plane (Hin, Win) resampled under the 2 x 3 matrix m onto (H, W) = out_hw (default: its own size)."""
    plane = np.asarray(plane, dtype=F)
    Hin, Win = plane.shape
    H, W = out_hw or (Hin, Win)
    xs, ys = _coords32(m, H, W)
    with np.errstate(all='ignore'):
        inside = (xs > -1) & (xs < Win) & (ys > -1) & (ys < Hin)
    xz, yz = np.where(inside, xs, F(0)), np.where(inside, ys, F(0))
    x0f, y0f = np.floor(xz), np.floor(yz)
    fx, fy = (xz - x0f).astype(F), (yz - y0f).astype(F)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

    def tap(y, x):
        ok = (x >= 0) & (x < Win) & (y >= 0) & (y < Hin)
        return np.where(ok, plane[np.clip(y, 0, Hin - 1), np.clip(x, 0, Win - 1)], F(0))

    r0 = _blend32(tap(y0, x0), tap(y0, x0 + 1), fx)
    r1 = _blend32(tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fx)
    out = _blend32(r0, r1, fy)
    return np.where(inside, out, F(0)).astype(F)


def sample64(plane, m, out_hw=None):
    """The float64 oracle: plain bilinear interpolation with zeros outside, coordinates and blend in float64."""
    plane = np.asarray(plane, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64).reshape(2, 3)
    Hin, Win = plane.shape
    H, W = out_hw or (Hin, Win)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xs = m[0, 0] * j + m[0, 1] * i + m[0, 2]
    ys = m[1, 0] * j + m[1, 1] * i + m[1, 2]
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = xs - x0, ys - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(y, x):
        ok = (x >= 0) & (x < Win) & (y >= 0) & (y < Hin)
        return np.where(ok, plane[np.clip(y, 0, Hin - 1), np.clip(x, 0, Win - 1)], 0.0)

    return (tap(y0, x0) * (1 - fx) + tap(y0, x0 + 1) * fx) * (1 - fy) + (tap(y0 + 1, x0) * (1 - fx) + tap(y0 + 1, x0 + 1) * fx) * fy


def warp_images(x, recs):
    """v[b, c] = x[b, c] sampled under recs[b].img."""
    x = np.asarray(x, dtype=F)
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            out[b, c] = sample32(x[b, c], recs[b, 0:6])
    return out


# ---------------------------------------------------------------- arg-max, flag, back-warp
def argmax2d(plane):
    """mi355_argmax2d's index: a NaN counts as the maximum (the first one wins), else the first maximum in row-major order."""
    flat = np.asarray(plane, dtype=F).reshape(-1)
    nan = np.isnan(flat)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(flat))


def valid_flag(plane, rec, margin):
    h, w = plane.shape
    i = argmax2d(plane)
    ux, uy = F(i % w), F(i // w)
    mg = F(margin)
    if not (ux >= mg and ux <= F(w - 1) - mg and uy >= mg and uy <= F(h - 1) - mg):
        return F(0)
    m = np.asarray(rec[12:18], dtype=F).reshape(2, 3)
    with np.errstate(all='ignore'):
        px = ((m[0, 0] * ux) + (m[0, 1] * uy)) + m[0, 2]
        py = ((m[1, 0] * ux) + (m[1, 1] * uy)) + m[1, 2]
    return F(1) if (px >= 0 and px <= F(w - 1) and py >= 0 and py <= F(h - 1)) else F(0)


def unwarp_heatmaps(y, recs, margin, w_in=None):
    """(y_hat, valid, w_out): y_hat[b, k] = y[b, k] sampled under recs[b].hm, valid (B, K), w_out = w_in * valid or None."""
    y = np.asarray(y, dtype=F)
    B, K = y.shape[:2]
    out, valid = np.empty_like(y), np.zeros((B, K), dtype=F)
    for b in range(B):
        for k in range(K):
            out[b, k] = sample32(y[b, k], recs[b, 6:12])
            valid[b, k] = valid_flag(y[b, k], recs[b], margin)
    w_out = None
    if w_in is not None:
        with np.errstate(all='ignore'):
            w_out = (np.asarray(w_in, dtype=F).reshape(B, K) * valid).astype(F).reshape(np.shape(w_in))
    return out, valid, w_out


# ---------------------------------------------------------------- weighted MSE
def _row_sum(e, vec):
    """mi355_mse_heatmap's fixed order over the squared differences e of one row: 256 lanes, each summing its elements in index
    order (vec: quads 4t, 4t + 1024, ...; scalar: t, t + 256, ...), the xor butterfly inside each wave, the four waves in order."""
    n = e.size
    lane = np.zeros(256, dtype=F)
    for t in range(256):
        if vec:
            idx = [j + q for j in range(4 * t, n, 1024) for q in range(4)]
        else:
            idx = range(t, n, 256)
        s = F(0)
        for j in idx:
            s = F(s + e[j])
        lane[t] = s
    v = lane.reshape(4, 64)
    ids = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, ids ^ o]).astype(F)
    r = F(0)
    for q in range(4):
        r = F(r + v[q, 0])
    return r


def mse_heatmap_w(pred, target, joint_mask, grad_scale, wmap, vec=None):
    """(rows (B, K), grad (B, K, H, W)) of mi355_mse_heatmap_w.  vec: the 16-byte build (default: HW % 4 == 0)."""
    pred, target = np.asarray(pred, dtype=F), np.asarray(target, dtype=F)
    B, K, H, W = pred.shape
    HW = H * W
    vec = (HW % 4 == 0) if vec is None else vec
    wmap = np.asarray(wmap, dtype=F).reshape(B, K)
    rows, grad = np.zeros((B, K), dtype=F), np.zeros(pred.shape, dtype=F)
    gs = F(grad_scale)
    with np.errstate(all='ignore'):
        for b in range(B):
            for k in range(K):
                w = wmap[b, k]
                if not ((joint_mask >> k) & 1) or w == 0:
                    continue
                d = (pred[b, k] - target[b, k]).reshape(-1)
                rows[b, k] = F(_row_sum((d * d).astype(F), vec) * w)
                grad[b, k] = ((d * gs) * w).astype(F).reshape(H, W)
    return rows, grad


# ---------------------------------------------------------------- round-trip helpers
def gaussian(h, w, cx, cy, sigma=2.0):
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.exp(-((j - cx) ** 2 + (i - cy) ** 2) / (2.0 * sigma * sigma)).astype(F)
