"""CPU references of the image-resolution evaluation (csrc/eval.hip, utils/keypoint_detection.py): float64 / torch-CPU
restatements of
  * compute_uv_from_heatmaps2 (reference utils/keypoint_detection.py:172-205): nn.Upsample(bilinear) then first-index arg-max;
  * the sequential float64 accumulation of mi355_pose_metrics (accuracy_2d :128-136 over visible joints, the `<` of
    accuracy_3d :95-126);
  * the PCK curve and its trapezoid AUC.
Nothing here touches the GPU or the library."""
import numpy as np
import torch


def upsample(hm, size, dtype=torch.float32):
    """nn.Upsample(size, mode='bilinear') (align_corners=False) of a (rows, h, w) or (B, K, h, w) array, on the CPU in `dtype`."""
    t = torch.as_tensor(np.asarray(hm)).to(dtype)
    lead = t.shape[:-2]
    t = t.reshape((1, -1) + tuple(t.shape[-2:]))
    up = torch.nn.Upsample(size=tuple(size) if not isinstance(size, int) else (size, size), mode='bilinear')(t)
    return up.reshape(tuple(lead) + tuple(up.shape[-2:]))


def first_argmax(maps):
    """(idx int32, xy float32, maxval) of (rows, H, W) maps by mi355_argmax2d's rules: first maximum in row-major order, NaN
    counts as maximum (numpy's argmax), x = idx % W, y = idx // W, both zero unless the maximum is > 0."""
    a = maps.numpy() if torch.is_tensor(maps) else np.asarray(maps)
    rows, H, W = a.shape
    flat = a.reshape(rows, -1)
    idx = flat.argmax(1)
    mv = flat[np.arange(rows), idx]
    pos = mv > 0
    xy = np.stack([np.where(pos, idx % W, 0), np.where(pos, idx // W, 0)], 1).astype(np.float32)
    return idx.astype(np.int32), xy, mv


def upsample_argmax(hm, size, dtype=torch.float32):
    """The reference of mi355_upsample_argmax on (rows, h, w) maps: (idx, xy, maxval as `dtype`)."""
    return first_argmax(upsample(hm, size, dtype))


def upsample_kernel_order(hm, size):
    """The up-sampling in the arithmetic mi355_upsample_argmax is specified with -- bilinear_up_kernel's index and weight rule and
    expression order, every fp32 operation rounded on its own (numpy float32: no contraction):
        v = hy * (hx * a + lx * b) + ly * (hx * c + lx * d).
    torch's fp32 CPU kernel evaluates the same formula but may contract or reorder it, which moves a value by an ulp; on maps
    of arbitrary floats that decides between outputs that replicate one border pixel (.875 a + .125 a against .625 a + .375 a),
    so bit comparisons on such maps are made against this function (test_eval_cpu.py ties it to torch: identical where the
    up-sampling is exact, within 4 * 2^-24 * max|in| of float64 elsewhere)."""
    f = np.float32
    maps = np.ascontiguousarray(hm, dtype=np.float32)
    rows, h, w = maps.shape
    H, W = (size, size) if isinstance(size, int) else size
    sy, sx = f(h) / f(H), f(w) / f(W)
    fy = np.maximum(sy * (np.arange(H, dtype=np.float32) + f(.5)) - f(.5), f(0))
    fx = np.maximum(sx * (np.arange(W, dtype=np.float32) + f(.5)) - f(.5), f(0))
    y0, x0 = np.minimum(fy.astype(np.int32), h - 1), np.minimum(fx.astype(np.int32), w - 1)
    y1, x1 = y0 + (y0 < h - 1), x0 + (x0 < w - 1)
    ly, lx = fy - y0.astype(np.float32), fx - x0.astype(np.float32)
    hy, hx = f(1) - ly, f(1) - lx
    ly, hy, lx, hx = ly[None, :, None], hy[None, :, None], lx[None, None, :], hx[None, None, :]
    with np.errstate(invalid='ignore'):
        top = hx * maps[:, y0][:, :, x0] + lx * maps[:, y0][:, :, x1]
        bot = hx * maps[:, y1][:, :, x0] + lx * maps[:, y1][:, :, x1]
        v = hy * top + ly * bot
    assert v.dtype == np.float32
    return v


def exact_upsampling(hm, size):
    """True when the fp32 CPU up-sampling of `hm` equals the float64 one bit for bit (every product and sum is exact, so any
    evaluation order gives these values): the claim the bit comparisons of the GPU tests rest on."""
    a, b = upsample(hm, size, torch.float32), upsample(hm, size, torch.float64)
    return bool(torch.equal(a.double(), b))


def integer_maps(rows, h, w, seed, lo=-512, hi=512):
    """Integer-valued fp32 maps in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(rows, h, w)).astype(np.float32)


def metrics_state(K, T):
    return np.zeros(K, np.float64), np.zeros(K, np.int64), np.zeros((K, T), np.int64)


def accumulate(pred, gt, vis, thr, state):
    """mi355_pose_metrics: per joint k, for b in order, where vis > 0: e = sqrt(dx^2 + dy^2) in float64 from the fp32 inputs,
    sum_err[k] += e, count[k] += 1, hits[k][t] += e < float64(thr[t])."""
    pred, gt = np.asarray(pred, np.float32).astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
    vis = np.asarray(vis, np.float32).reshape(pred.shape[0], pred.shape[1])
    thr = np.asarray(thr, np.float32).astype(np.float64)
    sum_err, count, hits = state
    B, K, _ = pred.shape
    for k in range(K):
        for b in range(B):
            if not vis[b, k] > 0:
                continue
            dx, dy = pred[b, k, 0] - gt[b, k, 0], pred[b, k, 1] - gt[b, k, 1]
            e = np.sqrt(dx * dx + dy * dy)
            sum_err[k] += e
            count[k] += 1
            hits[k] += e < thr
    return state


def trapz(y, x):
    """np.trapz(y, x), spelled out (numpy 2 renamed it)."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


def summary(state, thr, max_px, groups=None):
    """{'epe', 'epe_<group>', 'pck_curve', 'auc'} of accumulated state: sums over joints divided by counts; nan when nothing
    was visible."""
    sum_err, count, hits = state
    with np.errstate(divide='ignore', invalid='ignore'):
        n = np.float64(count.sum())
        out = {'epe': float(sum_err.sum() / n), 'pck_curve': hits.sum(0) / n}
        for name, ks in (groups or {}).items():
            out['epe_' + name] = float(sum_err[list(ks)].sum() / np.float64(count[list(ks)].sum()))
    out['auc'] = trapz(out['pck_curve'], np.asarray(thr, np.float32).astype(np.float64)) / float(max_px)
    return out


# ---------------------------------------------------------------- the cases the CPU and GPU tests share
# (rows, h, w, H, W): power-of-two ratios on integer maps, where the up-sampling is exact (test_eval_cpu.py asserts it per case).
# The last but one is the map at its own size (mi355_argmax2d's bits); the last is beyond the 64 KB the kernel stages in LDS.
EXACT_CASES = [(1, 1, 1, 4, 4), (3, 5, 7, 20, 28), (21, 8, 8, 16, 16), (42, 16, 16, 64, 64), (42, 64, 64, 256, 256),
               (2, 128, 128, 512, 512), (5, 32, 32, 256, 256), (4, 64, 64, 64, 64), (1, 130, 130, 260, 260)]


def exact_case_maps(case):
    rows, h, w, H, W = case
    return integer_maps(rows, h, w, seed=[1301, rows, h, w, H, W])


def special_maps(h=16, w=16):
    """{name: (rows, h, w) integer-valued maps}: all negative, all zero, one NaN pixel, and a single maximum in each corner and
    on each edge of the map."""
    rng = np.random.default_rng(77)
    out = {'negative': rng.integers(-512, 0, size=(3, h, w)).astype(np.float32), 'zero': np.zeros((2, h, w), np.float32)}
    nan = rng.integers(-512, 513, size=(4, h, w)).astype(np.float32)
    for r, (y, x) in enumerate(((0, 0), (h // 2, w // 3), (h - 1, w - 1), (3, w - 1))):
        nan[r, y, x] = np.nan
    out['nan'] = nan
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    one = rng.integers(-512, 400, size=(len(spots), h, w)).astype(np.float32)
    for r, (y, x) in enumerate(spots):
        one[r, y, x] = 512.0
    out['corners_edges'] = one
    return out
