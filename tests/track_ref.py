"""numpy restatement of mi355_roi_crop_normalize and mi355_track_update, written from the text of include/mi355pose.h ("hand
tracking"): fp32 operation by operation, every product, sum and quotient rounded on its own.  Nothing here calls the library."""
import numpy as np

f32 = np.float32
MAX_COORD = f32(1048576.0)
REC = np.dtype([('frame', '<i4'), ('x0', '<f4'), ('y0', '<f4'), ('side', '<f4'), ('mirror', '<i4'), ('live', '<i4'), ('lost', '<i4'),
                ('reserved', '<i4')])
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DEFAULTS = dict(tau=0.02, min_joints=8, scale=1.5, alpha=1.0, grow=1.25, max_lost=5, min_side=16.0)


def records(n, **fields):
    rec = np.zeros(n, REC)
    for k, v in fields.items():
        rec[k] = v
    return rec


def norm6(mean=MEAN, std=STD):
    return np.array(list(mean) + list(std), dtype=f32)


def byte_table(norm):
    """T[c][p] = fl(fl((float)p / 255.0f - mean[c]) / std[c])."""
    p = np.arange(256, dtype=f32) / f32(255.0)
    return np.stack([(p - norm[c]) / norm[3 + c] for c in range(3)]).astype(f32)


def usable(r, S, F=None):
    """live != 0, (0 <= frame < F when F is given), |x0|, |y0| <= 2^20 (a NaN and an infinity fail), 1 <= side <= 4 S."""
    with np.errstate(invalid='ignore'):
        ok = r['live'] != 0 and bool(np.abs(f32(r['x0'])) <= MAX_COORD) and bool(np.abs(f32(r['y0'])) <= MAX_COORD) \
            and bool(f32(r['side']) >= f32(1.0)) and bool(f32(r['side']) <= f32(4.0) * f32(S))
    if F is not None:
        ok = ok and 0 <= int(r['frame']) < F
    return bool(ok)


def subsamples(side, S):
    side, Sf = f32(side), f32(S)
    return 1 if side <= Sf else (2 if side <= f32(2.0) * Sf else (3 if side <= f32(3.0) * Sf else 4))


def _coord(o, j, off, step):
    """fl(fl(o + fl(fl(j + off) * step)) - 0.5f) for a vector j."""
    u = (j + off).astype(f32)
    p = (u * step).astype(f32)
    s = (f32(o) + p).astype(f32)
    return (s - f32(0.5)).astype(f32)


def _blend(v0, v1, f):
    om = (f32(1.0) - f).astype(f32)
    return ((v0 * om).astype(f32) + (v1 * f).astype(f32)).astype(f32)


def sample(tv, xs, ys):
    """Bilinear samples of the (Hf, Wf, 3) plane of table values at the grid ys x xs -> (len(ys), len(xs), 3)."""
    Hf, Wf = tv.shape[:2]
    with np.errstate(invalid='ignore'):
        in_x = (xs > f32(-1.0)) & (xs < f32(Wf))
        in_y = (ys > f32(-1.0)) & (ys < f32(Hf))
    xz, yz = np.where(in_x, xs, f32(0.0)).astype(f32), np.where(in_y, ys, f32(0.0)).astype(f32)
    xf, yf = np.floor(xz), np.floor(yz)
    fx, fy = (xz - xf).astype(f32), (yz - yf).astype(f32)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)

    def tap(y, x):                                           # (len(ys),), (len(xs),) -> (len(ys), len(xs), 3); +0 outside the frame
        ok = ((y >= 0) & (y < Hf))[:, None] & ((x >= 0) & (x < Wf))[None, :]
        v = tv[np.clip(y, 0, Hf - 1)[:, None], np.clip(x, 0, Wf - 1)[None, :]]
        return np.where(ok[..., None], v, f32(0.0)).astype(f32)

    def row(y):
        a, b = tap(y, x0), tap(y, x0 + 1)
        return np.where((fx == 0)[None, :, None], a, _blend(a, b, fx[None, :, None]))

    r0, r1 = row(y0), row(y0 + 1)
    v = np.where((fy == 0)[:, None, None], r0, _blend(r0, r1, fy[:, None, None]))
    return np.where((in_y[:, None] & in_x[None, :])[..., None], v, f32(0.0)).astype(f32)


def roi_crop_normalize(frames, recs, S, norm=None):
    """out (N, 3, S, S) fp32 of frames (F, Hf, Wf, 3) uint8 and the records."""
    norm = norm6() if norm is None else np.asarray(norm, dtype=f32)
    F, Hf, Wf = frames.shape[:3]
    T = byte_table(norm)
    out = np.zeros((len(recs), 3, S, S), f32)
    idx = np.arange(S)
    for b, r in enumerate(recs):
        if not usable(r, S, F):
            continue
        fr = frames[int(r['frame'])]
        tv = np.stack([T[c][fr[..., c]] for c in range(3)], axis=-1)
        side = f32(r['side'])
        step = side / f32(S)
        n = subsamples(side, S)
        jj = (S - 1 - idx if r['mirror'] != 0 else idx).astype(f32)
        ii = idx.astype(f32)
        acc = None
        for ay in range(n):
            ys = _coord(r['y0'], ii, (f32(ay) + f32(0.5)) / f32(n), step)
            for ax in range(n):
                xs = _coord(r['x0'], jj, (f32(ax) + f32(0.5)) / f32(n), step)
                v = sample(tv, xs, ys)
                acc = v if acc is None else (acc + v).astype(f32)
        out[b] = np.transpose((acc / f32(n * n)).astype(f32), (2, 0, 1))
    return out


def track_update(recs, xy, conf, Hf, Wf, S, **kw):
    """(kp (N, K, 2), vis (N, K), score (N,), next records) of the records, key points xy (N, K, 2) in crop pixels and conf (N, K)."""
    P = dict(DEFAULTS, **kw)
    tau, scale, alpha, grow, min_side = (f32(P[k]) for k in ('tau', 'scale', 'alpha', 'grow', 'min_side'))
    min_joints, max_lost = int(P['min_joints']), int(P['max_lost'])
    xy, conf = np.asarray(xy, dtype=f32), np.asarray(conf, dtype=f32)
    N, K = conf.shape
    Sf, Wff, Hff = f32(S), f32(Wf), f32(Hf)
    kp, vis, score = np.zeros((N, K, 2), f32), np.zeros((N, K), f32), np.zeros(N, f32)
    out = recs.copy()
    half = f32(0.5)
    cap = min(min(Wff, Hff), f32(4.0) * Sf)
    clamp = lambda s: (lambda t: cap if t > cap else t)(min_side if s < min_side else s)
    with np.errstate(all='ignore'):
        for b in range(N):
            r = recs[b]
            if not usable(r, S):
                out['live'][b] = 0
                continue
            x0, y0, side = f32(r['x0']), f32(r['y0']), f32(r['side'])
            st = side / Sf
            sm1 = Sf - f32(1.0)
            m, total = 0, f32(0.0)
            lx = ux = ly = uy = f32(0.0)
            for k in range(K):
                x, y, c = xy[b, k, 0], xy[b, k, 1], conf[b, k]
                xm = (sm1 - x) if r['mirror'] != 0 else x
                kx, ky = x0 + xm * st, y0 + y * st
                fin = bool(np.isfinite(kx) and np.isfinite(ky))
                v = fin and bool(c >= tau)
                kp[b, k] = (kx, ky) if fin else (0.0, 0.0)
                vis[b, k] = 1.0 if v else 0.0
                if v:
                    total = total + c
                    if m == 0:
                        lx = ux = kx
                        ly = uy = ky
                    else:
                        lx, ux = (kx if kx < lx else lx), (kx if kx > ux else ux)
                        ly, uy = (ky if ky < ly else ly), (ky if ky > uy else uy)
                    m += 1
            score[b] = total / f32(m) if m > 0 else f32(0.0)
            hx = side * half
            cx, cy = x0 + hx, y0 + hx
            dead = False
            if m >= min_joints:
                w, h = ux - lx, uy - ly
                e = w if w > h else h
                sn = clamp(scale * e)
                nx, ny = (lx + ux) * half, (ly + uy) * half
                cx, cy = cx + alpha * (nx - cx), cy + alpha * (ny - cy)
                side = clamp(side + alpha * (sn - side))
                lost = 0
            else:
                old = int(r['lost'])
                lost = 1 if old < 0 else (max_lost + 1 if old >= max_lost else old + 1)
                if lost > max_lost:
                    dead = True
                else:
                    t = side * grow
                    side = cap if t > cap else t
            out['lost'][b], out['reserved'][b] = lost, 0
            if dead:
                out['live'][b] = 0
            else:
                h2 = side * half

                def shift(v, L):
                    t = f32(0.0) if v < 0 else v
                    hi = L - side
                    return hi if t > hi else t
                out['x0'][b], out['y0'][b], out['side'][b], out['live'][b] = shift(cx - h2, Wff), shift(cy - h2, Hff), side, 1
    for a in (kp, vis, score):
        assert a.dtype == f32
    return kp, vis, score, out


def box_to_record(box, Wf, Hf, scale=1.5, S=None, min_side=1.0):
    """(x0, y0, side) of the square a tracker starts from: scale_box's rule on an (x0, y0, x1, y1) box without its rounding to whole
    pixels -- side = scale * max(w, h) capped by the frame (and 4 S when S is given), centred and shifted inside the frame.  float64."""
    x0, y0, x1, y1 = (float(v) for v in box)
    cap = min(Wf, Hf) if S is None else min(Wf, Hf, 4 * S)
    side = min(max(scale * max(x1 - x0, y1 - y0), min_side), cap)
    cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
    left = min(max(cx - side / 2, 0.0), Wf - side)
    upper = min(max(cy - side / 2, 0.0), Hf - side)
    return left, upper, side
