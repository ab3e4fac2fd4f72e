"""The image definition of mi355_render_hands (include/mi355pose.h, "rendered hands") restated in numpy, operation by operation in
float32 with the hash in uint32, and the record builders the render tests share.  render(recs, S, mean3, inv_std3) -> (out, out_ema,
ids), every pixel of every sample, no tiles and no culling: what the kernel must reproduce bit for bit."""
import numpy as np

F = np.float32
U = np.uint32
MAX_COORD = F(1048576.0)
NUM_PRIMS = 21


def hash01(s, a, b):
    """H(s, a, b) of the header on uint32 arrays: float(h >> 8) * 2^-24."""
    with np.errstate(over='ignore'):
        s, a, b = U(s) if np.isscalar(s) else s.astype(U), np.asarray(a).astype(U), np.asarray(b).astype(U)
        h = s ^ (a * U(0x9E3779B1))
        h = h ^ (h >> U(16))
        h = h * U(0x85EBCA6B)
        h = h ^ (b * U(0xC2B2AE35))
        h = h ^ (h >> U(13))
        h = h * U(0x27D4EB2F)
        h = h ^ (h >> U(16))
    return (h >> U(8)).astype(F) * F(2.0 ** -24)


def clamp01(q):
    return np.where(q < F(0), F(0), np.where(q > F(1), F(1), q)).astype(F)


def primitives(rec):
    """[(index, ax, ay, az, bx, by, bz, r)] of the VALID primitives of one record, ascending: float32 scalars."""
    out = []
    for k in range(NUM_PRIMS):
        if k < 20:
            ja, jb = (0 if k % 4 == 0 else k), k + 1
            v = (rec['jx'][ja], rec['jy'][ja], rec['jz'][ja], rec['jx'][jb], rec['jy'][jb], rec['jz'][jb], rec['radius'][k])
        else:
            v = (rec['occ_a'][0], rec['occ_a'][1], rec['occ_z'], rec['occ_b'][0], rec['occ_b'][1], rec['occ_z'], rec['occ_r'])
        v = tuple(F(x) for x in v)
        # magnitudes compared as floats (a NaN and an infinity fail); nothing of an invalid primitive is computed with
        if all(bool(np.abs(x) <= MAX_COORD) for x in v) and bool(v[6] > F(0)):
            out.append((k,) + v)
    return out


def trace(prims, px, py):
    """Front-most primitive at the points (px, py): (index or -1, wx, wy, d2, r) arrays."""
    shape = px.shape
    best = np.full(shape, np.inf, F)
    idx = np.full(shape, -1, np.int32)
    bwx, bwy, bd2, br = (np.zeros(shape, F) for _ in range(4))
    for k, ax, ay, az, bx, by, bz, r in prims:
        ex, ey, ez = F(bx - ax), F(by - ay), F(bz - az)
        ee = F(F(ex * ex) + F(ey * ey))
        dx, dy = px - ax, py - ay
        de = dx * ex + dy * ey
        q = de / ee if ee > F(0) else np.zeros(shape, F)           # selection: no quotient is formed for a zero-length bone
        t = clamp01(q)
        cx, cy = ax + t * ex, ay + t * ey
        wx, wy = px - cx, py - cy
        d2 = wx * wx + wy * wy
        r2 = F(r * r)
        cov = d2 <= r2
        depth = (az + t * ez) - np.sqrt(np.where(cov, r2 - d2, F(0)))
        win = cov & (depth < best)
        best = np.where(win, depth, best)
        idx = np.where(win, np.int32(k), idx)
        bwx, bwy, bd2, br = np.where(win, wx, bwx), np.where(win, wy, bwy), np.where(win, d2, bd2), np.where(win, r, br)
    return idx, bwx.astype(F), bwy.astype(F), bd2.astype(F), br.astype(F)


def shade(rec, prims, px, py):
    """(3,) + px.shape colours at the points."""
    idx, wx, wy, d2, r = trace(prims, px, py)
    hit = idx >= 0
    rs = np.where(hit, r, F(1))
    nx, ny = wx / rs, wy / rs
    nz = np.sqrt(F(1) - d2 / (rs * rs))
    l = rec['light'].astype(F)
    dot = nx * l[0] + ny * l[1] + nz * l[2]
    lam = np.where(dot > F(0), dot, F(0)).astype(F)
    amb = F(rec['ambient'])
    sh = amb + (F(1) - amb) * lam
    g = clamp01((px * F(rec['grad'][0]) + py * F(rec['grad'][1])) + F(rec['grad_off']))
    amp, inv = F(rec['noise_amp']), F(rec['noise_inv_cell'])
    add = None
    if bool(amp > F(0)) and bool(inv > F(0)) and bool(inv <= F(1)):
        u, v = (px + F(1)) * inv, (py + F(1)) * inv
        fu, fv = np.floor(u), np.floor(v)
        ix, iy = fu.astype(np.int32).astype(U), fv.astype(np.int32).astype(U)
        fx, fy = u - fu, v - fv
        sx, sy = (fx * fx) * (F(3) - F(2) * fx), (fy * fy) * (F(3) - F(2) * fy)
        sd = U(rec['noise_seed'])
        l00, l10 = hash01(sd, ix, iy), hash01(sd, ix + U(1), iy)
        l01, l11 = hash01(sd, ix, iy + U(1)), hash01(sd, ix + U(1), iy + U(1))
        top, bot = l00 + sx * (l10 - l00), l01 + sx * (l11 - l01)
        val = top + sy * (bot - top)
        add = amp * (val - F(0.5))
    out = np.empty((3,) + px.shape, F)
    for c in range(3):
        base = np.where(idx == NUM_PRIMS - 1, F(rec['occ_col'][c]), F(rec['skin'][c]))
        bg = F(rec['bg0'][c]) + g * F(F(rec['bg1'][c]) - F(rec['bg0'][c]))
        if add is not None:
            bg = bg + add
        out[c] = np.where(hit, base * sh, bg)
    return out


def render_one(rec, S, mean3, inv_std3):
    prims = primitives(rec)
    fi, fj = np.meshgrid(np.arange(S, dtype=F), np.arange(S, dtype=F), indexing='ij')
    q = F(0.25)
    acc = shade(rec, prims, fj - q, fi - q)
    acc = acc + shade(rec, prims, fj + q, fi - q)
    acc = acc + shade(rec, prims, fj - q, fi + q)
    acc = acc + shade(rec, prims, fj + q, fi + q)
    m = F(0.25) * acc
    out, ema = np.empty((3, S, S), F), np.empty((3, S, S), F)
    ui, uj = fi.astype(U), fj.astype(U)
    sigma = F(rec['sensor_sigma'])
    for c in range(3):
        ema[c] = (m[c] - F(mean3[c])) * F(inv_std3[c])
        w = m[c] * F(rec['gain'][c]) + F(rec['bias'][c])
        if bool(sigma > F(0)):
            with np.errstate(over='ignore'):
                seeds = [U(rec['sensor_seed']) ^ (U(4 * c + k + 1) * U(0x632BE5AB)) for k in range(4)]
            u = hash01(seeds[0], ui, uj)
            for k in (1, 2, 3):
                u = u + hash01(seeds[k], ui, uj)
            w = w + sigma * (u - F(2))
        out[c] = (w - F(mean3[c])) * F(inv_std3[c])
    ids = (trace(prims, fj, fi)[0] + 1).astype(np.uint8)
    return out, ema, ids


def render(recs, S, mean3, inv_std3):
    recs = np.atleast_1d(recs)
    res = [render_one(r, S, mean3, inv_std3) for r in recs]
    return tuple(np.stack([r[k] for r in res]) for k in range(3))


def norm():
    """The loaders' normalisation as the kernel takes it: (mean3, inv_std3) fp32, 1 / std formed in double and rounded once."""
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    return mean.astype(F), (1.0 / std).astype(F)


def case_records(S, dtype, dataset_cls):
    """The records of the GPU test at side S: both domains from the data set, then the degenerate ones."""
    cg = dataset_cls(length=8, image_size=S, heatmap_size=S // 4, seed=5, domain='cg')
    ph = dataset_cls(length=64, image_size=S, heatmap_size=S // 4, seed=5, domain='photo', gap=1.0)
    with_occ = next(ph[i][0] for i in range(64) if ph[i][0]['occ_r'] > 0)
    recs = [cg[0][0], ph[1][0], with_occ]
    z = with_occ.copy()                                     # a zero-length bone (joint 6 on joint 5) and a zero radius
    z['jx'][6], z['jy'][6], z['jz'][6] = z['jx'][5], z['jy'][5], z['jz'][5]
    z['radius'][9] = 0.0
    recs.append(z)
    n = ph[2][0].copy()                                     # NaN / inf coordinates, radius and occluder
    n['jx'][3], n['jy'][8], n['jz'][12], n['radius'][16] = np.nan, np.inf, -np.inf, np.inf
    n['occ_a'], n['occ_b'], n['occ_r'], n['occ_z'] = (np.nan, 3.0), (S / 2.0, S / 2.0), 5.0, 0.0
    recs.append(n)
    o = cg[1][0].copy()                                     # a hand wholly outside the frame
    o['jx'] += 4.0 * S
    recs.append(o)
    f = ph[3][0].copy()                                     # an occluder in front of everything, covering the whole frame
    f['occ_a'], f['occ_b'], f['occ_r'], f['occ_z'], f['occ_col'] = (0.0, 0.0), (float(S), float(S)), float(S), -1.0e5, (0.2, 0.6, 0.9)
    recs.append(f)
    return np.array(recs, dtype=dtype)
