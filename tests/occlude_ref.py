"""Numpy restatement of csrc/occlude.hip (include/mi355pose.h, "adaptive occlusion, teacher confidence"): mi355_peak_prob in
float64 (or, for the yardstick, in float32), mi355_teacher_select and mi355_occlude_images bit for bit, and the input builders
of tests/test_occlude_cpu.py, tests/test_gpu_occlude.py and tests/test_gpu_occlude_step.py.  No GPU-only code."""
import numpy as np

TAU_GAP = 1e-4                   # no float64 p may lie within this relative distance of the tau it is compared with
U_MAX = np.nextafter(np.float32(1.0), np.float32(0.0))      # the largest float32 below 1
SIDES = ((256, 64), (64, 16), (16, 16))                     # (image side, heat-map side) the project admits


def f32(x):
    """The float32 value the C ABI receives for a Python float argument."""
    return float(np.float32(x))


# --------------------------------------------------------------------------------------------------------------- peak_prob
def argmax2d(hm):
    """(idx int32 [rows], xy float32 [rows, 2]) by mi355_argmax2d's rules: numpy's arg-max (first index on ties, a NaN counts as
    the maximum), the coordinates 0 unless the maximum is > 0."""
    rows, H, W = hm.shape
    flat = hm.reshape(rows, H * W)
    idx = flat.argmax(1).astype(np.int32)
    mv = flat[np.arange(rows), idx]
    pos = np.greater(mv, 0.0)
    xy = np.stack([np.where(pos, idx % W, 0), np.where(pos, idx // W, 0)], 1).astype(np.float32)
    return idx, xy


def peak_prob(hm, beta, dtype=np.float64):
    """(idx, xy, p [rows] in `dtype`): p = 1 / sum(exp(beta * y - max(beta * y))), NaN for a map that holds a NaN or an inf.
    hm: float32 [rows, H, W]; beta: the float32 value the kernel receives."""
    rows = hm.shape[0]
    idx, xy = argmax2d(hm)
    z = hm.reshape(rows, -1).astype(dtype) * dtype(beta)
    with np.errstate(invalid='ignore', over='ignore'):
        mx = np.nanmax(np.where(np.isfinite(z), z, -np.inf), axis=1) if z.size else z
        s = np.exp(z - mx[:, None].astype(dtype)).sum(1, dtype=dtype)
        p = (dtype(1.0) / s).astype(dtype)
    p[~np.isfinite(hm.reshape(rows, -1)).all(1)] = np.nan
    return idx, xy, p


def gaussian_label(H, W, cx, cy, sigma=2.0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def maps(H, W, rows, seed=0):
    """float32 [rows, H, W] logits: a bump of another height (0.5 .. 14) at another place per map over noise, so that the peaks of
    the softmax spread from about 1 / HW to nearly 1."""
    r = np.random.RandomState(9100 + 131 * H + 17 * W + rows + seed)
    out = np.empty((rows, H, W), np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(rows):
        cx, cy = r.uniform(0, W - 1), r.uniform(0, H - 1)
        amp = 0.5 + 13.5 * ((i * 7 + seed) % 11) / 10.0
        out[i] = amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0) + 0.3 * r.randn(H, W)
    return out.astype(np.float32)


def tau_between(p64, k=None):
    """A threshold between two neighbours of the sorted finite p (their geometric mean): about half of the maps pass."""
    s = np.sort(p64[np.isfinite(p64)])
    if s.size < 2:
        return f32(0.5 * float(s[0])) if s.size else 0.5
    k = s.size // 2 if k is None else k
    return f32(np.sqrt(float(s[k - 1]) * float(s[k])))


def tau_in_widest_gap(p64):
    """A threshold in the widest relative gap between two neighbours of the sorted finite p (their geometric mean): peaks that
    come from a network crowd together, and the flags must not hang on the last bits of one of them."""
    s = np.sort(p64[np.isfinite(p64)])
    k = 1 + int(np.argmax(s[1:] / s[:-1]))
    return f32(np.sqrt(float(s[k - 1]) * float(s[k])))


def tau_clear(p64, tau):
    """True when no finite p lies within the relative TAU_GAP of tau (the flags are discontinuous in p there)."""
    p = p64[np.isfinite(p64)]
    return bool((np.abs(p - float(tau)) > TAU_GAP * abs(float(tau))).all())


# ---------------------------------------------------------------------------------------------------------- teacher_select
def teacher_select(p, xy, gate_in, w_in, u, tau, prob, N, lo, hi, S, H, W):
    """-> (conf float32 (B, K), w_out (w_in's shape) or None, boxes int32 (B, N, 4) or None, count int32 (B,) or None,
    stats float32 (2,)).  p float32 (B, K); xy float32 (B, K, 2); u float32 (B, 1 + 2N)."""
    B, K = p.shape
    tau32, prob32 = np.float32(tau), np.float32(prob)
    with np.errstate(invalid='ignore'):
        ok = p.astype(np.float32) >= tau32
    if gate_in is not None:
        ok = ok & (gate_in.reshape(B, K) > 0)
    conf = ok.astype(np.float32)
    w_out = None if w_in is None else (w_in.astype(np.float32) * conf.reshape(w_in.shape)).astype(np.float32)
    boxes = count = None
    if N > 0:
        boxes, count = np.zeros((B, N, 4), np.int32), np.zeros(B, np.int32)
        sx, sy = S // W, S // H
        for b in range(B):
            cand = [k for k in range(K) if ok[b, k] and (w_in is None or w_in.reshape(B, K)[b, k] > 0)]
            if u[b, 0] >= prob32:
                continue
            m = len(cand)
            for i in range(min(N, m)):
                mm = m - i
                t = np.float32(u[b, 1 + 2 * i]) * np.float32(mm)
                t = min(max(t, np.float32(0)), np.float32(mm - 1)) if t == t else np.float32(0)
                k = cand.pop(int(t))
                ts = np.float32(u[b, 2 + 2 * i]) * np.float32(hi - lo + 1)
                ts = min(max(ts, np.float32(0)), np.float32(hi - lo)) if ts == ts else np.float32(0)
                side = lo + int(ts)
                fx, fy = xy[b, k]
                fx = min(max(fx, np.float32(0)), np.float32(W - 1)) if fx == fx else np.float32(0)
                fy = min(max(fy, np.float32(0)), np.float32(H - 1)) if fy == fy else np.float32(0)
                cx, cy = int(fx) * sx + sx // 2, int(fy) * sy + sy // 2
                x0, y0 = cx - side // 2, cy - side // 2
                boxes[b, i] = (max(x0, 0), max(y0, 0), min(x0 + side, S), min(y0 + side, S))
                count[b] += 1
    stats = np.array([0.0 if count is None else np.float32(int(count.sum())) / np.float32(B),
                      np.float32(int(ok.sum())) / (np.float32(B) * np.float32(K))], np.float32)
    return conf, w_out, boxes, count, stats


def select_case(B, K, N, mode, sides=(256, 64), gate=False, w=None, u_mode='rand', seed=0):
    """Inputs of one teacher_select call.  mode: 'mixed' (about half of the joints pass), 'none' (no candidate), 'few' (one or two
    candidates), 'corners' (every joint passes, the key points sit in the four corners), 'equal' (lo == hi).  w: None, 'flat'
    (B, K) or 'col' (B, K, 1), with zeros and halves in it.  u_mode: 'rand', 'zero', 'max'."""
    S, Hs = sides
    r = np.random.RandomState(5200 + 97 * B + 13 * K + 7 * N + seed)
    p = np.exp(r.uniform(np.log(1e-4), np.log(0.9), size=(B, K))).astype(np.float32)
    xy = np.stack([r.randint(0, Hs, size=(B, K)), r.randint(0, Hs, size=(B, K))], 2).astype(np.float32)
    tau = tau_between(p.astype(np.float64))
    if mode == 'none':
        tau = f32(0.95)
    elif mode == 'few':
        tau = tau_between(p.astype(np.float64), k=max(p.size - min(2, p.size - 1), 1))
    elif mode == 'corners':
        tau = f32(5e-5)
        c = np.array([[0, 0], [Hs - 1, 0], [0, Hs - 1], [Hs - 1, Hs - 1]], np.float32)
        xy = c[np.arange(B * K) % 4].reshape(B, K, 2)
    lo, hi = max(1, S // 12), max(1, S // 6)
    if mode == 'equal':
        lo = hi
    if mode == 'corners':
        lo, hi = max(1, S // 4), max(1, S // 2)            # large boxes: clipped on two sides
    if u_mode == 'rand':
        u = r.uniform(0, 1, size=(B, 1 + 2 * N)).astype(np.float32)
        u = np.minimum(u, U_MAX)
        u[:, 0] = np.where(np.arange(B) % 3 == 2, 0.9, 0.1)   # every third sample draws no box (prob = 0.5)
    else:
        u = np.full((B, 1 + 2 * N), 0.0 if u_mode == 'zero' else U_MAX, np.float32)
        u[:, 0] = 0.0
    g = None
    if gate:
        g = (r.uniform(size=(B, K)) > 0.3).astype(np.float32)
    w_in = None
    if w is not None:
        w_in = np.array([1.0, 0.5, 0.0, 1.0], np.float32)[r.randint(0, 4, size=(B, K))]
        if w == 'col':
            w_in = w_in.reshape(B, K, 1)
    return dict(p=p, xy=xy, gate_in=g, w_in=w_in, u=u, tau=tau, prob=0.5, N=N, lo=lo, hi=hi, S=S, H=Hs, W=Hs)


SELECT_CASES = [(B, K, N, mode, sides, gate, w, u_mode)
                for B in (1, 3) for K in (21, 1) for N in (0, 1, 8)
                for (mode, sides, gate, w, u_mode) in (('mixed', SIDES[0], False, None, 'rand'), ('mixed', SIDES[1], True, 'flat', 'rand'),
                                                       ('mixed', SIDES[2], True, 'col', 'max'), ('none', SIDES[0], False, None, 'rand'),
                                                       ('few', SIDES[0], False, 'flat', 'zero'), ('corners', SIDES[0], False, None, 'max'),
                                                       ('corners', SIDES[2], False, None, 'zero'), ('equal', SIDES[1], True, None, 'rand'))]


# ---------------------------------------------------------------------------------------------------------- occlude_images
def occlude_images(x, boxes):
    """x (B, C, H, W) as float32 or uint32 words, boxes int32 (B, N, 4) = (x0, y0, x1, y1) half-open, any values -> the same words
    with the pixels inside any box of the sample set to +0.0 (all bits 0)."""
    bits = np.ascontiguousarray(x).view(np.uint32).copy()
    B, C, H, W = bits.shape
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        hit = np.zeros((H, W), bool)
        for (x0, y0, x1, y1) in boxes[b].astype(np.int64):
            hit |= (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
        bits[b][:, hit] = 0
    return bits.view(x.dtype) if x.dtype == np.float32 else bits


def random_words(shape, seed=0):
    """uint32 words of every kind: random bits, with NaN payloads, infinities, -0.0 and denormals planted."""
    r = np.random.RandomState(6400 + seed)
    w = r.randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    special = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x7FA00000, 0x00000000], np.uint32)
    pos = r.permutation(flat.size)[:max(flat.size // 6, 8)]
    flat[pos] = special[np.arange(pos.size) % special.size]
    return w


def image_boxes(B, H, W, kind, seed=0):
    """int32 (B, N, 4) boxes of one kind: 'empty', 'pixel', 'full', 'overlap', 'eight', 'wild' (partly or wholly outside)."""
    r = np.random.RandomState(7300 + seed)
    if kind == 'empty':
        return np.zeros((B, 1, 4), np.int32)
    if kind == 'pixel':
        return np.array([[[W - 1, H - 1, W, H]]] * B, np.int32)
    if kind == 'full':
        return np.array([[[0, 0, W, H]]] * B, np.int32)
    if kind == 'overlap':
        return np.array([[[1, 1, W // 2 + 2, H // 2 + 2], [W // 2 - 1, H // 2 - 1, W - 1, H - 1], [0, 0, 0, 0]]] * B, np.int32)
    if kind == 'wild':
        return np.array([[[-5, -7, 3, 2], [W - 2, H - 3, W + 40, H + 9], [5, 5, 2, 9], [-2 ** 31, 3, 2 ** 31 - 1, 4]]] * B, np.int32)
    out = np.zeros((B, 8, 4), np.int32)
    for b in range(B):
        for i in range(8):
            x0, y0 = r.randint(0, W), r.randint(0, H)
            out[b, i] = (x0, y0, min(x0 + r.randint(1, 6), W), min(y0 + r.randint(1, 6), H))
    return out
