"""Exact-operand references for the small hand-written kernels: csrc/pool_layout.hip (max-pool, NCHW <-> NHWC, space-to-depth,
stem pack / unpack), csrc/pw21.hip (C -> K, K -> C, their weight gradient, the heat-map row sum) and csrc/optim.hip (SGD, cast),
in the style of bn_exact_ref.py and conv_exact_ref.py.

Every function is float64 torch / numpy written from the operation's definition.  The operands are small integers (or short
dyadic rationals) chosen so that every product, every sum in any order and every result is a float32 value: a correct kernel
then returns the float64 result BIT FOR BIT, whatever its summation order or FMA contraction, and where the output type is bf16
the expectation is that exact value rounded once to nearest even.  check_exact() ASSERTS the range condition of a case, it is
never assumed: every operand is a value of the activation type, the sum of the magnitudes of the terms of every sum stays below
2^24, every named intermediate and every result survives a float32 round trip.

Operand recipes
  pw21      features and residual: integers in [-8, 8]; heat maps and weights: integers in [-4, 4]; bias: integers in [-8, 8];
            scale_dev 0.5 or 1.  A few "hot" pixels and channels are aligned in sign (y[k] = a * s_k, w[c][k] = b * s_k), so the
            K -> C result reaches 16 K: in bf16 it needs up to 10 significant bits and the cases hold real roundings, exact
            ties included (counted by ties()).
  SGD       p a multiple of 4 in [-64, 64], g an integer in [-8, 8], lr 2^-3 / 2^-4 / 2^-3 over three steps, mu = 2^-1,
            wd 2^-2 or 0, buf from zero: every term is a short dyadic rational.
  max-pool  integers in [-3, 3], about a fifth -inf, about a twentieth NaN, a block of zeros in half of the channels (whole
            windows of ties); dy integers in [-32, 32] (a sum of four is exact in bf16).
  layout    any floats, with the special values of SPECIALS sprinkled in; NaN is compared by position (bits_equal).

Window rule of the max-pool (maxpool_fwd_kernel's and ATen's): the window positions are visited row by row; a NaN wins over
everything and the LAST NaN is kept; otherwise the FIRST position of the maximum, which for a window of nothing but -inf is
its first valid position.  The code is kh * 3 + kw of the kept position.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32_EXACT = float(1 << 24)
PER = {'bf16': 8, 'f32': 4}           # CH: elements per 16-byte chunk
TDT = {'bf16': torch.bfloat16, 'f32': torch.float32}
DTS = ('bf16', 'f32')
INF = float('inf')


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def case_id(c):
    return '-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def rne(v, dt):
    """float64 -> the activation type, one round to nearest even (through fp32, which holds every expected value exactly or is
    the type itself), back as float64."""
    return v.float().to(TDT[dt]).double()


def _f32_exact(name, v):
    assert torch.equal(v.float().double(), v), '%s does not survive a float32 round trip' % name


def _is_dt(name, v, dt):
    assert torch.equal(rne(v, dt), v), '%s is not a %s value' % (name, dt)


def ties(v, dt):
    """Number of elements of the exact float64 result `v` that sit exactly half way between two neighbours of `dt`."""
    if dt != 'bf16':
        return 0
    f = v.float()
    assert torch.equal(f.double(), v)
    return int(((f.view(torch.int32) & 0xffff) == 0x8000).sum())


def bits_equal(a, b):
    """Same dtype, same shape, NaN at the same positions (whatever the payload), every other element the same bits (so -0.0 is
    not +0.0 and a flushed subnormal is not the subnormal)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[a.dtype]
    na, nb = a != a, b != b
    if not torch.equal(na, nb):
        return False
    ia, ib = a.contiguous().view(it), b.contiguous().view(it)
    return bool(((ia == ib) | na).all())


def nhwc(t, dtype):
    """A logical NCHW tensor in channels_last memory of `dtype` (plain torch)."""
    return t.to(dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


# ================================================================ A. max-pool 3x3 stride 2 pad 1
MP_MAPS = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 4), (5, 7), (7, 5), (18, 14)]
MP_CASES = {'%s-n%d-c%d-%dx%d' % (dt, N, C, H, W): (dt, N, C, H, W)
            for dt in DTS for N in (1, 3) for C in (PER[dt], 3 * PER[dt]) for H, W in MP_MAPS}
# two images of one chunk: the last row and column of the last image sit against whatever follows the operand
MP_EDGE_MAPS = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 5)]
MP_CASES.update({'%s-n%d-c%d-%dx%d' % (dt, 2, PER[dt], H, W): (dt, 2, PER[dt], H, W) for dt in DTS for H, W in MP_EDGE_MAPS})
# the grid-stride lap: 182 * 182 * 64 = 2 119 936 output chunks > 8192 blocks * 256, and four laps of the backward
MP_LAP = ('bf16', 1, 512, 364, 364)


def mp_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def mp_operands_np(dt, N, C, H, W):
    """int8 values, int8 category (0: NaN, 1..4: -inf, else the value) and int8 dy of one case; the zero block last."""
    rng = _rng('maxpool', dt, N, C, H, W)
    v = rng.integers(-3, 4, size=(N, C, H, W), dtype=np.int8)
    cat = rng.integers(0, 20, size=(N, C, H, W), dtype=np.int8)
    Ho, Wo = mp_out(H, W)
    dy = rng.integers(-32, 33, size=(N, C, Ho, Wo), dtype=np.int8)
    return v, cat, dy


def mp_assemble(v, cat, dtype=torch.float64):
    """The max-pool input from values and categories (torch tensors on any device)."""
    N, C, H, W = v.shape
    x = v.to(dtype)
    x[cat == 0] = float('nan')
    x[(cat >= 1) & (cat <= 4)] = -INF
    x[:, :C // 2, :min(H, 6), :min(W, 6)] = 0.0             # whole windows of ties in half of the channels
    return x


def mp_case(name):
    dt, N, C, H, W = MP_CASES[name]
    v, cat, dy = mp_operands_np(dt, N, C, H, W)
    return dict(dt=dt, x=mp_assemble(torch.from_numpy(v), torch.from_numpy(cat)), dy=_t(dy))


def maxpool_fwd(x):
    """x [N][C][H][W] (any float type that holds the values) -> pooled values and the window code kh * 3 + kw (uint8), both
    [N][C][Ho][Wo], by the window rule of the module docstring."""
    N, C, H, W = x.shape
    Ho, Wo = mp_out(H, W)
    xp = F.pad(x, (1, 2, 1, 2), value=-INF)
    inside = F.pad(torch.ones(H, W, dtype=torch.bool, device=x.device), (1, 2, 1, 2), value=False)
    pos = [(kh, kw) for kh in range(3) for kw in range(3)]
    win = torch.stack([xp[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh, kw in pos])          # [9][N][C][Ho][Wo]
    val = torch.stack([inside[kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh, kw in pos])[:, None, None]
    isn = win != win
    anyn = isn.any(0)
    last_nan = 8 - isn.flip(0).to(torch.uint8).argmax(0)           # argmax keeps the first of equal values
    w0 = torch.where(isn, torch.full_like(win, -INF), win)
    m = w0.max(0).values
    first_max = ((w0 == m) & val).to(torch.uint8).argmax(0)
    code = torch.where(anyn, last_nan, first_max).to(torch.uint8)
    y = torch.where(anyn, torch.full_like(m, float('nan')), m)
    return y, code


def mp_flat_index(code, H, W):
    """Flat input index iy * W + ix each output routes its gradient to."""
    Ho, Wo = code.shape[-2:]
    oy = torch.arange(Ho, device=code.device).view(Ho, 1)
    ox = torch.arange(Wo, device=code.device).view(1, Wo)
    c = code.long()
    iy, ix = 2 * oy - 1 + c // 3, 2 * ox - 1 + c % 3
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all())
    return iy * W + ix


def maxpool_bwd(dy, code, in_shape):
    """dx[n][c][iy][ix] = the sum of dy over the outputs whose kept position is (iy, ix)."""
    N, C, H, W = in_shape
    flat = mp_flat_index(code, H, W).view(N, C, -1)
    dx = torch.zeros(N, C, H * W, dtype=dy.dtype, device=dy.device)
    dx.scatter_add_(2, flat, dy.reshape(N, C, -1))
    return dx.view(N, C, H, W)


def maxpool_bwd_np(dy, code, in_shape):
    """The same scatter in numpy, from arg bytes of whatever origin (the GPU test feeds the kernel's own)."""
    N, C, H, W = in_shape
    Ho, Wo = mp_out(H, W)
    code = np.asarray(code).astype(np.int64)
    iy = 2 * np.arange(Ho).reshape(Ho, 1) - 1 + code // 3
    ix = 2 * np.arange(Wo).reshape(1, Wo) - 1 + code % 3
    assert ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()
    n = np.arange(N).reshape(N, 1, 1, 1)
    c = np.arange(C).reshape(1, C, 1, 1)
    dx = np.zeros((N, C, H, W))
    np.add.at(dx, (np.broadcast_to(n, code.shape), np.broadcast_to(c, code.shape), iy, ix), np.asarray(dy, dtype=np.float64))
    return dx


def check_exact_maxpool(c):
    dt = c['dt']
    x, dy = c['x'], c['dy']
    fin = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    _is_dt('max-pool x', fin, dt)
    _is_dt('max-pool dy', dy, dt)
    y, code = maxpool_fwd(x)
    dx = maxpool_bwd(dy, code, x.shape)
    mag = maxpool_bwd(dy.abs(), code, x.shape)
    assert float(mag.max()) < F32_EXACT
    _f32_exact('max-pool dx', dx)
    _is_dt('max-pool dx', dx, dt)
    _is_dt('max-pool dx magnitude', mag, dt)            # so every partial sum is a value of the type too
    return y, code, dx


# ================================================================ B. layout
BF16_MAX = 3.3895313892515355e38
SPECIALS = np.array([
    1.00390625,              # 1 + 2^-8: a bf16 tie, to even = down (1.0)
    1.01171875,              # 1 + 3 * 2^-8: a bf16 tie, to even = up (1.015625)
    -1.00390625, -1.01171875,
    -0.0, 0.0,
    1e-40,                   # an fp32 subnormal (and a bf16 subnormal after rounding)
    2.0 ** -133,             # the smallest bf16 subnormal
    BF16_MAX, -BF16_MAX,     # the largest finite bf16
    3.4e38,                  # rounds up to inf in bf16
    INF, -INF, float('nan'),
], dtype=np.float32)


def layout_values(tag, *shape):
    """fp32 values of any size with the special values sprinkled in (about one element in six; all of them when there is
    room)."""
    rng = _rng('layout', tag, shape)
    n = int(np.prod(shape))
    v = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 7, size=n))).astype(np.float32)
    k = max(1, n // 6)
    where = rng.permutation(n)[:k]
    v[where] = SPECIALS[(np.arange(k) + rng.integers(0, len(SPECIALS))) % len(SPECIALS)]
    return torch.from_numpy(v.reshape(shape))


def int_values(tag, lo, hi, *shape):
    return _t(_rng('ints', tag, shape).integers(lo, hi + 1, size=shape))


def default_cpad(C, dt):
    return (C + PER[dt] - 1) // PER[dt] * PER[dt]


TO_NHWC_MAPS = [(1, 1), (5, 7), (9, 33)]
TO_NHWC_C = [(1, None), (3, None), (5, None), (8, None), (21, None), (33, None), (3, 16), (21, 32)]        # (C, cpad)
TO_NHWC_LAP = (1, 65, 68, 512, 512)          # f32: 512 * 512 * 17 = 4 456 448 chunks > 16384 blocks * 256
TO_NCHW_C = [1, 8, 31, 32, 33, 72]
TO_NCHW_MAPS = [(1, 1), (1, 31), (4, 8), (3, 11), (35, 37)]          # H * W = 1, 31, 32, 33, 1295
S2D_SHAPES = [(1, 2, 2), (2, 6, 10), (3, 34, 18)]
STEM_CO = [1, 5, 64]


def to_nhwc(x, dt, cpad=None):
    """NCHW fp32 -> logical (N, cpad, H, W) of `dt`, the pad channels +0.0.  (The memory order is the caller's business: the
    tests compare logical tensors.)"""
    N, C, H, W = x.shape
    cpad = cpad or default_cpad(C, dt)
    out = torch.zeros(N, cpad, H, W, dtype=torch.float64)
    out[:, :C] = x.double()
    return out.float().to(TDT[dt])


def to_nchw_f32(x):
    return x.double().float().contiguous()


def s2d(x, dt=None):
    """(N, 3, H, W) -> (N, 16, H/2, W/2): channel (dy*2 + dx)*4 + c holds x[n][c][2 by + dy][2 bx + dx], c = 3 is zero."""
    N, C, H, W = x.shape
    assert C == 3 and H % 2 == 0 and W % 2 == 0
    v = x.double().view(N, 3, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4)          # [n][dy][dx][c][by][bx]
    out = torch.zeros(N, 2, 2, 4, H // 2, W // 2, dtype=torch.float64)
    out[:, :, :, :3] = v
    out = out.reshape(N, 16, H // 2, W // 2)
    return out if dt is None else out.float().to(TDT[dt])


def stem_pack(w):
    """w [Co][7][7][3] -> [Co][4][4][16]: tap (th, tw), channel (dy*2 + dx)*4 + c holds w[o][2 th + dy - 1][2 tw + dx - 1][c];
    kh = -1, kw = -1 and c = 3 are zero (the comment above nchw_to_s2d_kernel)."""
    Co = w.shape[0]
    out = torch.zeros(Co, 4, 4, 16, dtype=w.dtype)
    for th in range(4):
        for tw in range(4):
            for dy in range(2):
                for dx in range(2):
                    kh, kw = 2 * th + dy - 1, 2 * tw + dx - 1
                    if kh >= 0 and kw >= 0:
                        out[:, th, tw, (dy * 2 + dx) * 4:(dy * 2 + dx) * 4 + 3] = w[:, kh, kw, :]
    return out


def stem_unpack(gs, prior=None):
    """gs [Co][4][4][16] -> g [Co][7][7][3]: the adjoint of stem_pack (+ prior when accumulating)."""
    Co = gs.shape[0]
    g = torch.zeros(Co, 7, 7, 3, dtype=gs.dtype)
    for kh in range(7):
        for kw in range(7):
            th, dy, tw, dx = (kh + 1) // 2, (kh + 1) % 2, (kw + 1) // 2, (kw + 1) % 2
            g[:, kh, kw, :] = gs[:, th, tw, (dy * 2 + dx) * 4:(dy * 2 + dx) * 4 + 3]
    return g if prior is None else g + prior


# ================================================================ C. pw21
HW_GEOM = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 100: (10, 10), 120: (10, 12), 192: (12, 16), 255: (15, 17), 256: (16, 16),
           257: (1, 257), 4096: (64, 64)}
PW_K = [1, 21, 32]
PW_HW = [1, 63, 64, 65, 100]
PW_N = [1, 2, 3]
PW_EDGE_HW = [1, 63, 64, 65]                    # one pixel, a ragged tile, a whole tile, a tile and one pixel


def pw_c(dt, *more):
    return [PER[dt], 24, 256] + list(more)


# (dtype, C, K): every H*W of PW_HW and N of PW_N runs inside one test
C2K_CASES = [(dt, C, K) for dt in DTS for C in pw_c(dt) + ([512] if dt == 'bf16' else []) for K in PW_K]   # C = 512: 107 KB of LDS
K2C_CASES = [(dt, C, K) for dt in DTS for C in pw_c(dt, 264) for K in PW_K]
K2C_MODES = [(b, r, s) for b in (False, True) for r in (False, True) for s in (None, 0.5, 1.0)]       # bias, residual, scale_dev
K2C_STATS_CASES = [(dt, C, N) for dt in DTS for C in (24, 264) for N in PW_N]                      # H*W = 100, K = 21
WGRAD_CASES = [(dt, C, K, N, HW) for dt in DTS for C in pw_c(dt, 264) for K in PW_K for N in PW_N for HW in (64, 192)] + \
              [(dt, PER[dt], 21, 9, 4096) for dt in DTS]          # 36 864 pixels: 288 slices of two 64-pixel groups
ROWSUM_CASES = [(N, K, HW) for N in PW_N for K in (1, 21, 65) for HW in (1, 255, 256, 257, 4096)]


def pw_case(dt, N, C, K, HW):
    """Operands of one shape, all float64: x / res [N][C][H][W] features, y [N][K][H][W] heat maps, wkc [K][C] and wck [C][K]
    weights (independent), bias_k [K], bias_c [C]."""
    H, W = HW_GEOM[HW]
    rng = _rng('pw', dt, N, C, K, HW)
    y = rng.integers(-4, 5, size=(N, K, HW))
    wck = rng.integers(-4, 5, size=(C, K))
    s = rng.integers(0, 2, size=K) * 2 - 1
    hot_p = rng.random((N, HW)) < 0.125
    hot_p[0, 0] = True
    hot_c = rng.random(C) < 0.25
    hot_c[0] = True
    a = rng.choice(np.array([-4, -3, -2, 2, 3, 4]), size=(N, HW))
    b = rng.choice(np.array([-4, -3, 3, 4]), size=C)
    y = np.where(hot_p[:, None, :], a[:, None, :] * s[None, :, None], y)
    wck = np.where(hot_c[:, None], b[:, None] * s[None, :], wck)
    return dict(dt=dt, N=N, C=C, K=K, HW=HW, H=H, W=W,
                x=_t(rng.integers(-8, 9, size=(N, C, H, W))), res=_t(rng.integers(-8, 9, size=(N, C, H, W))),
                y=_t(y.reshape(N, K, H, W)), wck=_t(wck), wkc=_t(rng.integers(-4, 5, size=(K, C))),
                bias_k=_t(rng.integers(-8, 9, size=K)), bias_c=_t(rng.integers(-8, 9, size=C)),
                prior_w=_t(rng.integers(-8, 9, size=(K, C))))


def pw_c2k(x, wkc, bias=None):
    """y[n][k][p] = bias[k] + sum_c x[n][c][p] * w[k][c]"""
    y = torch.einsum('nchw,kc->nkhw', x, wkc)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def pw_k2c(y, wck, bias=None, res=None, scale=None):
    """out[n][c][p] = (bias[c] + sum_k y[n][k][p] * w[c][k] + residual) * scale"""
    o = torch.einsum('nkhw,ck->nchw', y, wck)
    if bias is not None:
        o = o + bias.view(1, -1, 1, 1)
    if res is not None:
        o = o + res
    return o if scale is None else o * scale


def pw_wgrad(x, y, prior=None):
    """dw[k][c] = sum over images and pixels of y[n][k][p] * x[n][c][p] (+ prior)"""
    d = torch.einsum('nkhw,nchw->kc', y, x)
    return d if prior is None else d + prior


def hm_rowsum(y, prior=None):
    s = y.sum(dim=(0, 2, 3))
    return s if prior is None else s + prior


def slice_stats(out, HW):
    """Per 64-pixel slice of each image (the last one ragged) and channel: count, mean and M2 of the STORED values.
    out: logical [N][C][H][W] float64 -> [N * ceil(HW / 64)][C][3]."""
    N, C = out.shape[:2]
    rows = out.reshape(N, C, HW)
    st = []
    for n in range(N):
        for p0 in range(0, HW, 64):
            s = rows[n, :, p0:p0 + 64]
            m = s.mean(1)
            st.append(torch.stack([torch.full_like(m, s.shape[1]), m, ((s - m[:, None]) ** 2).sum(1)], 1))
    return torch.stack(st)


def check_exact_pw(c):
    """Range condition of everything the pw21 tests compute from one shape's operands."""
    dt = c['dt']
    for k in ('x', 'res'):
        _is_dt(k, c[k], dt)
    for k in ('y', 'wck', 'wkc', 'bias_k', 'bias_c', 'prior_w'):
        _f32_exact(k, c[k])
    x, y = c['x'], c['y']
    # C -> K: sum_c |x| |w| + |bias|
    assert float((pw_c2k(x.abs(), c['wkc'].abs(), c['bias_k'].abs())).max()) < F32_EXACT
    assert float((pw_c2k(x.abs(), c['wck'].t().abs(), c['bias_k'].abs())).max()) < F32_EXACT
    # K -> C: sum_k |y| |w| + |bias| + |res| (scale <= 1 is a power of two: the product is exact)
    for w in (c['wck'], c['wkc'].t()):
        assert float(pw_k2c(y.abs(), w.abs(), c['bias_c'].abs(), c['res'].abs()).max()) < F32_EXACT
        for b, r, s in K2C_MODES:
            _f32_exact('pw_k2c', pw_k2c(y, w, c['bias_c'] if b else None, c['res'] if r else None, s))
    # weight gradient and row sum: sums over all pixels, with the prior
    assert float(pw_wgrad(x.abs(), y.abs(), c['prior_w'].abs()).max()) < F32_EXACT
    assert float(hm_rowsum(y.abs(), c['bias_k'].abs()).max()) < F32_EXACT
    _f32_exact('pw_c2k', pw_c2k(x, c['wkc'], c['bias_k']))
    _f32_exact('pw_wgrad', pw_wgrad(x, y, c['prior_w']))
    full = pw_k2c(y, c['wck'], c['bias_c'], c['res'], 0.5)
    return ties(full, dt) + ties(pw_k2c(y, c['wck'], c['bias_c'], c['res']), dt)


def needs_tie(dt, N, C, K, HW):
    """bf16 cases with K >= 21 and enough outputs (an eighth of the pixels times a quarter of the channels is hot) must hold at
    least one exact tie; with K = 1 the result stays below 32 in steps of 0.5: every value is a bf16 value and there is nothing
    to round."""
    return dt == 'bf16' and K >= 21 and N * HW * C >= 4096


def rowsum_case(N, K, HW):
    H, W = HW_GEOM[HW]
    rng = _rng('rowsum', N, K, HW)
    return dict(y=_t(rng.integers(-4, 5, size=(N, K, H, W))), prior=_t(rng.integers(-8, 9, size=K)))


def check_exact_rowsum(c):
    _f32_exact('y', c['y'])
    assert float(hm_rowsum(c['y'].abs(), c['prior'].abs()).max()) < F32_EXACT
    _f32_exact('rowsum', hm_rowsum(c['y'], c['prior']))


# ================================================================ D. optimiser
SGD_N = [1, 3, 4, 5, 6, 1023, 1024, 1025, 4195507]   # n % 4 = 0, 1, 2, 3; the last: one full lap of 4096 * 256 float4, 300 float4 of the second, a tail of 3
SGD_LRS = [2.0 ** -3, 2.0 ** -4, 2.0 ** -3]
SGD_MU = 0.5
SGD_CASES = [(n, nesterov, wd) for n in SGD_N for nesterov in (True, False) for wd in (0.25, 0.0)]
CAST_N = [1, 255, 256, 257, 1048653]           # the last: one lap of 4096 * 256 elements and 77 of the second


def sgd_case(n):
    rng = _rng('sgd', n)
    return dict(n=n, p=_t(rng.integers(-16, 17, size=n, dtype=np.int8)) * 4,
                g=[_t(rng.integers(-8, 9, size=n, dtype=np.int8)) for _ in SGD_LRS])


def sgd_steps(p, gs, lrs, mu, wd, nesterov, trace=None):
    """torch.optim.SGD's definition: d = g + wd p; buf = mu buf + d (buf starts at 0); p -= lr (d + mu buf  |  buf)."""
    buf = torch.zeros_like(p)
    for g, lr in zip(gs, lrs):
        d = g + wd * p
        mb = mu * buf
        buf = mb + d
        step = d + mu * buf if nesterov else buf
        if trace is not None:
            trace.append({'wd*p': wd * p, 'd': d, 'mu*buf(old)': mb, 'buf': buf, 'mu*buf': mu * buf, 'd+mu*buf': d + mu * buf,
                          'lr*buf': lr * buf, 'lr*(d+mu*buf)': lr * (d + mu * buf), 'p': p - lr * step})
        p = p - lr * step
    return p, buf


def check_exact_sgd(c, nesterov, wd):
    _f32_exact('p', c['p'])
    for g in c['g']:
        _f32_exact('g', g)
    for v in (SGD_MU, wd) + tuple(SGD_LRS):
        assert float(np.float32(v)) == v
    trace = []
    p, buf = sgd_steps(c['p'], c['g'], SGD_LRS, SGD_MU, wd, nesterov, trace)
    for i, t in enumerate(trace):
        for k, v in t.items():
            _f32_exact('step %d %s' % (i, k), v)
    if c['n'] >= 1023:          # the low-precision copy is a real rounding test: most of p is no bf16 value
        assert float((rne(p, 'bf16') != p).double().mean()) > (2.0 / 3.0 if wd else 1.0 / 3.0)
    return p, buf


def cast_values(n):
    return layout_values('cast', n)
