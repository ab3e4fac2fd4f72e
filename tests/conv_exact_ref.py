"""Exact-operand reference for the convolution kernels.

Operands are small integers chosen so that every product and every partial sum is an integer fp32 holds exactly and the
final value is one bf16 holds exactly: a correct kernel then returns the float64 result BIT FOR BIT, whatever its tile
shape, summation order, split-K, slab reduction or number of roundings.  The tolerance of every comparison built on this
module is zero, and it is derived (range condition below), not measured.

Generator: activations and gradients uniform in {-2..2}; weights +-1 kept with probability q = min(1, 300 / K), K the
longer of the two contracted lengths a weight tensor serves (Ci*kh*kw forward, Co*kh*kw input gradient).  A sum of K*q
products of variance 2 has a standard deviation of about 24.5, so |y| stays near 120 over a million outputs: below bf16's
exact-integer limit of 256 with room for an integer bias (|b| <= 8), a residual / accumulated tensor (|r| <= 16) and a
power-of-two scale.  The same integers are exact in e4m3 (integers to 15) and e5m2 (to 8).

The float64 reference is a plain tap loop over NHWC matrices (one matmul per tap); test_conv_exact_cpu.py holds it against
torch.nn.functional.conv2d / torch.nn.grad in float64.
"""
import zlib

import numpy as np
import torch

BF16_EXACT = 256.0           # every integer of magnitude <= 256 is a bf16 value
F32_EXACT = float(1 << 24)   # every integer of magnitude < 2^24 is an fp32 value


def density(K):
    return min(1.0, 300.0 / K)


def ints(seed, *shape, lo=-2, hi=2):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def weights(seed, Co, Ci, kh, kw, q=None):
    """+-1 with probability q (default: from the longer contracted length), 0 otherwise; NCHW-style [Co][Ci][kh][kw] fp32."""
    rng = np.random.default_rng(seed)
    q = density(max(Ci, Co) * kh * kw) if q is None else q
    sign = rng.integers(0, 2, size=(Co, Ci, kh, kw)) * 2 - 1
    keep = rng.random((Co, Ci, kh, kw)) < q
    return torch.from_numpy((sign * keep).astype(np.float32))


def mask_bytes(seed, n):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(n,)).astype(np.uint8))


def mask_bits(mask, N, C, H, W, per):
    """The accumulate mask of mi355_conv_dgrad_masked_acc as a 0/1 NCHW tensor: bit e of byte i belongs to NHWC element i*per + e."""
    bits = (mask.view(-1, 1).to(torch.int32) >> torch.arange(per, dtype=torch.int32).view(1, per)) & 1
    return bits.view(N, H, W, C).permute(0, 3, 1, 2).double()


def out_size(H, W, kh, kw, stride, pad):
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def _padded_nhwc(x, pad):
    N, C, H, W = x.shape
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x.double().permute(0, 2, 3, 1)
    return xp


def conv_fwd(x, w, stride, pad, out_hw=None):
    """float64 y[N][Co][Ho][Wo] of x[N][Ci][H][W] * w[Co][Ci][kh][kw]; out_hw = the top-left crop of a unit-stride conv."""
    N, Ci, H, W = x.shape
    Co, _, kh, kw = w.shape
    Ho, Wo = out_hw if out_hw is not None else out_size(H, W, kh, kw, stride, pad)
    xp, wd = _padded_nhwc(x, pad), w.double()
    y = torch.zeros(N * Ho * Wo, Co, dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride]
            y += xs.reshape(N * Ho * Wo, Ci) @ wd[:, :, i, j].t()
    return y.view(N, Ho, Wo, Co).permute(0, 3, 1, 2).contiguous()


def conv_dgrad(dy, w, stride, pad, in_hw):
    """float64 dx[N][Ci][H][W]: every dy pixel scattered through every tap (all strides, phases of any size)."""
    N, Co, Ho, Wo = dy.shape
    _, Ci, kh, kw = w.shape
    H, W = in_hw
    dyf, wd = dy.double().permute(0, 2, 3, 1).reshape(N * Ho * Wo, Co), w.double()
    Hp, Wp = max(H + 2 * pad, stride * (Ho - 1) + kh), max(W + 2 * pad, stride * (Wo - 1) + kw)
    dxp = torch.zeros(N, Hp, Wp, Ci, dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            dxp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride] += (dyf @ wd[:, :, i, j]).view(N, Ho, Wo, Ci)
    return dxp[:, pad:pad + H, pad:pad + W].permute(0, 3, 1, 2).contiguous()


def conv_wgrad(x, dy, kh, kw, stride, pad):
    """float64 dw[Co][Ci][kh][kw]; the output size (cropped or not) is dy's."""
    N, Ci, H, W = x.shape
    _, Co, Ho, Wo = dy.shape
    xp = _padded_nhwc(x, pad)
    dyf = dy.double().permute(0, 2, 3, 1).reshape(N * Ho * Wo, Co)
    dw = torch.zeros(Co, Ci, kh, kw, dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride]
            dw[:, :, i, j] = dyf.t() @ xs.reshape(N * Ho * Wo, Ci)
    return dw


def fwd_epilogue(y, bias=None, residual=None, relu=False):
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    return y.clamp_min(0.0) if relu else y


def dgrad_epilogue(dx, scale=1.0, base=None, bits=None):
    """dx * scale (+ base, or + base where the mask bit is set)."""
    out = dx * scale
    if base is not None:
        out = out + (base.double() if bits is None else base.double() * bits)
    return out


def cat_fwd(x, w, x2, w2, stride, pad):
    """concat-K forward: conv(x, w) + the 1x1 conv of x2 (at the output resolution) with w2[Co][c2]."""
    return conv_fwd(x, w, stride, pad) + conv_fwd(x2, w2.view(w2.shape[0], w2.shape[1], 1, 1), 1, 0)


def bn_stats(y):
    """Per-channel (n, mean, M2) of an NCHW tensor in float64."""
    C = y.shape[1]
    v = y.double().permute(1, 0, 2, 3).reshape(C, -1)
    mean = v.mean(1)
    return float(v.shape[1]), mean, ((v - mean[:, None]) ** 2).sum(1)


def fold_stats(partial, nslices, C):
    """The kernels' per-slice (n, mean, M2) records combined in float64 -> (n[C], mean[C], M2[C])."""
    pr = partial[:nslices * C * 3].detach().cpu().double().view(nslices, C, 3)
    n, mean, m2 = pr[..., 0], pr[..., 1], pr[..., 2]
    tot = n.sum(0)
    gm = (n * mean).sum(0) / tot
    return tot, gm, (m2 + n * (mean - gm) ** 2).sum(0)


def assert_exact_in(dtype, *values):
    """The range condition, asserted on the REFERENCE before any kernel result is looked at: every value (results, and the
    value before an addend is added) is one the result format holds exactly."""
    for v in values:
        v = v.double()
        if dtype == torch.bfloat16:
            assert float(v.abs().max()) <= BF16_EXACT, 'bf16 range condition: max |value| = %g' % float(v.abs().max())
            assert torch.equal(v.float().to(torch.bfloat16).double(), v), 'bf16 range condition: a value is not a bf16 number'
        else:
            assert float(v.abs().max()) < F32_EXACT, 'fp32 range condition: max |value| = %g' % float(v.abs().max())
            assert torch.equal(v.float().double(), v)


def to_dtype(ref, dtype):
    """float64 -> fp32 -> dtype: the expected bits (exact under the range condition; round to nearest even beyond it)."""
    return ref.float().to(dtype)


def same_bits(got, ref, dtype):
    """got (any device / memory layout, logical NCHW or flat) against the float64 reference: every bit, so -0.0 and NaN count."""
    g = got.detach().cpu().contiguous()
    e = to_dtype(ref, dtype).contiguous()
    if g.dtype != dtype or g.shape != e.shape:
        return False
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    return torch.equal(g.view(iv), e.view(iv))


def first_mismatch(got, ref, dtype):
    g = got.detach().cpu().contiguous().double()
    e = to_dtype(ref, dtype).double()
    bad = (g != e).nonzero()
    if bad.numel() == 0:
        return 'values equal (sign of zero or NaN differs)'
    idx = tuple(int(i) for i in bad[0])
    return '%d of %d elements differ; first at %s: got %r, expected %r' % (bad.shape[0], e.numel(), idx, float(g[idx]), float(e[idx]))


def window_products(x, w, stride, pad, n, o, oy, ox):
    """The K products x*w that make up the single output element (n, o, oy, ox), in [kh][kw][Ci] order (float64)."""
    Co, Ci, kh, kw = w.shape
    xp = _padded_nhwc(x, pad)
    win = xp[n, oy * stride:oy * stride + kh, ox * stride:ox * stride + kw, :]
    return (win * w.double()[o].permute(1, 2, 0)).reshape(-1)


def drop_one_product(y, x, w, stride, pad, n, o, oy, ox, k):
    """y with product k (window_products order) removed from the single output element (n, o, oy, ox): the smallest error a
    kernel can make.  Returns (mutated y, removed value)."""
    prod = window_products(x, w, stride, pad, n, o, oy, ox)
    out = y.clone()
    out[n, o, oy, ox] -= prod[k]
    return out, float(prod[k])


def seed_of(name):
    """A seed that depends on the case's name alone: adding or renaming a case leaves every other case's operands as they were."""
    return zlib.crc32(name.encode()) % (1 << 30)


# ---------------------------------------------------------------------------------------------- cases of the GPU module
# name: (group, N, Ci, H, W, Co, k, stride, pad, out_hw, dgrad).  group = the environment the case runs under
# (test_gpu_conv_exact.GROUPS); out_hw = cropped output; dgrad False where the library has no input gradient for the shape
# (contracted channel count not a power-of-two number of 16-byte chunks, or a cropped output).
CASES = {
    # small-channel tile: the 7x7 stem over the channel-padded image and the folded 4x4 stem (cropped), ragged M, Co = 72
    'small7':        ('default', 3, 8, 20, 36, 64, 7, 2, 3, None, True),
    'small7_co72':   ('default', 3, 8, 20, 36, 72, 7, 2, 3, None, False),
    'stem4_crop':    ('default', 3, 16, 10, 18, 64, 4, 1, 2, (10, 18), False),
    'small_dgrad':   ('default', 3, 64, 9, 13, 16, 3, 1, 1, None, True),           # 16 contracted channels in the input gradient
    # 64 x 64
    't64_co72':      ('default', 1, 64, 9, 13, 72, 3, 1, 1, None, False),
    't64_s2':        ('default', 5, 128, 12, 12, 64, 3, 2, 1, None, True),
    # 64 x 128 through the row-count rule (18000 rows: the last of 282 row tiles holds 16)
    't64x128':       ('default', 5, 64, 60, 60, 256, 1, 1, 0, None, True),
    't64x128_co136': ('default', 5, 64, 60, 60, 136, 1, 1, 0, None, False),      # 8 live columns in the second column tile
    't64x128_dgrad': ('default', 5, 256, 60, 60, 64, 1, 1, 0, None, True),      # the same build (and its BatchNorm-backward epilogue) from the input-gradient side
    # 128 x 64: 512 row tiles, the last one half full; width 62 keeps the shared-A-tile kernel away
    't128x64':       ('default', 16, 64, 66, 62, 64, 3, 1, 1, None, True),
    # 128 x 128 register-staged: 524 tiles, K = 576, Co = 136 (8 live columns in the second column tile)
    't128x128':      ('default', 9, 64, 62, 60, 136, 3, 1, 1, None, False),
    't128x128_dgrad': ('default', 16, 128, 66, 62, 64, 3, 1, 1, None, True),     # the same build from the input-gradient side (512 tiles)
    't128x128_f32_dgrad': ('default', 16, 128, 66, 62, 32, 3, 1, 1, None, True),  # fp32: K short enough for the register-staged build (+ its BatchNorm-backward epilogue)
    # two K groups per workgroup: 64-row tiles (128 tiles) and 128-row tiles (210 tiles), both with a partial last row tile
    'kg2_64':        ('default', 15, 128, 17, 16, 256, 3, 1, 1, None, True),
    'kg2_128':       ('default', 49, 128, 17, 16, 256, 3, 1, 1, None, True),
    'kg2_64_co136':  ('default', 15, 128, 17, 16, 136, 3, 1, 1, None, False),
    'kg2_128_co136': ('default', 49, 128, 17, 16, 136, 3, 1, 1, None, False),
    # one 256 x 256 tile per CU by shape: 49 x 4 tiles, the last row tile three quarters full
    't256d':         ('default', 13, 256, 32, 30, 1024, 1, 1, 0, None, True),
    # strided input gradients with odd extents: phases of unequal tile count, 3x3 and 4x4
    's2_3x3_odd':    ('default', 2, 64, 15, 17, 128, 3, 2, 1, None, True),
    's2_4x4_odd':    ('default', 2, 64, 15, 17, 64, 4, 2, 1, None, True),
    # weight-gradient kernels by shape: kw (3x3 / stride 1, every width 8 .. 128), kw2 (3x3 and 4x4 / stride 2, Wo 8 .. 64),
    # Co = 64 (one row tile of accumulators) and 128, slab-reduced and direct (one K step: M <= 64)
    'wkw_w8':        ('default', 3, 64, 8, 8, 128, 3, 1, 1, None, True),
    'wkw_w16':       ('default', 2, 64, 5, 16, 64, 3, 1, 1, None, True),
    'wkw_w32':       ('default', 1, 128, 6, 32, 256, 3, 1, 1, None, True),
    'wkw_w64':       ('default', 1, 64, 5, 64, 128, 3, 1, 1, None, True),
    'wkw_w128':      ('default', 1, 64, 3, 128, 64, 3, 1, 1, None, True),
    'wkw_direct':    ('default', 1, 64, 8, 8, 128, 3, 1, 1, None, True),
    'wkw2_wo8':      ('default', 2, 64, 10, 16, 128, 3, 2, 1, None, True),
    'wkw2_wo16':     ('default', 1, 64, 12, 32, 128, 4, 2, 1, None, True),       # 4x4 with two row tiles of accumulators
    'wkw2_wo32':     ('default', 1, 64, 6, 64, 128, 3, 2, 1, None, True),
    'wkw2_wo64':     ('default', 1, 64, 4, 128, 64, 4, 2, 1, None, True),
    'wkw2_direct':   ('default', 1, 64, 16, 16, 64, 3, 2, 1, None, True),
    'wgen_direct':   ('default', 1, 64, 5, 7, 72, 3, 1, 1, None, False),
    # the one full-size case: 4096 tiles of 128 x 128 select the 256 x 128 macro tile of the shared-A-tile kernel (no switch
    # reaches it); its input gradient (64 output columns, 2048 row tiles) is the shared-A-tile kernel's 128 x 64 build by shape
    'kw3_256x128':   ('default', 64, 64, 64, 64, 256, 3, 1, 1, None, True),
    # forced LDS-DMA ring and shared-A-tile builds on small maps, strided input gradients one launch per phase
    'dma_co136':     ('dma_kw3', 2, 64, 9, 13, 136, 3, 1, 1, None, False),
    'dma_s2':        ('dma_kw3', 3, 128, 12, 12, 128, 3, 2, 1, None, True),
    'dma_s2_4x4':    ('dma_kw3', 2, 128, 15, 17, 128, 4, 2, 1, None, True),
    'kw3_w8':        ('dma_kw3', 3, 64, 5, 8, 128, 3, 1, 1, None, True),
    'kw3_w16_co136': ('dma_kw3', 1, 128, 6, 16, 136, 3, 1, 1, None, False),
    'kw3_w32':       ('dma_kw3', 1, 64, 3, 32, 64, 3, 1, 1, None, True),
    'kw3_w64':       ('dma_kw3', 1, 64, 3, 64, 128, 3, 1, 1, None, True),
    'kw3_w128':      ('dma_kw3', 1, 128, 3, 128, 64, 3, 1, 1, None, True),
    'phase_s2_odd':  ('dma_kw3', 2, 64, 15, 17, 64, 3, 2, 1, None, True),
    # forced 256 x 256 LDS-DMA tiles: Co = 256 and 512, M = 300 (one full and one partial row tile), 4-phase input gradient
    't256d_m300':    ('t256d', 3, 64, 10, 10, 256, 3, 1, 1, None, True),
    't256d_co512':   ('t256d', 3, 64, 10, 10, 512, 1, 1, 0, None, True),
    't256d_s2':      ('t256d', 2, 256, 15, 17, 64, 4, 2, 1, None, True),
}

# concat-K forward: name: (group, N, Ci, H, W, Co, k, stride, pad); every case runs both second-operand widths of CAT_C2
CAT_CASES = {
    'cat_64x64':     ('default', 3, 64, 9, 13, 64, 3, 1, 1),
    'cat_64x64_s2':  ('default', 2, 64, 15, 17, 136, 3, 2, 1),
    'cat_64x128':    ('default', 5, 64, 60, 60, 256, 1, 1, 0),
    'cat_128x128':   ('default', 9, 512, 62, 60, 256, 1, 1, 0),
    'cat_dma':       ('dma_kw3', 2, 64, 9, 13, 136, 3, 1, 1),
    'cat_256x256':   ('t256d', 3, 64, 10, 10, 256, 3, 1, 1),
}
CAT_C2 = {torch.bfloat16: (8, 24), torch.float32: (4, 12)}      # one 16-byte chunk and three, per format

# fp8 / MX operands: name: (group, N, Ci, H, W, Co, k, stride, pad)
FP8_CASES = {
    'f8_3x3_w8':     ('default', 3, 128, 5, 8, 128, 3, 1, 1),
    'f8_3x3_w16':    ('default', 2, 256, 6, 16, 256, 3, 1, 1),
    'f8_s2_3x3':     ('default', 2, 128, 16, 16, 256, 3, 2, 1),
    'f8_s2_4x4':     ('default', 2, 256, 16, 32, 128, 4, 2, 1),
    'f8_64x128':     ('default', 31, 128, 17, 16, 256, 3, 1, 1),
    'f8_t128_w8':    ('fp8_tile0', 3, 128, 5, 8, 128, 3, 1, 1),
    'f8_t128_s2':    ('fp8_tile0', 2, 256, 16, 32, 256, 4, 2, 1),
    'f8_t64x128_w8': ('fp8_tile1', 3, 128, 5, 8, 128, 3, 1, 1),
    'f8_t64x128_s2': ('fp8_tile1', 2, 256, 16, 32, 256, 4, 2, 1),
}


class Case(object):
    pass


_cache = {}


def build_case(name):
    """Operands and float64 references of CASES[name], computed once per process and shared (never modified) by the tests."""
    if name in _cache:
        return _cache[name]
    group, N, Ci, H, W, Co, k, s, p, out_hw, dgrad = CASES[name]
    c = Case()
    c.name, c.group, c.shape, c.out_hw, c.has_dgrad = name, group, (N, Ci, H, W, Co, k, s, p), out_hw, dgrad
    seed = seed_of(name)
    Ho, Wo = out_hw if out_hw is not None else out_size(H, W, k, k, s, p)
    c.Ho, c.Wo = Ho, Wo
    c.x = ints(seed, N, Ci, H, W)
    c.w = weights(seed + 1, Co, Ci, k, k)
    c.bias = ints(seed + 2, Co, lo=-8, hi=8)
    c.res = ints(seed + 3, N, Co, Ho, Wo, lo=-16, hi=16)
    c.dy = ints(seed + 4, N, Co, Ho, Wo)
    c.base = ints(seed + 5, N, Ci, H, W, lo=-16, hi=16)
    c.dw0 = ints(seed + 6, Co, k, k, Ci, lo=-16, hi=16)
    c.bias_i = ints(seed + 8, Ci, lo=-8, hi=8)
    c.mask = {per: mask_bytes(seed + 7, N * H * W * Ci // per) for per in (4, 8)}
    c.y = conv_fwd(c.x, c.w, s, p, out_hw)
    c.y_b = fwd_epilogue(c.y, c.bias)
    c.y_br = fwd_epilogue(c.y, c.bias, c.res)
    c.y_brr = fwd_epilogue(c.y, c.bias, c.res, relu=True)
    c.fwd_values = (c.y, c.y_b, c.y_br, c.y_brr)
    c.dgrad_values = ()
    if dgrad:
        c.dx = conv_dgrad(c.dy, c.w, s, p, (H, W))
        c.dx_q = dgrad_epilogue(c.dx, 0.25)
        c.dx_acc = dgrad_epilogue(c.dx, 0.25, c.base)
        c.dx_macc = {per: dgrad_epilogue(c.dx, 1.0, c.base, mask_bits(c.mask[per], N, Ci, H, W, per)) for per in (4, 8)}
        c.dx_b = fwd_epilogue(c.dx, c.bias_i)
        c.dx_br = fwd_epilogue(c.dx, c.bias_i, relu=True)          # the inference form of a transposed conv
        c.dgrad_values = (c.dx, c.dx_q, c.dx_acc, c.dx_macc[4], c.dx_macc[8], c.dx_b, c.dx_br)
    c.dw = conv_wgrad(c.x, c.dy, k, k, s, p).permute(0, 2, 3, 1).contiguous()          # [Co][kh][kw][Ci], the library's order
    c.dw_acc = c.dw + c.dw0.double()
    _cache[name] = c
    return c


def assert_case_in_range(c):
    """The range condition of one case for both result formats (bf16 is the stricter one for the activations)."""
    for dtype in (torch.bfloat16, torch.float32):
        assert_exact_in(dtype, *c.fwd_values)
        assert_exact_in(dtype, *c.dgrad_values)
    assert_exact_in(torch.float32, c.dw, c.dw_acc)


def build_cat_case(name):
    """x2 / w2 / y / y_b are dicts keyed by the second operand's channel count (all four of CAT_C2)."""
    if name in _cache:
        return _cache[name]
    group, N, Ci, H, W, Co, k, s, p = CAT_CASES[name]
    c = Case()
    c.name, c.group, c.shape = name, group, (N, Ci, H, W, Co, k, s, p)
    seed = seed_of(name)
    c.Ho, c.Wo = out_size(H, W, k, k, s, p)
    c.x = ints(seed, N, Ci, H, W)
    c.w = weights(seed + 1, Co, Ci, k, k)
    c.b1, c.b2 = ints(seed + 2, Co, lo=-4, hi=4), ints(seed + 3, Co, lo=-4, hi=4)
    widths = sorted(set(n2 for v in CAT_C2.values() for n2 in v))
    c.x2 = {n2: ints(seed + 4 + n2, N, n2, c.Ho, c.Wo) for n2 in widths}
    c.w2 = {n2: weights(seed + 40 + n2, Co, n2, 1, 1, q=1.0).view(Co, n2) for n2 in widths}
    y1 = conv_fwd(c.x, c.w, s, p)
    c.y = {n2: y1 + conv_fwd(c.x2[n2], c.w2[n2].view(Co, n2, 1, 1), 1, 0) for n2 in widths}
    c.y_b = {n2: fwd_epilogue(c.y[n2], c.b1 + c.b2) for n2 in widths}
    _cache[name] = c
    return c


def build_fp8_case(name):
    if name in _cache:
        return _cache[name]
    group, N, Ci, H, W, Co, k, s, p = FP8_CASES[name]
    c = Case()
    c.name, c.group, c.shape = name, group, (N, Ci, H, W, Co, k, s, p)
    seed = seed_of(name)
    c.Ho, c.Wo = out_size(H, W, k, k, s, p)
    c.x = ints(seed, N, Ci, H, W)
    c.w = weights(seed + 1, Co, Ci, k, k)
    c.bias = ints(seed + 2, Co, lo=-8, hi=8)
    c.dy = ints(seed + 4, N, Co, c.Ho, c.Wo)
    c.base = ints(seed + 5, N, Ci, H, W, lo=-16, hi=16)
    c.dw0 = ints(seed + 6, Co, k, k, Ci, lo=-16, hi=16)
    c.y = conv_fwd(c.x, c.w, s, p)
    c.y_b = fwd_epilogue(c.y, c.bias)
    c.dx = conv_dgrad(c.dy, c.w, s, p, (H, W))
    c.dx_q = dgrad_epilogue(c.dx, 0.25)
    c.dx_acc = dgrad_epilogue(c.dx, 0.25, c.base)
    c.dw = conv_wgrad(c.x, c.dy, k, k, s, p).permute(0, 2, 3, 1).contiguous()
    c.dw_acc = c.dw + c.dw0.double()
    _cache[name] = c
    return c


ROUNDING_TAILS = (5, 6, 7, 9, 131, 129, 4, 8)       # sums 252 + tail: 257 258 259 261 383 381 256 260 (and their negatives)


def rounding_case(N=1, H=2, W=4, Co=8):
    """A 1x1 convolution with K = 64 whose exact sums lie just above 256, where bf16 is spaced by 2: ties (257, 259, 261,
    381, 383) and non-ties (258), both signs.  x = (1, 4, 4, ..., 4) per pixel, negated on odd pixels; w[o] = (tail, 1, 1, ...)
    with the tail cycling through ROUNDING_TAILS, so y = +-(252 + tail).  Every operand is a bf16 value.  Returns (x, w, sums)."""
    x = torch.full((N, 64, H, W), 4.0)
    x[:, 0] = 1.0
    sign = torch.ones(N * H * W)
    sign[1::2] = -1.0
    x = x * sign.view(N, 1, H, W)
    w = torch.ones(Co, 64, 1, 1)
    w[:, 0, 0, 0] = torch.tensor([float(ROUNDING_TAILS[o % len(ROUNDING_TAILS)]) for o in range(Co)])
    sums = [sgn * (252 + t) for t in ROUNDING_TAILS[:min(Co, len(ROUNDING_TAILS))] for sgn in (1, -1)]
    return x, w, sums


# rounding shapes: group: [(N, H, W, Co, pgemm mode or None)]: every tile build a 1x1 conv with K = 64 reaches
ROUNDING_CASES = {
    'default': [(1, 2, 4, 8, None), (5, 60, 60, 256, None), (16, 64, 64, 64, 0), (16, 64, 64, 64, None), (8, 64, 64, 256, None)],
    'dma_kw3': [(1, 9, 13, 136, None)],
    't256d':   [(3, 10, 10, 256, None)],
}

# persistent GEMM (mi355_set_pgemm(2), bf16): name: (N, Ci, H, W, Co, dgrad).  351 rows: the last of six row tiles holds 31.
# K = 64 .. 512: every ring depth the defaults choose; above 512 no weight slice fits LDS and the launch stays on the gather kernel.
PGEMM_CASES = {
    'pg_k64':  (3, 64, 9, 13, 256, True),
    'pg_k128': (3, 128, 9, 13, 64, True),
    'pg_k256': (3, 256, 9, 13, 128, True),
    'pg_k512': (3, 512, 9, 13, 128, True),
    'pg_co72': (3, 64, 9, 13, 72, False),
}


# ---------------------------------------------------------------------------------------------- expected builds
# The kernel build every case must run, as the launch-log label names it in brackets ("[g128x128 dma kg2 epi1]", csrc/common.h):
# read from choose_conv / choose_pgemm / choose_fp8 / plan_wgrad (csrc/conv_plan.h).  test_gpu_conv_exact.py asserts them on
# the launches, test_conv_dispatch_cpu.py on the choosers themselves.
# group: the switches its cases run under (read once per process)
GROUPS = {
    'dma_kw3':   {'MI355_DMA': '2', 'MI355_KW3': '2', 'MI355_PHASES': '0'},
    't256d':     {'MI355_T256D_MIN': '1', 'MI355_T256D_KMIN': '1'},
    'fp8_tile0': {'MI355_FP8_TILE': '0'},
    'fp8_tile1': {'MI355_FP8_TILE': '1'},
}

# name: (bf16, f32) x (forward, input gradient, accumulating input gradient, input gradient + BatchNorm-backward epilogue,
# weight gradient with its slab count).  'build *4': four launches (one per phase, MI355_PHASES=0).
EXPECT = {
    'small7':         (('g128x64 small', 'g64x64', 'g64x64', 'g64x64', 'wgrad S9'), ('g128x64 f32 small', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S17')),
    'small7_co72':    (('g128x64 small', None, None, None, 'wgrad S9'), ('g128x64 f32 small', None, None, None, 'wgrad S17')),
    'stem4_crop':     (('g128x64 small', None, None, None, 'wgrad S9'), ('g128x64 f32 small', None, None, None, 'wgrad S17')),
    'small_dgrad':    (('g64x64', 'g128x64 small', 'g128x64 small', 'g128x64 small', 'wgrad S6'), ('g64x64 f32', 'g128x64 f32 small', 'g128x64 f32 small', 'g128x64 f32 small', 'wgrad S11')),
    't64_co72':       (('g64x64', None, None, None, 'wgrad S2'), ('g64x64 f32', None, None, None, 'wgrad S4')),
    't64_s2':         (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad S3'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S6')),
    't64x128':        (('g64x128', 'g64x64', 'g64x64', 'g64x64', 'wgrad S94'), ('g64x128 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S113')),
    't64x128_co136':  (('g64x128', None, None, None, 'wgrad S94'), ('g64x128 f32', None, None, None, 'wgrad S113')),
    't64x128_dgrad':  (('g64x64', 'g64x128', 'g64x128', 'g64x128', 'wgrad S94'), ('g64x64 f32', 'g64x128 f32', 'g64x128 f32', 'g64x128 f32', 'wgrad S113')),
    't128x64':        (('g128x64', 'g128x64', 'g128x64', 'g128x64', 'wgrad S61'), ('g128x64 f32', 'g128x64 f32', 'g128x64 f32', 'g128x64 f32', 'wgrad S121')),
    't128x128':       (('g128x128', None, None, None, 'wgrad S31'), ('g128x128 f32 dma', None, None, None, 'wgrad S62')),
    't128x128_dgrad': (('g128x64', 'g128x128', 'g128x128', 'g128x128', 'wgrad S61'), ('g128x64 f32', 'g128x128 f32 dma', 'g128x128 f32 dma', 'g128x128 f32 dma', 'wgrad S86')),
    't128x128_f32_dgrad': (('g128x64', 'g128x64 small', 'g128x64 small', 'g128x64 small', 'wgrad S61'), ('g128x64 f32', 'g128x128 f32', 'g128x128 f32', 'g128x128 f32', 'wgrad S86')),
    'kg2_64_co136':   (('g64x128 dma kg2', None, None, None, 'wgrad_kw S22'), ('g64x128 f32 dma kg2', None, None, None, 'wgrad S15')),
    'kg2_128_co136':  (('g128x128 dma kg2', None, None, None, 'wgrad_kw S21'), ('g128x128 f32 dma kg2', None, None, None, 'wgrad S25')),
    'kg2_64':         (('g64x128 dma kg2', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S22'), ('g64x128 f32 dma kg2', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S15')),
    'kg2_128':        (('g128x128 dma kg2', 'g64x128 dma kg2', 'g64x128 dma kg2', 'g64x64', 'wgrad_kw S21'), ('g128x128 f32 dma kg2', 'g64x128 f32 dma kg2', 'g64x128 f32 dma kg2', 'g64x64 f32', 'wgrad S25')),
    't256d':          (('g256x256 dma', 'g128x128 dma kg2', 'g128x128 dma kg2', 'g64x64', 'wgrad S15'), ('g128x128 f32', 'g128x128 f32 dma kg2', 'g128x128 f32 dma kg2', 'g64x64 f32', 'wgrad S23')),
    's2_3x3_odd':     (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad S3'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S5')),
    's2_4x4_odd':     (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S4')),
    'wkw_w8':         (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S3'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S6')),
    'wkw_w16':        (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S3'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S5')),
    'wkw_w32':        (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S3'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S6')),
    'wkw_w64':        (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S5'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S10')),
    'wkw_w128':       (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S6'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S12')),
    'wkw_direct':     (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw S1'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S2')),
    'wkw2_wo8':       (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw2 S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S3')),
    'wkw2_wo16':      (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw2 S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S3')),
    'wkw2_wo32':      (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw2 S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S3')),
    'wkw2_wo64':      (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw2 S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S4')),
    'wkw2_direct':    (('g64x64', 'g64x64', 'g64x64', 'g64x64', 'wgrad_kw2 S1'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S2')),
    'wgen_direct':    (('g64x64', None, None, None, 'wgrad S1'), ('g64x64 f32', None, None, None, 'wgrad S2')),
    'kw3_256x128':    (('g256x128 kw3', 'g128x64 kw3', 'g128x64 kw3', 'g128x64', 'wgrad_kw S128'), ('g128x128 f32 dma', 'g128x64 f32', 'g128x64 f32', 'g128x64 f32', 'wgrad S77')),
    'dma_co136':      (('g128x128 dma', None, None, None, 'wgrad S4'), ('g128x128 f32 dma', None, None, None, 'wgrad S8')),
    'dma_s2':         (('g128x128 dma', 'g128x128 dma *4', 'g128x128 dma *4', 'g128x128 dma *4', 'wgrad S2'), ('g128x128 f32 dma', 'g128x128 f32 dma *4', 'g128x128 f32 dma *4', 'g128x128 f32 dma *4', 'wgrad S4')),
    'dma_s2_4x4':     (('g128x128 dma', 'g128x128 dma *4', 'g128x128 dma *4', 'g128x128 dma *4', 'wgrad S2'), ('g128x128 f32 dma', 'g128x128 f32 dma *4', 'g128x128 f32 dma *4', 'g128x128 f32 dma *4', 'wgrad S4')),
    'kw3_w8':         (('g128x128 kw3', 'g128x64 kw3', 'g128x64 kw3', 'g64x64', 'wgrad_kw S2'), ('g128x128 f32 dma', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S4')),
    'kw3_w16_co136':  (('g128x128 kw3', None, None, None, 'wgrad_kw S2'), ('g128x128 f32 dma', None, None, None, 'wgrad S3')),
    'kw3_w32':        (('g128x64 kw3', 'g128x64 kw3', 'g128x64 kw3', 'g64x64', 'wgrad_kw S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S3')),
    'kw3_w64':        (('g128x128 kw3', 'g128x64 kw3', 'g128x64 kw3', 'g64x64', 'wgrad_kw S3'), ('g128x128 f32 dma', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S6')),
    'kw3_w128':       (('g128x64 kw3', 'g128x128 kw3', 'g128x128 kw3', 'g128x128 dma', 'wgrad_kw S6'), ('g64x64 f32', 'g128x128 f32 dma', 'g128x128 f32 dma', 'g128x128 f32 dma', 'wgrad S12')),
    'phase_s2_odd':   (('g64x64', 'g64x64 *4', 'g64x64 *4', 'g64x64 *4', 'wgrad S3'), ('g64x64 f32', 'g64x64 f32 *4', 'g64x64 f32 *4', 'g64x64 f32 *4', 'wgrad S5')),
    't256d_m300':     (('g256x256 dma', 'g64x64', 'g64x64', 'g64x64', 'wgrad S5'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S10')),
    't256d_co512':    (('g256x256 dma', 'g64x64', 'g64x64', 'g64x64', 'wgrad S5'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S10')),
    't256d_s2':       (('g64x64', 'g256x256 dma', 'g64x64', 'g64x64', 'wgrad S2'), ('g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'g64x64 f32', 'wgrad S4')),
}
CAT_EXPECT = {      # name: (bf16, f32)
    'cat_64x64':    ('cat g64x64', 'cat g64x64 f32'),
    'cat_64x64_s2': ('cat g64x64', 'cat g64x64 f32'),
    'cat_64x128':   ('cat g64x128', 'cat g64x128 f32'),
    'cat_128x128':  ('cat g128x128', 'cat g128x128 f32 dma'),
    'cat_dma':      ('cat g128x128 dma', 'cat g128x128 f32 dma'),
    'cat_256x256':  ('cat g256x256 dma', 'cat g64x64 f32'),
}
FP8_EXPECT = {      # name: (forward / input-gradient tile, the same with mi355_set_fp8_kw3(1) or None where the shape has no such build)
    'f8_3x3_w8':   ('g64x64', 'g128x128 kw3'),
    'f8_3x3_w16':  ('g64x64', 'g128x128 kw3'),
    'f8_s2_3x3':   ('g64x64', None),
    'f8_s2_4x4':   ('g64x64', None),
    'f8_64x128':   (('g64x128', 'g64x64'), 'g128x128 kw3'),      # (forward, input gradient: 128 output columns are one column tile)
    'f8_t128_w8':  ('g128x128', 'g128x128 kw3'),
    'f8_t128_s2':  ('g128x128', None),
    'f8_t64x128_w8': ('g64x128', 'g128x128 kw3'),
    'f8_t64x128_s2': ('g64x128', None),
}
ROUNDING_EXPECT = {     # the builds of R.ROUNDING_CASES, in order
    'default': ['g64x64', 'g64x128', 'g128x64', 'pgemm bm64 bn64 ns8', 'pgemm bm64 bn128 ns6'],
    'dma_kw3': ['g128x128 dma'],
    't256d': ['g256x256 dma'],
}
PGEMM_EXPECT = {       # name: (forward builds (plain, addend ring), input-gradient builds (plain, addend ring)) of R.PGEMM_CASES
    'pg_k64':   (('pgemm bm64 bn128 ns6', 'pgemm bm64 bn128 ns4 add'), ('pgemm bm64 bn64 ns5', 'pgemm bm64 bn64 ns8 add')),
    'pg_k128':  (('pgemm bm64 bn64 ns6', 'pgemm bm64 bn64 ns8 add'), ('pgemm bm64 bn128 ns6', 'pgemm bm64 bn128 ns4 add')),
    'pg_k256':  (('pgemm bm64 bn128 ns8', 'pgemm bm64 bn128 ns4 add'), ('pgemm bm64 bn128 ns4', 'pgemm bm64 bn128 ns5 add')),
    'pg_k512':  (('pgemm bm64 bn64 ns8', 'pgemm bm64 bn64 ns8 add'), ('pgemm bm64 bn128 ns4', 'pgemm bm64 bn128 ns5 add')),
    'pg_co72':  (('pgemm bm64 bn128 ns6', 'pgemm bm64 bn128 ns4 add'), None),
}


def build_pgemm_case(name):
    if name in _cache:
        return _cache[name]
    N, Ci, H, W, Co, dgrad = PGEMM_CASES[name]
    c = Case()
    c.name, c.shape, c.has_dgrad = name, (N, Ci, H, W, Co), dgrad
    seed = seed_of(name)
    c.x, c.w = ints(seed, N, Ci, H, W), weights(seed + 1, Co, Ci, 1, 1)
    c.bias, c.res = ints(seed + 2, Co, lo=-8, hi=8), ints(seed + 3, N, Co, H, W, lo=-16, hi=16)
    c.y = conv_fwd(c.x, c.w, 1, 0)
    c.y_b, c.y_br, c.y_brr = fwd_epilogue(c.y, c.bias), fwd_epilogue(c.y, c.bias, c.res), fwd_epilogue(c.y, c.bias, c.res, relu=True)
    c.values = [c.y, c.y_b, c.y_br, c.y_brr]
    if dgrad:
        c.dy, c.base = ints(seed + 4, N, Co, H, W), ints(seed + 5, N, Ci, H, W, lo=-16, hi=16)
        c.mask = mask_bytes(seed + 7, N * H * W * Ci // 8)
        c.dx = conv_dgrad(c.dy, c.w, 1, 0, (H, W))
        c.dx_q = dgrad_epilogue(c.dx, 0.25)
        c.dx_acc = dgrad_epilogue(c.dx, 0.25, c.base)
        c.dx_macc = dgrad_epilogue(c.dx, 1.0, c.base, mask_bits(c.mask, N, Ci, H, W, 8))
        c.values += [c.dx, c.dx_q, c.dx_acc, c.dx_macc]
    _cache[name] = c
    return c


# 21-channel heat-map conv (128 x 32 tile, NCHW fp32 output): (N, C, K, H, W); HW = 120 and 4096
HM_CASES = {'hm_120': (3, 64, 21, 10, 12), 'hm_4096': (3, 64, 21, 64, 64)}


def build_hm_case(name):
    N, C, K, H, W = HM_CASES[name]
    c = Case()
    seed = seed_of(name)
    c.x, c.w, c.b = ints(seed, N, C, H, W), weights(seed + 1, K, C, 1, 1, q=1.0), ints(seed + 2, K, lo=-8, hi=8)
    c.ref = fwd_epilogue(conv_fwd(c.x, c.w, 1, 0), c.b)
    return c


# grouped weight gradients: form: (formats, [(N, H, W, Ci, Co, k, s, p, accumulate, index of the item whose dw it shares or None)])
GROUPED_CASES = {
    'wgrad_group':    (('bf16', 'f32'), [(4, 16, 16, 64, 128, 1, 1, 0, False, None), (4, 16, 16, 64, 72, 1, 2, 0, True, None),
                                         (2, 15, 17, 32, 64, 3, 2, 1, False, None), (4, 16, 16, 64, 128, 1, 1, 0, True, 0)]),
    'wgrad_group256': (('bf16',), [(3, 9, 7, 256, 512, 1, 1, 0, False, None), (2, 8, 8, 512, 256, 1, 1, 0, True, None),
                                   (3, 9, 7, 256, 512, 1, 1, 0, True, 0)]),
    'wgrad_kw_group': (('bf16',), [(2, 5, 16, 64, 128, 3, 1, 1, False, None), (2, 5, 16, 64, 128, 3, 1, 1, True, 0),
                                   (1, 6, 32, 128, 256, 3, 1, 1, True, None), (2, 5, 16, 64, 64, 3, 1, 1, False, None)]),
}


def build_grouped_case(form):
    """-> [(shape, x, dy, dw0 or None)], refs: the float64 gradient each dw must hold after the call (None for an item that
    writes another item's dw: its share is in that item's reference)."""
    _, shapes = GROUPED_CASES[form]
    items, refs = [], []
    for i, shape in enumerate(shapes):
        N, H, W, Ci, Co, k, s, p, acc, share = shape
        seed = seed_of('%s/%d' % (form, i))
        Ho, Wo = out_size(H, W, k, k, s, p)
        x, dy = ints(seed, N, Ci, H, W), ints(seed + 1, N, Co, Ho, Wo)
        ref = conv_wgrad(x, dy, k, k, s, p).permute(0, 2, 3, 1).contiguous()
        dw0 = None
        if share is not None:
            refs[share] = refs[share] + ref
            ref = None
        elif acc:
            dw0 = ints(seed + 2, Co, k, k, Ci, lo=-16, hi=16)
            ref = ref + dw0.double()
        items.append((shape, x, dy, dw0))
        refs.append(ref)
    return items, refs
