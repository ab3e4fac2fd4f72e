"""'mxfp8' compute mode: MX (block-scaled e4m3) operands for the K-heavy conv GEMMs (csrc/mx_fp8.hip, the MX build of the fp8
gather kernel).  Quantiser and weight packs bit-exact against the reference rule (tests/mx_ref.py), the scale-to-lane map
with exact integer data, the GEMMs against fp64 torch on the dequantised operands, then layer- and model-level behaviour.

Guards (tests/guarded.py).  Sections 1 - 3 (the quantiser, the weight packs, the scale-to-lane map) place every operand and the
item table, call the wrappers inside a window and check the flanks after each call.  The outputs of sections 1 and 2 are bytes
(e4m3 elements, E8M0 scales) for which 0xFF is a right answer (a NaN block), so equality with the reference is the check; the
one-block case and the pack cases assert that their references hold no 0xFF byte, so a skipped byte cannot pass there.  The bf16
outputs of section 3 must be written completely.  The row pitch is C (times the element size) of the widest operand row."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
from conftest import PKG
from mx_ref import mx_dequantize, mx_pack_weights_ref, mx_quantize_ref
from seeded import fill_module_, randn

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guard(label, fn, *args, **kw):
    with G.window(_ops(), label):
        out = fn(*args, **kw)
    torch.cuda.synchronize()
    G.check(label)
    return out


def _ops():
    import mi355
    mi355.load()
    from mi355 import ops
    return ops


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(x):
    """NHWC tensor -> its [rows][C] memory as a CPU tensor"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).cpu()


def _assert_q_equal(q, s, qr, sr, src):
    """bytes equal, except that a NaN source element only has to stay NaN (its sign bit is not pinned)"""
    nan = torch.isnan(src.float())
    assert torch.equal(s.cpu(), sr), 'scale bytes differ at %s' % (torch.nonzero(s.cpu() != sr)[:8].tolist(),)
    qc = q.cpu()
    assert torch.equal(qc[~nan], qr[~nan]), 'element bytes differ at %s' % (torch.nonzero((qc != qr) & ~nan)[:8].tolist(),)
    assert torch.isnan(qc[nan].view(torch.float8_e4m3fn).float()).all()


# ---------------------------------------------------------------- 1. quantiser
@pytest.mark.parametrize('src', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [128, 256, 2048])
def test_mx_quantize_is_bit_exact_with_the_reference_rule(gpu, src, C):
    ops = _ops()
    tdt = torch.bfloat16 if src == 'bf16' else torch.float32
    rows = 37 if C == 2048 else 1001                            # not a multiple of any tile
    x = (randn(41, rows, C) * torch.exp(randn(42, rows, C // 32, 1).expand(rows, C // 32, 32).reshape(rows, C) * 4)).to(tdt)
    x[0, :32] = 0.0                                              # all-zero block
    x[0, 32:64] = torch.tensor([0.0, -0.0] * 16)                 # +-0
    x[1, :32] = 1.0; x[1, 5] = -448.0 * 2 ** 3                   # amax exactly 448 * 2^k: e = k, no saturation
    x[1, 32:64] = 0.5; x[1, 40] = 1.7578125 * 2 ** 4            # just above 448 * 2^-4 (m > 1.75, exact in bf16): e = -3
    x[1, 64:96] = 1.0; x[1, 70] = 460.0                          # (bf16: 460 -> 460, m = 1.797)
    x[2, :32] = 2.0 ** -130; x[2, 3] = -3 * 2.0 ** -133          # bf16 subnormal range: the -127 clamp
    x[2, 32:64] = 1e-3; x[2, 33] = float('nan')                  # NaN: 0xFF scale
    x[2, 64:96] = 3.0; x[2, 90] = -float('inf')                  # -Inf: 0xFF scale
    x[3, :32] = 2.0 ** 100                                       # large exponents
    G.row_pitch(C * x.element_size())
    xg = G.place(x.to(gpu), 'x')
    q, s = _guard('mx_quantize %s rows=%d C=%d' % (src, rows, C), ops.mx_quantize, xg)
    assert torch.equal(xg.cpu().view(torch.int16 if src == 'bf16' else torch.int32), x.view(torch.int16 if src == 'bf16' else torch.int32))
    qr, sr = mx_quantize_ref(x)
    assert q.shape == x.shape and s.numel() == rows * C // 32
    _assert_q_equal(q, s.view(rows, C // 32), qr, sr, x)
    assert [int(v) for v in sr[0, :2]] == [0, 0] and int(sr[1, 0]) == 127 + 3 and int(sr[1, 1]) == 127 + 1 - 4
    assert int(sr[2, 0]) == 0 and int(sr[2, 1]) == 255 and int(sr[2, 2]) == 255
    d = mx_dequantize(q.cpu(), s.view(rows, C // 32).cpu())
    assert torch.isnan(d[2, 32:96]).all()                        # the 0xFF blocks dequantise to NaN
    fin = torch.isfinite(x.float()).all(1)
    assert float((d[fin] - x[fin].float()).abs().max()) <= 2.0 ** -4 * float(x[fin].float().abs().max())


@pytest.mark.parametrize('src', ['bf16', 'f32'])
@pytest.mark.parametrize('rows,C', [(1, 32), (3, 32), (1, 64)])
def test_mx_quantize_smallest_shapes_leave_no_byte_unwritten(gpu, src, rows, C):
    """One row of one block, and its neighbours: finite data, so the reference holds no 0xFF byte (asserted) and an element or a
    scale byte the kernel skipped would still be the fill."""
    ops = _ops()
    x = (randn(47, rows, C) * 3).to(torch.bfloat16 if src == 'bf16' else torch.float32)
    qr, sr = mx_quantize_ref(x)
    assert not bool((qr == 0xFF).any()) and not bool((sr == 0xFF).any())
    G.row_pitch(C * x.element_size())
    q, s = _guard('mx_quantize %s rows=%d C=%d' % (src, rows, C), ops.mx_quantize, G.place(x.to(gpu), 'x'))
    assert q.shape == x.shape and s.numel() == rows * C // 32
    assert torch.equal(q.cpu(), qr) and torch.equal(s.view(rows, C // 32).cpu(), sr)


def test_mx_quantize_nhwc_rows(gpu):
    """an NHWC feature map is blocked along its channels: the [rows][C] memory of the map"""
    ops = _ops()
    G.row_pitch(11 * 256 * 2)
    x = G.place(_nhwc(randn(43, 3, 256, 9, 11).to(gpu).to(torch.bfloat16)), 'x')
    q, s = _guard('mx_quantize nhwc', ops.mx_quantize, x)
    qr, sr = mx_quantize_ref(_rows(x))
    assert not bool((qr == 0xFF).any()) and not bool((sr == 0xFF).any())      # finite data: no 0xFF in the reference
    assert q.stride() == x.stride()
    assert torch.equal(_rows(q), qr) and torch.equal(s.view(-1, 8).cpu(), sr)


# ---------------------------------------------------------------- 2. weight packs
@pytest.mark.parametrize('O,T,I', [(32, 1, 32), (128, 9, 128), (256, 16, 128), (64, 9, 96), (136 + 24, 9, 512)])
def test_mx_weight_packs_are_bit_exact(gpu, O, T, I):
    ops = _ops()
    w = randn(44, O, T, I) * torch.exp(randn(45, O, T, 1) * 3)
    w[0, 0, :32] = 0.0
    w[1, min(1, T - 1), 7] = 448.0 * 4
    G.row_pitch(max(O, I) * 4)
    wg = G.place(w.to(gpu).contiguous(), 'w')
    got = _guard('pack_weights_mx %s' % ((O, T, I),), ops.pack_weights_mx, wg, O, T, I)
    ref = mx_pack_weights_ref(w, O, T, I)
    for name, a, b in zip(('wf', 'sf', 'wt', 'st'), got, ref):
        assert not bool((b == 0xFF).any()), name          # finite weights: no 0xFF in the reference, a skipped byte would show
        assert torch.equal(a.cpu(), b), name
    # the batched form (two items in one launch) writes the same bytes
    w2 = G.place((randn(46, 128, 9, 256)).to(gpu).contiguous(), 'w2')
    packs = [[G.empty((n,), torch.uint8, gpu, 'pack') for n in (o * t * i, o * t * i // 32) * 2]
             for (o, t, i) in ((O, T, I), (128, 9, 256))]
    rec = np.zeros(2, dtype=[('w', '<u8'), ('wf', '<u8'), ('sf', '<u8'), ('wt', '<u8'), ('st', '<u8'), ('O', '<i4'), ('T', '<i4'),
                             ('I', '<i4'), ('blk0', '<i4')])
    blk0 = (O // 32) * (I // 32) * T
    rec[0] = (wg.data_ptr(), *[p.data_ptr() for p in packs[0]], O, T, I, 0)
    rec[1] = (w2.data_ptr(), *[p.data_ptr() for p in packs[1]], 128, 9, 256, blk0)
    tab = G.place(torch.from_numpy(rec.view(np.uint8).copy()).to(gpu), 'pack table')
    _guard('pack_weights_mx_batched', ops.pack_weights_mx_batched, tab, 2, blk0 + 4 * 8 * 9)
    for p, b in zip(packs[0], ref):
        assert torch.equal(p.cpu(), b)
    for p, b in zip(packs[1], mx_pack_weights_ref(w2.cpu(), 128, 9, 256)):
        assert torch.equal(p.cpu(), b)


# ---------------------------------------------------------------- 3. scale-to-lane map with exact data
def _exact_operands(seed, rows, C, lo=125, hi=130):
    """small-integer e4m3 elements and a distinct-ish power-of-two scale per (row, block): every product and every partial
    sum of the GEMM is exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, 4, (rows, C), generator=g).float()
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    s = torch.randint(lo, hi, (rows, C // 32), generator=g).to(torch.uint8)
    return q, s


@pytest.mark.parametrize('case', [(2, 8, 8, 128, 128, 3, 1, 1), (2, 8, 8, 256, 128, 3, 2, 1), (1, 8, 8, 128, 128, 4, 2, 1),
                                  (3, 9, 11, 128, 64, 3, 1, 1)])
def test_mx_scale_to_lane_map_is_exact(gpu, case):
    """Every scale byte must reach the lanes that hold its block: with exact integer data the bf16 result of the kernel equals
    the fp64 result rounded to bf16, element for element -- a lane reading a neighbouring block's byte changes it by 2^k."""
    ops = _ops()
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xq, xs = _exact_operands(51, N * H * W, Ci)
    wq, ws = _exact_operands(52, Co * k * k, Ci)
    wtq, wts = _exact_operands(53, Ci * k * k, Co)
    desc = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
    G.row_pitch(max(Ci, Co) * 2)
    pl = lambda t, name: G.place(t.to(gpu), name)
    y = _guard('conv_fwd_mx %s' % (case,), ops.conv_fwd_mx, desc, pl(xq, 'x8'), pl(xs, 'sx'), pl(wq, 'w8'), pl(ws, 'sw'))
    assert G.unwritten(y) == 0
    xr = mx_dequantize(xq, xs).view(N, H, W, Ci).permute(0, 3, 1, 2).double()
    wr = mx_dequantize(wq, ws).view(Co, k, k, Ci).permute(0, 3, 1, 2).double()
    ref = F.conv2d(xr, wr, stride=s, padding=p)
    assert torch.equal(y.float().cpu(), ref.float().to(torch.bfloat16).float()), 'fwd %s' % (case,)
    if Co % 128 == 0:
        dq, dsc = _exact_operands(54, N * Ho * Wo, Co)
        dx = _guard('conv_dgrad_mx %s' % (case,), ops.conv_dgrad_mx, desc, pl(dq, 'dy8'), pl(dsc, 'sdy'), pl(wtq, 'wT8'), pl(wts, 'swT'))
        assert G.unwritten(dx) == 0
        dyr = mx_dequantize(dq, dsc).view(N, Ho, Wo, Co).permute(0, 3, 1, 2).double()
        wtr = mx_dequantize(wtq, wts).view(Ci, k, k, Co).permute(3, 0, 1, 2).double()    # -> (Co, Ci, kh, kw)
        xx = torch.zeros(N, Ci, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, wtr, stride=s, padding=p).backward(dyr)
        assert torch.equal(dx.float().cpu(), xx.grad.float().to(torch.bfloat16).float()), 'dgrad %s' % (case,)


# ---------------------------------------------------------------- 4. GEMMs against fp64 on the dequantised operands
CASES = [  # test_gpu_fp8.CASES, and the full-size 3x3 256->256 @64x64, B=64
    (2, 16, 16, 128, 128, 3, 1, 1), (3, 9, 11, 256, 64, 3, 1, 1), (2, 16, 16, 256, 256, 3, 2, 1), (2, 8, 8, 512, 136, 1, 1, 0),
    (2, 16, 16, 128, 256, 4, 2, 1), (1, 32, 32, 256, 256, 3, 1, 1), (16, 32, 32, 128, 128, 3, 1, 1), (64, 64, 64, 256, 256, 3, 1, 1)]


@pytest.mark.parametrize('case', CASES)
def test_conv_fwd_dgrad_mx_vs_fp64_on_dequantised_operands(gpu, case):
    ops = _ops()
    N, H, W, Ci, Co, k, s, p = case
    x = _nhwc(randn(21, N, Ci, H, W).to(gpu).to(torch.bfloat16))
    w = (randn(22, Co, Ci, k, k) / np.sqrt(Ci * k * k)).to(gpu)
    bias = randn(23, Co).to(gpu)
    Co_p = (Co + 31) // 32 * 32                                            # the weight pack works on 32-channel tiles
    w_conv = w.permute(0, 2, 3, 1).contiguous()
    if Co_p != Co:
        w_conv = torch.cat([w_conv, torch.zeros(Co_p - Co, k, k, Ci, device=gpu)], 0)
    wf, sf, wt, st = ops.pack_weights_mx(w_conv, Co_p, k * k, Ci)
    x8, sx = ops.mx_quantize(x)
    desc = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
    res = _nhwc(randn(26, N, Co, desc.Ho, desc.Wo).to(gpu).to(torch.bfloat16)) if N == 3 else None
    want = res is None
    out = ops.conv_fwd_mx(desc, x8, sx, wf, sf, bias, residual=res, want_stats=want)
    y, part = out if want else (out, None)
    torch.cuda.synchronize()
    imgs = [0, N // 2, N - 1] if N > 4 else list(range(N))                 # (images are independent: fp64 on a sample of them)
    xr = mx_dequantize(_rows(x8), sx.view(-1, Ci // 32).cpu()).view(N, H, W, Ci).permute(0, 3, 1, 2)[imgs].double()
    wr = mx_dequantize(wf.view(Co_p * k * k, Ci).cpu(), sf.view(-1, Ci // 32).cpu()).view(Co_p, k, k, Ci)[:Co].permute(0, 3, 1, 2).double()
    ref = F.conv2d(xr, wr, bias.cpu().double(), stride=s, padding=p)
    if res is not None:
        ref = ref + res.float().cpu().double()
    got = y[imgs].float().cpu().double()
    err = float((got - ref).norm() / ref.norm())
    assert err <= 6e-3, 'fwd %s: %.3e' % (case, err)
    if part is not None:                                                   # statistics of the rounded result, fused
        buf, ns = part
        pr = buf[:ns * Co * 3].view(ns, Co, 3).double().cpu()
        n = pr[..., 0].sum(0)
        mean = (pr[..., 0] * pr[..., 1]).sum(0) / n
        assert float(n.min()) == float(n.max()) == N * y.shape[2] * y.shape[3]
        ref_mean = y.float().double().mean(dim=(0, 2, 3)).cpu()
        assert float((mean - ref_mean).abs().max()) <= 1e-4 * float(ref_mean.abs().max() + 1)
    if Co % 128:
        return
    dy = _nhwc((randn(24, N, Co, y.shape[2], y.shape[3]) * 1e-3).to(gpu).to(torch.bfloat16))
    dy8, sdy = ops.mx_quantize(dy)
    lam = torch.full((), 0.25, device=gpu)
    base = _nhwc(randn(25, N, Ci, H, W).to(gpu).to(torch.bfloat16) * 1e-3)
    dx = ops.conv_dgrad_mx(desc, dy8, sdy, wt, st, scale_dev=lam, out=base.clone(), accumulate=True)
    dyr = mx_dequantize(_rows(dy8), sdy.view(-1, Co // 32).cpu()).view(N, desc.Ho, desc.Wo, Co).permute(0, 3, 1, 2)[imgs].double()
    wtr = mx_dequantize(wt.view(Ci * k * k, Co).cpu(), st.view(-1, Co // 32).cpu()).view(Ci, k, k, Co).permute(3, 0, 1, 2).double()
    xx = torch.zeros(len(imgs), Ci, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xx, wtr, None, stride=s, padding=p).backward(dyr)
    ref = 0.25 * xx.grad + base[imgs].float().cpu().double()
    err = float((dx[imgs].float().cpu().double() - ref).norm() / ref.norm())
    assert err <= 8e-3, 'dgrad %s: %.3e' % (case, err)
    if k == 3 and s == 1:                                                  # dgrad with fused statistics, no accumulate
        dx2, part2 = ops.conv_dgrad_mx(desc, dy8, sdy, wt, st, want_stats=True)
        assert part2 is not None and torch.equal(dx2, ops.conv_dgrad_mx(desc, dy8, sdy, wt, st))


# ---------------------------------------------------------------- 5. what block scaling is for
def test_mx_input_gradient_keeps_every_image_where_per_tensor_fp8_loses_one(gpu):
    """dy whose 4 images differ in magnitude by 2^-16 / 1 / 2^8 / 2^16: MX input gradient within 8e-2 (relative L2) of fp64
    on the bf16 operands for every image; 'fp8' mode's per-tensor e5m2 path (scale from the largest image) flushes the
    2^-16 image to zero (error 1.0 > 0.5).  Measured: MX 0.0375 / 0.0377 / 0.0376 / 0.0377, per-tensor fp8 1.0 / 0.059 / 0.060 /
    0.059."""
    ops = _ops()
    N, H, W, C, k = 4, 16, 16, 256, 3
    mag = torch.tensor([2.0 ** -16, 1.0, 2.0 ** 8, 2.0 ** 16]).view(N, 1, 1, 1)
    dy = _nhwc((randn(61, N, C, H, W) * mag).to(gpu).to(torch.bfloat16))
    w = (randn(62, C, C, k, k) / np.sqrt(C * k * k)).to(gpu)
    w_conv = w.permute(0, 2, 3, 1).contiguous()
    desc = ops.make_desc_fp8(N, H, W, C, C, k, k, 1, 1)
    xx = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xx, w.cpu().double(), None, padding=1).backward(dy.float().cpu().double())
    ref = xx.grad
    _, _, wt, st = ops.pack_weights_mx(w_conv, C, k * k, C)
    dy8, sdy = ops.mx_quantize(dy)
    dx_mx = ops.conv_dgrad_mx(desc, dy8, sdy, wt, st).float().cpu().double()
    sw, sd = ops.fp8_state(gpu), ops.fp8_state(gpu)
    _, wt8 = ops.pack_weights_fp8(w_conv, C, k * k, C, sw)
    q8 = ops.fp8_quantize(dy, sd, ops.E5M2, jit=True)
    dx_8 = ops.conv_dgrad_fp8(desc, q8, sd, wt8, sw, dy_fmt=ops.E5M2).float().cpu().double()
    e_mx = [float((dx_mx[i] - ref[i]).norm() / ref[i].norm()) for i in range(N)]
    e_8 = [float((dx_8[i] - ref[i]).norm() / ref[i].norm()) for i in range(N)]
    print('per-image relative L2: mx %s, per-tensor fp8 %s' % (['%.3g' % e for e in e_mx], ['%.3g' % e for e in e_8]))
    assert max(e_mx) <= 8e-2, e_mx
    assert max(e_8) > 0.5, e_8


# ---------------------------------------------------------------- 6 - 9. compute dtype 'mxfp8'
def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture
def mx_mode():
    import mi355
    mi355.load()
    yield mi355
    mi355.set_compute_dtype('bf16')


@pytest.mark.parametrize('kind,k,s,p', [('conv', 3, 1, 1), ('conv', 3, 2, 1), ('deconv', 4, 2, 1)])
def test_mxfp8_layers_track_the_bf16_layers(gpu, mx_mode, kind, k, s, p):
    """Conv2d / ConvTranspose2d in 'mxfp8' mode against the same layer in 'bf16' mode: forward output and input gradient within
    8e-2 relative L2 (the bound test_fp8_layers_track_the_bf16_layers allows; measured values are printed), the weight
    gradient identical (it stays on the bf16 kernels), fused BatchNorm statistics equal to a statistics pass.  Measured (y, dx):
    3x3 s1 0.0376 / 0.0376, 3x3 s2 0.0377 / 0.0376, 4x4 s2 transposed 0.0377 / 0.0377."""
    from mi355.nn import Conv2d, ConvTranspose2d, BatchNorm2d
    mi355 = mx_mode
    torch.manual_seed(0)
    mod = (Conv2d(256, 256, k, s, p, bias=(s == 1)) if kind == 'conv' else ConvTranspose2d(256, 256, k, s, p)).to(gpu)
    fill_module_(mod, 31)
    x0 = _nhwc(randn(32, 4, 256, 16, 16).to(gpu).to(torch.bfloat16))
    res = {}
    for dt in ('bf16', 'mxfp8'):
        mi355.set_compute_dtype(dt)
        x = x0.clone().requires_grad_(True)
        mod.weight.grad = None
        y = mod(x)
        g = _nhwc((randn(33, *y.shape) * 1e-2).to(gpu).to(torch.bfloat16))
        y.backward(g)
        res[dt] = (y.detach().float(), x.grad.float(), mod.weight.grad.clone())
    e_y, e_dx = _rel(res['mxfp8'][0], res['bf16'][0]), _rel(res['mxfp8'][1], res['bf16'][1])
    print('%s k%d s%d: relative L2 y %.4f, dx %.4f' % (kind, k, s, e_y, e_dx))
    assert 1e-3 < e_y <= 8e-2, e_y                   # > 1e-3: the MX path really ran
    assert 1e-3 < e_dx <= 8e-2, e_dx
    assert torch.equal(res['mxfp8'][2], res['bf16'][2])
    mi355.set_compute_dtype('mxfp8')
    bn = BatchNorm2d(256).to(gpu)
    mod.bn_follows = True
    y = mod(x0)
    assert getattr(y, '_mi_bn_partial', None) is not None
    z = bn(y, relu=True)
    mod.bn_follows = False
    bn2 = BatchNorm2d(256).to(gpu)
    z2 = bn2(mod(x0).clone(), relu=True)
    assert _rel(z.float(), z2.float()) <= 1e-3
    assert torch.allclose(bn.running_var, bn2.running_var, rtol=1e-4, atol=1e-6)


def _r18(gpu, seed=1):
    import uda.model as models
    from mi355.da_step import build_training
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    torch.manual_seed(seed)
    bb = models.resnet18(pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True)
    fill_module_(model, 700 + seed)
    model = model.to(gpu)
    step, opts, scheds = build_training(model, heatmap_size=32)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    return model, step, scheds


def test_mxfp8_training_reduces_the_supervised_loss(gpu, mx_mode):
    """80 A/B/C iterations on one fixed synthetic batch (ResNet-18, 128x128, B=4) in 'mxfp8' mode, graph replay from
    iteration 5 on: finite losses and the supervised loss falls by more than a third (measured 27.7 -> 8.8)."""
    from utils.synthetic import make_batch
    mx_mode.set_compute_dtype('mxfp8')
    model, step, scheds = _r18(gpu)
    batch = make_batch(4, 128, 32, seed=3, device=gpu)
    first = None
    for it in range(80):
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        if it == 0:
            first = float(out['loss_s'])
        if it == 5:
            step.capture(batch, warmup=0)
    last = [float(out[k]) for k in ('loss_s', 'loss_gf', 'loss_gt')]
    print('mxfp8 ResNet-18 loss_s: %.4f -> %.4f' % (first, last[0]))
    assert all(np.isfinite(v) for v in last), last
    assert last[0] < 0.66 * first, (first, last)


def test_mxfp8_graph_replay_is_bit_identical_to_eager(gpu, mx_mode):
    """Twin models in 'mxfp8' mode: one runs 6 iterations eagerly, the other 3 eagerly, captures and replays 3.  Losses and
    every parameter agree bit for bit: the replayed graphs read MX packs of the updated weights (FusedSGD repacks them inside
    the captured step)."""
    from utils.synthetic import make_batch
    mx_mode.set_compute_dtype('mxfp8')
    m1, s1, sch1 = _r18(gpu)
    m2, s2, sch2 = _r18(gpu)
    batch = make_batch(4, 128, 32, seed=3, device=gpu)
    l1, l2 = [], []
    for _ in range(6):
        l2.append(float(s2.run(batch)['loss_s']))
        for s in sch2.values():
            s.step()
    for it in range(6):
        if it == 3:
            s1.capture(batch, warmup=0)
        out = s1.replay(batch) if it >= 3 else s1.run(batch)
        l1.append(float(out['loss_s']))
        for s in sch1.values():
            s.step()
    torch.cuda.synchronize()
    assert l1 == l2, (l1, l2)
    assert len(set(l1)) > 1                           # the weights moved
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


def test_mxfp8_resnet50_iteration_vs_reference(gpu, mx_mode):
    """One complete ResNet-50 A/B/C iteration in 'mxfp8' mode against golden G8 with the bounds of the 'fp8' test: step-A
    loss within 3 % of the reference's (measured 32.51 against 32.36), finite losses, every parameter updated."""
    from conftest import golden
    from test_gpu_model import _g8_setup, _g8_batch
    from mi355.da_step import build_training
    g = golden('g8_bottleneck')
    mx_mode.set_compute_dtype('mxfp8')
    model = _g8_setup(gpu)
    model.gl_layer.iter_num = 500
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    step, opts, scheds = build_training(model)
    out = step.run(_g8_batch(gpu))
    torch.cuda.synchronize()
    vals = np.array([float(out[k]) for k in ('loss_s', 'loss_gf', 'loss_gt')])
    print('mxfp8 ResNet-50 losses %s, reference %s' % (vals, g['losses']))
    assert np.isfinite(vals).all(), vals
    assert abs(vals[0] - g['losses'][0]) <= 3e-2 * g['losses'][0], (vals, g['losses'])
    for k, p in model.named_parameters():
        if not k.startswith('backbone.fc.'):
            inert = k.endswith('.bias') and p.grad is not None and float(p.grad.abs().max()) == 0.0 and float(before[k].abs().max()) == 0.0
            assert torch.isfinite(p).all() and (inert or not torch.equal(p, before[k])), k


def test_mxfp8_inference_takes_the_folded_bf16_path(gpu, mx_mode):
    from test_gpu_model import _g8_setup
    mi355 = mx_mode
    mi355.set_compute_dtype('bf16')
    m = _g8_setup(gpu, 'resnet50', 811)
    x = randn(813, 2, 3, 256, 256).to(gpu)
    m.train()
    with torch.no_grad():
        m(x)
    m.eval()
    outs = {}
    for dt in ('bf16', 'mxfp8'):
        mi355.set_compute_dtype(dt)
        with torch.no_grad():
            y = m(x)
        outs[dt] = (y[0] if isinstance(y, (tuple, list)) else y).float().clone()
    assert torch.isfinite(outs['mxfp8']).all() and torch.equal(outs['bf16'], outs['mxfp8'])


def test_mxfp8_layer_state_across_modes_edits_and_loads(gpu, mx_mode):
    """One Conv2d through bf16 -> mxfp8 -> bf16 -> mxfp8, an in-place weight edit (x2: the MX pack of 2w has the same
    elements and every scale one higher, so y doubles exactly) and load_state_dict of the original weights (y as at first).
    The MX pack follows every change; state_dict keys are the same in every mode."""
    from mi355.nn import Conv2d
    mi355 = mx_mode
    mod = Conv2d(128, 128, 3, 1, 1, bias=False).to(gpu)
    fill_module_(mod, 71)
    sd0 = {k: v.clone() for k, v in mod.state_dict().items()}
    x = _nhwc(randn(72, 2, 128, 16, 16).to(gpu).to(torch.bfloat16))
    ys, keys = {}, []
    for i, dt in enumerate(('bf16', 'mxfp8', 'bf16', 'mxfp8')):
        mi355.set_compute_dtype(dt)
        ys[i] = mod(x).detach().clone()
        keys.append(sorted(mod.state_dict()))
    assert torch.equal(ys[0], ys[2]) and torch.equal(ys[1], ys[3]) and not torch.equal(ys[0], ys[1])
    assert all(k == keys[0] for k in keys)
    with torch.no_grad():
        mod.weight.mul_(2.0)
    y2 = mod(x).detach()
    assert torch.equal(y2.float(), 2 * ys[1].float())
    mod.load_state_dict(sd0)
    assert torch.equal(mod(x).detach(), ys[1])


# ---------------------------------------------------------------- 10. loud failures
def test_mx_argument_checks_are_loud(gpu):
    import mi355
    ops = _ops()
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=gpu)
    desc = ops.make_desc_fp8(1, 8, 8, 64, 128, 3, 3, 1, 1)                # 64 contracted channels: below one K tile
    with pytest.raises(mi355.Mi355Error, match='multiple of 128'):
        ops.conv_fwd_mx(desc, u8(64 * 64), u8(2 * 64), u8(128 * 9 * 64), u8(128 * 9 * 2))
    desc = ops.make_desc_fp8(1, 8, 8, 128, 128, 3, 3, 1, 1)
    y = torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(mi355.Mi355Error, match='null'):                   # null scale pointer, straight through the C ABI
        mi355.call('mi355_conv_fwd_mx', ctypes_desc(desc), u8(64 * 128).data_ptr(), 0, u8(128 * 9 * 128).data_ptr(),
                   u8(128 * 9 * 4).data_ptr(), 0, 0, y.data_ptr(), 0, 0, None, mi355.stream_ptr())
    with pytest.raises(mi355.Mi355Error, match='sx'):                     # undersized scale buffer
        ops.conv_fwd_mx(desc, u8(64 * 128), u8(64 * 4 - 1), u8(128 * 9 * 128), u8(128 * 9 * 4))
    with pytest.raises(mi355.Mi355Error, match='out'):
        ops.conv_dgrad_mx(desc, u8(64 * 128), u8(64 * 4), u8(128 * 9 * 128), u8(128 * 9 * 4),
                          out=torch.zeros(10, dtype=torch.bfloat16, device=gpu))
    with pytest.raises(mi355.Mi355Error):
        ops.mx_quantize(torch.zeros(4, 48, device=gpu))                   # C not a multiple of 32
    with pytest.raises(mi355.Mi355Error, match='scales'):
        ops.mx_quantize(torch.zeros(4, 64, device=gpu), scales=u8(7))
    with pytest.raises(mi355.Mi355Error):
        ops.pack_weights_mx(torch.zeros(48 * 9 * 128, device=gpu), 48, 9, 128)   # O not a multiple of 32
    with pytest.raises(mi355.Mi355Error, match='wt'):
        ops.pack_weights_mx(torch.zeros(128 * 9 * 128, device=gpu), 128, 9, 128, wt=u8(100))
    torch.cuda.synchronize()


def ctypes_desc(desc):
    import ctypes
    return ctypes.byref(desc)


# ---------------------------------------------------------------- 11. command line
def test_train_cli_mxfp8_then_test_cli_bf16(gpu, tmp_path):
    log = str(tmp_path / 'run')
    common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '4', '-p', '2', '-j', '0',
              '--pretrain_epochs', '1', '--log', log]
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(script, extra):
        r = subprocess.run([sys.executable, os.path.join(PKG, script)] + common + extra, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    out = run('train1.py', ['--epochs', '1', '--dtype', 'mxfp8', '--pretrain', str(tmp_path / 'none.pth')])
    assert 'Start regression domain adaptation.' in out and "dtype='mxfp8'" in out
    ck_path = os.path.join(log, 'checkpoints', '0.pth')
    ck = torch.load(ck_path, map_location='cpu', weights_only=False)
    assert len(ck['model']) == 222 and all(torch.isfinite(v).all() for v in ck['model'].values() if v.is_floating_point())
    out = run('test.py', ['--checkpoint', ck_path, '--dtype', 'bf16'])
    assert 'Source:' in out and 'fingertip:' in out
