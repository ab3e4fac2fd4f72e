"""Opt-in MX inference (mi355.set_mx_eval / MI355_MX_EVAL): eval-mode convs whose BatchNorm is folded run on MX operands with
bias, residual and ReLU in the kernel (mi355_conv_fwd_mx_act / mi355_conv_dgrad_mx_act, EPI 3 of gather_fp8_kernel) and can
write the MX copy of their own output for the next MX layer.

1  exact integer operands: y equals the float64 reference bit for bit (range condition asserted on the reference), every build
2  the fused copy (y8, sy) equals tests/mx_ref.py's quantiser applied to the same launch's y, bit for bit
3  relu = 0 returns the bits of the two-launch entry points  4  loud argument checks
5  layers against the ABI call on the folded packs, and the refresh events  6  the chain launches no stand-alone quantiser
7  ResNet-101 against the fp32 reference  8  switch off = the folded bf16 path  9  graphs  10  argmax agreement"""
import ctypes
import re

import numpy as np
import pytest
import torch

import conv_exact_ref as R
from mx_ref import mx_dequantize, mx_quantize_ref
from seeded import fill_module_, randn

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _mi():
    import mi355
    mi355.load()
    return mi355


def _ops():
    _mi()
    from mi355 import ops
    return ops


@pytest.fixture
def mx_eval():
    """the switch, restored to off (and the compute dtype to bf16) afterwards"""
    mi355 = _mi()
    yield mi355
    mi355.set_mx_eval(False)
    mi355.set_compute_dtype('bf16')


def _run(ops, fn):
    """fn() with the labels of the conv-family launches it made (the launch log is on for this call only: it must stay off
    while the graph tests of this module capture)."""
    ops.prof_enable(1)
    try:
        ops.prof_reset()
        out = fn()
        torch.cuda.synchronize()
        return out, [l['label'] for l in ops.prof_launches() if l['family'] == 0]
    finally:
        ops.prof_enable(0)


def _check_build(what, labels, expect):
    print('\nLABEL %s %s' % (what, ' | '.join(labels)))
    assert len(labels) == 1, '%s: %r' % (what, labels)
    m = re.search(r'\[([^\]]*)\]$', labels[0])
    assert m and m.group(1) == expect, '%s: launched %r, expected [%s]' % (what, labels, expect)


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(x):
    """NHWC tensor -> its [rows][C] memory as a CPU tensor"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).cpu()


def _same(what, got, ref):
    assert R.same_bits(got, ref, BF16), '%s: %s' % (what, R.first_mismatch(got, ref, BF16))


# ---------------------------------------------------------------- operands
# (N, H, W, Ci, Co, k, s, p): the smallest of ...                                   forward build   dgrad-form build
CASES = [
    ((2, 8, 8, 128, 128, 3, 1, 1), 'g64x64', 'g64x64'),         # the 64x64 build
    ((3, 9, 11, 128, 64, 3, 1, 1), 'g64x64', None),             # ragged rows, 64-wide (Co = 64 cannot be contracted)
    ((2, 8, 8, 256, 128, 3, 2, 1), 'g64x64', 'g64x64'),         # stride 2
    ((1, 8, 8, 128, 128, 4, 2, 1), 'g64x64', 'g64x64'),         # 4x4; dgrad form = four phases, scattered rows
    ((5, 60, 60, 128, 128, 3, 1, 1), 'g64x128', 'g64x128'),     # 64x128 by choose_fp8's own rule, last row tile 16 of 64
    ((10, 60, 58, 128, 256, 3, 1, 1), 'g128x128', 'g64x128'),   # 128x128, last row tile 112 of 128 (dgrad form: 128 columns)
]
_IDS = ['x'.join(str(v) for v in c[0]) for c in CASES]


def _mx_encode(v, seed, mixed):
    """Integer matrix v [rows][C] as MX operands that dequantise to exactly v: all scale bytes 127, or (mixed) a byte in
    125 .. 129 per (row, block) -- the range of test_mx_scale_to_lane_map_is_exact's _exact_operands -- with the elements
    holding v * 2^(127 - byte), which e4m3 represents exactly for |v| <= 2.  A lane that reads a neighbouring block's byte changes
    the result by a power of two."""
    rows, C = v.shape
    if mixed:
        g = torch.Generator().manual_seed(seed)
        s = torch.randint(125, 130, (rows, C // 32), generator=g)
    else:
        s = torch.full((rows, C // 32), 127)
    el = v.view(rows, C // 32, 32) * torch.pow(2.0, (127 - s).float())[..., None]
    q = el.reshape(rows, C).to(torch.float8_e4m3fn).view(torch.uint8)
    s = s.to(torch.uint8)
    assert torch.equal(mx_dequantize(q, s), v)
    return q.contiguous(), s.contiguous()


_case_cache = {}


def _case(i):
    """Operands and float64 references of CASES[i], computed once per process and shared (never modified) by the tests."""
    if i in _case_cache:
        return _case_cache[i]
    (N, H, W, Ci, Co, k, s, p), _, dg = CASES[i]
    c = R.Case()
    c.shape, mixed, seed = CASES[i][0], bool(i % 2), 9100 + 16 * i
    c.Ho, c.Wo = R.out_size(H, W, k, k, s, p)
    c.x = R.ints(seed, N, Ci, H, W)
    c.w = R.weights(seed + 1, Co, Ci, k, k)                            # +-1, density min(1, 300 / K)
    c.bias, c.res = R.ints(seed + 2, Co, lo=-8, hi=8), R.ints(seed + 3, N, Co, c.Ho, c.Wo, lo=-16, hi=16)
    c.x8 = _mx_encode(c.x.permute(0, 2, 3, 1).reshape(-1, Ci), seed + 4, mixed)
    c.w8 = _mx_encode(c.w.permute(0, 2, 3, 1).reshape(-1, Ci), seed + 5, mixed)
    c.y = R.conv_fwd(c.x, c.w, s, p)
    c.y_b = R.fwd_epilogue(c.y, c.bias)
    c.fwd = {(relu, res): R.fwd_epilogue(c.y, c.bias, c.res if res else None, relu=relu) for relu in (False, True) for res in (False, True)}
    R.assert_exact_in(BF16, c.y, c.y_b, *c.fwd.values())               # the range condition, on the reference
    if dg:
        c.dy = R.ints(seed + 6, N, Co, c.Ho, c.Wo)
        c.bias_i = R.ints(seed + 7, Ci, lo=-8, hi=8)
        c.dy8 = _mx_encode(c.dy.permute(0, 2, 3, 1).reshape(-1, Co), seed + 8, mixed)
        c.wt8 = _mx_encode(c.w.permute(1, 2, 3, 0).reshape(-1, Co), seed + 9, mixed)
        c.dx = R.conv_dgrad(c.dy, c.w, s, p, (H, W))
        c.dgrad = {relu: R.fwd_epilogue(c.dx, c.bias_i, relu=relu) for relu in (False, True)}
        R.assert_exact_in(BF16, c.dx, *c.dgrad.values())
    _case_cache[i] = c
    return c


def _check_copy(what, y, y8, sy):
    """the fused copy against the reference quantiser applied to the bf16 tensor the same launch stored"""
    C = y.shape[1]
    qr, sr = mx_quantize_ref(_rows(y))
    assert y8.stride() == y.stride() and sy.numel() == y.numel() // 32, what
    s = sy.view(-1, C // 32).cpu()
    assert torch.equal(s, sr), '%s: scale bytes differ at %s' % (what, torch.nonzero(s != sr)[:8].tolist())
    q = _rows(y8)
    assert torch.equal(q, qr), '%s: element bytes differ at %s' % (what, torch.nonzero(q != qr)[:8].tolist())


# ---------------------------------------------------------------- 1 + 2. exact values and the fused quantiser
@pytest.mark.parametrize('i', range(len(CASES)), ids=_IDS)
def test_act_epilogue_returns_the_reference_bits_and_its_own_mx_copy(gpu, i):
    """Integer operands (activations in {-2..2}, weights +-1 with density min(1, 300 / K), integer bias and residual; scale
    bytes all 127 for the even cases, mixed 125 .. 129 for the odd ones): y = relu(conv + bias + residual) equals the float64
    reference bit for bit, with ReLU on and off, with and without residual, forward and (Co % 128 == 0) dgrad form, on the build
    choose_fp8 picks.  The copy requested with it equals mx_quantize_ref(y); y is the same bits without the copy."""
    ops = _ops()
    (N, H, W, Ci, Co, k, s, p), e_fwd, e_dgrad = CASES[i]
    c = _case(i)
    desc = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
    x8, sx, w8, sw = (t.to(gpu) for t in c.x8 + c.w8)
    bias, res = c.bias.to(gpu), ops.to_nhwc(c.res.to(gpu), BF16)
    for (relu, with_res), ref in c.fwd.items():
        what = 'fwd %s relu=%d res=%d' % (_IDS[i], relu, with_res)
        r = res if with_res else None
        (y, y8, sy), labels = _run(ops, lambda: ops.conv_fwd_mx_act(desc, x8, sx, w8, sw, bias, r, relu=relu, want_copy=True))
        _check_build(what, labels, 'mx %s epi3' % e_fwd)
        _same(what, y, ref)
        _check_copy(what, y, y8, sy)
        y0, labels = _run(ops, lambda: ops.conv_fwd_mx_act(desc, x8, sx, w8, sw, bias, r, relu=relu))
        _check_build(what + ' (no copy)', labels, 'mx %s epi3' % e_fwd)
        assert torch.equal(y0.view(torch.int16), y.view(torch.int16)), what + ': y differs when the copy is requested'
    if e_dgrad is None:
        return
    dy8, sdy, wt8, swt = (t.to(gpu) for t in c.dy8 + c.wt8)
    bias_i = c.bias_i.to(gpu)
    for relu, ref in c.dgrad.items():
        what = 'dgrad %s relu=%d' % (_IDS[i], relu)
        (dx, dx8, sdx), labels = _run(ops, lambda: ops.conv_dgrad_mx_act(desc, dy8, sdy, wt8, swt, bias_i, relu=relu, want_copy=True))
        _check_build(what, labels, 'mx %s epi3' % e_dgrad)
        _same(what, dx, ref)
        _check_copy(what, dx, dx8, sdx)
        dx0 = ops.conv_dgrad_mx_act(desc, dy8, sdy, wt8, swt, bias_i, relu=relu)
        assert torch.equal(dx0.view(torch.int16), dx.view(torch.int16)), what + ': dx differs when the copy is requested'


GAUSS = [((2, 8, 8, 128, 128, 3, 1, 1), 'g64x64'), ((5, 60, 60, 128, 128, 3, 1, 1), 'g64x128'), ((10, 60, 58, 128, 256, 3, 1, 1), 'g128x128'),
         ((1, 8, 8, 128, 128, 4, 2, 1), 'g64x64')]


def _gauss(ops, gpu, case, seed):
    N, H, W, Ci, Co, k, s, p = case
    x = _nhwc(randn(seed, N, Ci, H, W).to(gpu).to(BF16))
    w = (randn(seed + 1, Co, k, k, Ci) / np.sqrt(Ci * k * k)).to(BF16).float().to(gpu).contiguous()      # bf16 weights / sqrt(K)
    wf, sf, wt, st = ops.pack_weights_mx(w, Co, k * k, Ci)
    x8, sx = ops.mx_quantize(x)
    return x8, sx, wf, sf, wt, st, ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)


@pytest.mark.parametrize('case,build', GAUSS, ids=['x'.join(str(v) for v in c[0]) for c in GAUSS])
def test_fused_copy_of_gaussian_outputs_is_the_quantiser_s(gpu, case, build):
    """Gaussian activations, bf16 weights / sqrt(K), random bias, one case per build (and the four-phase transposed form): (y8, sy)
    equals mx_quantize_ref(y) of the same launch's y bit for bit -- every exponent and every mantissa rounding of the rule --
    and y is bit-identical whether or not the copy is requested."""
    ops = _ops()
    N, H, W, Ci, Co, k, s, p = case
    x8, sx, wf, sf, wt, st, desc = _gauss(ops, gpu, case, 9300)
    bias = (randn(9303, Co) * 0.5).to(gpu)
    res = _nhwc(randn(9304, N, Co, desc.Ho, desc.Wo).to(gpu).to(BF16))
    for relu in (False, True):
        (y, y8, sy), labels = _run(ops, lambda: ops.conv_fwd_mx_act(desc, x8, sx, wf, sf, bias, res, relu=relu, want_copy=True))
        _check_build('gauss fwd', labels, 'mx %s epi3' % build)
        _check_copy('gauss fwd relu=%d' % relu, y, y8, sy)
        y0 = ops.conv_fwd_mx_act(desc, x8, sx, wf, sf, bias, res, relu=relu)
        assert torch.equal(y0.view(torch.int16), y.view(torch.int16))
        assert float(y.float().abs().max()) > 0.5 and torch.isfinite(y.float()).all()
    if k == 4:            # the transposed conv's forward: dy = an MX copy at the small resolution, every stride-2 phase
        dy = _nhwc(randn(9305, N, Co, desc.Ho, desc.Wo).to(gpu).to(BF16))
        dy8, sdy = ops.mx_quantize(dy)
        bias_i = (randn(9306, Ci) * 0.5).to(gpu)
        dx, dx8, sdx = ops.conv_dgrad_mx_act(desc, dy8, sdy, wt, st, bias_i, relu=True, want_copy=True)
        _check_copy('gauss dgrad', dx, dx8, sdx)
        assert torch.equal(ops.conv_dgrad_mx_act(desc, dy8, sdy, wt, st, bias_i, relu=True).view(torch.int16), dx.view(torch.int16))


def test_fused_copy_of_a_block_relu_zeroed_by_its_bias(gpu):
    """A bias of -1e4 on channels 32 .. 63 under ReLU: that block of every pixel is all zero -- scale byte 0x00, elements zero --
    while its neighbours keep their own scales."""
    ops = _ops()
    case = (2, 8, 8, 128, 128, 3, 1, 1)
    x8, sx, wf, sf, _, _, desc = _gauss(ops, gpu, case, 9320)
    bias = (randn(9323, 128) * 0.5)
    bias[32:64] = -1e4
    y, y8, sy = ops.conv_fwd_mx_act(desc, x8, sx, wf, sf, bias.to(gpu), relu=True, want_copy=True)
    _check_copy('zero block', y, y8, sy)
    s, q = sy.view(-1, 4).cpu(), _rows(y8)
    assert int(s[:, 1].max()) == 0 and int(q[:, 32:64].max()) == 0 and float(_rows(y)[:, 32:64].float().abs().max()) == 0.0
    assert int(s[:, 0].min()) > 0 and int(s[:, 2].min()) > 0


# ---------------------------------------------------------------- 3. against the two-launch entry points
@pytest.mark.parametrize('case', [(3, 9, 11, 128, 64, 3, 1, 1), (2, 16, 16, 128, 256, 4, 2, 1), (5, 60, 60, 128, 128, 3, 1, 1)],
                         ids=lambda c: 'x'.join(str(v) for v in c))
def test_without_relu_the_bits_are_those_of_the_mx_entry_points(gpu, case):
    ops = _ops()
    N, H, W, Ci, Co, k, s, p = case
    x8, sx, wf, sf, wt, st, desc = _gauss(ops, gpu, case, 9340)
    bias = (randn(9343, Co) * 0.5).to(gpu)
    res = _nhwc(randn(9344, N, Co, desc.Ho, desc.Wo).to(gpu).to(BF16))
    for r in (None, res):
        a = ops.conv_fwd_mx_act(desc, x8, sx, wf, sf, bias, r, relu=False)
        b = ops.conv_fwd_mx(desc, x8, sx, wf, sf, bias, residual=r)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    if Co % 128 == 0:
        dy8, sdy = ops.mx_quantize(_nhwc(randn(9345, N, Co, desc.Ho, desc.Wo).to(gpu).to(BF16)))
        b = ops.conv_dgrad_mx(desc, dy8, sdy, wt, st)
        for bias_i in (None, torch.zeros(Ci, device=gpu)):
            a = ops.conv_dgrad_mx_act(desc, dy8, sdy, wt, st, bias_i, relu=False)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------- 4. loud argument checks
def test_act_argument_checks_are_loud_and_touch_nothing(gpu):
    mi355, ops = _mi(), _ops()
    u8 = lambda n, v=0: torch.full((n,), v, dtype=torch.uint8, device=gpu)
    D = ctypes.byref

    def outputs(C):
        return (torch.full((64 * C,), 7.0, dtype=BF16, device=gpu), u8(64 * C, 0xAB), u8(64 * C // 32 + 1, 0xCD))

    def untouched(y, y8, sy):
        torch.cuda.synchronize()
        assert float(y.float().min()) == 7.0 == float(y.float().max()) and int(y8.min()) == 0xAB == int(y8.max()) and \
            int(sy.min()) == 0xCD == int(sy.max())

    x8, sx, w8, sw, bias = u8(64 * 128), u8(64 * 4), u8(128 * 9 * 128), u8(128 * 9 * 4), torch.zeros(128, device=gpu)
    desc = ops.make_desc_fp8(1, 8, 8, 128, 128, 3, 3, 1, 1)
    y, y8, sy = outputs(128)
    st = mi355.stream_ptr()
    with pytest.raises(mi355.Mi355Error, match='both'):                   # y8 without sy
        mi355.call('mi355_conv_fwd_mx_act', D(desc), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 0, 1,
                   y.data_ptr(), y8.data_ptr(), 0, st)
    with pytest.raises(mi355.Mi355Error, match='both'):                   # sy without y8
        mi355.call('mi355_conv_fwd_mx_act', D(desc), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 0, 1,
                   y.data_ptr(), 0, sy.data_ptr(), st)
    with pytest.raises(mi355.Mi355Error, match='null'):                   # null y
        mi355.call('mi355_conv_fwd_mx_act', D(desc), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 0, 1,
                   0, y8.data_ptr(), sy.data_ptr(), st)
    with pytest.raises(mi355.Mi355Error, match='both'):                   # the dgrad form: dx8 without sdx
        mi355.call('mi355_conv_dgrad_mx_act', D(desc), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 1,
                   y.data_ptr(), y8.data_ptr(), 0, st)
    with pytest.raises(mi355.Mi355Error, match='null'):
        mi355.call('mi355_conv_dgrad_mx_act', D(desc), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 1,
                   0, 0, 0, st)
    untouched(y, y8, sy)
    desc72 = ops.make_desc_fp8(1, 8, 8, 128, 72, 3, 3, 1, 1)              # Co % 32 != 0 with a copy requested
    y, y8, sy = outputs(72)
    with pytest.raises(mi355.Mi355Error, match='multiple of 32'):
        mi355.call('mi355_conv_fwd_mx_act', D(desc72), x8.data_ptr(), sx.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), 0, 0,
                   y.data_ptr(), y8.data_ptr(), sy.data_ptr(), st)
    with pytest.raises(mi355.Mi355Error, match='multiple of 32'):
        ops.conv_fwd_mx_act(desc72, x8, sx, w8, sw, bias, want_copy=True, out=y.view(1, 8, 8, 72).permute(0, 3, 1, 2))
    untouched(y, y8, sy)
    with pytest.raises(mi355.Mi355Error, match='out_scales'):             # the wrappers' room checks
        ops.conv_fwd_mx_act(desc, x8, sx, w8, sw, bias, out_scales=u8(64 * 4 - 1))
    with pytest.raises(mi355.Mi355Error, match='sdy'):
        ops.conv_dgrad_mx_act(desc, x8, u8(64 * 4 - 1), w8, sw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. layers
def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _abi_folded(ops, conv, bn, x, deconv, relu=True):
    """the ABI call on operands folded and packed here, independently of mi355.nn's cache"""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.float() * scale
    if conv.bias is not None:
        shift = shift + conv.bias.detach().float() * scale
    wm = conv.weight.detach().permute(0, 2, 3, 1)
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    N, C, H, W = x.shape
    x8, sx = ops.mx_quantize(x)
    if deconv:
        wm = (wm * scale.view(1, 1, 1, -1)).contiguous()
        _, _, wt, st = ops.pack_weights_mx(wm, conv.in_channels, k * k, conv.out_channels)
        desc = ops.make_desc_fp8(N, (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k, conv.out_channels, conv.in_channels, k, k, s, p)
        return ops.conv_dgrad_mx_act(desc, x8, sx, wt, st, shift.contiguous(), relu=relu)
    wm = (wm * scale.view(-1, 1, 1, 1)).contiguous()
    wf, sf, _, _ = ops.pack_weights_mx(wm, conv.out_channels, k * k, conv.in_channels)
    desc = ops.make_desc_fp8(N, H, W, C, conv.out_channels, k, k, s, p)
    return ops.conv_fwd_mx_act(desc, x8, sx, wf, sf, shift.contiguous(), relu=relu)


@pytest.mark.parametrize('kind,k,s,p', [('conv', 3, 1, 1), ('conv', 3, 2, 1), ('deconv', 4, 2, 1)])
def test_mx_eval_layers_match_the_abi_and_track_the_bf16_layers(gpu, mx_eval, kind, k, s, p):
    """conv / transposed conv + BatchNorm + ReLU in eval mode under no-grad with the switch on: the bits of the ABI call on the
    folded and packed operands, within 8e-2 relative L2 of the folded bf16 launch (test_mxfp8_layers_track_the_bf16_layers'
    bound).  The folded MX pack follows an in-place weight edit, a load_state_dict and a train-mode forward that moves the
    running statistics."""
    from mi355.nn import Conv2d, ConvTranspose2d, BatchNorm2d, ReLU, FusedSequential
    mi355, ops = mx_eval, _ops()
    conv = Conv2d(256, 256, k, s, p, bias=(s == 1)) if kind == 'conv' else ConvTranspose2d(256, 256, k, s, p)
    seq = FusedSequential(conv, BatchNorm2d(256), ReLU()).to(gpu)
    fill_module_(seq, 9400)
    sd0 = {n: v.clone() for n, v in seq.state_dict().items()}
    seq.eval()
    x = _nhwc(randn(9401, 4, 256, 16, 16).to(gpu).to(BF16))

    def run(on):
        mi355.set_mx_eval(on)
        with torch.no_grad():
            return seq(x).clone()

    y_bf, y_mx = run(False), run(True)
    assert torch.equal(y_mx.view(torch.int16), _abi_folded(ops, seq[0], seq[1], x, kind == 'deconv').view(torch.int16))
    e = _rel(y_mx.float(), y_bf.float())
    print('%s k%d s%d eval: relative L2 MX vs folded bf16 %.4f' % (kind, k, s, e))
    assert 1e-3 < e <= 8e-2, e                                    # > 1e-3: the MX path really ran
    with torch.no_grad():                                         # in-place edit: 2w folds to the same elements, every scale one higher
        seq[0].weight.mul_(2.0)
    y2 = run(True)
    assert torch.equal(y2.view(torch.int16), _abi_folded(ops, seq[0], seq[1], x, kind == 'deconv').view(torch.int16))
    assert not torch.equal(y2, y_mx)
    seq.load_state_dict(sd0)
    assert torch.equal(run(True), y_mx)
    seq.train()                                                   # a train-mode forward moves the running statistics
    mi355.set_mx_eval(False)
    seq(x * 3 + 1)
    seq.eval()
    y3 = run(True)
    assert not torch.equal(y3, y_mx)
    assert torch.equal(y3.view(torch.int16), _abi_folded(ops, seq[0], seq[1], x, kind == 'deconv').view(torch.int16))
    assert sorted(seq.state_dict()) == sorted(sd0)


# ---------------------------------------------------------------- 6, 8, 9. the pose network
@pytest.fixture(scope='module')
def r50(gpu):
    from test_gpu_model import _g8_setup
    mi355 = _mi()
    mi355.set_compute_dtype('bf16')
    m = _g8_setup(gpu, 'resnet50', 811)
    x = randn(813, 2, 3, 256, 256).to(gpu)
    m.train()
    with torch.no_grad():
        m(x)
    m.eval()
    return m, x


def _eval(m, x):
    with torch.no_grad():
        y = m(x)
    return (y[0] if isinstance(y, (tuple, list)) else y).float().clone()


def test_chain_issues_no_standalone_quantise_behind_an_mx_producer(gpu, mx_eval, r50, monkeypatch):
    """Eval forward of the ResNet-50 pose network (B=2, 256x256) with the switch on: ops.mx_quantize runs exactly once per MX layer
    whose producer is not an MX layer -- the backbone's eligible 3x3 convs (fed by bf16 1x1 convs) and the first transposed conv
    -- and the second and third transposed convs and the head's 3x3 conv find the copy their producer wrote on their input."""
    from mi355 import ops
    from mi355.nn import Conv2d
    m, x = r50
    calls = []
    real = ops.mx_quantize
    monkeypatch.setattr(ops, 'mx_quantize', lambda t, *a, **kw: (calls.append(tuple(t.shape)), real(t, *a, **kw))[1])
    fed = {}
    hooks = [mod.register_forward_pre_hook(lambda mod_, args, name=name: fed.__setitem__(name, getattr(args[0], '_mi_mx', None) is not None))
             for name, mod in (('up3', m.upsampling[3]), ('up6', m.upsampling[6]), ('head0', m.head[0]), ('up0', m.upsampling[0]))]
    mx_eval.set_mx_eval(True)
    try:
        y = _eval(m, x)
    finally:
        for h in hooks:
            h.remove()
    backbone = [c for c in m.backbone.modules() if isinstance(c, Conv2d) and c.bn_follows and c._mx_layer_ok()]
    assert len(backbone) == 13 and all(c.kernel_size[0] == 3 for c in backbone)      # conv2 of layer2 (4), layer3 (6), layer4 (3)
    print('stand-alone quantise launches: %d %s' % (len(calls), calls))
    assert len(calls) == len(backbone) + 1
    assert calls[-1] == (2, 2048, 8, 8)                                               # the first transposed conv's input
    assert fed == {'up0': False, 'up3': True, 'up6': True, 'head0': True}
    assert torch.isfinite(y).all()


def test_switch_off_is_the_folded_bf16_path(gpu, mx_eval, r50):
    m, x = r50
    mi355 = mx_eval
    mi355.set_mx_eval(False)
    outs = {}
    for dt in ('bf16', 'mxfp8'):
        mi355.set_compute_dtype(dt)
        outs[dt] = _eval(m, x)
    assert torch.equal(outs['bf16'], outs['mxfp8'])
    mi355.set_compute_dtype('bf16')
    mi355.set_mx_eval(True)
    on = _eval(m, x)
    assert not torch.equal(on, outs['bf16']) and torch.isfinite(on).all()
    mi355.set_mx_eval(False)
    assert torch.equal(_eval(m, x), outs['bf16'])                  # and back: nothing of the MX path lingers


def test_graph_replay_with_the_switch_on_and_after_flipping_it(gpu, mx_eval, r50):
    """GraphedForward replay with the switch on is bit-identical to eager; flipping the switch drops the graphs, and the next
    output is the other setting's eager output."""
    from mi355.infer import GraphedForward
    m, x = r50
    mi355 = mx_eval
    mi355.set_mx_eval(False)
    eager_off = _eval(m, x)
    mi355.set_mx_eval(True)
    eager_on = _eval(m, x)
    gf = GraphedForward(m, warmup=1)
    with torch.no_grad():
        ys = [gf(x).float().clone() for _ in range(3)]            # eager warm-up, capture + replay, replay
        assert len(gf._graphs) == 1
        assert all(torch.equal(y, eager_on) for y in ys)
        mi355.set_mx_eval(False)
        y_off = gf(x).float().clone()
        assert len(gf._graphs) == 0                               # dropped: this call was a warm-up of the other setting
        assert torch.equal(y_off, eager_off) and not torch.equal(eager_off, eager_on)
        assert torch.equal(gf(x).float(), eager_off) and len(gf._graphs) == 1
        mi355.set_mx_eval(True)
        assert torch.equal(gf(x).float(), eager_on)


# ---------------------------------------------------------------- 7, 10. ResNet-101 against the fp32 reference
@pytest.fixture(scope='module')
def r101_maps(gpu):
    """heat-maps of golden G8's ResNet-101 (B=2, 256x256; one train-mode fp32 forward first, as the golden's eval output
    follows one) in eval mode: folded bf16 and MX eval, computed once"""
    from test_gpu_model import _g8_setup
    mi355 = _mi()
    x = randn(812, 2, 3, 256, 256).to(gpu)
    mi355.set_compute_dtype('f32')
    m = _g8_setup(gpu, 'resnet101', 811)
    m.train()
    with torch.no_grad():
        m(x)
    mi355.set_compute_dtype('bf16')
    m.eval()
    out = {}
    try:
        for name, on in (('bf16', False), ('mx', True)):
            mi355.set_mx_eval(on)
            out[name] = _eval(m, x).cpu()
    finally:
        mi355.set_mx_eval(False)
    return out


def test_resnet101_mx_eval_vs_the_fp32_reference(gpu, r101_maps):
    """The construction of test_fp8_resnet101_forward_and_resnet50_iteration_vs_reference: relative L2 of the eval heat-maps against
    the reference's own classes in fp32 (golden g8_bottleneck / r101_y_eval): bf16 <= 1e-2, MX eval <= 6e-2 -- the bound the
    project holds per-tensor fp8 inference to (measured 0.021 there)."""
    from conftest import golden
    ref = torch.from_numpy(golden('g8_bottleneck')['r101_y_eval'])
    e_bf, e_mx = _rel(r101_maps['bf16'][:, ::5], ref), _rel(r101_maps['mx'][:, ::5], ref)
    print('eval heat-maps vs the fp32 reference, relative L2: bf16 %.4f, MX eval %.4f' % (e_bf, e_mx))
    assert e_bf <= 1e-2, e_bf
    assert e_mx <= 6e-2, e_mx
    assert not torch.equal(r101_maps['bf16'], r101_maps['mx'])


def _argmax_xy(h):
    idx = h.flatten(2).argmax(-1)
    return torch.stack([idx % h.shape[3], idx // h.shape[3]], -1)


def test_resnet101_argmax_agreement(gpu, r101_maps):
    """Key-point coordinates (argmax of each heat-map) of the MX-eval maps against the folded-bf16 maps, on the ten maps the golden
    holds (channels ::5 of two images); the share that agrees is printed.

    The cap on disagreement is derived from the fp32 oracle alone.  This random-initialised fixture has flat maps (mean 0.41,
    standard deviation 0.04 on the second channel) whose two highest pixels lie 0.0004 .. 0.007 apart, often 16 and more pixels from
    each other, so an argmax is only pinned for a key point whose top-1 / top-2 margin exceeds twice the pointwise error a map
    may carry.  Test 7 admits a relative L2 error of 6e-2, i.e. (spread evenly) an rms pointwise error of 6e-2 * rms(map): key points
    with a smaller margin may move, the others may not, and the cap is the share of the former (9 of 10 on this fixture -- the
    fixture pins one key point at that error level, and 4 of 10 at the 1e-2 bound of the bf16 path).
    Basis, checked on the CPU before the cap was chosen: the oracle rounded to bf16 against the oracle itself moves none of the
    ten key points (two of them become exact ties of their maximum, resolved by position), which is within this cap and within
    the tighter one at 1e-2.  The same check is asserted below."""
    from conftest import golden
    ref = torch.from_numpy(golden('g8_bottleneck')['r101_y_eval'])
    top = ref.flatten(2).topk(2, -1).values
    margin = top[..., 0] - top[..., 1]
    rms = ref.flatten(2).pow(2).mean(-1).sqrt()                  # per map
    cap = float((margin < 2 * 6e-2 * rms).float().mean())
    basis = float((_argmax_xy(ref.to(BF16).float()) != _argmax_xy(ref)).any(-1).float().mean())
    assert basis <= cap and basis <= float((margin < 2 * 1e-2 * rms).float().mean())
    a, b = _argmax_xy(r101_maps['mx'][:, ::5]), _argmax_xy(r101_maps['bf16'][:, ::5])
    agree = float((a == b).all(-1).float().mean())
    full = float((_argmax_xy(r101_maps['mx']) == _argmax_xy(r101_maps['bf16'])).all(-1).float().mean())
    vs_ref = float((a == _argmax_xy(ref)).all(-1).float().mean())
    print('argmax agreement MX eval vs folded bf16: %.2f of the 10 golden key points (cap on disagreement %.2f), %.2f of all 42; '
          'MX eval vs the fp32 oracle %.2f' % (agree, cap, full, vs_ref))
    assert 1.0 - agree <= cap, (agree, cap)
