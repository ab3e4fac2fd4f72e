"""The glue of mi355.nn -- autograd Functions and address-keyed hand-off tables -- on whole composites: the stem, BasicBlock and
Bottleneck (identity and downsample), a two-block stage, the transposed-conv neck and the four heads.  Every kernel below is held
bit for bit by the exact suites; here the host code that wires them together is held to two references of tests/block_ref.py.

Every compared tensor carries one of three kinds:
  [equal]   nn vs Plain (the same kernels called one by one by straightforward host code) in the same compute dtype, torch.equal
  [bound]   weight gradients formed inside `with mi355.grouped_wgrads():` vs their float64 value, forward error bound of the sum
  [anchor]  nn in f32 mode vs T64 (torch autograd, float64, CPU), max|err| <= 3 e_cpu + 1e-4 max|ref|

Which fused path each test pins:
  test_composite_equals_plain[*-default]        _ConvSkipFn (fork sum in conv1's dgrad epilogue), _LAZY_MASK (identity: masked
                                                accumulate; downsample: BatchNorm backward with relu_mask=lazy), statistics partials
                                                (_take_partial), _BnReluPoolFn and the folded / padded stem, _DeconvFn
  ...[*-_LAZY_RES]                              the last BatchNorm writes a masked dres of its own
  ...[*-_SKIP_FUSE]                             the fork sum as autograd's add; the lazy mask settled by _as_grad / downsample BN
  ...[*-_RELU_BITMASK], [*-_MASK_FROM_Y]        y kept instead of the bit mask / for every ReLU mask
  ...[*-_FUSE_STATS]                            stand-alone statistics passes
  ...[*-_FUSE_BNBWD]                            _BWD_PARTIALS: sums handed from a dgrad epilogue to the BatchNorm backward
  ...[*-_BN_POOL_FUSE], [*-_STEM_S2D]           the stem's three separate layers / its padded form at even extents
  test_grouped_weight_gradients_within_bound    mi355.grouped_wgrads (deferred weight gradients, the path da_step takes)
  test_composite_against_float64                all of the above end to end, element by element
  test_heads_against_float64                    _ConvCatFn, _claim_gl (lambda in the dgrad epilogue), GradFanIn, _BN_DX / _bias_grad

Call forms Plain does NOT borrow from the glue: it forms the fork sum with ops.conv_dgrad(out=dres, accumulate=True) onto the
separate masked dres of ops.bn_bwd(want_dres=True), where the glue calls ops.conv_dgrad_masked_acc on the unmasked gradient or hands
the bit mask to the downsample BatchNorm's backward; it runs BatchNorm + ReLU and the max-pool as two kernels.
Call forms it borrows (block_ref.Choices), each pinned by an exact suite:
  the source of a BatchNorm backward's ReLU mask (recomputed from x / bit mask / y): it selects the one-launch or the three-launch
      form of mi355_bn_bwd, whose sums run in another order -- tests/test_gpu_bn_exact.py::test_backward_bit_for_bit (mask sources
      0 - 3 in both forms) and ::test_forward_apply_eval_and_mask_bits (the bits the forward writes)
  statistics from the conv epilogue, sums for the BatchNorm backward from the dgrad epilogue, accumulate in the dgrad epilogue --
      tests/test_gpu_conv_exact.py::test_conv_builds_return_the_reference_bits (fwd+stats, dgrad+stats, conv_dgrad_bnbwd,
      dgrad*scale+acc) and tests/test_gpu_bn_exact.py::test_forward_from_crafted_partials / ::test_backward_from_crafted_partials

Each composite runs at an even and an odd extent, and twice on one module instance with new inputs (a stale hand-off entry of step
1 would be consumed in step 2).  After every backward the four hand-off tables must be empty."""
import contextlib

import pytest
import torch
import torch.nn as nn

import block_ref as R
from seeded import fill_module_, randn

pytestmark = pytest.mark.gpu

DT = R.DT
SWITCHES = ['default', '_LAZY_RES', '_SKIP_FUSE', '_RELU_BITMASK', '_MASK_FROM_Y', '_FUSE_STATS', '_FUSE_BNBWD', '_BN_POOL_FUSE', '_STEM_S2D']


@pytest.fixture
def rt(gpu):
    import mi355
    mi355.load()
    mi355.set_compute_dtype('bf16')
    yield mi355
    mi355.set_compute_dtype('bf16')


@contextlib.contextmanager
def _flipped(name):
    """One A/B switch of mi355.nn assigned for the duration (never through the environment), restored in `finally`."""
    from mi355 import nn as mnn
    if name == 'default':
        yield
        return
    old = getattr(mnn, name)
    setattr(mnn, name, not old)
    try:
        yield
    finally:
        setattr(mnn, name, old)


def _choices(what, even):
    """The structural arguments of Plain that match the switches as they stand now (read here, never by Plain)."""
    from mi355 import nn as mnn
    from_y = mnn._MASK_FROM_Y
    if what == 'stem':            # the fused BatchNorm + ReLU + max-pool pass keeps no y: its backward always recomputes the mask
        from_y = from_y and not (mnn._BN_POOL_FUSE and mnn._FUSE_STATS)
    return R.Choices(stats='epilogue' if mnn._FUSE_STATS else 'pass', fork='epilogue' if mnn._SKIP_FUSE else 'add',
                     stem='folded' if (mnn._STEM_S2D and even) else 'padded', bnbwd=mnn._FUSE_BNBWD, mask='y' if from_y else 'x',
                     mask_res='y' if (from_y or mnn._FUSE_BNBWD or not mnn._RELU_BITMASK) else 'bits')


def _tables():
    import mi355
    from mi355 import nn as mnn
    return {'_LAZY_MASK': len(mnn._LAZY_MASK), '_BWD_PARTIALS': len(mnn._BWD_PARTIALS), '_BN_DX': len(mnn._BN_DX),
            'grouped-wgrad list': len(mi355._group_items)}


# ---------------------------------------------------------------- composites
class _Stem(nn.Module):
    """conv1 7x7 s2 -> bn1.forward_relu_maxpool, as ResNet.forward runs it"""

    def __init__(self):
        super().__init__()
        from mi355 import nn as mnn
        self.conv1 = mnn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = mnn.BatchNorm2d(64)
        self.relu = mnn.ReLU(inplace=True)
        self.maxpool = mnn.MaxPool2d(3, 2, 1)
        mnn.link_conv_bn(self)

    def forward(self, x):
        return self.bn1.forward_relu_maxpool(self.conv1(x), self.maxpool)


def _down(cin, cout, stride):
    from mi355 import nn as mnn
    return mnn.FusedSequential(mnn.Conv2d(cin, cout, 1, stride, 0, bias=False), mnn.BatchNorm2d(cout))


BLOCK_SHAPES = [(3, 12, 12), (3, 9, 7)]
# name -> (builder, input channels, 'block' | 'stage' | 'stem' | 'neck', [(N, H, W)])
COMPOSITES = {
    'basic-id': (lambda B, K: B(64, 64), 64, 'block', BLOCK_SHAPES),
    'basic-down2': (lambda B, K: B(64, 128, 2, _down(64, 128, 2)), 64, 'block', BLOCK_SHAPES),
    'bottleneck-id': (lambda B, K: K(128, 32), 128, 'block', BLOCK_SHAPES),
    'bottleneck-down1': (lambda B, K: K(64, 32, 1, _down(64, 128, 1)), 64, 'block', BLOCK_SHAPES),
    'bottleneck-down2': (lambda B, K: K(128, 64, 2, _down(128, 256, 2)), 128, 'block', BLOCK_SHAPES),
    # as ResNet._make_layer builds a stage: downsample block, then identity block
    'stage-basic': (lambda B, K: nn.Sequential(B(64, 128, 2, _down(64, 128, 2)), B(128, 128)), 64, 'stage', BLOCK_SHAPES),
    'stage-bottleneck': (lambda B, K: nn.Sequential(K(128, 64, 2, _down(128, 256, 2)), K(256, 64)), 128, 'stage', BLOCK_SHAPES),
    'stem': (lambda B, K: _Stem(), 3, 'stem', [(2, 32, 32), (2, 31, 33)]),
    'neck': (None, 256, 'neck', [(2, 4, 4), (2, 3, 5)]),
}


def _build(name, gpu, seed):
    from uda.model.resnet import BasicBlock, Bottleneck
    from uda.model.pose_resnet2 import Upsampling
    mk, cin, what, shapes = COMPOSITES[name]
    mod = Upsampling(256, (256, 256), (4, 4)) if what == 'neck' else mk(BasicBlock, Bottleneck)
    fill_module_(mod, seed)
    return mod.to(gpu).train(), cin, what, shapes


def _inputs(what, dt, seed, N, C, H, W, gpu):
    """operands rounded to the compute dtype first: (x for the module, the same values on the CPU in float32)"""
    x32 = randn(seed, N, C, H, W).to(DT[dt]).float()
    if what == 'stem':                                   # an NCHW fp32 image; its gradient is never formed
        return x32.to(gpu), x32
    x = x32.to(gpu).to(DT[dt]).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    return x, x32


def _dy_like(y, dt, seed, gpu):
    d32 = randn(seed, *y.shape).to(DT[dt]).float()
    return d32.to(gpu).to(DT[dt]).contiguous(memory_format=torch.channels_last), d32


def _nn_step(mod, x, dt, dy_seed, gpu, grouped=False):
    """forward + backward of the module under test; every gradient slot NaN-filled first, so a skipped write shows.
    -> (y, dx, dy, the values of dy on the CPU)"""
    import mi355
    from mi355.nn import mark_grads_fresh
    ps = [p for p in mod.parameters() if p.grad is not None]
    for p in ps:
        p.grad.fill_(R.NAN)
    mark_grads_fresh(ps)
    if x.requires_grad:
        x.grad = None
    with (mi355.grouped_wgrads() if grouped else contextlib.nullcontext()):
        y = mod(x)
        dy, dy32 = _dy_like(y, dt, dy_seed, gpu)
        y.backward(dy.clone())            # (the fork accumulates in place onto the gradient it is handed)
    return y.detach(), (x.grad if x.requires_grad else None), dy, dy32


def _plain_step(mod, what, bufs, dt, choices, x, dy):
    P = R.plain(bufs, DT[dt], choices)
    x, dy = x.detach(), dy.clone()
    if what == 'block':
        y = P.block_f('', mod, x)
        dx, _ = P.block_b('', mod, dy)
    elif what == 'stage':
        y = P.stage_f('', mod, x)
        dx = P.stage_b('', mod, dy)
    elif what == 'stem':
        y = P.stem_f('', mod, x)
        dx = P.stem_b('', mod, dy)
    else:
        y = P.neck_f('', mod, x)
        dx = P.neck_b('', mod, dy)
    return P, y, dx


def _same(bad, what, got, ref):
    if got is None or ref is None or got.shape != ref.shape or not torch.equal(got, ref):
        n = -1 if (got is None or ref is None or got.shape != ref.shape) else int((got != ref).sum())
        bad.append('%s (%d elements differ)' % (what, n))


def _compare_equal(bad, tag, mod, P, bufs, y, y_p, dx, dx_p, weights=True):
    _same(bad, tag + ' output', y, y_p)                                                   # [equal]
    if dx_p is not None:
        _same(bad, tag + ' input gradient', dx, dx_p)                                     # [equal]
    for k, p in mod.named_parameters():
        if p.dim() == 4:
            if weights:
                _same(bad, tag + ' gradient of ' + k, p.grad.permute(0, 2, 3, 1), P.g[k])  # [equal] weight gradients
        else:
            _same(bad, tag + ' gradient of ' + k, p.grad, P.g[k])                         # [equal] dgamma / dbeta
    sd = mod.state_dict()
    for k, b in bufs.items():
        _same(bad, tag + ' ' + k, sd[k], b)                                               # [equal] running statistics, counter


def _empty_tables(bad, tag):
    for k, n in _tables().items():
        if n:
            bad.append('%s: %d entries left in %s after the backward' % (tag, n, k))
    from mi355.nn import mark_grads_fresh
    mark_grads_fresh([])                   # (a left-over entry is reported once, not again by every later step)


@pytest.mark.parametrize('switch', SWITCHES)
@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('name', sorted(COMPOSITES))
def test_composite_equals_plain(rt, gpu, name, dt, switch):
    rt.set_compute_dtype(dt)
    bad = []
    with _flipped(switch):
        for si, (N, H, W) in enumerate(COMPOSITES[name][3]):
            mod, cin, what, _ = _build(name, gpu, 40 + si)           # (the stem reads _STEM_S2D when it is constructed)
            choices = _choices(what, H % 2 == 0 and W % 2 == 0)
            for step in (1, 2):                                      # twice on one module instance, new inputs
                tag = '%s %s %s %dx%dx%d step %d:' % (name, dt, switch, N, H, W, step)
                x, _ = _inputs(what, dt, 500 + 10 * si + step, N, cin, H, W, gpu)
                bufs = R.snapshot(mod)
                y, dx, dy, _ = _nn_step(mod, x, dt, 700 + 10 * si + step, gpu)
                _empty_tables(bad, tag)
                P, y_p, dx_p = _plain_step(mod, what, bufs, dt, choices, x, dy)
                _compare_equal(bad, tag, mod, P, bufs, y, y_p, dx, dx_p)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['stage-basic', 'stage-bottleneck'])
def test_identity_gradient_is_masked_when_the_fork_is_an_autograd_add(rt, gpu, name):
    """Found by test_composite_equals_plain[stage-*-_SKIP_FUSE]: with the fork sum left to autograd, the second block's residual
    is the first block's output, whose grad_fn is a _BnFnBackward like a downsample BatchNorm's.  The last BatchNorm took that for
    a consumer that applies the bit mask and handed its dy on unmasked; the autograd add knows nothing of the mask, so the
    identity-branch gradient reached the first block without the ReLU mask and the _LAZY_MASK entry stayed behind.  Now only a
    BatchNorm without ReLU (the downsample one) or conv1's alias qualifies.  The step twice on the same operands: the same bits."""
    bad, runs = [], []
    with _flipped('_SKIP_FUSE'):
        N, H, W = COMPOSITES[name][3][1]
        for _ in range(2):
            mod, cin, what, _ = _build(name, gpu, 41)
            x, _ = _inputs(what, 'bf16', 511, N, cin, H, W, gpu)
            bufs = R.snapshot(mod)
            y, dx, dy, _ = _nn_step(mod, x, 'bf16', 711, gpu)
            _empty_tables(bad, name)
            P, y_p, dx_p = _plain_step(mod, what, bufs, 'bf16', _choices(what, False), x, dy)
            _compare_equal(bad, name, mod, P, bufs, y, y_p, dx, dx_p)                      # [equal]
            runs.append([y, dx] + [p.grad.clone() for p in mod.parameters()])
    assert not bad, '\n'.join(bad)
    assert all(torch.equal(a, b) for a, b in zip(*runs))                                  # [equal] run after run


GROUPED = [n for n in sorted(COMPOSITES) if n != 'stem']      # (the stem's weight gradient is never deferred: its channels are padded)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('name', GROUPED)
def test_grouped_weight_gradients_within_bound(rt, gpu, name, dt):
    """Inside `with mi355.grouped_wgrads():` the weight gradients are collected and launched together by kernels that sum in
    another order: everything else stays [equal]; each weight gradient is held to the forward error bound of an fp32 sum of
    M = N*Ho*Wo products around its float64 value, formed from Plain's operands of that layer (bit-identical to nn's by the
    [equal] checks of the same step)."""
    rt.set_compute_dtype(dt)
    bad = []
    for si, (N, H, W) in enumerate(COMPOSITES[name][3]):
        mod, cin, what, _ = _build(name, gpu, 40 + si)
        choices = _choices(what, H % 2 == 0 and W % 2 == 0)
        for step in (1, 2):
            tag = '%s %s grouped %dx%dx%d step %d:' % (name, dt, N, H, W, step)
            x, _ = _inputs(what, dt, 500 + 10 * si + step, N, cin, H, W, gpu)
            bufs = R.snapshot(mod)
            y, dx, dy, _ = _nn_step(mod, x, dt, 700 + 10 * si + step, gpu, grouped=True)
            _empty_tables(bad, tag)
            P, y_p, dx_p = _plain_step(mod, what, bufs, dt, choices, x, dy)
            _compare_equal(bad, tag, mod, P, bufs, y, y_p, dx, dx_p, weights=False)
            for k, p in mod.named_parameters():
                if p.dim() != 4:
                    continue
                s = P.t[k[:-len('.weight')]]
                d = s['desc']
                ref = R.wgrad64(d, s['wx'], s['wdy'])
                sum_abs = R.wgrad_bound_terms(d, s['wx'], s['wdy'])
                # [bound] |dw - dw64| <= gamma_M * sum|x||dy| + one fp32 ulp of dw64, M = N*Ho*Wo, gamma_M = M u / (1 - M u), u = 2^-24:
                # derivation in block_ref.wgrad_bound (f32 operands add one rounding per product: M factors instead of M - 1)
                lim = R.wgrad_bound(d.N * d.Ho * d.Wo, sum_abs, ref)
                err = (p.grad.permute(0, 2, 3, 1).double() - ref).abs()
                worst = float((err / lim).max())
                print('%s %s: max err %.3g, max err / bound %.3g (M = %d)' % (tag, k, float(err.max()), worst, d.N * d.Ho * d.Wo))
                if not bool((err <= lim).all()):
                    bad.append('%s gradient of %s: %d elements beyond the bound, worst err / bound %.3g' % (tag, k, int((err > lim).sum()), worst))
    assert not bad, '\n'.join(bad)


def _t64_fwd(mod, what):
    if what == 'block':
        return lambda T, x: T.block('', mod, x)
    if what == 'stage':
        return lambda T, x: T.stage('', mod, x)
    if what == 'stem':
        return lambda T, x: T.stem('', mod, x)
    return lambda T, x: T.seq('', mod, x)


def _anchor(bad, tag, got, out64, out32):
    """[anchor] every tensor of `got` against float64: max|err| <= 3 e_cpu + 1e-4 max|ref|; -> worst err / max|ref|"""
    worst = 0.0
    for k, ref in out64.items():
        if k.endswith('num_batches_tracked'):
            if int(got[k]) != int(ref):
                bad.append('%s %s: %d, reference %d' % (tag, k, int(got[k]), int(ref)))
            continue
        e_cpu = R.anchor_err(out32[k], ref)
        err = R.anchor_err(got[k], ref)
        lim = R.anchor_bound(e_cpu, ref)
        scale = float(ref.abs().max())
        print('%s %s: e_cpu %.3g, err %.3g, bound %.3g, max|ref| %.3g' % (tag, k, e_cpu, err, lim, scale))
        if R.ANCHOR_REL * scale >= e_cpu:     # (not a gradient that is zero in exact arithmetic: rounding noise on either side)
            worst = max(worst, err / scale)
        if not err <= lim:
            bad.append('%s %s: max|err| %.4g > 3 * e_cpu (%.3g) + 1e-4 * max|ref| (%.3g)' % (tag, k, err, e_cpu, scale))
    return worst


def _collect(mod, ys, dxs):
    got = {}
    for i, y in enumerate(ys):
        got['y%d' % i] = y.float()
    for i, d in enumerate(dxs):
        if d is not None:
            got['dx%d' % i] = d.float()
    for k, p in mod.named_parameters():
        got['grad ' + k] = p.grad
    for k, b in R.snapshot(mod).items():
        got[k] = b
    return got


@pytest.mark.parametrize('name', sorted(COMPOSITES))
def test_composite_against_float64(rt, gpu, name):
    rt.set_compute_dtype('f32')
    bad, worst = [], 0.0
    for si, (N, H, W) in enumerate(COMPOSITES[name][3]):
        mod, cin, what, _ = _build(name, gpu, 40 + si)
        T64, T32 = R.T64(mod, torch.float64), R.T64(mod, torch.float32)
        fwd = _t64_fwd(mod, what)
        for step in (1, 2):
            tag = '%s f32 %dx%dx%d step %d:' % (name, N, H, W, step)
            x, x32 = _inputs(what, 'f32', 500 + 10 * si + step, N, cin, H, W, gpu)
            y, dx, dy, dy32 = _nn_step(mod, x, 'f32', 700 + 10 * si + step, gpu)
            _empty_tables(bad, tag)
            x32.requires_grad_(what != 'stem')
            _, out64 = R.run_t64(None, T64, fwd, [x32], [dy32])
            _, out32 = R.run_t64(None, T32, fwd, [x32], [dy32])
            worst = max(worst, _anchor(bad, tag, _collect(mod, [y], [dx]), out64, out32))
    print('%s: worst max|err| / max|ref| %.3g' % (name, worst))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('switch', ['default', '_ZERO_BN_BIAS_GRAD'])
def test_heads_against_float64(rt, gpu, switch):
    """f (a leaf carrying a GradFanIn) feeds the main head and, through the gradient layer, the three cascaded adversarial heads;
    one loss sums the four outputs against fixed gradients.  fp32 anchor only."""
    from mi355.nn import GradFanIn
    from uda.model.regda_7 import PoseResNetx9
    rt.set_compute_dtype('f32')
    bad, worst = [], 0.0
    with _flipped(switch):
        mod = PoseResNetx9(nn.Identity(), nn.Identity(), 256, 21)
        fill_module_(mod, 61)
        mod = mod.to(gpu).train()
        mod.gl_layer.iter_num = 300
        lam = mod.gl_layer.coeff
        T64, T32 = R.T64(mod, torch.float64), R.T64(mod, torch.float32)
        fwd = lambda T, f: T.heads(mod, f, lam)
        for step in (1, 2):
            tag = 'heads f32 %s step %d:' % (switch, step)
            f, f32 = _inputs('feat', 'f32', 900 + step, 2, 256, 16, 16, gpu)
            ps = [p for p in mod.parameters() if p.grad is not None]
            for p in ps:
                p.grad.fill_(R.NAN)
            from mi355.nn import mark_grads_fresh
            mark_grads_fresh(ps)
            f._mi_fan = GradFanIn()
            ys = (mod.head(f),) + tuple(mod.adv_heads(f))
            dys32 = [randn(950 + 10 * step + i, *y.shape) for i, y in enumerate(ys)]
            torch.autograd.backward(list(ys), [d.to(gpu) for d in dys32])
            _empty_tables(bad, tag)
            f32.requires_grad_(True)
            _, out64 = R.run_t64(None, T64, fwd, [f32], dys32)
            _, out32 = R.run_t64(None, T32, fwd, [f32], dys32)
            worst = max(worst, _anchor(bad, tag, _collect(mod, [y.detach() for y in ys], [f.grad]), out64, out32))
    print('heads %s: worst max|err| / max|ref| %.3g' % (switch, worst))
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------- NaN and Inf through the glue (tests/nonfinite_ref.py)
NONFINITE_COMPOSITES = ['basic-id', 'bottleneck-down1', 'stem']


def _nonfinite_step(mod, what, dt, x32, dy_of, gpu):
    """One forward + backward of the module under test and of its float64 torch twin on the same operands.  dy_of(y64) -> the
    float32 output gradient on the CPU, chosen after the float64 forward.  Gradient slots start from a finite sentinel: a
    skipped write would read as finite.  -> (got, out64): the compared tensors by name."""
    from mi355.nn import mark_grads_fresh
    T = R.T64(mod, torch.float64)
    T.params()
    x64 = x32.double().requires_grad_(what != 'stem')
    y64 = _t64_fwd(mod, what)(T, x64)
    dy32 = dy_of(y64.detach())
    y64.backward(dy32.double())
    out64 = {'y': y64.detach()}
    if what != 'stem':
        out64['dx'] = x64.grad.detach()
    for k, p in T.P.items():
        out64['grad ' + k] = p.grad.detach()
    if what == 'stem':
        x = x32.to(gpu)
    else:
        x = x32.to(gpu).to(DT[dt]).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ps = [p for p in mod.parameters() if p.grad is not None]
    for p in ps:
        p.grad.fill_(12345.0)
    mark_grads_fresh(ps)
    y = mod(x)
    y.backward(dy32.to(gpu).to(DT[dt]).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    got = {'y': y.detach().float()}
    if what != 'stem':
        got['dx'] = x.grad.float()
    for k, p in mod.named_parameters():
        got['grad ' + k] = p.grad
    return got, out64


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('name', NONFINITE_COMPOSITES)
def test_non_finite_values_reach_the_gradients_as_in_float64(rt, gpu, name, dt):
    """One +Inf in the input, then one NaN in the output gradient (where the last ReLU passes it), through the lazy ReLU mask and
    the gradient fan-in of mi355.nn: the output and the input gradient have the float64 torch block's class at EVERY element
    (pointwise rule), every parameter gradient is finite exactly where torch's is (reduced rule: dgamma / dbeta and weight
    gradients are sums).  With the NaN in one element of dy, torch keeps the last conv's weight gradient finite in every other
    output channel and the last BatchNorm's dgamma / dbeta finite in every other channel: so must the glue."""
    import nonfinite_ref as NF
    rt.set_compute_dtype(dt)
    N, H, W = COMPOSITES[name][3][-1]
    bad = []
    for case in ('+inf in x', 'nan in dy'):
        mod, cin, what, _ = _build(name, gpu, 43)
        _, x32 = _inputs(what, dt, 531, N, cin, H, W, gpu)
        x32 = x32.clone()
        if case == '+inf in x':
            x32[N - 1, cin - 1, H // 2, W // 2] = float('inf')

        def dy_of(y64):
            d = randn(731, *y64.shape).to(DT[dt]).float()
            if case == 'nan in dy':
                d.view(-1)[int(y64.reshape(-1).argmax())] = float('nan')          # the largest output: the ReLU (and the pool) pass it
            return d

        got, out64 = _nonfinite_step(mod, what, dt, x32, dy_of, gpu)
        _empty_tables(bad, '%s %s %s' % (name, dt, case))
        finite = {k: float(torch.isfinite(v).double().mean()) for k, v in out64.items()}
        print('%s %s %s: finite share in float64: %s' % (name, dt, case, '  '.join('%s %.3g' % kv for kv in sorted(finite.items()))))
        if case == 'nan in dy':          # the case must not be all-NaN: torch keeps most of the last layers' gradients finite
            assert bool(torch.isfinite(out64['y']).all()) and any(0.5 < f < 1.0 for k, f in finite.items() if k.startswith('grad '))
        else:
            assert not bool(torch.isfinite(out64['y']).all())
        for k, ref in out64.items():
            g = got[k].detach().cpu()
            g = g.permute(0, 3, 1, 2) if (k.startswith('grad ') and g.dim() == 4 and g.shape != ref.shape) else g
            if k in ('y', 'dx'):
                if not torch.equal(NF.classes(g), NF.classes(ref)):
                    bad.append('%s %s %s: %d elements of %s differ in class from float64' % (name, dt, case, int((NF.classes(g) != NF.classes(ref)).sum()), k))
            elif not torch.equal(torch.isfinite(g), torch.isfinite(ref)):
                bad.append('%s %s %s: %s is finite in %d elements, float64 in %d' % (name, dt, case, k, int(torch.isfinite(g).sum()), int(torch.isfinite(ref).sum())))
    assert not bad, '\n'.join(bad)
