"""What tests/test_gpu_blocks.py relies on, checked without a GPU:

  * the [anchor] yardstick: for every case of the GPU file, torch's own CPU float32 run of the float64 reference stays within
    1e-4 * max|ref| of it, so 3 * e_cpu never dominates the bound's floor;
  * the [bound] function holds for torch's CPU float32 weight gradients against float64;
  * seeded mistakes, each made in a copy of the float64 composite, fail the [anchor] comparison.
"""
import functools
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import block_ref as R
import test_gpu_blocks as G
from seeded import fill_module_, randn

CPU = torch.device('cpu')
CASES = [(n, si) for n in sorted(G.COMPOSITES) for si in range(len(G.COMPOSITES[n][3]))] + [('heads', 0)]


def _heads_module():
    from uda.model.regda_7 import PoseResNetx9
    mod = PoseResNetx9(nn.Identity(), nn.Identity(), 256, 21)
    fill_module_(mod, 61)
    mod.gl_layer.iter_num = 300
    return mod.train()


def _case_inputs(name, si, step, mod, what, cin):
    """the operands the GPU file gives this case at this step (same seeds), on the CPU: ([x], fwd -> output shapes -> [dy])"""
    if name == 'heads':
        _, f = G._inputs('feat', 'f32', 900 + step, 2, 256, 16, 16, CPU)
        return [f.requires_grad_(True)], lambda ys: [randn(950 + 10 * step + i, *y.shape) for i, y in enumerate(ys)]
    N, H, W = G.COMPOSITES[name][3][si]
    _, x = G._inputs(what, 'f32', 500 + 10 * si + step, N, cin, H, W, CPU)
    return [x.requires_grad_(what != 'stem')], lambda ys: [randn(700 + 10 * si + step, *ys[0].shape)]


def _run(T, fwd, xs, make_dys):
    """run_t64 with the output gradients made from the output shapes (one dry forward without gradients)"""
    with torch.no_grad():
        keep = {k: v.clone() for k, v in T.B.items()}
        T.params()
        ys = fwd(T, *[x.detach().to(T.dtype) for x in xs])
        ys = ys if isinstance(ys, (tuple, list)) else (ys,)
        for k, v in keep.items():
            T.B[k].copy_(v)
    return R.run_t64(None, T, fwd, xs, make_dys(ys))[1]


def _setup(name, si):
    if name == 'heads':
        mod = _heads_module()
        lam = mod.gl_layer.coeff
        return mod, 'heads', 256, (lambda T, f: T.heads(mod, f, lam))
    mod, cin, what, _ = G._build(name, CPU, 40 + si)
    return mod, what, cin, G._t64_fwd(mod, what)


@functools.lru_cache(maxsize=None)
def _reference(name, si):
    """[(out64, out32)] of the two steps of one case"""
    mod, what, cin, fwd = _setup(name, si)
    T64, T32 = R.T64(mod, torch.float64), R.T64(mod, torch.float32)
    steps = []
    for step in (1, 2):
        xs, dys = _case_inputs(name, si, step, mod, what, cin)
        steps.append((_run(T64, fwd, xs, dys), _run(T32, fwd, xs, dys)))
    return steps


def _exactly_zero(kinds, key):
    """Gradient of a conv bias whose output goes straight into a training-mode BatchNorm: zero in exact arithmetic (the sum over
    the batch of a BatchNorm input gradient), rounding noise in either precision.  Only the heads have conv biases: every one of
    them except the last 1x1 conv of a head (child 3 of a [conv, BN, ReLU, conv] stack) is followed by a BatchNorm."""
    if not (key.startswith('grad ') and key.endswith('.bias')):
        return False
    layer = key[len('grad '):-len('.bias')]
    return kinds[layer] == 'Conv2d' and not layer.endswith('.3')


@pytest.mark.parametrize('name,si', CASES, ids=['%s-%d' % c for c in CASES])
def test_anchor_yardstick_stays_below_the_floor(name, si):
    mod = _setup(name, si)[0]
    kinds = {k: R.kind(m) for k, m in mod.named_modules()}
    for step, (out64, out32) in enumerate(_reference(name, si), 1):
        for k, ref in out64.items():
            if k.endswith('num_batches_tracked'):
                assert int(out32[k]) == int(ref) == step
                continue
            e_cpu, scale = R.anchor_err(out32[k], ref), float(ref.abs().max())
            if _exactly_zero(kinds, k):
                top = max(float(v.abs().max()) for kk, v in out64.items() if kk.startswith('grad '))
                assert scale <= 1e-9 * top, '%s step %d %s: not a zero gradient (%.3g)' % (name, step, k, scale)
                continue
            assert e_cpu <= R.ANCHOR_REL * scale, '%s step %d %s: e_cpu %.3g, max|ref| %.3g' % (name, step, k, e_cpu, scale)


# ---------------------------------------------------------------- the derived bound on torch's own fp32 weight gradients
WGRAD_CASES = [(3, 64, 12, 12, 64, 3, 1, 1), (3, 64, 9, 7, 128, 3, 2, 1), (3, 128, 9, 7, 256, 1, 2, 0), (3, 128, 12, 12, 32, 1, 1, 0),
               (2, 256, 8, 8, 256, 4, 2, 1)]


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('case', WGRAD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_derived_bound_holds_for_cpu_float32_weight_gradients(case, dt):
    N, Ci, H, W, Co, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    desc = types.SimpleNamespace(N=N, Ci=Ci, Co=Co, kh=k, kw=k, stride=s, pad=p, Ho=Ho, Wo=Wo)
    x = randn(31, N, Ci, H, W).to(R.DT[dt]).float()
    dy = randn(32, N, Co, Ho, Wo).to(R.DT[dt]).float()
    w = torch.zeros(Co, Ci, k, k, requires_grad=True)
    F.conv2d(x, w, None, s, p).backward(dy)
    ref = R.wgrad64(desc, x, dy)
    w64 = torch.zeros(Co, Ci, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, s, p).backward(dy.double())
    assert float((w64.grad.permute(0, 2, 3, 1) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())     # wgrad64 is the weight gradient
    lim = R.wgrad_bound(N * Ho * Wo, R.wgrad_bound_terms(desc, x, dy), ref)
    err = (w.grad.permute(0, 2, 3, 1).double() - ref).abs()
    assert bool((err <= lim).all()), 'worst err / bound %.3g' % float((err / lim).max())
    assert float((err / lim).max()) > 1e-4          # ... and is no idle bound: fp32 noise reaches a visible fraction of it
    dy2 = dy.clone()
    dy2[0, :, 0, 0] = 0            # a weight gradient that lost one of its M terms is outside
    assert not bool(((R.wgrad64(desc, x, dy2) - ref).abs() <= lim).all())


# ---------------------------------------------------------------- seeded mistakes
class _Edit(torch.autograd.Function):
    """identity forward; the gradient passes through fn"""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


class _Wrong(R.T64):
    """A copy of the float64 composites (block, bn, heads) with one mistake of the glue's kind built in."""

    def __init__(self, mod, mistake):
        super().__init__(mod, torch.float64)
        self.mistake, self.prev = mistake, {}

    def bn(self, name, m, x, residual=None, relu=False):
        stale = self.prev.get(name) if self.mistake == 'statistics of the previous step reused' else None
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        self.prev[name] = (mean.detach(), var.detach())
        if stale is None:
            return super().bn(name, m, x, residual, relu)
        self.B[name + '.num_batches_tracked'] += 1
        g, b = self.P[name + '.weight'], self.P[name + '.bias']
        y = (x - stale[0].view(1, -1, 1, 1)) / torch.sqrt(stale[1].view(1, -1, 1, 1) + m.eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y

    def block(self, pre, blk, x):
        mk = self.mistake
        n = 3 if hasattr(blk, 'conv3') else 2
        x_id = x.detach() if mk == 'the fork add skipped' else x                 # the identity branch's gradient never reaches x
        idn = x_id if blk.downsample is None else self.seq(pre + 'downsample.', blk.downsample, x_id)
        if mk == 'the downsample BatchNorm given the masked gradient twice':
            idn = _Edit.apply(idn, lambda g: 2 * g)
        y = x
        for i in range(1, n):
            y = self.bn(pre + 'bn%d' % i, getattr(blk, 'bn%d' % i), self.conv(pre + 'conv%d' % i, getattr(blk, 'conv%d' % i), y), relu=True)
        a_prev = y
        z = self.bn(pre + 'bn%d' % n, getattr(blk, 'bn%d' % n), self.conv(pre + 'conv%d' % n, getattr(blk, 'conv%d' % n), y))
        s = z + idn
        mask = s > 0
        if mk == 'the identity-branch mask dropped on 1 % of the elements':
            sel = (torch.arange(s.numel()).view_as(s) % 100) == 0
            return F.relu(z + idn.detach()) + (idn - idn.detach()) * (mask | sel)
        if mk == "the ReLU mask taken from bn2's output instead of bn3's":
            wrong = (a_prev > 0).repeat(1, s.shape[1] // a_prev.shape[1], 1, 1)   # (bn2 is narrower: its mask repeated along the channels)
            return F.relu(s).detach() + (s - s.detach()) * wrong
        return F.relu(s)

    def heads(self, m, f, lam):
        mk = self.mistake
        lam = lam * lam if mk == 'lambda applied twice on the adversarial branch' else lam
        # the main head is the first consumer of f: a later one that overwrites instead of accumulating erases its share
        y = self.seq('head.', m.head, f.detach() if mk == 'one fan-in consumer overwriting instead of accumulating' else f)
        f_adv = f.detach() + lam * (f - f.detach())
        y_adv = self.seq('head_adv.', m.head_adv, f_adv)
        y_adv2 = self.fusion_head('head_adv2.', m.head_adv2, f_adv, y_adv)
        y_adv3 = self.fusion_head('head_adv3.', m.head_adv3, f_adv, y_adv2)
        return y, y_adv, y_adv2, y_adv3


MISTAKES = [('bottleneck-id', 'the identity-branch mask dropped on 1 % of the elements'),
            ('bottleneck-id', "the ReLU mask taken from bn2's output instead of bn3's"),
            ('bottleneck-id', 'the fork add skipped'),
            ('bottleneck-down2', 'the downsample BatchNorm given the masked gradient twice'),
            ('bottleneck-down1', 'statistics of the previous step reused'),
            ('heads', 'lambda applied twice on the adversarial branch'),
            ('heads', 'one fan-in consumer overwriting instead of accumulating')]


def _beyond(got, out64, out32):
    """names of the tensors that fail the [anchor] comparison"""
    return [k for k, ref in out64.items() if not k.endswith('num_batches_tracked') and
            not R.anchor_err(got[k], ref) <= R.anchor_bound(R.anchor_err(out32[k], ref), ref)]


@pytest.mark.parametrize('name,mistake', MISTAKES, ids=[m.replace(' ', '_') for _, m in MISTAKES])
def test_seeded_mistake_fails_the_anchor(name, mistake):
    mod, what, cin, fwd = _setup(name, 0)
    ref = _reference(name, 0)
    for mk in (None, mistake):
        T = _Wrong(mod, mk)
        failed = []
        for step in (1, 2):
            xs, dys = _case_inputs(name, 0, step, mod, what, cin)
            failed.append(_beyond(_run(T, fwd, xs, dys), *ref[step - 1]))
        if mk is None:
            assert failed == [[], []], 'the copy itself differs from the composite: %s' % failed
        else:
            assert failed[1], 'the [anchor] comparison did not notice: %s' % mistake
