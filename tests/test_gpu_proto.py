"""Prototype alignment on the GPU: the proto_pool / proto_update / proto_kl / proto_scatter launches against the reference's own
lossx / lossx3 over three consecutive calls (tests/golden/g16_proto.npz) and against the restatement of tests/proto_ref.py in
float64, at the shapes where the tiling can go wrong and at one workload-shaped case; their bit-level properties on exact
operands; the memory state in eager calls and in graph replay; the gradient requests; the refused arguments; the deviations; the
GradFanIn protocol of the pooling's backward in every order; DAStep's `proto`; the command line.

The tolerance, everywhere (proto_ref.bounds = jfa_ref.bounds): a kernel result may be as far from the float64 result as 4 times the
distance of a float32 run of the reference expression from it (the fixture's float32 arrays for the fixture cases, proto_ref in
float32 otherwise), with the floors jfa_ref.py writes down.  A gradient that is STORED in bf16 (bf16 features) may in addition,
element by element, be one bf16 rounding from the value before storage: bf16 keeps 8 significant bits, so round-to-nearest moves a
value v by at most 2^-8 |v|; v itself is within the bound of the float64 value r, so the allowance of an element is
2^-8 (|r| + bound), as tests/test_gpu_jfa.py states it.  The format, not the kernel's arithmetic.

Guards (tests/guarded.py), as in tests/test_gpu_jfa.py: the kernel-level tests of section 3 and the KL test of section 5 place
feature maps, key points, descriptors, the blend record, the memory and the gradients, call the wrappers in a window and check
the flanks after every call; P, the descriptors and the rows come from torch.empty inside the window and must be written
completely.  proto_update's memory is rewritten in place: its flanks are checked and its bits compared.  The tests through the
loss classes and autograd go through _call, which keeps one window open over the forward and the backward: every descriptor,
prototype and gradient the wrappers allocate is guarded too (the running memories belong to the criterion and are not).  The
graph replay, the GradFanIn test and DAStep are not guarded."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden
import guarded as G
import proto_ref
from test_gpu_jfa import (CORNER_C, POISON, _bits, _corners, _feat, _gdev, _gfeat, _gout, _guard, _nchw, _points, _same, guards,  # noqa: F401
                          ops_is_nhwc)

pytestmark = pytest.mark.gpu

KEYS = proto_ref.KEYS
CLASSES = {'x': 'kl', 'x3': 'softkl'}


def _check(tag, got, ref32, ref64, stored_bf16=False):
    own, bound = proto_ref.bounds(ref32, ref64)
    err = proto_ref.errors(got, ref64)
    for k in err:
        b = bound[k]
        print('%s %s: kernel |err| %.3e; float32 reference %.3e; bound %.3e' % (tag, k, err[k], own[k], b))
        if stored_bf16 and k.startswith('grad'):
            r = np.asarray(ref64[k], np.float64)
            over = np.abs(np.asarray(got[k], np.float64) - r) - (b + 2.0 ** -8 * (np.abs(r) + b))
            print('%s %s: stored in bf16, largest excess over the element-wise allowance %.3e' % (tag, k, float(over.max())))
            assert (over <= 0).all(), (tag, k)
        else:
            assert err[k] <= b, (tag, k)
    assert set(err) == {k for k in ref64 if ref64[k] is not None and got.get(k) is not None}


def _crit(mode, **opts):
    from uda.model import loss as L
    return (L.lossx if mode == 'kl' else L.lossx3)(**opts)


def _call(gpu, crit, f1, f2, p1, p2, dtype=torch.float32, want=(True, True), onto=None, up=None):
    """One forward + backward of a lossx / lossx3 instance: dict of loss, both feature gradients and both memories.  `onto`
    (B, C, H, W): the target features carry a GradFanIn whose buffer holds it, so the backward takes the accumulate path."""
    from mi355 import nn as mnn
    from mi355 import ops
    # inside guards: features, key points and the fan-in buffer are placed; descriptors, prototypes, rows and gradients are made
    # by the wrappers while the window is open, the backward included (the memories are the criterion's own tensors)
    a, b = _gfeat(gpu, f1, dtype, 'f1').requires_grad_(want[0]), _gfeat(gpu, f2, dtype, 'f2').requires_grad_(want[1])
    fan = None
    if onto is not None:
        fan = mnn.GradFanIn()
        fan.buf = _gfeat(gpu, onto, dtype, 'fan-in buffer')
        a._mi_fan = fan
    x1, x2 = _gdev(gpu, np.asarray(p1, np.float32), 'pre1'), _gdev(gpu, np.asarray(p2, np.float32), 'pre2')
    label = 'prototype criterion + backward %s %s' % (tuple(a.shape), dtype)
    with G.window(ops, label):
        loss = crit(a, b, x1, x2)
        if any(want):
            (loss if up is None else loss * up).backward()
    torch.cuda.synchronize()
    G.check(label)
    assert all(G.unwritten(t) == 0 for t in (a.grad, b.grad, loss.detach()) if t is not None)
    if fan is not None:
        assert a.grad is None
    ga = fan.buf if fan is not None else a.grad
    for g in (ga, b.grad):
        assert g is None or (g.dtype == dtype and ops_is_nhwc(g))
    assert crit.val1.dtype == torch.float32 and not crit.val1.requires_grad
    return dict(loss=float(loss.detach()), grad_f1=None if ga is None else _nchw(ga), grad_f2=None if b.grad is None else _nchw(b.grad),
                val1=crit.val1.cpu().numpy().copy(), val2=crit.val2.cpu().numpy().copy())


# ---------------------------------------------------------------- 1. the fixture: three calls in sequence
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('cls', ['x', 'x3'])
@pytest.mark.parametrize('case', ['a', 'b'])
def test_kernels_against_the_reference(gpu, case, cls, dtype):
    """Through uda.model.loss.lossx / lossx3 and autograd, one instance over the fixture's three calls: calls two and three see
    the memory of the call before.  The fixture's features are exact in bf16 (multiples of 1/4 below 2), so the bf16 copy is the
    same problem; its gradients come back stored in bf16."""
    g = golden('g16_proto')
    crit = _crit(CLASSES[cls])
    ptrs = None
    for i, (f1, f2, p1, p2) in enumerate(proto_ref.fixture_calls(g, case)):
        assert np.array_equal(proto_ref.bf16_round(f1), f1) and np.array_equal(proto_ref.bf16_round(f2), f2)
        got = _call(gpu, crit, f1, f2, p1, p2, dtype)
        _check('fixture %s %s call %d' % (case, cls, i), got, proto_ref.fixture_results(g, case, cls, i),
               proto_ref.fixture_results(g, case, cls, i, '_64'), stored_bf16=dtype == torch.bfloat16)
        now = (crit.val1.data_ptr(), crit.val2.data_ptr())
        assert ptrs is None or now == ptrs                  # the memories stay at their addresses
        ptrs = now
    # reset() zeroes in place, and the first call is reproduced bit for bit
    crit.reset()
    assert (crit.val1.data_ptr(), crit.val2.data_ptr()) == ptrs and not crit.val1.any() and not crit.val2.any()
    f1, f2, p1, p2 = proto_ref.fixture_calls(g, case)[0]
    first = _call(gpu, crit, f1, f2, p1, p2, dtype)
    fresh = _call(gpu, _crit(CLASSES[cls]), f1, f2, p1, p2, dtype)
    assert first['loss'] == fresh['loss'] and all(_same(first[k], fresh[k]) for k in KEYS[1:])
    # a non-unit upstream gradient goes through the scale kernel
    up = _call(gpu, _crit(CLASSES[cls]), f1, f2, p1, p2, dtype, up=3.0)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-6
    for k in ('grad_f1', 'grad_f2'):
        assert np.abs(up[k] - 3.0 * fresh[k]).max() <= tol * np.abs(3.0 * fresh[k]).max()
    # a plain NCHW fp32 tensor is accepted as the reference's callers would pass it; updata() copies into the memories
    c2 = _crit(CLASSES[cls])
    c2(torch.from_numpy(f1).to(gpu), torch.from_numpy(f2).to(gpu), torch.from_numpy(p1).to(gpu), torch.from_numpy(p2).to(gpu))
    assert _same(c2.val1, fresh['val1']) and _same(c2.val2, fresh['val2'])       # (exact operands: the same bits from either kernel)
    q = c2.val1.data_ptr()
    c2.updata(torch.full_like(c2.val1, 0.25), torch.full_like(c2.val2, 0.5))
    assert c2.val1.data_ptr() == q and float(c2.val1.min()) == 0.25 and float(c2.val2.max()) == 0.5


# ---------------------------------------------------------------- 2. shapes where the tiling can go wrong
# proto_pool / proto_scatter: channel tiles of 256, 16-byte chunks (8 bf16 / 4 fp32 channels), 256 threads = G pixel groups x
# chunks, strips of 256 pixels; proto_update: one thread per 4 channels, blocks of 64, images in groups of 8; proto_kl: one wave per joint, 4 joints per
# block, 256 channels per pass of a wave.  `acc`: the backward accumulates onto a GradFanIn buffer.
SHAPES = [
    # name          B  K   C    H   W  radius axes   dtype          mode      m     acc
    ('C8', 1, 21, 8, 64, 64, 6, 'ref', torch.float32, 'kl', 0.999, False),
    ('C8bf16', 3, 21, 8, 64, 64, 6, 'xy', torch.bfloat16, 'softkl', 0.999, True),
    ('C24', 2, 21, 24, 64, 64, 6, 'ref', torch.float32, 'softkl', 0.5, True),          # 3 / 6 chunks: idle threads behind the last group
    ('C24bf16', 1, 1, 24, 64, 64, 6, 'ref', torch.bfloat16, 'kl', 1.0, False),         # K = 1; m = 1: the memory drops out
    ('C24xy', 3, 32, 24, 16, 16, 1, 'xy', torch.bfloat16, 'kl', 0.5, False),
    ('C256', 1, 32, 256, 64, 64, 6, 'xy', torch.float32, 'kl', 0.5, False),            # K = 32, 64 chunks a pixel
    ('C256bf16', 3, 21, 256, 64, 64, 1, 'ref', torch.bfloat16, 'softkl', 0.999, False),   # radius 1: windows of 2 x 2 pixels and less
    ('C256acc', 2, 21, 256, 16, 16, 6, 'xy', torch.bfloat16, 'kl', 0.999, True),
    ('K1', 2, 1, 8, 16, 16, 6, 'xy', torch.float32, 'softkl', 1.0, True),
    ('K32', 2, 32, 8, 32, 48, 16, 'ref', torch.bfloat16, 'softkl', 0.5, False),
    ('map16', 3, 21, 24, 16, 16, 6, 'ref', torch.float32, 'kl', 0.999, True),          # the window is larger than half the map
    ('map16r16', 1, 32, 8, 16, 16, 16, 'xy', torch.float32, 'softkl', 0.5, False),     # ... larger than the map
    ('r16', 1, 21, 24, 64, 64, 16, 'ref', torch.bfloat16, 'kl', 1.0, True),            # 32 x 32 windows
    ('r1', 2, 21, 8, 64, 64, 1, 'xy', torch.float32, 'kl', 0.5, False),
    ('m32x48xy', 3, 21, 24, 32, 48, 6, 'xy', torch.float32, 'kl', 0.999, False),       # non-square: a swapped axis or stride shows
    ('m32x48ref', 3, 21, 24, 32, 48, 6, 'ref', torch.float32, 'softkl', 0.999, False),
    ('m32x48bf16', 2, 21, 256, 32, 48, 6, 'ref', torch.bfloat16, 'kl', 0.5, True),
    ('m32x48r1', 1, 1, 8, 32, 48, 1, 'xy', torch.bfloat16, 'softkl', 1.0, False),
]


@pytest.mark.parametrize('name,B,K,C,H,W,radius,axes,dtype,mode,m,acc', SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_shapes(gpu, name, B, K, C, H, W, radius, axes, dtype, mode, m, acc):
    """Two calls in sequence on one instance, against proto_ref with the same memories."""
    rng = np.random.default_rng(len(name) * 977 + C + H)
    scale = 0.3 if name.startswith('C24') else 1.0
    crit = _crit(mode, radius=radius, axes=axes, m=m, scale=scale)
    ref64 = proto_ref.Loss(mode, radius, axes, m, scale, np.float64)
    ref32 = proto_ref.Loss(mode, radius, axes, m, scale, np.float32)
    for i in range(2):
        f1 = proto_ref.bf16_round(rng.random((B, C, H, W)).astype(np.float32) * 2)
        f2 = proto_ref.bf16_round((rng.random((B, C, H, W)) * (rng.random((B, C, H, W)) < 0.4)).astype(np.float32))     # sparse, as after a ReLU
        p1, p2 = _points(rng, B, K, H, W), _points(rng, B, K, H, W)
        if axes == 'ref':             # the reference indexes the rows by x: keep the points inside the map under that reading
            p1, p2 = p1[..., ::-1].copy(), p2[..., ::-1].copy()
        onto = proto_ref.bf16_round(rng.standard_normal((B, C, H, W)).astype(np.float32) * 1e-3) if acc else None
        r64, r32 = ref64(f1, f2, p1, p2), ref32(f1, f2, p1, p2)
        if acc:
            r64['grad_f1'], r32['grad_f1'] = r64['grad_f1'] + onto, (r32['grad_f1'] + onto).astype(np.float32)
        got = _call(gpu, crit, f1, f2, p1, p2, dtype, onto=onto)
        _check('%s call %d' % (name, i), got, {k: r32[k] for k in KEYS}, {k: r64[k] for k in KEYS}, stored_bf16=dtype == torch.bfloat16)
        assert np.abs(r64['grad_f1']).max() > 0 and np.abs(r64['val2']).max() > 0


def test_workload_shaped_case(gpu):
    """B = 64, K = 21, C = 256, 64 x 64, bf16: the neck output's shape.  All prototypes, and the gradient on a random sample of 64
    pixels x all channels (proto_ref computes the prototypes from the windows alone and the gradient only where it is asked)."""
    from mi355 import ops
    from uda.model.loss import prototype, prototype_kl_loss
    rng = np.random.default_rng(64)
    B, K, C, H, W, m = 64, 21, 256, 64, 64, 0.999
    gen = torch.Generator(device='cpu').manual_seed(64)
    f = (torch.rand((B, H, W, C), generator=gen) * (torch.rand((B, H, W, C), generator=gen) < 0.5)).to(torch.bfloat16)
    p = (20 + rng.random((B, K, 2)) * 24).astype(np.float32)               # neighbouring joints: overlapping windows
    ps = torch.from_numpy(rng.random((K, C)).astype(np.float32)).to(gpu)
    mem0 = rng.random((K, C)).astype(np.float32)
    x = f.to(gpu).permute(0, 3, 1, 2).requires_grad_(True)
    mem, blend = torch.from_numpy(mem0).to(gpu), ops.proto_blend(m, device=gpu)
    pt = prototype(x, torch.from_numpy(p).to(gpu), mem, blend, 6, 'xy')
    loss = prototype_kl_loss(pt, ps, 'kl', 1.0)
    loss.backward()
    torch.cuda.synchronize()
    assert _same(mem, pt) and x.grad.dtype == torch.bfloat16 and ops_is_nhwc(x.grad)
    fh = f.float().numpy()                                                  # (B, H, W, C)
    win = proto_ref.windows(p, H, W, 6, 'xy')
    div = proto_ref.divisors(win)
    ref = {}
    for dt in (np.float64, np.float32):
        desc = np.zeros((B, K, C), dt)
        for b in range(B):
            for j, (r0, r1, q0, q1) in enumerate(win[b]):
                desc[b, j] = fh[b, r0:r1, q0:q1].astype(dt).sum(axis=(0, 1), dtype=dt) / dt(div[b, j])
        P = proto_ref.blend(desc, mem0, m, dt)
        l, rows, gt, gs = proto_ref.criterion(P, ps.cpu().numpy(), 'kl', 1.0, dt)
        ref[dt] = dict(loss=l, val1=P, gt=gt)
    pix = [(int(rng.integers(B)), int(rng.integers(12, 52)), int(rng.integers(12, 52))) for _ in range(56)] + \
          [(int(rng.integers(B)), int(rng.integers(H)), int(rng.integers(W))) for _ in range(8)]
    gx = x.grad.permute(0, 2, 3, 1)
    got_g = np.stack([gx[b, r, q].float().cpu().numpy() for b, r, q in pix])
    for dt in ref:
        want = np.zeros((64, C), dt)
        for n, (b, r, q) in enumerate(pix):
            for j, (r0, r1, q0, q1) in enumerate(win[b]):
                if r0 <= r < r1 and q0 <= q < q1:
                    want[n] += ref[dt]['gt'][j] * dt(m / B) / dt(div[b, j])
        ref[dt]['grad_f1'] = want
    assert np.abs(ref[np.float64]['grad_f1']).max() > 0
    # the sample's bound is scaled by the whole map's largest gradient, which the sample need not hold: it holds a covered pixel
    got = dict(loss=float(loss.detach()), val1=pt.detach().cpu().numpy(), grad_f1=got_g)
    keys = ('loss', 'val1', 'grad_f1')
    _check('workload', got, {k: ref[np.float32][k] for k in keys}, {k: ref[np.float64][k] for k in keys}, stored_bf16=True)


# ---------------------------------------------------------------- 3. exact operands: bits
def _exact(B=3, K=21, C=24, H=32, W=48, axes='xy', seed=8):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 16, (B, C, H, W)).astype(np.float32)                # small integers: every sum is exact in fp32 in any order
    p = np.round(_points(rng, B, K, H, W))                                  # integer key points
    p[:, 5:8] = p[:, 4:5]                                                   # three joints on one pixel
    p[:, 8] = (-40, 3)                                                      # an empty window
    if axes == 'ref':
        p = p[..., ::-1].copy()
    return rng, f, p.astype(np.float32)


@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_pool_update_and_memory_are_bit_identical_on_exact_operands(gpu, axes):
    """Small-integer features and integer key points: the window sums and the fixed-order batch sum are exact, so pool, update and
    memory equal the float32 numpy model that does the same single divisions and products in the same order -- over two calls."""
    from mi355 import ops
    rng, f, p = _exact(axes=axes)
    xy = _gdev(gpu, p, 'xy')
    want_d = proto_ref.pool_model(f.transpose(0, 2, 3, 1), p, 6, axes)
    assert (want_d[:, 8] == 0).all() and want_d.max() > 0.5
    for m in (0.999, 0.5, 1.0):
        blend = G.place(ops.proto_blend(m, device=gpu), 'blend')
        assert _same(blend, np.array(proto_ref.blend_record(m), np.float32))
        for dtype in (torch.bfloat16, torch.float32):
            mem0 = rng.integers(-4, 5, (21, 24)).astype(np.float32)
            mem = _gdev(gpu, mem0, 'memory')
            d = _guard('proto_pool %s %s' % (axes, dtype), ops.proto_pool, _gfeat(gpu, f, dtype), xy, 6, axes)
            P = _guard('proto_update m=%g' % m, ops.proto_update, d, mem, blend)
            assert G.unwritten(d) == 0 and G.unwritten(P) == 0
            want_P = proto_ref.update_model(want_d, mem0, m)
            assert _same(d, want_d) and _same(P, want_P) and _same(mem, want_P) and P.data_ptr() != mem.data_ptr(), (m, dtype)
            d2 = _guard('proto_pool %s %s again' % (axes, dtype), ops.proto_pool, _gfeat(gpu, f, dtype), xy, 6, axes)
            P2 = _guard('proto_update m=%g again' % m, ops.proto_update, d2, mem, blend)      # the second call sees the first's memory
            assert G.unwritten(P2) == 0
            want_P2 = proto_ref.update_model(want_d, want_P, m)
            assert _same(P2, want_P2) and _same(mem, want_P2) and (m == 1.0 or not _same(P2, P))


def test_update_adds_the_images_in_ascending_order_at_every_batch_size(gpu):
    """proto_update loads the descriptors of 8 images at a time behind the first: batch sizes below, at and past a group, and the
    workload's 64 (1 + 7 groups + 7), on inexact operands against the fp32 model that adds b = 0, 1, 2, ... in turn."""
    from mi355 import ops
    rng = np.random.default_rng(17)
    blend = G.place(ops.proto_blend(0.999, device=gpu), 'blend')
    for B, K, C in ((1, 21, 24), (8, 21, 24), (9, 1, 8), (10, 32, 24), (17, 21, 264), (64, 21, 256)):
        d = rng.standard_normal((B, K, C)).astype(np.float32)
        mem0 = rng.standard_normal((K, C)).astype(np.float32)
        G.row_pitch(C * 4)
        mem = _gdev(gpu, mem0, 'memory')
        P = _guard('proto_update B%d K%d C%d' % (B, K, C), ops.proto_update, _gdev(gpu, d, 'desc'), mem, blend)
        assert G.unwritten(P) == 0
        want = proto_ref.update_model(d, mem0, 0.999)
        assert _same(P, want) and _same(mem, want), (B, K, C)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_scatter_is_bit_identical_with_the_fixed_order_model(gpu, axes, dtype):
    from mi355 import ops
    B, K, C, H, W, m = 3, 21, 24, 32, 48, 0.999
    rng, f, p = _exact(B, K, C, H, W, axes=axes)
    xy = _gdev(gpu, p, 'xy')
    gp = rng.standard_normal((K, C)).astype(np.float32)
    rnd = proto_ref.bf16_round if dtype == torch.bfloat16 else None
    want, cov = proto_ref.scatter_model(gp, p, (B, H, W, C), m, 6, axes, round_to=rnd)
    assert cov.any() and not cov.all()
    gdev, blend = _gdev(gpu, gp, 'gp'), G.place(ops.proto_blend(m, device=gpu), 'blend')
    G.row_pitch(W * C * (2 if dtype == torch.bfloat16 else 4))
    out = _gout(gpu, B, C, H, W, dtype)
    _guard('proto_scatter = %s %s' % (axes, dtype), ops.proto_scatter, gdev, xy, blend, out, False, 6, axes)
    assert G.unwritten(out) == 0
    got = out.permute(0, 2, 3, 1).float().cpu().numpy()
    assert _same(got, want)
    assert (got[~cov] == 0).all() and not np.signbit(got[~cov]).any()                      # +0 outside every window
    # accumulate mode onto a poisoned-then-filled buffer
    base = rng.standard_normal((B, H, W, C)).astype(np.float32)
    base = proto_ref.bf16_round(base) if dtype == torch.bfloat16 else base
    out.fill_(POISON)
    out.copy_(torch.from_numpy(base).to(gpu).permute(0, 3, 1, 2))
    _guard('proto_scatter += %s %s' % (axes, dtype), ops.proto_scatter, gdev, xy, blend, out, True, 6, axes)
    again = out.clone()
    torch.cuda.synchronize()
    want_acc, _ = proto_ref.scatter_model(gp, p, (B, H, W, C), m, 6, axes, onto=base, round_to=rnd)
    got = out.permute(0, 2, 3, 1).float().cpu().numpy()
    assert _same(got, want_acc)
    assert _bits(got[~cov]) == _bits(base[~cov]) and not np.array_equal(got[cov], base[cov])
    # two runs give the same bits
    out.copy_(torch.from_numpy(base).to(gpu).permute(0, 3, 1, 2))
    _guard('proto_scatter += %s %s again' % (axes, dtype), ops.proto_scatter, gdev, xy, blend, out, True, 6, axes)
    assert _same(out, again)


@pytest.mark.parametrize('radius', [1, 16])
@pytest.mark.parametrize('C', CORNER_C)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_pool_and_scatter_at_the_corners_of_the_first_and_last_image(gpu, axes, dtype, C, radius):
    """B = 2, K = 4, a 5 x 7 map, key points on the four corners of both images, windows of one pixel and windows larger than the
    map: the first and the last pixel of the feature map sit against the guard flanks."""
    from mi355 import ops
    B, K, H, W, m = 2, 4, 5, 7, 0.999
    rng = np.random.default_rng(C * 10 + radius)
    f = rng.integers(0, 16, (B, C, H, W)).astype(np.float32)               # small integers: every sum is exact in fp32 in any order
    p = _corners(B, K, H, W, axes)
    xy = _gdev(gpu, p, 'xy')
    want_d = proto_ref.pool_model(f.transpose(0, 2, 3, 1), p, radius, axes)
    d = _guard('proto_pool corners', ops.proto_pool, _gfeat(gpu, f, dtype), xy, radius, axes)
    assert G.unwritten(d) == 0 and _same(d, want_d) and want_d.min() >= 0 and want_d.max() > 0.5
    gp = rng.standard_normal((K, C)).astype(np.float32)
    rnd = proto_ref.bf16_round if dtype == torch.bfloat16 else None
    want, cov = proto_ref.scatter_model(gp, p, (B, H, W, C), m, radius, axes, round_to=rnd)
    assert cov[0, 0, 0] and cov[B - 1].any() and not cov.all()
    gdev, blend = _gdev(gpu, gp, 'gp'), G.place(ops.proto_blend(m, device=gpu), 'blend')
    out = _gout(gpu, B, C, H, W, dtype)
    _guard('proto_scatter = corners', ops.proto_scatter, gdev, xy, blend, out, False, radius, axes)
    assert G.unwritten(out) == 0 and _same(out.permute(0, 2, 3, 1).float().cpu().numpy(), want)
    base = rng.standard_normal((B, H, W, C)).astype(np.float32)
    base = proto_ref.bf16_round(base) if dtype == torch.bfloat16 else base
    acc = G.place(torch.from_numpy(base).to(gpu).to(dtype), 'out +=').permute(0, 3, 1, 2)
    _guard('proto_scatter += corners', ops.proto_scatter, gdev, xy, blend, acc, True, radius, axes)
    want_acc, _ = proto_ref.scatter_model(gp, p, (B, H, W, C), m, radius, axes, onto=base, round_to=rnd)
    assert _same(acc.permute(0, 2, 3, 1).float().cpu().numpy(), want_acc)


@pytest.mark.parametrize('mode', ['kl', 'softkl'])
def test_two_runs_give_the_same_bits(gpu, mode):
    rng = np.random.default_rng(21)
    f1, f2 = rng.random((3, 24, 32, 48)).astype(np.float32), rng.random((3, 24, 32, 48)).astype(np.float32)
    p1, p2 = _points(rng, 3, 21, 32, 48), _points(rng, 3, 21, 32, 48)
    runs = []
    for _ in range(2):
        crit = _crit(mode, axes='xy')
        runs.append([_call(gpu, crit, f1, f2, p1, p2, torch.bfloat16) for _ in range(2)])
    for a, b in zip(*runs):
        assert a['loss'] == b['loss'] and all(_same(a[k], b[k]) for k in KEYS[1:])
    assert runs[0][0]['loss'] != runs[0][1]['loss']                          # (the memory changed the second call)


# ---------------------------------------------------------------- 4. the memory state: eager calls and graph replay
def test_memory_after_replays_equals_memory_after_eager_calls(gpu):
    """n eager pool + update calls against n replays of one captured graph; then m is rewritten in device memory and both go on:
    the graph follows without a recapture."""
    import mi355
    from mi355 import ops
    rng = np.random.default_rng(4)
    B, K, C, H, W = 3, 21, 24, 32, 48
    f = _feat(gpu, rng.random((B, C, H, W)).astype(np.float32), torch.bfloat16)
    xy = torch.from_numpy(_points(rng, B, K, H, W)).to(gpu)
    mem_e, mem_g = torch.zeros(K, C, device=gpu), torch.zeros(K, C, device=gpu)
    blend_e, blend_g = ops.proto_blend(0.9, device=gpu), ops.proto_blend(0.9, device=gpu)
    desc, P = torch.empty(B, K, C, device=gpu), torch.empty(K, C, device=gpu)
    ops.proto_update(ops.proto_pool(f, xy, 6, 'xy', out=desc), torch.zeros(K, C, device=gpu), blend_g, out=P)      # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with mi355.no_gc_in_capture():
        with torch.cuda.graph(graph):
            ops.proto_update(ops.proto_pool(f, xy, 6, 'xy', out=desc), mem_g, blend_g, out=P)
    torch.cuda.synchronize()
    assert not mem_g.any()                                   # capturing executes nothing
    seen = []
    for n in range(5):
        if n == 3:
            ops.proto_blend(0.5, out=blend_e)
            ops.proto_blend(0.5, out=blend_g)
        Pe = ops.proto_update(ops.proto_pool(f, xy, 6, 'xy'), mem_e, blend_e)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(mem_e, mem_g) and _same(Pe, P) and _same(P, mem_g), n
        seen.append(mem_g.cpu().numpy().copy())
    assert all(not np.array_equal(seen[i], seen[i + 1]) for i in range(4))
    d = ops.proto_pool(f, xy, 6, 'xy').cpu().numpy()
    want = np.zeros((K, C), np.float32)
    for n in range(5):
        want = proto_ref.update_model(d, want, 0.9 if n < 3 else 0.5)
    # (update_model sums the descriptors in the kernel's order: the same bits, also on inexact operands)
    assert _same(seen[-1], want)


# ---------------------------------------------------------------- 5. gradient requests
@pytest.mark.parametrize('mode', ['kl', 'softkl'])
@pytest.mark.parametrize('want', [(True, False), (False, True), (True, True), (False, False)], ids=['t', 's', 'both', 'neither'])
def test_gradient_requests(gpu, want, mode):
    from mi355 import ops
    from uda.model.loss import prototype_kl_loss
    rng = np.random.default_rng(5)
    K, C = 21, 24
    a, b = rng.random((K, C)).astype(np.float32), rng.random((K, C)).astype(np.float32)
    ad, bd = _gdev(gpu, a, 'pt'), _gdev(gpu, b, 'ps')
    # both gradient buffers are handed over whatever is wanted, as neighbours inside one poisoned allocation with guard zones:
    # a side that is not wanted, and everything around a side that is, must keep the poison
    n = ad.numel()
    flat = G.place(torch.full((3 * n + 64,), POISON, device=gpu), 'gradients')
    ga, gb = flat[32:32 + n].view(ad.shape), flat[32 + n:32 + 2 * n].view(bd.shape)
    assert ga.data_ptr() % 16 == 0 and gb.data_ptr() % 16 == 0
    G.row_pitch(C * 4)
    rows, ra, rb = _guard('proto_kl %s %s' % (mode, want), ops.proto_kl, ad, bd, want[0], want[1], mode, 0.5, grad_t=ga, grad_s=gb)
    loss = _guard('reduce_sum', ops.reduce_sum, rows, 0.5 / K if mode == 'kl' else 0.5)
    assert G.unwritten(rows) == 0 and G.unwritten(loss) == 0
    # ... and with the gradients left to the wrapper (torch.empty_like inside the window): the same bits, all of them written
    rows2, ra2, rb2 = _guard('proto_kl %s %s, own gradients' % (mode, want), ops.proto_kl, ad, bd, want[0], want[1], mode, 0.5)
    assert _same(rows2, rows) and G.unwritten(rows2) == 0
    for mine, theirs, w in ((ra2, ga, want[0]), (rb2, gb, want[1])):
        assert (mine is None) == (not w) and (not w or (G.unwritten(mine) == 0 and _same(mine, theirs)))
    assert (ra is None) == (not want[0]) and (rb is None) == (not want[1])
    l64, r64, ga64, gb64 = proto_ref.criterion(a, b, mode, 0.5, np.float64)
    l32, r32, ga32, gb32 = proto_ref.criterion(a, b, mode, 0.5, np.float32)
    got = dict(loss=float(loss), grad_f1=ga.cpu().numpy() if want[0] else None, grad_f2=gb.cpu().numpy() if want[1] else None)
    _check('%s %s' % (mode, want), got, dict(loss=l32, grad_f1=ga32, grad_f2=gb32),
           dict(loss=l64, grad_f1=ga64 if want[0] else None, grad_f2=gb64 if want[1] else None))
    assert np.allclose(rows.cpu().numpy(), r64, rtol=1e-4, atol=1e-7)
    for g, w in ((ga, want[0]), (gb, want[1])):
        assert (g == POISON).all() if not w else not (g == POISON).any()    # an unwanted buffer keeps its poison, a wanted one none
    assert (flat[:32] == POISON).all() and (flat[32 + 2 * n:] == POISON).all()
    # through autograd: only the side that requires a gradient gets one, and nothing is allocated for the other
    x, y = ad.clone().requires_grad_(want[0]), bd.clone().requires_grad_(want[1])
    out = prototype_kl_loss(x, y, mode, 0.5)
    if any(want):
        out.backward()
        assert (x.grad is not None) == want[0] and (y.grad is not None) == want[1]
        assert not want[0] or _same(x.grad, ga)
        assert not want[1] or _same(y.grad, gb)
    assert float(out.detach()) == float(loss)
    # and through the loss class on features
    f1, f2 = rng.random((2, 8, 16, 16)).astype(np.float32), rng.random((2, 8, 16, 16)).astype(np.float32)
    p = _points(rng, 2, 21, 16, 16)
    got = _call(gpu, _crit(mode, axes='xy'), f1, f2, p, p[:, ::-1].copy(), want=want)
    assert (got['grad_f1'] is not None) == want[0] and (got['grad_f2'] is not None) == want[1]


# ---------------------------------------------------------------- 6. refused arguments
def test_refused_arguments_launch_nothing(gpu):
    import mi355
    from mi355 import ops
    from uda.model import loss as L
    z = lambda *shape: torch.zeros(shape, device=gpu)
    f = ops.nhwc_empty(2, 16, 8, 8, torch.bfloat16, gpu).zero_()
    xy, d, P, blend = z(2, 21, 2), z(2, 21, 16), z(21, 16), ops.proto_blend(0.999, device=gpu)
    mem = z(21, 16)
    flat = torch.zeros(2 * 16 * 8 * 8 + 8, dtype=torch.float32, device=gpu)
    off = flat[1:1 + 2048].view(2, 8, 8, 16).permute(0, 3, 1, 2)               # one element off a 16-byte boundary: refused
    assert ops.is_nhwc(off) and off.data_ptr() % 16 == 4
    doff = torch.zeros(2 * 21 * 16 + 8, device=gpu)[1:1 + 672].view(2, 21, 16)
    poff = torch.zeros(21 * 16 + 8, device=gpu)[1:1 + 336].view(21, 16)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        bad = [
            lambda: ops.proto_pool(off, xy),
            lambda: ops.proto_pool(f, xy, out=doff),
            lambda: ops.proto_update(doff, mem, blend),
            lambda: ops.proto_update(d, poff, blend),
            lambda: ops.proto_update(d, mem, blend, out=poff),
            lambda: ops.proto_kl(poff, P, False, False),
            lambda: ops.proto_kl(P, P, True, False, grad_t=poff),
            lambda: ops.proto_kl(P, P, False, True, grad_s=poff),
            lambda: ops.proto_scatter(P, xy, blend, off, False),
            lambda: ops.proto_scatter(poff, xy, blend, f, True),
            lambda: ops.proto_pool(ops.nhwc_empty(2, 12, 8, 8, torch.float32, gpu), xy),       # C = 12: not a multiple of 8
            lambda: ops.proto_pool(ops.nhwc_empty(2, 4, 8, 8, torch.float32, gpu), xy),
            lambda: ops.proto_pool(f, z(2, 33, 2)),                                            # K = 33
            lambda: ops.proto_pool(f, z(2, 0, 2)),
            lambda: ops.proto_pool(f, z(3, 21, 2)),                                            # another batch size
            lambda: ops.proto_pool(f, xy.double()),
            lambda: ops.proto_pool(f, xy, radius=0),
            lambda: ops.proto_pool(f, xy, radius=2.5),
            lambda: ops.proto_pool(f, xy, axes='yx'),
            lambda: ops.proto_pool(f.contiguous(), xy),                                        # NCHW memory
            lambda: ops.proto_pool(f.half(), xy),
            lambda: ops.proto_pool(f, xy, out=z(2, 21, 8)),
            lambda: ops.proto_pool(f.cpu(), xy.cpu()),
            lambda: ops.proto_update(d, z(21, 8), blend),
            lambda: ops.proto_update(d, z(20, 16), blend),
            lambda: ops.proto_update(z(2, 21, 12), z(21, 12), blend),
            lambda: ops.proto_update(z(2, 33, 16), z(33, 16), blend),
            lambda: ops.proto_update(d, mem, blend, out=mem),                                  # P must survive the memory update
            lambda: ops.proto_update(d, mem, z(3)),
            lambda: ops.proto_update(d, mem, blend.double()),
            lambda: ops.proto_kl(P, z(21, 8), False, False),
            lambda: ops.proto_kl(z(21, 12), z(21, 12), False, False),
            lambda: ops.proto_kl(z(33, 16), z(33, 16), False, False),
            lambda: ops.proto_kl(P, P, False, False, mode='on'),
            lambda: ops.proto_kl(P, P, False, False, rows=z(20)),
            lambda: ops.proto_kl(P, P, True, False, grad_t=z(21, 8)),
            lambda: ops.proto_kl(P.cpu(), P.cpu(), False, False),
            lambda: ops.proto_scatter(z(20, 16), xy, blend, f, False),
            lambda: ops.proto_scatter(d, xy, blend, f, False),                                 # a (B, K, C) gradient is not what it reads
            lambda: ops.proto_scatter(P, xy, blend, f.contiguous(), False),
            lambda: ops.proto_scatter(P, xy, blend, f, False, radius=0),
            lambda: ops.proto_scatter(P, z(2, 33, 2), blend, f, False),
            lambda: ops.proto_scatter(P, xy, z(1), f, False),
            lambda: ops.proto_blend(0.0, device=gpu),                                          # m outside (0, 1]
            lambda: ops.proto_blend(1.0001, device=gpu),
            lambda: ops.proto_blend(-0.5, out=blend),
            lambda: ops.proto_blend(float('nan'), out=blend),
        ]
        for i, fn in enumerate(bad):
            with pytest.raises(mi355.Mi355Error):
                fn()
                pytest.fail('case %d was accepted' % i)
        for kw in (dict(radius=0), dict(radius=17.5), dict(m=0.0), dict(m=1.5), dict(axes='yx')):
            with pytest.raises(ValueError):
                L.lossx(**kw)
        with pytest.raises(ValueError):
            L.lossx()(z(2, 16, 8), f, xy, xy)
        with pytest.raises(ValueError):
            L.lossx3()(f, f, xy, z(3, 21, 2))
        with pytest.raises(ValueError):
            L.lossx3()(f, f, xy, z(2, 20, 2))
        with pytest.raises(ValueError):
            L.prototype_kl_loss(P, P, 'on')
        # radius 17 is the command line's and PrototypeAlign's limit (the kernels take any radius of at least 1)
        from mi355.da_step import PrototypeAlign
        for kw in (dict(radius=0), dict(radius=17), dict(m=0.0), dict(m=1.5), dict(weight=0.0), dict(criterion='on')):
            with pytest.raises(ValueError):
                PrototypeAlign(**kw)
        torch.cuda.synchronize()
        assert ops.prof_launches() == [] and _same(blend, np.array(proto_ref.blend_record(0.999), np.float32))
        g = ops.proto_kl(ops.proto_update(ops.proto_pool(f, xy), mem, blend), P, True, False)[1]
        ops.proto_scatter(g, xy, blend, f, True)
        torch.cuda.synchronize()
        assert [e['label'].split()[0] for e in ops.prof_launches()] == ['proto_pool', 'proto_update', 'proto_kl', 'proto_scatter']
    finally:
        ops.prof_enable(0); ops.prof_reset()


# ---------------------------------------------------------------- 7. the deviations from the reference
@pytest.mark.parametrize('mode', ['kl', 'softkl'])
def test_empty_windows_nan_and_outside_coordinates(gpu, mode):
    from mi355 import ops
    rng = np.random.default_rng(3)
    f1, f2 = rng.random((2, 8, 16, 16)).astype(np.float32), rng.random((2, 8, 16, 16)).astype(np.float32)
    out = np.array([[-7, 3], [3, -7], [40, 3], [3, 40], [1e9, 0], [-1e9, -1e9], [15.5, 22.5], [np.nan, 5], [5, np.nan],
                    [np.inf, 5], [5, -np.inf], [3e38, 3e38]], np.float32)
    p = np.stack([out, out[::-1]])
    for axes in ('xy', 'ref'):
        assert (proto_ref.divisors(proto_ref.windows(p, 16, 16, 6, axes)) == 1).all()
        d = ops.proto_pool(_feat(gpu, f1), torch.from_numpy(p).to(gpu), 6, axes)
        assert not d.any()                                                   # zero descriptors
        got = _call(gpu, _crit(mode, axes=axes), f1, f2, p, p)
        assert not got['val1'].any() and not got['val2'].any() and not got['grad_f1'].any() and not got['grad_f2'].any()
        assert np.isfinite(got['loss']) and abs(got['loss']) < 1e-6          # kl: every source prototype sums to 0; softkl: uniform both
    # mixed: some empty, and all the others on one pixel
    p = np.tile(np.array([7.25, 9.5], np.float32), (2, 21, 1))
    p[:, ::4] = (-30, 5)
    p[1, 2] = (np.nan, 3)
    p2 = p[:, ::-1].copy()
    got = _call(gpu, _crit(mode, axes='xy'), f1, f2, p, p2)
    r64, r32 = (proto_ref.Loss(mode, 6, 'xy', dtype=dt)(f1, f2, p, p2) for dt in (np.float64, np.float32))
    _check('one pixel %s' % mode, got, {k: r32[k] for k in KEYS}, {k: r64[k] for k in KEYS})
    assert not got['val1'][::4].any() and _same(got['val1'][1], got['val1'][3]) and np.isfinite(got['grad_f2']).all()
    win = proto_ref.windows(p, 16, 16, 6, 'xy')
    hole = np.ones((2, 16, 16), bool)
    for b in range(2):
        for r0, r1, q0, q1 in win[b]:
            hole[b, r0:r1, q0:q1] = False
    assert not got['grad_f1'].transpose(0, 2, 3, 1)[hole].any() and hole.any()


def test_zero_sum_source_joint_contributes_nothing(gpu):
    from mi355 import ops
    rng = np.random.default_rng(9)
    K, C = 5, 24
    pt, ps = rng.random((K, C)).astype(np.float32), rng.random((K, C)).astype(np.float32)
    ps[1] = 0                                     # the reference returns NaN for this joint
    ps[3, ::2] = 0                                # zero elements: each contributes 0
    ps[4] = -ps[0]                                # a negative sum is treated likewise
    rows, gt, gs = ops.proto_kl(torch.from_numpy(pt).to(gpu), torch.from_numpy(ps).to(gpu), True, True, 'kl', 2.0)
    loss = ops.reduce_sum(rows, 2.0 / K)
    torch.cuda.synchronize()
    rows, gt, gs = rows.cpu().numpy(), gt.cpu().numpy(), gs.cpu().numpy()
    assert np.isfinite(rows).all() and np.isfinite(gt).all() and np.isfinite(gs).all() and np.isfinite(float(loss))
    for j in (1, 4):
        assert rows[j] == 0 and not gt[j].any() and not gs[j].any()
    assert not gs[3, ::2].any() and gs[3, 1::2].any() and (gt[3, ::2] > 0).all()
    ps[4] = 0
    l64, r64, gt64, gs64 = proto_ref.criterion(pt, ps, 'kl', 2.0, np.float64)
    l32, r32, gt32, gs32 = proto_ref.criterion(pt, ps, 'kl', 2.0, np.float32)
    _check('zero sum', dict(loss=float(loss), grad_f1=gt, grad_f2=gs), dict(loss=l32, grad_f1=gt32, grad_f2=gs32), dict(loss=l64, grad_f1=gt64, grad_f2=gs64))
    # softkl has no zero sum: the same rows give finite, non-zero results
    rows3, _, gs3 = ops.proto_kl(torch.from_numpy(pt).to(gpu), torch.from_numpy(ps).to(gpu), False, True, 'softkl', 2.0)
    assert torch.isfinite(rows3).all() and torch.isfinite(gs3).all() and float(rows3[1]) > 0


# ---------------------------------------------------------------- 8. the gradient fan-in of the neck output
@pytest.mark.parametrize('order', ['pool_first', 'pool_middle', 'pool_last'])
def test_pooling_joins_the_gradient_fan_in(gpu, order):
    """As tests/test_gpu_jfa.py's: two mi355.nn.Conv2d heads and the prototype pooling consume one tensor that carries a
    GradFanIn; the three recordings put the pooling's backward last, between the convs' and first.  The tensor's gradient is the
    sum of the three separately computed ones within the bf16 roundings of the buffer."""
    import mi355
    from mi355 import nn as mnn, ops
    from uda.model.loss import prototype
    mi355.set_compute_dtype('bf16')
    rng = np.random.default_rng(11)
    B, C, H, W, K = 2, 64, 16, 16, 21
    torch.manual_seed(5)
    convs = [mnn.Conv2d(C, C, 3, 1, 1, bias=False).to(gpu) for _ in range(2)]
    x0 = _feat(gpu, rng.standard_normal((B, C, H, W)), torch.bfloat16)
    xy = torch.from_numpy(_points(rng, B, K, H, W)).to(gpu)
    wy = [torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).to(gpu) for _ in range(2)]
    wp = torch.from_numpy((rng.standard_normal((K, C)) * 169 * B).astype(np.float32)).to(gpu)
    blend = ops.proto_blend(0.999, device=gpu)

    def run(which, order='pool_last', fan=True):
        leaf = x0.clone().requires_grad_(True)
        x = leaf * 1.0
        assert ops_is_nhwc(x) and x.dtype == torch.bfloat16
        if fan:
            x._mi_fan = mnn.GradFanIn()
        terms = {}
        seq = {'pool_first': ('p', 0, 1), 'pool_middle': (0, 'p', 1), 'pool_last': (0, 1, 'p')}[order]
        for s in seq:
            if s not in which:
                continue
            if s == 'p':
                terms[s] = (prototype(x, xy, torch.zeros(K, C, device=gpu), blend, 6, 'xy') * wp).sum()
            else:
                terms[s] = (convs[s](x).float() * wy[s]).sum()
        sum(terms.values()).backward()
        torch.cuda.synchronize()
        return leaf.grad.float().cpu().numpy()

    try:
        parts = [run((w,), fan=False) for w in (0, 1, 'p')]
        assert all(np.abs(p).max() > 0 for p in parts)
        mags = [np.abs(p).max() for p in parts]
        assert max(mags) < 30 * min(mags), mags                                 # every consumer matters at the tolerance below
        got = run((0, 1, 'p'), order)
        want = parts[0].astype(np.float64) + parts[1] + parts[2]
        # six bf16 roundings of at most 2^-8 of sum |part| each: one per separately computed part, one per write / addition here
        tol = 6 * 2.0 ** -8 * (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])) + 1e-30
        assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
        for drop in range(3):                                                   # the tolerance does tell a lost consumer
            less = want - parts[drop]
            assert not (np.abs(got - less) <= tol).all()
    finally:
        mi355.set_compute_dtype('bf16')


# ---------------------------------------------------------------- 9. the iteration
W_PROTO, M_PROTO = 0.5, 0.9


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


def _align(criterion='kl'):
    from mi355.da_step import PrototypeAlign
    return PrototypeAlign(weight=W_PROTO, radius=3, axes='xy', m=M_PROTO, criterion=criterion)


def _training(gpu, mode, **extra):
    """mode: 'on' (DAStep with the term), 'off' (proto=None passed explicitly), 'plain' (a DAStep built without the argument)."""
    import mi355
    from mi355.da_step import DAStep, build_training
    from uda.model.regda_7 import PoseResNetx9
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    if mode != 'plain':
        step = DAStep(model, opts, step.crit, step.trade_off, step.skip, step.track_acc, proto=_align() if mode == 'on' else None, **extra)
    assert getattr(step, 'proto', None) is None or mode == 'on'
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    return model, step, scheds


def _iterate(gpu, mode, iters, capture_at=None, resume_at=None, probe=False, **extra):
    from utils.synthetic import make_batch
    from uda.model.regda_4 import cached_centres
    model, step, scheds = _training(gpu, mode, **extra)
    batch = make_batch(2, 128, 32, seed=3, device=gpu)
    rec = dict(model=[], loss_gt=[], loss_proto=[], mem=[], probe=[], out=[])
    if probe:                                   # eager runs only: what step C's term saw, copied before the memory is overwritten
        inner = step.proto.term

        def term(f_t, proto_s, y_t):
            mem = step.proto.mem_t.val
            rec['probe'].append(dict(f_t=f_t.detach().float().cpu().numpy(), xy=cached_centres(y_t).cpu().numpy().copy(), proto_s=proto_s.cpu().numpy().copy(),
                                     mem=mem.cpu().numpy().copy() if torch.is_tensor(mem) else np.zeros(tuple(proto_s.shape), np.float32)))
            return inner(f_t, proto_s, y_t)
        step.proto.term = term
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        if resume_at is not None and i == resume_at:
            # checkpoint -> resume: the state goes through torch.save / torch.load into a NEW PrototypeAlign whose memories start empty
            buf = io.BytesIO()
            torch.save({'proto_state': step.proto.state_dict()}, buf)
            buf.seek(0)
            old = step.proto
            step.proto = _align()
            step.proto.load_state_dict(torch.load(buf, map_location='cpu', weights_only=False)['proto_state'], gpu)
            assert step.proto.mem_s.val.data_ptr() != old.mem_s.val.data_ptr() and step.proto.m == M_PROTO
            assert _same(step.proto.mem_s.val, old.mem_s.val) and _same(step.proto.mem_t.val, old.mem_t.val) and old.mem_t.val.any()
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        rec['model'].append(_host(model))
        rec['loss_gt'].append(float(out['loss_gt']))
        if mode == 'on':
            rec['loss_proto'].append(float(out['loss_proto']))
            rec['mem'].append((step.proto.mem_s.val.cpu().numpy().copy(), step.proto.mem_t.val.cpu().numpy().copy()))
            rec['out'].append((out['proto_s'].cpu().numpy().copy(), out['proto_t'].cpu().numpy().copy()))
        else:
            assert 'loss_proto' not in out and 'proto_s' not in out and 'proto_t' not in out
    return rec, step, batch


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        eager, _, _ = _iterate(gpu, 'on', 5, probe=True)
        graph, step, _ = _iterate(gpu, 'on', 5, capture_at=2)
        assert step.graphs is not None and len(step.graphs) == 6
        resumed, _, _ = _iterate(gpu, 'on', 3, resume_at=2)
        off, _, _ = _iterate(gpu, 'off', 2)
        plain, _, _ = _iterate(gpu, 'plain', 2)
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(eager=eager, graph=graph, resumed=resumed, off=off, plain=plain)


def test_step_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    assert a['loss_proto'] == b['loss_proto'] and a['loss_gt'] == b['loss_gt'] and len(set(a['loss_proto'])) == 5
    for it in range(5):                                             # iterations 2, 3 and 4 of `graph` are replays
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)
        for x, y in zip(a['mem'][it] + a['out'][it], b['mem'][it] + b['out'][it]):
            assert _same(x, y), it
        assert _same(a['mem'][it][0], a['out'][it][0]) and _same(a['mem'][it][1], a['out'][it][1])       # memory <- prototype
    assert not np.array_equal(a['mem'][3][0], a['mem'][4][0])


def test_step_off_equals_a_step_built_without_the_argument(runs):
    a, b = runs['off'], runs['plain']
    assert a['loss_gt'] == b['loss_gt']
    for it in range(2):
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_resume_restores_the_memories(runs):
    """Iteration 2 after a checkpoint -> resume of the prototype state equals the uninterrupted run's."""
    a, b = runs['eager'], runs['resumed']
    assert a['loss_proto'][:3] == b['loss_proto'] and a['loss_gt'][:3] == b['loss_gt']
    for it in range(3):
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)
        assert _same(a['mem'][it][0], b['mem'][it][0]) and _same(a['mem'][it][1], b['mem'][it][1])


def test_step_loss_proto_is_the_recomputed_term(runs):
    """proto_ref on what step C saw: f_t, the key points of y_t, proto_s and the target memory before the call."""
    r = runs['eager']
    assert len(r['probe']) == 5
    for it, (got, pr) in enumerate(zip(r['loss_proto'], r['probe'])):
        assert pr['f_t'].shape == (2, 256, 32, 32) and pr['proto_s'].shape == (21, 256) and got > 0
        assert (it == 0) == (not pr['mem'].any())
        res = {}
        for dt in (np.float64, np.float32):
            P = proto_ref.blend(proto_ref.pool(pr['f_t'], pr['xy'], 3, 'xy', dt), pr['mem'], M_PROTO, dt)
            res[dt] = (float(proto_ref.criterion(P, pr['proto_s'], 'kl', W_PROTO, dt)[0]), P)
        (l64, P64), (l32, P32) = res[np.float64], res[np.float32]
        print('iteration %d: loss_proto %.6e, float64 %.6e, float32 %.6e' % (it, got, l64, l32))
        assert abs(got - l64) <= max(4 * abs(l32 - l64), proto_ref.LOSS_FLOOR * abs(l64))
        tol = max(4 * np.abs(P32 - P64).max(), proto_ref.PROTO_FLOOR * np.abs(P64).max())
        assert np.abs(r['out'][it][1] - P64).max() <= tol and _same(r['out'][it][0], pr['proto_s'])


def test_step_moves_the_feature_extractor_and_nothing_else(runs):
    """After one iteration: the parameters optimizer_f steps (backbone, neck) differ from the off run, the heads' -- which only
    change in steps A and B -- do not."""
    on, off = runs['eager']['model'][0], runs['off']['model'][0]
    assert not _same(on['backbone.layer1.0.conv1.weight'], off['backbone.layer1.0.conv1.weight'])
    assert any(k.startswith('upsampling.') and on[k].dtype.kind == 'f' and not _same(on[k], off[k]) for k in on)
    heads = [k for k in on if k.startswith(('head.', 'head_adv.', 'head_adv2.', 'head_adv3.'))]
    assert len(heads) >= 8
    for k in heads:
        assert _same(on[k], off[k]), k


def test_step_with_the_jfa_and_mmd_terms(gpu):
    """All three alignment terms in one step, eager and replayed: each reports its loss, and the prototype term's loss is the one
    a step with it alone reports in the first iteration (the terms do not see each other before the first optimizer step of C)."""
    import mi355
    from mi355.da_step import JointFeatureAlign, MMDAlign
    try:
        rec, step, batch = _iterate(gpu, 'on', 3, capture_at=2, jfa=JointFeatureAlign(weight=0.5, radius=3, axes='xy'), mmd=MMDAlign(weight=0.1))
        alone, _, _ = _iterate(gpu, 'on', 1)
        out = step.out
        for k in ('loss_proto', 'loss_jfa', 'loss_mmd'):
            assert np.isfinite(float(out[k])) and float(out[k]) > 0, k
        assert rec['loss_proto'][0] == alone['loss_proto'][0] and len(set(rec['loss_proto'])) == 3
        assert not _same(rec['model'][0]['backbone.layer1.0.conv1.weight'], alone['model'][0]['backbone.layer1.0.conv1.weight'])
    finally:
        mi355.set_compute_dtype('bf16')


def test_step_with_all_four_terms_eager_and_replay(gpu):
    """The mean-teacher, MMD, JFA and prototype terms in one step: an eager iteration and a replayed one give the same four losses
    and the same weights bit for bit, and step C issues the terms' kernels in the order mt, mmd, jfa, proto (the labels of a
    term's forward kernels; the gathers of the backward follow behind all of them)."""
    import mi355
    from mi355 import ops
    from mi355.da_step import JointFeatureAlign, MMDAlign
    from mi355.optim import EMATeacher
    from mi355.teacher import MeanTeacher
    from uda.model.regda_7 import PoseResNetx10
    from utils.synthetic import make_batch
    from test_gpu_ema import _pose
    keys = ('loss_mt', 'loss_mmd', 'loss_jfa', 'loss_proto')

    def iterate(capture_at, log_at=None):
        model, step, scheds = _training(gpu, 'on', jfa=JointFeatureAlign(weight=0.5, radius=3, axes='xy'), mmd=MMDAlign(weight=0.1))
        teacher = _pose(gpu, PoseResNetx10, 5)
        teacher.load_state_dict(model.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        step.ema = EMATeacher(model, teacher, step.opt, 0.8, warmup=True)
        step.mt = MeanTeacher(step.ema, weight=0.5, k='all')
        assert [t.key for t in step.terms()] == ['mt', 'mmd', 'jfa', 'proto']
        batch = make_batch(2, 128, 32, seed=3, device=gpu)
        losses, labels = [], None
        for i in range(3):
            if i == capture_at:
                step.capture(batch, warmup=0)
            if i == log_at:                            # the labels of step C alone
                inner = step._fwdbwd_C

                def logged_C(b):
                    torch.cuda.synchronize()
                    ops.prof_reset()
                    inner(b)
                    torch.cuda.synchronize()
                    seen.extend(e['label'] for e in ops.prof_launches())
                    ops.prof_reset()
                seen, step._fwdbwd_C = [], logged_C
                ops.prof_reset(); ops.prof_enable(2)
            try:
                out = step.run(batch)
                torch.cuda.synchronize()
            finally:
                if i == log_at:
                    ops.prof_enable(0); ops.prof_reset()
                    step._fwdbwd_C, labels = inner, seen
            for s in scheds.values():
                s.step()
            losses.append(tuple(float(out[k]) for k in keys))
        return losses, _host(model), labels

    try:
        eager, w_eager, labels = iterate(None, log_at=2)
        graph, w_graph, _ = iterate(2)                 # iteration 2 is a replay
        assert eager == graph and all(np.isfinite(v) and v > 0 for it in eager for v in it), (eager, graph)
        for k in w_eager:
            assert _same(w_eager[k], w_graph[k]), k
        terms = [l.split()[0] for l in labels if l.startswith(('mse_heatmap', 'mmd_', 'jfa_', 'proto_')) and '_scatter' not in l]
        families = [t.split('_')[0] for t in terms]
        assert [f for i, f in enumerate(families) if i == 0 or f != families[i - 1]] == ['mse', 'mmd', 'jfa', 'proto'], terms
        assert terms[-5:] == ['jfa_pool', 'jfa_kl', 'proto_pool', 'proto_update', 'proto_kl'], terms
    finally:
        mi355.set_compute_dtype('bf16')


def test_step_launch_log(gpu):
    """An iteration with `proto` on holds one proto_pool and one proto_update in step A (the source prototypes) and one proto_pool,
    one proto_update, one proto_kl (the gradient of the target side only) and one proto_scatter in step C; with `proto` off an
    iteration holds none."""
    import mi355
    from mi355 import ops
    from utils.synthetic import make_batch
    try:
        batch = make_batch(2, 128, 32, seed=3, device=gpu)
        logs = {}
        for mode in ('on', 'off'):
            model, step, scheds = _training(gpu, mode)
            step.run(batch)
            inner = step._fwdbwd_C
            seen = {}

            def logged_C(b, inner=inner, seen=seen):
                torch.cuda.synchronize()
                seen['before'] = [e['label'] for e in ops.prof_launches()]
                ops.prof_reset()
                inner(b)
                torch.cuda.synchronize()
                seen['C'] = [e['label'] for e in ops.prof_launches()]
                ops.prof_reset()

            step._fwdbwd_C = logged_C
            torch.cuda.synchronize()
            ops.prof_reset(); ops.prof_enable(2)
            try:
                step.run(batch)
                torch.cuda.synchronize()
                seen['after'] = [e['label'] for e in ops.prof_launches()]
            finally:
                ops.prof_enable(0); ops.prof_reset()
            logs[mode] = seen
        on, off = logs['on'], logs['off']
        assert len(on['C']) > 50 and len(on['before']) > 100
        assert [l.split()[0] for l in on['before'] if l.startswith('proto_')] == ['proto_pool', 'proto_update']
        assert [l.split()[0] for l in on['C'] if l.startswith('proto_')] == ['proto_pool', 'proto_update', 'proto_kl', 'proto_scatter']
        kl = [l for l in on['C'] if l.startswith('proto_kl')][0]
        assert kl.split()[1:] == ['K21', 'C256', 'kl', 'grads10'], kl
        sc = [l for l in on['C'] if l.startswith('proto_scatter')][0]
        print(sc)
        assert sc.split()[1:4] == ['B2', 'K21', 'C256'] and (' acc' in sc or ' write' in sc), sc
        assert not any(l.startswith('proto_') for l in on['after'])
        assert not any(l.startswith('proto_') for l in off['before'] + off['C'] + off['after'])
        assert len(on['C']) >= len(off['C']) + 4 and len(on['before']) >= len(off['before']) + 2
    finally:
        mi355.set_compute_dtype('bf16')


# ---------------------------------------------------------------- 10. the command line
def test_train_cli_with_the_prototype_term_and_resume(gpu, tmp_path):
    """train1.py --synthetic --proto-loss kl: two iterations per epoch, two epochs, resnet18, --resume across the epochs; the
    checkpoint carries both memories and m."""
    log = str(tmp_path / 'run')
    common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '2', '-p', '1', '-j', '0',
              '--pretrain_epochs', '1', '--log', log, '--proto-loss', 'kl', '--proto-m', '0.9']
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    out = run(['--epochs', '1', '--pretrain', str(tmp_path / 'none.pth')])
    assert 'Loss (proto)' in out and 'Target(best)' in out
    ck0 = torch.load(os.path.join(log, 'checkpoints', '0.pth'), map_location='cpu', weights_only=False)
    st0 = ck0['proto_state']
    assert st0['m'] == 0.9 and st0['memory_s'].shape == st0['memory_t'].shape == (21, 256) and st0['memory_s'].dtype == torch.float32
    assert torch.isfinite(st0['memory_s']).all() and st0['memory_s'].abs().max() > 0 and st0['memory_t'].abs().max() > 0
    out = run(['--epochs', '2', '--resume', os.path.join(log, 'checkpoints', '0.pth')])
    assert 'Epoch: [1]' in out and 'Epoch: [0]' not in out and 'Loss (proto)' in out
    st1 = torch.load(os.path.join(log, 'checkpoints', '1.pth'), map_location='cpu', weights_only=False)['proto_state']
    assert st1['m'] == 0.9 and not torch.equal(st1['memory_s'], st0['memory_s']) and torch.isfinite(st1['memory_t']).all()
