"""Mean-teacher consistency on the GPU: mi355_bn_fold_batched and mi355_mse_heatmap against tests/mt_ref.py,
uda.model.loss.mt_loss against the reference's live function (tests/golden/g12_mt.npz), the in-iteration teacher
(mi355.teacher.InIterationTeacher) against today's host-folded eval path, DAStep's `mt` and the command lines.

Guards (tests/guarded.py).  The two loss-kernel tests place the prediction, the label and the record, call mse_heatmap inside a
window (rows from torch.empty, the unit gradient from torch.empty_like, both written completely; the row pitch is H * W * 4) and
check the flanks after every call; the unaligned case places its views 4 bytes off a 16-byte boundary and hands in a G.empty()
gradient at the same offset.  The fold kernel keeps its own canaries; MeanTeacherLoss, the teacher, DAStep and the command lines
are not guarded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden
import guarded as G
import mt_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guard(label, fn, *args, **kw):
    from mi355 import ops
    with G.window(ops, label):
        out = fn(*args, **kw)
    torch.cuda.synchronize()
    G.check(label)
    return out

CANARY = np.float32(-7777.25)


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


# ---------------------------------------------------------------- the fold kernel
# (O, T, I, axis, conv bias, float offset of w and out_w inside their buffers modulo 4)
FOLD_ITEMS = [(1, 1, 1, 0, False, 0), (5, 9, 3, 0, True, 1), (4, 16, 7, 1, False, 0), (64, 1, 64, 0, True, 0),
              (33, 31, 1, 0, False, 3),        # 1023 elements
              (41, 5, 5, 1, True, 2),          # 1025
              (3, 25, 33, 0, True, 1),         # 2475: two chunks, channels straddle the chunk boundary, unaligned
              (2, 2, 1100, 1, False, 0),       # 4400: three chunks, all 1100 channels cached per block
              (1, 2, 2100, 1, True, 0)]        # more channels than a chunk: the per-element scale path


def test_fold_kernel_bit_exact_with_canaries(gpu):
    """One launch over nine records: every output equals the numpy restatement bit for bit, and every float of the output
    buffers that belongs to no record -- the gaps behind each out_w and out_bias -- keeps its canary value."""
    from mi355 import ops
    rng = np.random.default_rng(12)
    src, dst_w, dst_b, want_w, want_b, recs_np = [], [], [], [], [], []
    wpos = bpos = 8
    for O, T, I, axis, bias, off in FOLD_ITEMS:
        n, C = O * T * I, (O if axis == 0 else I)
        w = rng.standard_normal((O, T, I)).astype(np.float32)
        gamma, beta, mean = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
        var = (rng.random(C) * 2).astype(np.float32)
        var[0] = 0.0
        gamma[C // 2] = 0.0
        if C > 2:
            gamma[1] = -abs(gamma[1]) - 0.5
        cb = rng.standard_normal(C).astype(np.float32) if bias else None
        eps = 1e-5 if (O + I) % 2 else 1e-3
        wo = (wpos + 3) // 4 * 4 + off                    # float offset: 16-byte aligned + off
        bo = (bpos + 3) // 4 * 4 + (off % 2)
        recs_np.append((w, gamma, beta, mean, var, cb, eps, O, T, I, axis, wo, bo))
        wpos, bpos = wo + n + 9, bo + C + 5               # a gap of at least 9 / 5 canary floats behind every output
    out_w0 = np.full(wpos + 16, CANARY, np.float32)
    out_b0 = np.full(bpos + 16, CANARY, np.float32)
    out_w, out_b = torch.from_numpy(out_w0).to(gpu), torch.from_numpy(out_b0).to(gpu)
    want_w, want_b = out_w0.copy(), out_b0.copy()
    recs, keep = [], []
    for w, gamma, beta, mean, var, cb, eps, O, T, I, axis, wo, bo in recs_np:
        n, C = O * T * I, (O if axis == 0 else I)
        wbuf = torch.zeros(n + 8, device=gpu)              # the source at the same misalignment as its output
        wv = wbuf[wo % 4: wo % 4 + n]
        wv.copy_(torch.from_numpy(w.reshape(-1)))
        ts = [torch.from_numpy(a).to(gpu) if a is not None else None for a in (gamma, beta, mean, var, cb)]
        keep += [wbuf] + ts
        recs.append((wv, ts[0], ts[1], ts[2], ts[3], ts[4], out_w[wo:wo + n], out_b[bo:bo + C], eps, O, T, I, axis))
        fw, fb = mt_ref.fold(w, gamma, beta, mean, var, cb, eps, axis)
        want_w[wo:wo + n], want_b[bo:bo + C] = fw.reshape(-1), fb
    assert out_w.data_ptr() % 16 == 0 and sorted({r[6].data_ptr() % 16 for r in recs}) == [0, 4, 8, 12]
    host, table, count, blocks = ops.fold_table(recs, gpu)
    assert count == 9 and blocks == 1 + 1 + 1 + 2 + 1 + 1 + 2 + 3 + 3
    ops.bn_fold_batched(host, table, count, blocks)
    torch.cuda.synchronize()
    got_w, got_b = out_w.cpu().numpy(), out_b.cpu().numpy()
    for (w, _, _, _, _, _, _, O, T, I, axis, wo, bo), item in zip(recs_np, FOLD_ITEMS):
        n, C = O * T * I, (O if axis == 0 else I)
        assert _same(got_w[wo:wo + n], want_w[wo:wo + n]), item
        assert _same(got_b[bo:bo + C], want_b[bo:bo + C]), item
    assert _same(got_w, want_w) and _same(got_b, want_b)          # ... and every canary is where it was
    assert (want_w != CANARY).sum() == sum(o * t * i for o, t, i, _, _, _ in FOLD_ITEMS)


def test_fold_wrappers_refuse_short_buffers(gpu):
    import mi355
    from mi355 import ops
    z = lambda n: torch.zeros(n, device=gpu)
    ok = (z(12), z(3), z(3), z(3), z(3), None, z(12), z(3), 1e-5, 3, 2, 2, 0)
    host, table, count, blocks = ops.fold_table([ok], gpu)
    for i, n in ((6, 11), (7, 2), (1, 2), (0, 11)):                 # out_w, out_bias, gamma, w one element short
        bad = list(ok)
        bad[i] = z(n)
        with pytest.raises(mi355.Mi355Error):
            ops.fold_table([tuple(bad)], gpu)
    with pytest.raises(mi355.Mi355Error):
        ops.fold_table([ok[:12] + (2,)], gpu)                        # axis
    with pytest.raises(mi355.Mi355Error):
        ops.bn_fold_batched(host, table[:40], count, blocks)         # device table shorter than one record
    with pytest.raises(mi355.Mi355Error):
        ops.bn_fold_batched(host, table, count, blocks + 1)          # refused by the library: block count
    with pytest.raises(mi355.Mi355Error):
        ops.mse_heatmap(z(21 * 4).view(1, 21, 2, 2), z(21 * 4).view(1, 21, 2, 2), ops.mse_record(1, 1.0, gpu), True, rows=z(20))
    with pytest.raises(mi355.Mi355Error):
        ops.mse_heatmap(z(33 * 4).view(1, 33, 2, 2), z(33 * 4).view(1, 33, 2, 2), ops.mse_record(1, 1.0, gpu), False)   # K > 32


# ---------------------------------------------------------------- the loss kernel
def _bound(pre, label, k, want64):
    """Allowed distance of an fp32 loss from float64: twice that of torch's own fp32 CPU MSELoss on the same operands, or 2^-20
    relative, whichever is larger.  Returns (torch's distance, the bound)."""
    j = list(mt_ref.subset(k, pre.shape[1]))
    t = torch.nn.MSELoss()(torch.from_numpy(pre[:, j].copy()), torch.from_numpy(label[:, j].copy()))
    ref = abs(float(t) - want64)
    return ref, max(2 * ref, 2.0 ** -20 * abs(want64))


@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (8, 8), (64, 64)])
@pytest.mark.parametrize('B', [1, 3])
def test_loss_kernel(gpu, B, hw):
    from mi355 import ops
    from uda.model.loss import MeanTeacherLoss
    H, W = hw
    rng = np.random.default_rng(B * 100 + H)
    pre = rng.standard_normal((B, 21, H, W)).astype(np.float32)
    label = rng.random((B, 21, H, W)).astype(np.float32)
    G.row_pitch(H * W * 4)
    p, t = G.place(torch.from_numpy(pre).to(gpu), 'pred'), G.place(torch.from_numpy(label).to(gpu), 'target')
    for k, m in ((0, 1.0), (100, 0.05), (200, 1.0), (300, 0.3), (400, 1.0)):
        mask, gs = mt_ref.mask(k), mt_ref.grad_scale(m, pre.shape, k)
        rec = G.place(ops.mse_record(mask, gs, gpu), 'record')
        rows, g = _guard('mse_heatmap B%d %dx%d k=%d grad' % (B, H, W, k), ops.mse_heatmap, p, t, rec, True)
        rows2, g2 = _guard('mse_heatmap B%d %dx%d k=%d' % (B, H, W, k), ops.mse_heatmap, p, t, rec, False)
        assert G.unwritten(rows) == 0 and G.unwritten(g) == 0 and G.unwritten(rows2) == 0
        assert _same(p, pre) and _same(t, label)                    # the operands are only read
        assert g2 is None and _same(rows, rows2)                    # two launches: the same bits
        assert _same(g, mt_ref.unit_grad(pre, label, mask, gs)), (k, m)
        off = [j for j in range(21) if not (mask >> j) & 1]
        r = rows.cpu().numpy()
        assert _same(r[:, off], np.zeros((B, len(off)), np.float32)) and (r[:, list(mt_ref.subset(k))] > 0).all()
        assert _same(g[:, off], np.zeros((B, len(off), H, W), np.float32))
        d = pre.astype(np.float64) - label.astype(np.float64)
        want_rows = (d * d).sum(axis=(2, 3))
        on = list(mt_ref.subset(k))
        assert np.allclose(r[:, on], want_rows[:, on], rtol=1e-5, atol=0)
        # the scalar: fixed-order sum of the rows times the device-resident m / n
        crit = MeanTeacherLoss(gpu).set(m, k, pre.shape)
        a, b = float(crit(p, t)), float(crit(p, t))
        want64 = m * mt_ref.mt_loss64(pre, label, k)
        ref, bound = _bound(pre, label, k, mt_ref.mt_loss64(pre, label, k))
        print('B=%d %dx%d k=%d m=%g: kernel |err| %.3e, torch fp32 CPU |err| %.3e, bound %.3e'
              % (B, H, W, k, m, abs(a - want64), m * ref, m * bound))
        assert a == b
        assert abs(a - want64) <= m * bound


def test_loss_kernel_unaligned_views_take_the_scalar_path(gpu):
    """HW = 64 is a multiple of 4, but the views start 4 bytes off a 16-byte boundary."""
    from mi355 import ops
    rng = np.random.default_rng(3)
    pre = rng.standard_normal((2, 21, 8, 8)).astype(np.float32)
    label = rng.random((2, 21, 8, 8)).astype(np.float32)
    n = pre.size
    G.row_pitch(64 * 4)
    pb, tb, gb = (G.place(torch.full((n + 8,), float(CANARY), device=gpu), name) for name in ('pred', 'target', 'grad'))
    pv, tv, gv = (b[1:1 + n].view(2, 21, 8, 8) for b in (pb, tb, gb))
    pv.copy_(torch.from_numpy(pre)); tv.copy_(torch.from_numpy(label))
    assert pv.data_ptr() % 16 == 4 and pv.is_contiguous()
    mask, gs = mt_ref.mask(200), mt_ref.grad_scale(0.3, pre.shape, 200)
    rec = G.place(ops.mse_record(mask, gs, gpu), 'record')
    rows, g = _guard('mse_heatmap, views 4 bytes off', ops.mse_heatmap, pv, tv, rec, True, grad=gv)
    rows_al, g_al = _guard('mse_heatmap, aligned copies', ops.mse_heatmap, G.place(pv.clone(), 'pred'), G.place(tv.clone(), 'target'), rec, True)
    assert G.unwritten(rows) == 0 and G.unwritten(rows_al) == 0 and G.unwritten(g_al) == 0
    # ... and with nothing between the operands and their flanks: the views themselves start 4 bytes off
    off = G.START + 4
    tight = G.empty(pre.shape, torch.float32, gpu, 'grad, tight', start=off)
    rows_t, g_t = _guard('mse_heatmap, tight and 4 bytes off', ops.mse_heatmap, G.place(pv.clone(), 'pred', start=off),
                         G.place(tv.clone(), 'target', start=off), rec, True, grad=tight)
    assert tight.data_ptr() % 16 == 4 and G.unwritten(tight) == 0 and _same(g_t, g_al) and _same(rows_t, rows)
    assert g.data_ptr() == gv.data_ptr() and _same(g, mt_ref.unit_grad(pre, label, mask, gs)) and _same(g, g_al)
    assert float(gb[0]) == CANARY and _same(gb[1 + n:], np.full(7, CANARY, np.float32))
    assert np.allclose(rows.cpu().numpy(), rows_al.cpu().numpy(), rtol=1e-6)      # (another lane order: not the same bits)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_mt_loss_against_the_reference(gpu, case):
    from uda.model.loss import mt_loss
    g = golden('g12_mt')
    pre, label, weight = g[case + '/pre'], g[case + '/label'], g[case + '/weight']
    for k in mt_ref.GOLDEN_KS:
        p = torch.from_numpy(pre).to(gpu).requires_grad_(True)
        loss = mt_loss(p, torch.from_numpy(label).to(gpu), torch.from_numpy(weight).to(gpu), k)
        loss.backward()
        want64 = mt_ref.mt_loss64(pre, label, k)
        gold = float(g['%s/loss_%d' % (case, k)])
        ref = abs(gold - want64)                                    # the golden value IS torch's fp32 CPU MSELoss
        bound = max(2 * ref, 2.0 ** -20 * abs(want64))
        print('%s k=%d: kernel |err| %.3e, torch fp32 CPU |err| %.3e, bound %.3e' % (case, k, abs(float(loss) - want64), ref, bound))
        assert abs(float(loss) - want64) <= bound
        gg = mt_ref.golden_grad(g, case, k)[0]
        got = p.grad.cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - gg) <= np.spacing(np.abs(gg))), k      # within 1 ulp of torch's backward
        off = [j for j in range(21) if j not in mt_ref.subset(k)]
        assert not got[:, off].any()
    # a non-unit upstream gradient goes through the scale kernel
    p = torch.from_numpy(pre).to(gpu).requires_grad_(True)
    (mt_loss(p, torch.from_numpy(label).to(gpu), None, 400) * 3.0).backward()
    assert np.allclose(p.grad.cpu().numpy(), 3.0 * mt_ref.golden_grad(g, case, 400)[0], rtol=1e-6, atol=0)


# ---------------------------------------------------------------- the teacher inside the iteration
def _training(gpu, dtype, mt_weight, epoch=0, with_ema=True):
    import mi355
    from mi355.da_step import build_training
    from mi355.optim import EMATeacher
    from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
    from test_gpu_ema import _pose
    mi355.set_compute_dtype(dtype)
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    teacher = None
    if with_ema:
        teacher = _pose(gpu, PoseResNetx10, 5)
        teacher.load_state_dict(model.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        step.ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)
    if mt_weight is not None:
        from mi355.teacher import MeanTeacher
        step.mt = MeanTeacher(step.ema, weight=mt_weight, k='all')
        step.mt.set_epoch(epoch)
    return model, teacher, step, scheds


@pytest.fixture
def bf16_after():
    yield
    import mi355
    mi355.set_compute_dtype('bf16')


def _batch(gpu):
    from utils.synthetic import make_batch
    b = make_batch(2, 128, 32, seed=3, device=gpu)
    b['x_t_ema'] = (b['x_t'] * 0.5 + 0.25).contiguous()              # the teacher sees another view of the target batch
    return b


def _host_folded_copy(gpu, teacher, x):
    """A fresh copy of the teacher through today's host-folded eval path (nothing pinned)."""
    from uda.model.regda_7 import PoseResNetx9
    from test_gpu_ema import _pose
    fresh = _pose(gpu, PoseResNetx9, 9)
    fresh.load_state_dict(teacher.state_dict())
    fresh.eval()
    with torch.no_grad():
        return fresh(x).float().clone()


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_teacher_refresh_equals_the_host_fold(gpu, dtype, bf16_after):
    model, teacher, step, scheds = _training(gpu, dtype, 0.5)
    batch = _batch(gpu)
    x = batch['x_t_ema']

    def iterate():
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        return out

    for _ in range(3):
        iterate()
    it = step.mt.teacher
    assert it._pairs is not None and len(it._pairs) == 24 and all(f.pin is not None for f, *_ in it._pairs)
    # ResNet-18: the stem, 16 block convs, 3 down-sample convs; the neck's three transposed convs; the main head's 3x3 conv
    assert sum(1 for p in it._pairs if p[5]) == 1 and sum(1 for p in it._pairs if p[4]) == 3
    y3 = it.forward(x).float().clone()
    assert torch.equal(y3, _host_folded_copy(gpu, teacher, x))
    iterate()                                                       # a further eager update
    y4 = it.forward(x).float().clone()
    assert torch.equal(y4, _host_folded_copy(gpu, teacher, x)) and not torch.equal(y4, y3)
    step.capture(batch, warmup=0)
    ys = [y4]
    for _ in range(2):                                              # replayed updates: the refresh sits in the graph
        iterate()
        y = it.forward(x).float().clone()
        assert torch.equal(y, _host_folded_copy(gpu, teacher, x)) and not torch.equal(y, ys[-1])
        ys.append(y)
    assert step.graphs is not None
    # validation of the teacher reads the same pinned operands: same answer as the unpinned copy
    from uda.model.regda_7 import MainOutput
    scored = MainOutput(teacher).eval()
    with torch.no_grad():
        assert torch.equal(scored(x).float(), ys[-1])


class _GroupedNet(torch.nn.Module):
    """features / head like the pose models, with grouped convs (the ResNeXt form) in front of BatchNorms: groups 4 without and
    groups 8 with a conv bias and stride 2, between an ordinary conv and a point-wise head."""

    def __init__(self):
        super().__init__()
        from mi355.nn import BatchNorm2d, Conv2d, FusedSequential, ReLU
        self.body = FusedSequential(Conv2d(8, 32, 3, 1, 1, bias=False), BatchNorm2d(32), ReLU(),
                                    Conv2d(32, 32, 3, 1, 1, bias=False, groups=4), BatchNorm2d(32), ReLU(),
                                    Conv2d(32, 64, 3, 2, 1, bias=True, groups=8), BatchNorm2d(64), ReLU())
        self.head = FusedSequential(Conv2d(64, 21, 1, 1, 0))

    def features(self, x):
        return self.body(x)

    def forward(self, x):
        return self.head(self.features(x))


def _scramble(net, seed):
    """New weights and statistics, as an EMA update leaves them: written behind autograd's back, then announced."""
    from mi355 import nn as mnn
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if 'num_batches' in k:
                continue
            r = torch.randn(v.shape, generator=gen).to(v.device)
            if 'running_var' in k:
                r = r.abs() + 0.1
            dst = v.permute(0, 2, 3, 1) if v.dim() == 4 else v          # conv weights: the memory-order view
            dst.copy_(r.permute(0, 2, 3, 1) if v.dim() == 4 else r)
        for p in net.parameters():
            p._mi_epoch = getattr(p, '_mi_epoch', 0) + 1
        mnn._BN_GEN[0] += 1


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_teacher_refresh_with_grouped_convs(gpu, dtype, bf16_after):
    """Grouped convs go through the dense block-diagonal form, as the host fold does: the pinned teacher equals a fresh copy run
    through the host-folded path bit for bit, after eager refreshes and after a refresh replayed from a captured graph."""
    import types
    import mi355
    from mi355.teacher import InIterationTeacher
    mi355.set_compute_dtype(dtype)
    torch.manual_seed(2)
    net = _GroupedNet().to(gpu)
    for p in net.parameters():
        p.requires_grad = False
    _scramble(net, 1)
    x = torch.randn(2, 8, 10, 12, device=gpu)
    it = InIterationTeacher(types.SimpleNamespace(model_ema=net))

    def host():
        fresh = _GroupedNet().to(gpu)
        fresh.load_state_dict(net.state_dict())
        fresh.eval()
        with torch.no_grad():
            return fresh(x).float().clone()

    y = it.forward(x).float().clone()
    assert len(it._pairs) == 3 and sum(d is not None for d in it._dense) == 2 and len(it._plain) == (1 if dtype == 'bf16' else 0)
    assert all(f.pin is not None for f, *_ in it._pairs)
    assert torch.equal(y, host())
    outs = [y]
    for seed in (2, 3):
        _scramble(net, seed)
        it.refresh()
        y = it.forward(x).float().clone()
        assert torch.equal(y, host()) and not torch.equal(y, outs[-1])
        outs.append(y)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        it.refresh()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        it.refresh()
    _scramble(net, 4)
    g.replay()
    torch.cuda.synchronize()
    y = it.forward(x).float().clone()
    assert torch.equal(y, host()) and not torch.equal(y, outs[-1])
    # off-diagonal elements of the dense masters were never written
    for d, (_, conv, *_r) in zip(it._dense, it._pairs):
        if d is not None:
            assert int((d != 0).sum()) <= conv.weight.numel()


def test_prefetcher_stages_image_ema(gpu):
    """--mt-loss on the CPU data path: meta['image_ema'] travels with the batch on the prefetcher's side stream."""
    from utils.data import DevicePrefetcher
    gen = torch.Generator().manual_seed(0)
    batches = [(torch.randn(2, 3, 8, 8, generator=gen), torch.randn(2, 21, 4, 4, generator=gen), torch.ones(2, 21, 1),
                {'image_ema': torch.randn(2, 3, 8, 8, generator=gen), 'index': torch.tensor([i, i + 1])}) for i in range(3)]
    got = list(DevicePrefetcher(iter(batches), gpu, meta_keys=('image_ema',)))
    assert len(got) == 3
    for (x, t, w, meta), (x0, t0, w0, meta0) in zip(got, batches):
        assert x.is_cuda and meta['image_ema'].is_cuda and not meta['index'].is_cuda
        assert torch.equal(meta['image_ema'].cpu(), meta0['image_ema']) and torch.equal(x.cpu(), x0)
        assert not meta0['image_ema'].is_cuda                         # the loader's dict is not modified
    plain = list(DevicePrefetcher(iter(batches), gpu))
    assert not plain[0][3]['image_ema'].is_cuda                       # default: the meta dicts pass through


# ---------------------------------------------------------------- the step
def _run(gpu, mt_weight, epoch, iters, capture_at=None, with_ema=True, recompute=False):
    from uda.model.loss import MeanTeacherLoss
    model, teacher, step, scheds = _training(gpu, 'bf16', mt_weight, epoch, with_ema)
    batch = _batch(gpu)
    rec = dict(model=[], loss_mt=[], loss_gt=[], want_mt=[])
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        y_ema = None
        if recompute and i > 0:
            y_ema = step.mt.teacher.forward(batch['x_t_ema']).clone()         # the teacher as the coming iteration will see it
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        rec['model'].append(_host(model))
        rec['loss_gt'].append(float(out['loss_gt']))
        if mt_weight is not None:
            rec['loss_mt'].append(float(out['loss_mt']))
            if y_ema is not None:
                crit = MeanTeacherLoss(gpu).set(step.mt.m(), 400, tuple(out['y_t'].shape))
                rec['want_mt'].append((float(out['loss_mt']), float(crit(out['y_t'], y_ema)),
                                       step.mt.m() * mt_ref.mt_loss64(out['y_t'].cpu().numpy(), y_ema.cpu().numpy(), 400)))
        else:
            assert 'loss_mt' not in out
    return rec, step


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        eager, _ = _run(gpu, 'ref', 5, 6, recompute=True)
        graph, step = _run(gpu, 'ref', 5, 6, capture_at=3, recompute=True)
        assert step.graphs is not None and len(step.graphs) == 6
        zero, _ = _run(gpu, 0.0, 0, 2)
        off, _ = _run(gpu, None, 0, 6)
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(eager=eager, graph=graph, zero=zero, off=off)


def test_step_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    assert a['loss_mt'] == b['loss_mt'] and a['loss_gt'] == b['loss_gt'] and len(set(a['loss_mt'])) == 6
    for it in range(6):                                             # iterations 3 .. 5 of `graph` are replays
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_loss_mt_is_the_recomputed_term(runs):
    for name in ('eager', 'graph'):
        assert len(runs[name]['want_mt']) == 5
        for got, again, want64 in runs[name]['want_mt']:
            assert got == again and got > 0                         # the same kernels on the same operands outside the step
            assert abs(got - want64) <= 1e-5 * want64               # and m * MSE in float64 (m = 0.05 at epoch 5)


def test_step_zero_weight_changes_nothing_and_the_reference_weight_does(runs):
    """`--mt-weight 0` against `off` after 2 iterations, 1e-6 relative, element by element: |a - b| <= 1e-6 |b|, with an absolute
    floor of 1e-12 times the tensor's largest element for the elements at or near zero (an fp32 parameter that a zero gradient
    moved by less than that has not moved).  The largest difference relative to the tensor's largest element is printed too."""
    zero, off, on = runs['zero'], runs['off'], runs['eager']
    worst = 0.0
    for k, a in zero['model'][1].items():
        b = off['model'][1][k]
        if a.dtype.kind != 'f':
            assert _same(a, b)
            continue
        scale = float(np.abs(b).max())
        diff = np.abs(a.astype(np.float64) - b)
        assert np.all(diff <= 1e-6 * np.abs(b).astype(np.float64) + 1e-12 * scale), k
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()) / scale if scale else 0.0)
    print('m = 0 against off after 2 iterations: largest difference relative to the tensor\'s largest element %.3e' % worst)
    assert worst <= 1e-6
    assert zero['loss_mt'] == [0.0, 0.0]
    k = 'backbone.layer1.0.conv1.weight'
    assert not _same(on['model'][1][k], off['model'][1][k])         # m = 0.05: the backbone moves differently
    kh = 'head_adv.0.weight'
    assert kh in on['model'][0]


def test_step_off_launch_log_is_unchanged_by_the_module(gpu):
    """With `mt` off an iteration launches what it launched before mi355.teacher existed in the process: the logged launches of
    an iteration are the same before and after importing the module, and none of them is one of the new kernels."""
    import importlib
    import mi355
    from mi355 import ops
    saved = sys.modules.pop('mi355.teacher', None)
    try:
        model, teacher, step, scheds = _training(gpu, 'bf16', None)
        batch = _batch(gpu)
        for _ in range(2):
            step.run(batch)

        def logged():
            torch.cuda.synchronize()
            ops.prof_reset(); ops.prof_enable(2)
            try:
                step.run(batch)
                torch.cuda.synchronize()
                return [(e['family'], e['label']) for e in ops.prof_launches()]
            finally:
                ops.prof_enable(0); ops.prof_reset()

        before = logged()
        assert 'mi355.teacher' not in sys.modules
        importlib.import_module('mi355.teacher')
        after = logged()
        assert len(before) > 100 and before == after
        assert not any(l.startswith(('bn_fold', 'mse_heatmap')) for _, l in after)
        # and with it on, the new launches are in the log: the teacher's fold behind the update, the loss in step C
        step.mt = sys.modules['mi355.teacher'].MeanTeacher(step.ema, weight=0.5)
        step.run(batch)
        on = [l for _, l in logged()]
        assert sum(l.startswith('bn_fold') for l in on) == 1 and sum(l.startswith('mse_heatmap') for l in on) == 1
    finally:
        if saved is not None:
            sys.modules['mi355.teacher'] = saved
        mi355.set_compute_dtype('bf16')


# ---------------------------------------------------------------- command lines
def test_train_and_test_cli_with_the_mt_switch(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(script, log, extra, ok=True):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0',
                  '--pretrain_epochs', '1', '--log', log]
        r = subprocess.run([sys.executable, os.path.join(PKG, script)] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout, r.stderr

    ema_line = re.compile(r'^ema: +\d+\.\d{3}$', re.M)
    log = str(tmp_path / 'mt')
    mt = ['--ema-update', 'const', '--ema-decay', '0.9', '--mt-loss', 'on', '--mt-weight', '0.1']
    out, _ = run('train1.py', log, ['--epochs', '1', '--pretrain', str(tmp_path / 'none.pth')] + mt)
    assert 'Loss (mt)' in out and len(ema_line.findall(out)) == 1 and 'HIP graphs captured' in out
    vals = [float(v) for v in re.findall(r'Loss \(mt\) (\S+) \(', out)]
    assert len(vals) == 3 and all(v > 0 for v in vals)
    ck0 = os.path.join(log, 'checkpoints', '0.pth')
    out, _ = run('train1.py', log, ['--epochs', '2', '--resume', ck0] + mt)                # the second epoch, resumed
    assert 'Epoch: [1]' in out and 'Epoch: [0]' not in out and 'Loss (mt)' in out and len(ema_line.findall(out)) == 1
    ck1 = torch.load(os.path.join(log, 'checkpoints', '1.pth'), map_location='cpu', weights_only=False)
    assert ck1['ema_state']['step'] == 12 and ck1['epoch'] == 1
    out, _ = run('test.py', log, ['--checkpoint', os.path.join(log, 'checkpoints', '1.pth'),
                                  '--ema_model', os.path.join(log, 'checkpoints', 'model_ema.pth')])
    assert 'Source:' in out and len(ema_line.findall(out)) == 1
    # the switch needs a moving teacher
    out, err = run('train1.py', str(tmp_path / 'bad'), ['--epochs', '1', '--mt-loss', 'on'], ok=False)
    assert '--ema-update' in err and not os.path.exists(str(tmp_path / 'bad'))
