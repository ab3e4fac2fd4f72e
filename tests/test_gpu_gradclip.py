"""Global gradient-norm clipping with the non-finite step guard on the GPU (include/mi355pose.h: mi355_grad_sumsq_batched,
mi355_grad_clip_coef, mi355_sgd_nesterov_clipped; mi355.optim.GradClipper; DAStep(clip=...); train1.py --clip-grad-norm):

  1. exact operands: integer gradients, so every partial sum is exact in float64 -- the record equals tests/gradclip_ref.py bit
     for bit at every range length around the chunk size, each range surrounded by NaN;
  2. random data: the norm within one float32 rounding plus the worst case of a float64 summation; the same bits from run to run
     and from a replayed graph;
  3. the clipped SGD kernel bit for bit against the unclipped one fed g * coef;
  4. the guard: an inf or a NaN in the gradients skips the update and counts it;
  5. FusedSGD + GradClipper beside a float64 network under clip_grad_norm_ + torch.optim.SGD, eager and replayed;
  6. DAStep: clip=GradClipper(inf) changes nothing bit for bit; a finite max_norm records the float64 norm of the flat
     gradients, changes the parameters, and replays as it runs eagerly;
  7. the command line.

Guards (tests/guarded.py).  Sections 1 - 4 keep the gradient ranges (with their NaN or sentinel bands), the item table, the
partials -- a G.empty() buffer of exactly total_blocks doubles, all of them written by grad_sumsq_batched --, the clip record,
lr, p, buf and the bf16 copy in guarded buffers; the launches run inside a window and every flank is checked after them (the
captured launches of section 2 run as they did: nothing is allocated there).  test_one_table_of_every_tail_length_against_the_flanks
has ranges that end where their flanks begin.  FusedSGD + GradClipper, DAStep and the command line are not guarded.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradclip_ref as ref
import guarded as G
from conftest import PKG
from seeded import randn

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guard(label, fn, *args):
    with G.window(_ops(), label):
        out = fn(*args)
    torch.cuda.synchronize()
    G.check(label)
    return out


@pytest.fixture
def rt(gpu):
    import mi355
    mi355.load()
    mi355.set_compute_dtype('bf16')
    yield mi355
    mi355.set_compute_dtype('bf16')


def _ops():
    from mi355 import ops
    return ops


def _host_rec(rec):
    """A device mi355_clip_rec as a numpy record."""
    return rec.cpu().numpy().view(_ops().clip_rec_dtype())[0].copy()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Measure:
    """The two launches over `ranges` (device views) into one record."""

    def __init__(self, ranges, max_norm, gpu):
        ops = _ops()
        self.ranges = ranges
        self.table, self.count, self.blocks = ops.gn_table(ranges, gpu)
        self.table = G.place(self.table, 'gn table')
        assert self.table.numel() == self.count * ops.GN_ITEM_BYTES
        self.partials = G.empty((self.blocks,), torch.float64, gpu, 'partials')       # exactly total_blocks doubles
        self.rec = G.place(ops.clip_records(1, max_norm, gpu), 'clip record')

    def set_max_norm(self, max_norm):
        self.rec.view(torch.float32)[2].fill_(max_norm)

    def launch(self):
        ops = _ops()
        ops.grad_sumsq_batched(self.table, self.count, self.blocks, self.partials)
        ops.grad_clip_coef(self.partials, self.blocks, self.rec)

    def __call__(self):
        _guard('grad_sumsq_batched + grad_clip_coef, %d blocks' % self.blocks, self.launch)
        assert G.unwritten(self.partials) == 0
        return _host_rec(self.rec)


# ---------------------------------------------------------------- 1. exact operands
def _lens():
    C = _ops().GN_CHUNK
    return [1, 3, 4, 5, C - 4, C, C + 4, 2 * C + 8]


def _int_range(seed, n, gpu, band=4):
    """(device view [band : band + n] of a guarded buffer that is NaN everywhere else, its integer values in [-8, 8]); the view
    keeps the whole buffer under the flank checks (band = 0: the range ends where its flank begins)."""
    vals = np.random.default_rng(seed).integers(-8, 9, n).astype(np.float32)
    vals[0] = 5.0                                   # (never an all-zero range)
    buf = np.full(n + 2 * band, np.nan, dtype=np.float32)
    buf[band:band + n] = vals
    full = G.place(torch.from_numpy(buf).to(gpu), 'g[%d]' % n)
    view = full[band:band + n]
    view.whole = full
    return view, vals


@pytest.mark.parametrize('case', list(range(8)) + ['all'])
def test_exact_integer_gradients_give_the_reference_record_bit_for_bit(rt, gpu, case):
    lens = _lens()
    pick = lens if case == 'all' else [lens[case]]
    views, vals = zip(*[_int_range(50 + i, n, gpu) for i, n in enumerate(pick)])
    want_ss = int(sum(int((v.astype(np.int64) ** 2).sum()) for v in vals))
    norm64 = float(np.sqrt(np.float64(want_ss)))
    m = _Measure(list(views), 1.0, gpu)
    assert m.blocks == sum((n + _ops().GN_CHUNK - 1) // _ops().GN_CHUNK for n in pick)
    for max_norm in (0.5 * norm64, 2.0 * norm64 + 1.0, float('inf')):
        m.set_max_norm(max_norm)
        got = m()
        ss, norm, coef, skip = ref.clip_record(vals, np.float32(max_norm))
        assert ss == want_ss and got['sumsq'] == want_ss, (case, got['sumsq'], want_ss)          # (nothing NaN was read)
        assert _bits(got['norm']) == _bits(norm) and _bits(got['coef']) == _bits(coef), (case, max_norm, got, norm, coef)
        assert got['skip'] == skip == 0 and got['n_skipped'] == 0
        assert _bits(got['max_norm']) == _bits(np.float32(max_norm))
    assert (coef == 1.0) and ref.clip_record(vals, np.float32(0.5 * norm64))[2] < 1.0


def test_one_table_of_every_tail_length_against_the_flanks(rt, gpu):
    """Ranges of 1, 3, 4, 5, 1023, 1024, 1025 and 1 elements in one launch, none with a band around it: the float4 a lane loads
    behind a tail of 1, 3 or 5 elements would read the 0xFF of the flank, a NaN that the sum of squares cannot hide."""
    lens = [1, 3, 4, 5, 1023, 1024, 1025, 1]
    views, vals = zip(*[_int_range(90 + i, n, gpu, band=0) for i, n in enumerate(lens)])
    want_ss = int(sum(int((v.astype(np.int64) ** 2).sum()) for v in vals))
    m = _Measure(list(views), 1.0, gpu)
    assert m.blocks == m.count == len(lens) and m.partials.numel() == len(lens)
    got = m()
    ss, norm, coef, skip = ref.clip_record(vals, np.float32(1.0))
    assert ss == want_ss and got['sumsq'] == want_ss
    assert _bits(got['norm']) == _bits(norm) and _bits(got['coef']) == _bits(coef) and got['skip'] == skip == 0
    per_block = [float((v.astype(np.float64) ** 2).sum()) for v in vals]
    assert m.partials.cpu().tolist() == per_block


# ---------------------------------------------------------------- 2. random data
def test_random_gradients_within_the_summation_bound_and_reproducible(rt, gpu):
    lens = [100000, 150001, 50003]
    host = [(randn(60 + i, n + 8, scale=0.3 * (i + 1))).numpy() for i, n in enumerate(lens)]
    whole = [G.place(torch.from_numpy(h).to(gpu), 'g[%d]' % n) for h, n in zip(host, lens)]
    views = [w[4:4 + n] for w, n in zip(whole, lens)]
    n_tot = sum(lens)
    ref64 = float(np.sqrt(sum(np.sum(h[4:4 + n].astype(np.float64) ** 2) for h, n in zip(host, lens))))
    m = _Measure(views, 0.5 * ref64, gpu)
    a = m()
    bound = ref64 * (2.0 ** -24 + n_tot * 2.0 ** -52)       # one float32 rounding + the worst case of a float64 summation
    print('norm %.9g  float64 reference %.17g  |difference| %.3g  bound %.3g' % (a['norm'], ref64, abs(float(a['norm']) - ref64), bound))
    assert abs(float(a['norm']) - ref64) <= bound
    assert a['skip'] == 0 and 0.0 < a['coef'] < 1.0
    m.partials.zero_()
    b = m()
    assert _bits(a) == _bits(b)
    # captured and replayed: the same bits as the eager launches
    m.partials.fill_(-1.0)
    m.rec.copy_(_ops().clip_records(1, 0.5 * ref64, gpu))
    g = torch.cuda.CUDAGraph()
    with rt.no_gc_in_capture():
        with torch.cuda.graph(g, capture_error_mode=rt.graph_capture_mode()):
            m.launch()
    torch.cuda.synchronize()
    assert _host_rec(m.rec)['sumsq'] == 0.0            # (capture executed nothing)
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host_rec(m.rec)) == _bits(a)


# ---------------------------------------------------------------- 3. the clipped SGD kernel
def _make_rec(coef, skip, gpu, n_skipped=0):
    ops = _ops()
    r = np.zeros(1, dtype=ops.clip_rec_dtype())
    r['coef'], r['skip'], r['n_skipped'], r['max_norm'] = np.float32(coef), skip, n_skipped, 1.0
    return G.place(torch.from_numpy(r.view(np.uint8).copy()).to(gpu), 'clip record')


def _sgd_state(seed, n, gpu):
    """p, g, buf (float32) and a bf16 copy, each a view [4 : 4 + n] of a guarded buffer with sentinels around it."""
    full = [randn(seed + i, n + 8).to(gpu) for i in range(3)] + [torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=gpu)]
    full = [G.place(t, name) for t, name in zip(full, ('p', 'g', 'buf', 'p_lowp'))]
    return full, [t[4:4 + n] for t in full]


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025, 4100])
def test_clipped_sgd_equals_the_unclipped_kernel_on_scaled_gradients(rt, gpu, n):
    ops = _ops()
    lr = G.place(torch.tensor(0.05, device=gpu), 'lr')
    for coef in (np.float32(0.3712345), np.float32(1.0)):
        rec = _make_rec(coef, 0, gpu)
        for nesterov in (True, False):
            for wd in (0.0, 1e-4):
                for lowp in (True, False):
                    fa, (pa, ga, ba, la) = _sgd_state(70, n, gpu)
                    fb, (pb, gb, bb, lb) = _sgd_state(70, n, gpu)
                    before = [t.clone() for t in fa]
                    for _ in range(2):                       # (the second step reads a non-zero momentum written by the first)
                        _guard('sgd_nesterov_clipped n=%d' % n, ops.sgd_nesterov_clipped, pa, ga, ba, lr, rec, 0.9, wd, nesterov, la if lowp else None)
                        scaled = gb if coef == 1.0 else G.place(gb * torch.tensor(coef, dtype=torch.float32, device=gpu), 'g * coef')
                        _guard('sgd_nesterov n=%d' % n, ops.sgd_nesterov, pb, scaled, bb, lr, 0.9, wd, nesterov, lb if lowp else None)
                    torch.cuda.synchronize()
                    what = (n, float(coef), nesterov, wd, lowp)
                    for x, y, z in zip(fa, fb, before):
                        assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), what
                        assert torch.equal(x[:4], z[:4]) and torch.equal(x[4 + n:], z[4 + n:]), what       # outside the view: untouched
                    assert not torch.equal(fa[0][4:4 + n], before[0][4:4 + n]) and torch.equal(fa[1], before[1]), what
                    assert torch.equal(fa[3], before[3]) != lowp, what


# ---------------------------------------------------------------- 4. the guard
def test_non_finite_gradients_skip_the_update_and_are_counted(rt, gpu):
    ops = _ops()
    C = ops.GN_CHUNK
    lens = [1000, C + 5, 37]
    offs = np.cumsum([0] + [(n + 3) // 4 * 4 for n in lens])
    total = int(offs[-1])
    P, Gr, M = (G.place(t, name) for t, name in zip((randn(80, total).to(gpu), randn(81, total, scale=0.1).to(gpu), randn(82, total).to(gpu)),
                                                     ('p', 'g', 'buf')))
    L = G.place(P.to(torch.bfloat16), 'p_lowp')
    views = [Gr[o:o + n] for o, n in zip(offs[:-1], lens)]
    m = _Measure(views, 1.0, gpu)
    lr = G.place(torch.tensor(0.05, device=gpu), 'lr')

    def launches():
        m.launch()
        for o, n in zip(offs[:-1], lens):
            ops.sgd_nesterov_clipped(P[o:o + n], Gr[o:o + n], M[o:o + n], lr, m.rec, 0.9, 1e-4, True, L[o:o + n])

    def step():
        _guard('measure + three clipped steps', launches)
        return _host_rec(m.rec)

    state = lambda: [t.clone() for t in (P, M, L)]
    same = lambda a, b: all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                        y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)) for x, y in zip(a, b))
    s0 = state()
    r = step()
    assert r['skip'] == 0 and r['n_skipped'] == 0 and 0.0 < r['coef'] < 1.0 and not same(s0, state())
    # the fault is in the data only: one element of the middle range
    at = int(offs[1]) + C + 2
    good = float(Gr[at])
    for k, bad in enumerate((float('inf'), float('nan'))):
        Gr[at] = bad
        s1 = state()
        r = step()
        assert r['skip'] == 1 and r['coef'] == 0.0 and r['n_skipped'] == k + 1, r
        assert not np.isfinite(r['sumsq']) and not np.isfinite(r['norm'])
        assert same(s1, state())
    Gr[at] = good
    s2 = state()
    r = step()
    assert r['skip'] == 0 and r['n_skipped'] == 2 and 0.0 < r['coef'] < 1.0 and not same(s2, state())
    assert all(bool(torch.isfinite(t.float()).all()) for t in state())


# ---------------------------------------------------------------- 5. FusedSGD + GradClipper beside torch
MAX_NORM_NET = 20.0                # between the gradient norms of the two output-gradient scales below, thousands and below 5 in the
                                   # float64 reference (asserted on the reference: it clips in some iterations and not in others)
DY_SCALES = (1.0, 0.001, 1.0, 0.001, 0.001, 1.0)


@pytest.mark.parametrize('replayed', [False, True])
def test_fused_sgd_with_grad_clipper_follows_torch(rt, gpu, replayed):
    """conv (bias) -> BatchNorm -> ReLU -> conv (tests/test_gpu_layer_state.py's small network) under TWO FusedSGD optimizers and
    one GradClipper, next to a float64 copy under clip_grad_norm_ + one torch.optim.SGD.  A further parameter receives a gradient
    in the first iteration only: afterwards it is outside the norm and is not stepped, as a parameter whose grad is None.  Replayed:
    forward + backward and the update captured as two graphs after two eager iterations."""
    from mi355.optim import FusedSGD, GradClipper
    from test_gpu_layer_state import _small_net, _near, REL
    rt.set_compute_dtype('f32')
    mine, net64 = _small_net(gpu, 9)
    mine.train(); net64.train()
    extra = torch.nn.Parameter(randn(402, 37).to(gpu))
    extra64 = torch.nn.Parameter(extra.detach().double().cpu())
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt1 = FusedSGD(list(mine[0].parameters()) + list(mine[1].parameters()), **kw)
    opt2 = FusedSGD(list(mine[3].parameters()) + [extra], **kw)
    params64 = list(net64.parameters()) + [extra64]
    opt64 = torch.optim.SGD(params64, **kw)
    clip = GradClipper(MAX_NORM_NET, gpu)
    x64 = randn(400, 4, 32, 12, 12).double()
    dy64 = randn(401, 4, 32, 12, 12).double()
    x = x64.float().to(gpu).contiguous(memory_format=torch.channels_last)
    dy1 = dy64.float().to(gpu).contiguous(memory_format=torch.channels_last)
    dy = dy1.clone()
    g_extra = randn(403, 37)

    def fwdbwd():
        opt1.zero_grad(); opt2.zero_grad()
        mine(x).backward(dy)
        rt.join_side()

    def update():
        rec = clip.measure([opt1, opt2], 'a')
        opt1.step(clip=rec); opt2.step(clip=rec)

    clipped, g_fb = [], None
    for i, s in enumerate(DY_SCALES):
        if replayed and i == 2:
            torch.cuda.synchronize()
            mode = rt.graph_capture_mode()
            g_fb, g_st = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with rt.no_gc_in_capture():
                with torch.cuda.graph(g_fb, capture_error_mode=mode):
                    fwdbwd()
                with torch.cuda.graph(g_st, capture_error_mode=mode):
                    update()
        dy.copy_(dy1 * s)
        if g_fb is not None:
            g_fb.replay(); g_st.replay()
        else:
            fwdbwd()
            if i == 0:
                extra.grad = g_extra.to(gpu)
            update()
        opt64.zero_grad()
        net64(x64).backward(dy64 * s)
        if i == 0:
            extra64.grad = g_extra.double()
        total = float(torch.nn.utils.clip_grad_norm_(params64, MAX_NORM_NET))
        opt64.step()
        clipped.append(total > MAX_NORM_NET)
        torch.cuda.synchronize()
        norm, coef, skip = clip.read()[0]['a']
        what = 'iteration %d%s' % (i, ' (replayed)' if g_fb is not None else '')
        print('%s: float64 norm %.6g, device norm %.6g coef %.6g' % (what, total, norm, coef))
        assert skip == 0 and (coef < 1.0) == clipped[-1], what
        got = dict(mine.named_parameters())
        for k, p in net64.named_parameters():
            _near('%s: %s' % (what, k), got[k], p, REL['f32'])
        _near(what + ': extra', extra, extra64, REL['f32'])
        # the gradients are only read: after a clipped step the flat buffers still hold the unclipped norm
        fresh = [G[lo:hi] for o in (opt1, opt2) for f, lo, hi in o._runs() for G in (f['G'],)]
        unclipped = float(torch.sqrt(sum((t.double() ** 2).sum() for t in fresh)))
        assert abs(unclipped - norm) <= 1e-6 * norm, what
        if i >= 1:          # `extra` got no gradient since zero_grad(): outside the table, one run less in its optimizer
            covered = sum(hi - lo for _, lo, hi in clip._tables['a']['sig'])
            assert covered == sum(f['P'].numel() for o in (opt1, opt2) for f in o._flat if f is not None) - 40, what
    assert any(clipped) and not all(clipped), clipped
    assert clip.read()[1] == 0


# ---------------------------------------------------------------- 6. DAStep
def _da_run(gpu, clip_norm, iters=4, capture_at=2):
    """resnet18, B = 2, 64 x 64 images, 16 x 16 heat-maps, synthetic: `iters` iterations, the last ones replayed."""
    import mi355
    from mi355.da_step import DAStep, build_training
    from mi355.optim import GradClipper
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic import make_batch
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=16)
    clip = GradClipper(clip_norm, gpu) if clip_norm is not None else None
    if clip is not None:
        step = DAStep(model, opts, step.crit, step.trade_off, step.skip, step.track_acc, clip=clip)
    assert step.clip is clip
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    batch = make_batch(2, 64, 16, seed=3, device=gpu)
    recs, f_norm = [], []
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        if clip is not None:
            recs.append({s: _host_rec(clip.record(s)) for s in clip.SLOTS})
            f_norm.append((float(torch.sqrt(sum((G.double() ** 2).sum() for G in opts['f'].flat_grads()))),
                           sum(G.numel() for G in opts['f'].flat_grads())))
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    outs = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    return dict(params=params, out=outs, recs=recs, f_norm=f_norm, graphs=step.graphs, skipped=clip.read()[1] if clip else 0)


@pytest.fixture(scope='module')
def da_runs(gpu):
    import mi355
    try:
        plain = _da_run(gpu, None)
        inf = _da_run(gpu, float('inf'))
        for i, r in enumerate(inf['recs']):
            print('iteration %d: ' % i + '  '.join('gn_%s %.6g' % (s, r[s]['norm']) for s in 'abc'))
        # a tenth of the smallest norm the run has seen that is not zero (update C's gradient is exactly zero in the first iteration
        # of this synthetic set-up and of the order of 1e-3 afterwards; A's is of the order of 10, B's of 1)
        seen = [float(r[s]['norm']) for r in inf['recs'] for s in 'abc' if r[s]['norm'] > 0]
        assert len(seen) >= 9
        max_norm = 0.1 * min(seen)
        eager = _da_run(gpu, max_norm, capture_at=None)
        graph = _da_run(gpu, max_norm)
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(plain=plain, inf=inf, eager=eager, graph=graph, max_norm=max_norm)


def _same_tensors(a, b, keys):
    """The keys at which the two dicts of tensors differ in any bit."""
    raw = lambda t: t.contiguous().view(-1).view(torch.uint8)
    return [k for k in keys if a[k].shape != b[k].shape or not torch.equal(raw(a[k]), raw(b[k]))]


def test_da_step_with_an_infinite_max_norm_changes_nothing(da_runs):
    plain, inf = da_runs['plain'], da_runs['inf']
    assert plain['graphs'] is not None and len(inf['graphs']) == 6
    assert _same_tensors(plain['params'], inf['params'], plain['params']) == []
    shared = sorted(set(plain['out']) & set(inf['out']))
    assert {'loss_s', 'loss_gf', 'loss_gt', 'y_s', 'y_t'} <= set(shared) and 'gn_a' not in plain['out']
    assert _same_tensors(plain['out'], inf['out'], shared) == []
    assert {'gn_a', 'gn_b', 'gn_c'} <= set(inf['out']) and inf['skipped'] == 0
    for r in inf['recs']:
        for s in 'abc':
            assert r[s]['coef'] == 1.0 and r[s]['skip'] == 0 and np.isfinite(r[s]['norm']) and r[s]['norm'] >= 0


def test_da_step_records_the_float64_norm_and_clips(da_runs):
    plain, eager = da_runs['plain'], da_runs['eager']
    assert eager['graphs'] is None and eager['skipped'] == 0
    for r, (ref64, n) in zip(eager['recs'], eager['f_norm']):
        got = float(r['c']['norm'])
        bound = ref64 * (2.0 ** -24 + n * 2.0 ** -52)
        print('gn_c %.9g  float64 norm of the flat gradients %.17g  |difference| %.3g  bound %.3g' % (got, ref64, abs(got - ref64), bound))
        assert abs(got - ref64) <= bound
        for s in 'abc':
            want = ref.norm_coef_skip(r[s]['sumsq'], np.float32(da_runs['max_norm']))
            assert r[s]['skip'] == 0 and _bits(r[s]['coef']) == _bits(want[1]) and _bits(r[s]['norm']) == _bits(want[0])
        print('  '.join('gn_%s %.6g coef %.6g' % (s, r[s]['norm'], r[s]['coef']) for s in 'abc'))
    # updates A and B see norms orders of magnitude above max_norm in every iteration: both clip throughout
    assert all(r[s]['coef'] < 1.0 for r in eager['recs'] for s in 'ab')
    assert _same_tensors(plain['params'], eager['params'], plain['params']) != []


def test_da_step_with_the_clip_replays_as_it_runs_eagerly(da_runs):
    eager, graph = da_runs['eager'], da_runs['graph']
    assert graph['graphs'] is not None and len(graph['graphs']) == 6
    assert _same_tensors(eager['params'], graph['params'], eager['params']) == []
    assert _same_tensors(eager['out'], graph['out'], sorted(eager['out'])) == [] and sorted(eager['out']) == sorted(graph['out'])
    for a, b in zip(eager['recs'], graph['recs']):
        for s in 'abc':
            assert _bits(a[s]) == _bits(b[s])


# ---------------------------------------------------------------- 6b. the guard end to end
# A non-finite value that arises in an image or a label must reach the flat gradient buffers as a non-finite value, through every
# kernel between them, or the guard of section 4 protects nothing.  resnet18, B = 2, 64 x 64 images, 16 x 16 maps, GradClipper(inf),
# an EMA teacher attached: two warm-up iterations (the optimizers go flat, the clipper's tables settle, then the capture), and the
# four iterations clean / poisoned / clean / clean.
GUARD_POISONS = ['x_s', 'label_s', 'x_t']


def _opt_state(opts, keys):
    """Clones of everything the optimizers `keys` own on the device: flat parameters, momentum / Adam moments, step counts and
    the packed low-precision working copies of the conv weights."""
    out = []

    def walk(v):
        if torch.is_tensor(v):
            out.append(v.detach().clone())
        elif isinstance(v, dict):
            for k in sorted(v, key=repr):
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            for q in v:
                walk(q)

    for k in keys:
        for f in opts[k]._flat:
            if f is not None:
                for name in ('P', 'M', 'V', 'S'):
                    if name in f:
                        out.append(f[name].detach().clone())
                walk(f.get('pack_cache', {}))
    return out


def _same_state(a, b):
    raw = lambda t: t.contiguous().view(-1).view(torch.uint8)
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(raw(x), raw(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _reference_says_b_is_non_finite(poisoned=True):
    """Update B of the float64 torch copy of the step (oracle/train_step.py, its step B on the CPU): are the gradients of the three
    adversarial heads non-finite when one pixel of x_t is +Inf?  The oracle's label generators are built for 64 x 64 maps, so it
    runs at its own size (256 x 256 images) with the same poison; whether a gradient is finite does not depend on the size."""
    from oracle.train_step import build_model, DATrainer
    from seeded import fill_module_
    from utils.synthetic import make_batch
    ref = build_model('resnet18')
    fill_module_(ref, 731)
    ref = ref.double()
    tr = DATrainer(ref)
    m, to = tr.model, tr.trade_off
    m.train()
    batch = make_batch(2, 256, 64, seed=3, device='cpu')
    if poisoned:
        batch['x_t'][1, 2, 133, 68] = float('inf')
    x_t, w_t = batch['x_t'].double(), batch['w_t'].double()
    y_t, y_t_adv, y_t_adv2, y_t_adv3, _ = m(x_t)
    H = y_t.shape[-1]
    up = lambda t, size: torch.nn.Upsample(size=size, mode='bilinear')(t.detach())
    loss_gf = 0.3 * to * tr.rd1(y_t, y_t_adv3, w_t, mode='max') + to * tr.rd(y_t, y_t_adv, 0.5 * up(y_t_adv3, H) + up(y_t_adv2, H), w_t, mode='max') + \
        0.3 * to * tr.rd2(y_t, y_t_adv2, up(y_t_adv3, H // 2), w_t, mode='max')
    loss_gf.backward()
    grads = [p.grad for h in (m.head_adv, m.head_adv2, m.head_adv3) for p in h.parameters() if p.grad is not None]
    assert grads
    return not all(bool(torch.isfinite(g).all()) for g in grads)


def _guard_run(gpu, optimizer, replayed, poison):
    import mi355
    from mi355.da_step import DAStep, build_training
    from mi355.optim import GradClipper, EMATeacher
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic import make_batch
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model, teacher = _pose(gpu, PoseResNetx9, 731), _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=16, optimizer=optimizer)
    clip = GradClipper(float('inf'), gpu)
    ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)
    step = DAStep(model, opts, step.crit, step.trade_off, step.skip, step.track_acc, ema=ema, clip=clip)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    clean = make_batch(2, 64, 16, seed=3, device=gpu)
    bad = {k: v.clone() for k, v in clean.items()}
    if poison == 'label_s':
        bad['label_s'][1, 7, 5, 9] = float('nan')
    else:
        bad[poison][1, 2, 33, 17] = float('inf')
    KEYS = {'a': ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'), 'b': ('h_adv2', 'h_adv', 'h_adv3'), 'c': ('f',)}
    watch = {}                     # slot -> (state before, state after, record after) of the update, filled while armed

    def around(slot, fn):
        def wrapped():
            if not watch.get('armed'):
                return fn()
            torch.cuda.synchronize()
            before = _opt_state(opts, KEYS[slot])
            out = fn()
            torch.cuda.synchronize()
            watch[slot] = (before, _opt_state(opts, KEYS[slot]), _host_rec(clip.record(slot)))
            return out
        return wrapped

    class _Graph:
        def __init__(self, g, slot):
            self.g, self.slot = g, slot
            self.replay = around(slot, g.replay)

    def iterate(batch):
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        return {k: float(out[k]) for k in ('loss_s', 'loss_gf', 'loss_gt')}, {s: _host_rec(clip.record(s)) for s in clip.SLOTS}

    for _ in range(2):
        iterate(clean)
    if replayed:
        step.capture(clean, warmup=0)
        step.graphs = [g if i % 2 == 0 else _Graph(g, 'abc'[i // 2]) for i, g in enumerate(step.graphs)]
    else:
        step._update_A, step._update_B, step._update_C = around('a', step._update_A), around('b', step._update_B), around('c', step._update_C)
    log = []
    params = lambda: torch.cat([f['P'] for o in opts.values() for f in o._flat if f is not None]).clone()
    for it, batch in enumerate((clean, bad, clean, clean)):
        watch.clear()
        watch['armed'] = it == 1
        p0 = params()
        losses, recs = iterate(batch)
        moved = not torch.equal(p0, params())
        teacher_ok = all(bool(torch.isfinite(p).all()) for p in teacher.parameters())
        stats = sorted(k for k, v in model.state_dict().items() if 'running_' in k and not bool(torch.isfinite(v).all()))
        log.append(dict(losses=losses, recs=recs, moved=moved, teacher_ok=teacher_ok, bad_stats=stats, watch=dict(watch)))
    from mi355 import ops
    return dict(log=log, n_skipped=clip.read()[1], replayed=step.graphs is not None, timeouts=ops.bn_resident_timeouts())


@pytest.mark.parametrize('poison', GUARD_POISONS)
@pytest.mark.parametrize('replayed', [False, True], ids=['eager', 'replayed'])
@pytest.mark.parametrize('optimizer', ['sgd', 'adamw'])
def test_a_non_finite_input_skips_its_updates_and_training_goes_on(rt, gpu, optimizer, replayed, poison):
    """+Inf in one pixel of x_s, NaN in one element of label_s, +Inf in one pixel of x_t, in iteration 2 of 4.
    x_s / label_s: update A is skipped.  x_t: update C is skipped, and B where the float64 torch step says its gradients are
    non-finite.  A skipped update leaves everything its optimizers own bit-identical (parameters, momentum or Adam moments and
    step counts, packed working copies) and is counted; the clean iterations before and after skip nothing, have finite losses
    and move the parameters; the EMA teacher's weights stay finite.  The BatchNorm running statistics of the poisoned forward
    may be non-finite (torch's are, tests/test_nonfinite_cpu.py): the guard does not cover them, the layers are recorded and
    the assertion is only that iterations 3 and 4 do not care (train-mode BatchNorm normalises by batch statistics)."""
    try:
        r = _guard_run(gpu, optimizer, replayed, poison)
    finally:
        rt.set_compute_dtype('bf16')
    assert r['replayed'] == replayed and r['timeouts'] == 0
    want = {'a': poison in ('x_s', 'label_s'), 'b': False, 'c': poison == 'x_t'}
    if poison == 'x_t':
        want['b'] = _reference_says_b_is_non_finite()
        assert want['b']          # (a +Inf pixel makes every feature NaN behind the first BatchNorm, in torch too)
    log = r['log']
    for it in (0, 2, 3):
        e = log[it]
        assert all(e['recs'][s]['skip'] == 0 and e['recs'][s]['coef'] == 1.0 and np.isfinite(e['recs'][s]['norm']) for s in 'abc'), (it, e['recs'])
        assert all(np.isfinite(v) for v in e['losses'].values()), (it, e['losses'])
        assert e['moved'] and e['teacher_ok'], it
    e = log[1]
    print('%s %s %s: running statistics non-finite after the poisoned iteration in %d tensors (%s ...); losses %s' % (
        optimizer, 'replayed' if replayed else 'eager', poison, len(e['bad_stats']), ', '.join(e['bad_stats'][:3]), e['losses']))
    assert e['teacher_ok']
    assert set(e['watch']) - {'armed'} == {'a', 'b', 'c'}
    for s in 'abc':
        before, after, rec = e['watch'][s]
        if want[s]:
            assert rec['skip'] == 1 and rec['coef'] == 0.0 and not np.isfinite(rec['norm']), (s, rec)
            assert _same_state(before, after), 'the skipped update %s changed what it owns' % s.upper()
        else:
            assert rec['skip'] == 0 and rec['coef'] == 1.0 and np.isfinite(rec['norm']), (s, rec)
            assert not _same_state(before, after), s
    assert r['n_skipped'] == sum(want.values())
    assert log[2]['bad_stats'] == log[1]['bad_stats'] or set(log[2]['bad_stats']) <= set(log[1]['bad_stats'])


# ---------------------------------------------------------------- 7. the command line
def test_train_cli_prints_the_gradient_norms_and_the_skipped_steps(gpu, tmp_path):
    log = str(tmp_path / 'run')
    pre = str(tmp_path / 'pre.pth')
    common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0', '--epochs', '1',
              '--pretrain_epochs', '1', '--pretrain', pre]
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    out = run(['--log', log, '--clip-grad-norm', '1.0'])
    assert 'GradNorm (A)' in out and 'GradNorm (B)' in out and 'GradNorm (C)' in out and 'skipped steps: 0' in out
    assert 'HIP graphs captured' in out and 'Target(best)' in out
    assert os.path.exists(os.path.join(log, 'checkpoints', 'pretrain.pth'))
    os.replace(os.path.join(log, 'checkpoints', 'pretrain.pth'), pre)          # (the second run starts from it: no second pre-training)
    out = run(['--log', str(tmp_path / 'run2')])
    assert 'GradNorm' not in out and 'skipped steps' not in out and 'Target(best)' in out
