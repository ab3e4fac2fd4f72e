"""mi355_coord_heatmap (the coordinate loss on a differentiable soft-arg-max), uda.model.loss.JointsCoordLoss and the
CoordRegression term of the training step, against the float64 reference of tests/coord_ref.py.

Forms.  `row_form()` of csrc/heatmap.hip picks the register-resident kernel of the map size (64 x 64: block per map; 32 x 32 and
16 x 16: wave per map) for 16-byte-aligned `pred` and `unit_grad`, and the loop kernel for any other size or pointer.  Every case
runs from aligned buffers, with `pred` one float past a 16-byte boundary and with `unit_grad` one float past it (the loop
kernel at every size), as tests/test_gpu_heatmap_rows.py selects the forms; rows 1, 4 and 5 give the wave-per-map forms a
partial workgroup.  Operands and outputs live in the 0xFF-filled guard buffers of tests/guarded.py: the flanks must survive and
every output word must be written.  Every call is made twice and must give the same bits.

Ceilings: tests/test_coord_cpu.py coord_yardstick (uv: 1e-3 + 1e-4 |ref|; rows and gradient: 8 x the float32 CPU expression's
error on the same inputs + 2^-23 max |ref|).  The kernel's error is printed beside each ceiling."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import coord_ref as C
import guarded
from conftest import PKG
from test_coord_cpu import CASES, SIDES, coord_yardstick

pytestmark = pytest.mark.gpu

ALIGN = {'aligned': (guarded.START, guarded.START), 'pred+4': (guarded.START + 4, guarded.START), 'grad+4': (guarded.START, guarded.START + 4)}


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kernel(mi, gpu, pred, coord, weight, beta, delta, coef, want_grad=True, want_uv=True, align='aligned'):
    """Two launches on the same guarded buffers -> (loss_rows, unit_grad or None, uv or None) on the CPU."""
    rows, H, W = pred.shape
    s_pred, s_grad = ALIGN[align]
    p = guarded.place(pred.to(gpu), 'pred', start=s_pred)
    c = guarded.place(coord.to(gpu), 'coord')
    w = None if weight is None else guarded.place(weight.to(gpu), 'weight')
    assert p.data_ptr() % 16 == s_pred % 16
    lr = guarded.empty((rows,), torch.float32, gpu, 'loss_rows')
    g = guarded.empty((rows, H, W), torch.float32, gpu, 'unit_grad', start=s_grad) if want_grad else None
    uv = guarded.empty((rows, 2), torch.float32, gpu, 'uv') if want_uv else None
    outs = []
    for _ in range(2):
        mi.call('mi355_coord_heatmap', mi.ptr(p), mi.ptr(c), mi.ptr(w), float(beta), float(delta), float(coef), mi.ptr(lr), mi.ptr(g),
                mi.ptr(uv), rows, H, W, mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append(tuple(None if t is None else t.cpu().clone() for t in (lr, g, uv)))
    guarded.check('coord_heatmap %dx%d rows %d %s' % (H, W, rows, align))
    for t in (lr, g, uv):
        # (0xFF.. is a NaN: only a row that is NaN by construction may hold it, and those tests pass their own check)
        assert t is None or guarded.unwritten(t) == 0 or not torch.isfinite(t).all()
    for a, b in zip(*outs):
        assert a is None or _same(a, b), 'two launches, different bits'
    return outs[0]


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('side', SIDES, ids=lambda s: '%dx%d' % s)
def test_every_form_within_the_yardstick_ceilings(gpu, side):
    mi, ops = _mi()
    worst = {}
    for case in [c for c in CASES if (c[0], c[1]) == side]:
        H, W, rows, beta, delta, wmode = case
        y = coord_yardstick(*case)
        got = {}
        for align in ALIGN:
            lr, g, uv = _kernel(mi, gpu, y['pred'], y['coord'], y['weight'], beta, delta, y['coef'], align=align)
            got[align] = (lr, g, uv)
            for name, out, ref, bnd in (('rows', lr, y['ref_rows'], y['bound_rows']), ('grad', g, y['ref_grad'], y['bound_grad'])):
                err = float((out.double() - ref).abs().max())
                key = (name, align)
                if err / bnd > worst.get(key, (0, 0, 0, 0))[0]:
                    worst[key] = (err / bnd, err, y['yard_' + name], bnd)
                assert err <= bnd, '%s %s %s: error %.3e, float32 yardstick %.3e, ceiling %.3e' % (case, align, name, err, y['yard_' + name], bnd)
            err_uv = (uv.double() - y['ref_uv']).abs()
            assert bool((err_uv <= y['bound_uv']).all()), (case, align, float(err_uv.max()))
            if y['weight'] is not None:                  # skipped rows: exact zeros
                skip = y['weight'] == 0
                assert bool((lr[skip] == 0).all()) and bool((g[skip] == 0).all())
        # uv is mi355_softargmax with out_scale 1, bit for bit, in the form the dispatcher picks for the same pointer
        assert _same(got['aligned'][2].view(rows, 1, 2), ops.softargmax(y['pred'].view(rows, 1, H, W).to(gpu), beta, 1.0).cpu())
    for (name, align), (ratio, err, yard, bnd) in sorted(worst.items()):
        print('%dx%d %-5s %-8s worst error / ceiling %.3f: error %.3e, float32 yardstick %.3e, ceiling %.3e' % (side + (name, align, ratio, err, yard, bnd)))


@pytest.mark.parametrize('name', C.EXACT)
def test_exact_cases_bit_for_bit_in_every_form_that_fits(gpu, name):
    mi, _ = _mi()
    for embed in ((4, 8, 0, 0), (16, 16, 9, 7), (32, 32, 20, 3), (64, 64, 1, 50), (24, 20, 11, 12)):
        e = C.exact_case(name, *embed)
        for align in ALIGN:
            lr, g, uv = _kernel(mi, gpu, e['pred'], e['coord'], None, e['beta'], e['delta'], e['coef'], align=align)
            assert torch.equal(uv, e['uv']) and torch.equal(lr, e['loss']) and torch.equal(g, e['grad']), (name, embed, align)


@pytest.mark.parametrize('side', [(16, 16), (32, 32), (64, 64), (6, 10)], ids=lambda s: '%dx%d' % s)
def test_zero_weight_row_is_skipped_whatever_it_holds(gpu, side):
    mi, _ = _mi()
    H, W = side
    y = coord_yardstick(H, W, 5, 1.0, 1.0, 'none')
    weight = torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0])
    clean = _kernel(mi, gpu, y['pred'], y['coord'], weight, 1.0, 1.0, y['coef'])
    pred, coord = y['pred'].clone(), y['coord'].clone()
    pred[2, H // 2, 1] = float('nan')
    pred[2, 0, 0] = float('inf')
    coord[2, 0] = float('nan')
    coord[2, 1] = float('-inf')
    for align in ALIGN:
        lr, g, uv = _kernel(mi, gpu, pred, coord, weight, 1.0, 1.0, y['coef'], align=align)
        assert _bits(lr)[2] == 0 and bool((_bits(g[2]) == 0).all())                      # exact (positive) zeros
        keep = [0, 1, 3, 4]
        ref = clean if align == 'aligned' else _kernel(mi, gpu, y['pred'], y['coord'], weight, 1.0, 1.0, y['coef'], align=align)
        assert _same(lr[keep], ref[0][keep]) and _same(g[keep], ref[1][keep]) and _same(uv[keep], ref[2][keep])
        assert bool(torch.isnan(uv[2]).all())                                             # uv is still written


@pytest.mark.parametrize('side', [(16, 16), (32, 32), (64, 64), (6, 10)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('where', ['pred', 'coord'])
def test_nan_in_a_weighted_row_stays_in_that_row(gpu, side, where):
    mi, _ = _mi()
    H, W = side
    y = coord_yardstick(H, W, 5, 1.0, 1.0, 'none')
    pred, coord = y['pred'].clone(), y['coord'].clone()
    if where == 'pred':
        pred[3, H - 1, W - 1] = float('nan')
    else:
        coord[3, 1] = float('nan')
    for align in ALIGN:
        clean = _kernel(mi, gpu, y['pred'], y['coord'], None, 1.0, 1.0, y['coef'], align=align)
        lr, g, uv = _kernel(mi, gpu, pred, coord, None, 1.0, 1.0, y['coef'], align=align)
        assert bool(torch.isnan(lr[3])) and bool(torch.isnan(g[3]).all())
        keep = [0, 1, 2, 4]
        assert _same(lr[keep], clean[0][keep]) and _same(g[keep], clean[1][keep]) and _same(uv[keep], clean[2][keep])


@pytest.mark.parametrize('side', SIDES, ids=lambda s: '%dx%d' % s)
def test_nullable_outputs_leave_the_other_bits_alone(gpu, side):
    mi, _ = _mi()
    H, W = side
    y = coord_yardstick(H, W, 5, 1.0, 1.0, 'mixed')
    for align in ('aligned', 'pred+4'):
        full = _kernel(mi, gpu, y['pred'], y['coord'], y['weight'], 1.0, 1.0, y['coef'], align=align)
        no_g = _kernel(mi, gpu, y['pred'], y['coord'], y['weight'], 1.0, 1.0, y['coef'], want_grad=False, align=align)
        no_uv = _kernel(mi, gpu, y['pred'], y['coord'], y['weight'], 1.0, 1.0, y['coef'], want_uv=False, align=align)
        neither = _kernel(mi, gpu, y['pred'], y['coord'], y['weight'], 1.0, 1.0, y['coef'], want_grad=False, want_uv=False, align=align)
        assert no_g[1] is None and no_uv[2] is None
        assert _same(no_g[0], full[0]) and _same(no_g[2], full[2]) and _same(no_uv[0], full[0]) and _same(no_uv[1], full[1])
        assert _same(neither[0], full[0])


def test_refused_arguments(gpu):
    mi, ops = _mi()
    t = torch.zeros(2, 3, 4, 4, device=gpu)
    c = torch.zeros(2, 3, 2, device=gpu)
    for kw in (dict(beta=0.0), dict(beta=float('inf')), dict(beta=float('nan')), dict(delta=-1.0), dict(delta=float('inf')),
               dict(coef=float('nan'))):
        with pytest.raises(mi.Mi355Error, match='coord_heatmap'):
            ops.coord_heatmap(t, c, None, **kw)
    with pytest.raises(mi.Mi355Error, match='coordinates'):
        ops.coord_heatmap(t, c[:, :2], None)


# ----------------------------------------------------------------------------------------------------------- JointsCoordLoss
@pytest.mark.parametrize('shape', [(2, 3, 16, 16), (2, 21, 64, 64), (1, 5, 6, 10)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('delta', [0.0, 1.0])
def test_joints_coord_loss_and_its_gradient(gpu, shape, delta):
    mi, ops = _mi()
    from uda.model.loss import JointsCoordLoss, soft_argmax
    B, K, H, W = shape
    n = B * K
    pred = C.maps(H, W, n, 1.0, seed=3)
    weight = C.weights(n)
    uv0 = C.coord(pred, torch.zeros(n, 2), weight, 1.0, delta, 1.0)[2]
    coord = C.coords_for(uv0, delta, shift=2)
    assert C.kink_clear(uv0, coord, C.f32(delta))
    crit = JointsCoordLoss(beta=1.0, delta=delta)
    for scale, upstream in ((1.0, None), (0.7, None), (0.7, 1.5)):
        k = C.f32(C.f32(scale) / n)
        r_rows, r_grad, r_uv = C.coord(pred, coord, weight, 1.0, C.f32(delta), k)
        o_rows, o_grad, _ = C.coord(pred, coord, weight, 1.0, C.f32(delta), k, dtype=torch.float32)
        up = 1.0 if upstream is None else upstream
        b_grad = up * (8.0 * float((o_grad.double() - r_grad).abs().max()) + 2.0 ** -23 * float(r_grad.abs().max())) * (1 + 2.0 ** -23)
        b_rows = 8.0 * float((o_rows.double() - r_rows).abs().max()) + 2.0 ** -23 * float(r_rows.abs().max())
        # the scalar: a fixed-order float32 sum of n rows and one product behind the rows' own ceiling
        b_loss = float(k) * (n * b_rows + (n + 1) * 2.0 ** -24 * float(r_rows.abs().sum()))
        out = pred.view(B, K, H, W).to(gpu).clone().requires_grad_(True)
        loss = crit(out, coord.view(B, K, 2).to(gpu), weight.view(B, K, 1).to(gpu), scale=scale)
        assert loss.dim() == 0 and not crit.uv.requires_grad
        if upstream is None:
            loss.backward(mi.unit_grad(loss))
        else:
            (loss * upstream).backward()
        want = float(r_rows.sum()) * float(k)
        err_l = abs(float(loss.detach()) - want)
        err_g = float((out.grad.cpu().double().view(n, H, W) - up * r_grad).abs().max())
        print('%s delta %g scale %g upstream %s: loss error %.3e (ceiling %.3e), gradient error %.3e (ceiling %.3e)'
              % (shape, delta, scale, upstream, err_l, b_loss, err_g, b_grad))
        assert err_l <= b_loss and err_g <= b_grad
        assert bool(((crit.uv.cpu().double().view(n, 2) - r_uv).abs() <= 1e-3 + 1e-4 * r_uv.abs()).all())
        assert _same(crit.uv.cpu(), soft_argmax(out, 1.0).cpu())
        skip = weight == 0
        assert bool((out.grad.cpu().view(n, H, W)[skip] == 0).all())
    # no gradient wanted: none is computed
    with torch.no_grad():
        again = crit(out.detach(), coord.view(B, K, 2).to(gpu), weight.view(B, K, 1).to(gpu), scale=0.7)
    assert float(again) == float(loss.detach())


# ------------------------------------------------------------------------------------------------------------------ the step
def _training(gpu, **kw):
    from test_gpu_mixup import _training as base
    return base(gpu, kw.pop('mixup', None), **kw)


def _batches(gpu, n):
    from utils.synthetic import make_batch
    b = make_batch(2, 128, 32, seed=3, device=gpu, with_keypoints=True)
    b['x_t_ema'] = (b['x_t'] * 0.5 + 0.25).contiguous()
    del b['kp_t']
    out = []
    for i in range(n):
        bi = dict(b)
        bi['kp_s'] = (b['kp_s'] + 0.3 * i).contiguous()
        out.append(bi)
    return out


def _host_out(out):
    return {k: v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)}


def _logged(step, batch):
    from test_gpu_mixup import _logged as base
    return base(step, batch)


def _coord_ref_loss(y, kp, w, weight, delta=1.0, beta=1.0):
    """(weight * mean of the float64 rows, its ceiling) for heat-maps y (B, K, H, W), key points (B, K, 2), weights (B, K, 1)."""
    B, K, H, W = y.shape
    n = B * K
    k = C.f32(C.f32(weight) / n)
    args = (y.float().cpu().view(n, H, W), kp.float().cpu().view(n, 2), w.float().cpu().view(n), C.f32(beta), C.f32(delta), k)
    r_rows = C.coord(*args)[0]
    o_rows = C.coord(*args, dtype=torch.float32)[0]
    b_rows = 8.0 * float((o_rows.double() - r_rows).abs().max()) + 2.0 ** -23 * float(r_rows.abs().max())
    return float(r_rows.sum()) * float(k), float(k) * (n * b_rows + (n + 1) * 2.0 ** -24 * float(r_rows.abs().sum()))


@pytest.fixture(scope='module')
def step_runs(gpu):
    import mi355
    import mi355.da_step as ds
    from mi355 import ops
    from test_gpu_mixup import _host
    runs = {}
    try:
        batches = _batches(gpu, 4)
        # off, constructed without the keyword and with coord=None
        for name in ('off', 'off_kw'):
            orig = ds.DAStep
            if name == 'off_kw':
                class WithKeyword(orig):
                    def __init__(self, *a, **k):
                        super().__init__(*a, coord=None, **k)
                ds.DAStep = WithKeyword
            try:
                model, step, scheds = _training(gpu, with_ema=False)
            finally:
                ds.DAStep = orig
            assert step.coord is None
            out = _host_out(step.run(batches[0]))                       # (the first iteration: what `source` starts from as well)
            for _ in range(3):
                step.run(batches[0])
            torch.cuda.synchronize()
            runs[name] = dict(out=out, log=_logged(step, batches[0]))
        # source: four eager iterations; two eager and two replayed ones
        for name, capture_at in (('eager', None), ('graph', 2)):
            model, step, scheds = _training(gpu, with_ema=False)
            step.coord = ds.CoordRegression(weight=0.5, beta=1.0, delta=1.0)
            rec = []
            for i, b in enumerate(batches):
                if capture_at == i:
                    step.capture(b, warmup=0)
                out = step.run(b)
                for s in scheds.values():
                    s.step()
                torch.cuda.synchronize()
                rec.append(dict(out=_host_out(out), model=_host(model)))
            assert (step.graphs is not None) == (capture_at is not None)
            runs[name] = rec
            if name == 'eager':
                runs['source_log'] = _logged(step, batches[0])
        # both, with and without the consistency term and the teacher-labelled mixup
        for name, kw in (('both', {}), ('both_mt', dict(mt=True)), ('both_mix', dict(mixup=dict(beta=1.0, weight=0.5, labels='teacher'))),
                         ('both_mt_mix', dict(mt=True, mixup=dict(beta=1.0, weight=0.5, labels='teacher')))):
            model, step, scheds = _training(gpu, with_ema=True, **kw)
            step.coord = ds.CoordRegression(weight=0.5, target='teacher', target_weight=0.25, ema=step.ema)
            teacher = step.coord.teacher(step)
            calls = [0]
            fwd = teacher.forward
            teacher.forward = lambda x, fwd=fwd, calls=calls: (calls.__setitem__(0, calls[0] + 1), fwd(x))[1]
            per_iter = []
            for b in batches[:2]:
                calls[0] = 0
                out = step.run(b)
                torch.cuda.synchronize()
                per_iter.append(calls[0])
            runs[name] = dict(out=_host_out(out), calls=per_iter, batch={k: v.cpu() for k, v in batches[1].items()},
                              own=step.coord._teacher is not None, mix_own=step.mixup is not None and step.mixup._teacher is not None)
    finally:
        mi355.set_compute_dtype('bf16')
    return runs


def test_step_without_the_term_is_unchanged(step_runs):
    a, b = step_runs['off'], step_runs['off_kw']
    assert set(a['out']) == set(b['out']) and 'loss_coord' not in a['out'] and len(a['out']) > 5
    for k in a['out']:
        assert _same(a['out'][k], b['out'][k]), k
    assert len(a['log']) > 100 and a['log'] == b['log']                 # the same launches, one for one
    assert not any(l.startswith('coord_heatmap') for _, l in a['log'])
    on = [l for _, l in step_runs['source_log']]
    assert sum(l.startswith('coord_heatmap') for l in on) == 1 and len(on) == len(a['log']) + 1      # one launch, nothing else


def test_step_source_term_is_the_reference_and_leaves_loss_s_alone(step_runs):
    first = step_runs['eager'][0]['out']
    assert _same(first['loss_s'], step_runs['off']['out']['loss_s']) and _same(first['y_s'], step_runs['off']['out']['y_s'])
    batches = _batches('cpu', 4)
    for it, rec in enumerate(step_runs['eager']):
        want, ceiling = _coord_ref_loss(rec['out']['y_s'], batches[it]['kp_s'], batches[it]['w_s'], 0.5)
        got = float(rec['out']['loss_coord'])
        print('iteration %d: loss_coord %.8e, float64 reference %.8e, error %.3e, ceiling %.3e' % (it, got, want, abs(got - want), ceiling))
        assert want > 0 and abs(got - want) <= ceiling
    # the term trains backbone and head: the parameters differ from the run without it after one update
    assert len({float(r['out']['loss_coord']) for r in step_runs['eager']}) == 4


def test_step_eager_and_replay_agree_bit_for_bit(step_runs):
    a, b = step_runs['eager'], step_runs['graph']
    for it in range(4):                                                 # iterations 2 and 3 of `graph` are replays, kp_s changes
        for k in ('loss_coord', 'loss_s', 'loss_gt', 'y_s'):
            assert _same(a[it]['out'][k], b[it]['out'][k]), (it, k)
        for k in a[it]['model']:
            assert np.array_equal(a[it]['model'][k].view(np.uint8), b[it]['model'][k].view(np.uint8)), (it, k)


@pytest.mark.parametrize('name', ['both', 'both_mt', 'both_mix', 'both_mt_mix'])
def test_step_target_term_and_one_teacher_forward_per_iteration(gpu, step_runs, name):
    _, ops = _mi()
    r = step_runs[name]
    assert r['calls'] == [1, 1], r['calls']
    assert r['own'] == (name in ('both', 'both_mix')) and not r['mix_own']
    out = r['out']
    assert _same(out['kp_t_ema'], ops.softargmax(out['y_t_ema'].to(gpu), 1.0, 1.0).cpu())
    want, ceiling = _coord_ref_loss(out['y_t'], out['kp_t_ema'], r['batch']['w_t'], 0.25)
    got = float(out['loss_coordt'])
    print('%s: loss_coordt %.8e, float64 reference %.8e, error %.3e, ceiling %.3e' % (name, got, want, abs(got - want), ceiling))
    assert abs(got - want) <= ceiling
    assert 'loss_coord' in out and ('loss_mt' in out) == ('mt' in name) and ('loss_mix' in out) == ('mix' in name)


def test_step_needs_the_key_points(gpu):
    import mi355
    import mi355.da_step as ds
    try:
        model, step, scheds = _training(gpu, with_ema=False)
        step.coord = ds.CoordRegression()
        b = _batches(gpu, 1)[0]
        del b['kp_s']
        with pytest.raises(KeyError, match='kp_s'):
            step.run(b)
    finally:
        mi355.set_compute_dtype('bf16')


# --------------------------------------------------------------------------------------------------------------- command line
def test_train_cli_with_the_coord_switch(gpu, tmp_path):
    """train1.py --synthetic with --coord-loss both: the source key points travel from the loader's meta to the step, the meter
    columns appear with positive values, the graphs are captured; --coord-loss source needs no teacher."""
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(log, extra):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0',
                  '--pretrain_epochs', '1', '--epochs', '1', '--pretrain', str(tmp_path / 'none.pth'), '--log', log]
        r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    values = lambda out, col: [float(v) for v in re.findall(r'Loss \(%s\) (\S+) \(' % col, out)]
    out = run(str(tmp_path / 'both'), ['--coord-loss', 'both', '--ema-update', 'const', '--coord-weight', '0.5', '--coord-target-weight', '0.25'])
    assert 'HIP graphs captured' in out and 'replay six graphs' in out
    for col in ('coord', 'coordt'):
        assert len(values(out, col)) == 3 and all(v > 0 for v in values(out, col)), (col, values(out, col))
    out = run(str(tmp_path / 'source'), ['--coord-loss', 'source', '--coord-delta', '0'])
    assert len(values(out, 'coord')) == 3 and all(v > 0 for v in values(out, 'coord')) and 'Loss (coordt)' not in out
