"""mi355_softargmax_backward, mi355_bone_prior, mi355_bone_stats_update, uda.model.loss.BonePriorLoss and the KinematicPrior term
of the training step, against the float64 reference of tests/bone_ref.py.

Forms of the backward.  `row_form()` of csrc/heatmap.hip picks the register-resident kernel of the map size (64 x 64: block per
map; 32 x 32 and 16 x 16: wave per map) for 16-byte-aligned `pred` and `grad`, and the loop kernel for any other size or pointer.
Every case runs from aligned buffers, with `pred` one float past a 16-byte boundary and with `grad` one float past it; rows 1, 4
and 5 give the wave-per-map forms a partial workgroup.  Operands and outputs live in the 0xFF-filled guard buffers of
tests/guarded.py: the flanks must survive and every output word must be written.  Every call is made twice and must give the
same bits.

Ceilings: tests/test_bone_cpu.py.  The backward: 8 x the float32 CPU expression's error on the same inputs + 2^-23 max |ref|.
The bone kernels: per element 2^-23 |ref| + 2^-40 x the largest |ref| of the sample.  The kernel's error is printed beside each
ceiling, and whether the bone kernels are in fact bit for bit.

BonePriorLoss is three launches in a chain, and each link is held to its own float64 reference on the operands the link before
it produced: the soft-arg-max to the project's 1e-3 + 1e-4 |ref|; the loss rows and d loss / d uv to the bone ceiling on that
very uv; the heat-map gradient to the backward's ceiling on the float64 d loss / d uv, widened by what the bone ceiling lets
through the (linear) backward."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bone_ref as R
import coord_ref as C
import guarded
from conftest import PKG
from test_bone_cpu import BONE_CASES, BWD_CASES, TABLES, backward_yardstick, bone_bound, bone_yardstick
from test_coord_cpu import SIDES, coord_yardstick

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


def _backward(mi, gpu, pred, g_uv, beta, align='aligned', nan_ok=False):
    """Two launches on the same guarded buffers -> grad on the CPU."""
    rows, H, W = pred.shape
    s_pred, s_grad = ALIGN[align]
    p = guarded.place(pred.to(gpu), 'pred', start=s_pred)
    u = guarded.place(g_uv.to(gpu), 'g_uv')
    assert p.data_ptr() % 16 == s_pred % 16
    g = guarded.empty((rows, H, W), torch.float32, gpu, 'grad', start=s_grad)
    outs = []
    for _ in range(2):
        mi.call('mi355_softargmax_backward', mi.ptr(p), mi.ptr(u), float(beta), mi.ptr(g), rows, H, W, mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append(g.cpu().clone())
    guarded.check('softargmax_backward %dx%d rows %d %s' % (H, W, rows, align))
    assert nan_ok or guarded.unwritten(g) == 0                # (0xFF.. is a NaN: the NaN tests make their own check)
    assert _same(outs[0], outs[1]), 'two launches, different bits'
    return outs[0]


# ------------------------------------------------------------------------------------------------- soft-arg-max backward
@pytest.mark.parametrize('side', SIDES, ids=lambda s: '%dx%d' % s)
def test_backward_every_form_within_the_yardstick_ceiling(gpu, side):
    mi, _ = _mi()
    worst = 0.0
    for case in [c for c in BWD_CASES if (c[0], c[1]) == side]:
        H, W, rows, beta = case
        y = backward_yardstick(*case)
        for align in ALIGN:
            got = _backward(mi, gpu, y['pred'], y['g_uv'], beta, align)
            err = float((got.double() - y['ref']).abs().max())
            print('%dx%d rows %d beta %g %s: error %.3e, ceiling %.3e (float32 CPU expression %.3e)' % (H, W, rows, beta, align, err, y['bound'], y['yard']))
            assert err <= y['bound']
            worst = max(worst, err / y['bound'])
            if rows > 2:                                      # the zero row: +0, every bit
                assert int(_bits(got[2]).abs().max()) == 0
    print('%dx%d: worst error %.2f of its ceiling' % (side + (worst,)))


@pytest.mark.parametrize('side', SIDES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('delta', [0.0, 1.0])
def test_backward_with_the_coordinate_loss_factors_is_its_unit_grad(gpu, side, delta):
    """g_uv = coef * w * h'(uv - coord), built in float32 from the coordinate kernel's own uv as that kernel builds it: the two
    gradients then agree within the ceiling tests/test_gpu_coord.py holds unit_grad to."""
    mi, ops = _mi()
    H, W = side
    y = coord_yardstick(H, W, 5, 1.0, delta, 'mixed')
    B = 5
    rows, unit, uv = ops.coord_heatmap(y['pred'].view(1, B, H, W).to(gpu), y['coord'].view(1, B, 2).to(gpu), y['weight'].view(1, B).to(gpu),
                                       1.0, delta, float(y['coef']) * B, want_grad=True)
    d = uv.cpu().view(B, 2) - y['coord']
    dh = torch.where(d.abs() < delta, d / max(delta, 1e-30), torch.sign(d)) if delta > 0 else torch.sign(d)
    g_uv = ((y['weight'][:, None] * dh) * float(y['coef'])).float()
    for align in ALIGN:
        got = _backward(mi, gpu, y['pred'], g_uv, 1.0, align)
        err = float((got.double() - unit.cpu().view(B, H, W).double()).abs().max())
        err_ref = float((got.double() - y['ref_grad']).abs().max())
        print('%dx%d delta %g %s: |backward - unit_grad| %.3e, |backward - float64 reference| %.3e, ceiling %.3e' % (H, W, delta, align, err, err_ref, y['bound_grad']))
        assert err <= y['bound_grad']
        assert int(_bits(got[2]).abs().max()) == 0            # the row of weight 0


@pytest.mark.parametrize('side', SIDES, ids=lambda s: '%dx%d' % s)
def test_backward_zero_row_is_plus_zero_and_a_nan_stays_in_its_row(gpu, side):
    mi, _ = _mi()
    H, W = side
    y = backward_yardstick(H, W, 5, 1.0)
    for align in ALIGN:
        pred = y['pred'].clone()
        pred[2] = float('nan')                                # the zero-g_uv row: never read
        pred[2, 0, 0] = float('inf')
        got = _backward(mi, gpu, pred, y['g_uv'], 1.0, align)
        assert int(_bits(got[2]).abs().max()) == 0 and torch.isfinite(got).all()
        clean = _backward(mi, gpu, y['pred'], y['g_uv'], 1.0, align)
        assert _same(got, clean)
        pred[3, H - 1, W - 1] = float('nan')                  # a NaN in a live row: the whole row, and no other
        got = _backward(mi, gpu, pred, y['g_uv'], 1.0, align, nan_ok=True)
        assert bool(torch.isnan(got[3]).all()) and _same(got[[0, 1, 2, 4]], clean[[0, 1, 2, 4]])
        g_uv = y['g_uv'].clone()
        g_uv[0, 1] = float('nan')                             # ... and a NaN of the upstream gradient likewise
        got = _backward(mi, gpu, y['pred'], g_uv, 1.0, align, nan_ok=True)
        assert bool(torch.isnan(got[0]).all()) and _same(got[1:], clean[1:])


def test_backward_refused_arguments(gpu):
    mi, ops = _mi()
    t = torch.zeros(2, 3, 4, 4, device=gpu)
    g = torch.zeros(2, 3, 2, device=gpu)
    for beta in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(mi.Mi355Error, match='softargmax_backward'):
            ops.softargmax_backward(t, g, beta)
    with pytest.raises(mi.Mi355Error, match='gradient'):
        ops.softargmax_backward(t, g[:, :2], 1.0)
    for a in ((None, g, t), (t, None, t), (t, g, None)):
        with pytest.raises(mi.Mi355Error, match='null'):
            mi.call('mi355_softargmax_backward', mi.ptr(a[0]), mi.ptr(a[1]), 1.0, mi.ptr(a[2]), 6, 4, 4, mi.stream_ptr())
    for shape in ((0, 4, 4), (6, 0, 4), (6, 4, -1), (1, 46341, 46341)):
        with pytest.raises(mi.Mi355Error, match='softargmax_backward'):
            mi.call('mi355_softargmax_backward', mi.ptr(t), mi.ptr(g), 1.0, mi.ptr(t), *shape, mi.stream_ptr())


# ------------------------------------------------------------------------------------------------------ the bone kernels
def _table(gpu, bones):
    return guarded.place(torch.tensor(bones, dtype=torch.int32).to(gpu), 'bones')


def _prior(mi, gpu, uv, w, bones, mean, var, seen, margin, eps, coef, want_grad=True):
    """Two launches on the same guarded buffers -> (loss_rows, g_uv or None) as float32 numpy arrays."""
    B, K, _ = uv.shape
    d = lambda a, n: guarded.place(torch.from_numpy(np.ascontiguousarray(a)).to(gpu), n)
    u, t, m, v, s = d(uv, 'uv'), _table(gpu, bones), d(mean, 'mean'), d(var, 'var'), d(seen, 'seen')
    wt = None if w is None else d(w, 'weight')
    rows = guarded.empty((B,), torch.float32, gpu, 'loss_rows')
    g = guarded.empty((B, K, 2), torch.float32, gpu, 'g_uv') if want_grad else None
    outs = []
    for _ in range(2):
        mi.call('mi355_bone_prior', mi.ptr(u), mi.ptr(wt), mi.ptr(t), mi.ptr(m), mi.ptr(v), mi.ptr(s), float(margin), float(eps), float(coef),
                mi.ptr(rows), mi.ptr(g), B, K, len(bones), mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append((rows.cpu().clone(), None if g is None else g.cpu().clone()))
    guarded.check('bone_prior B%d K%d E%d' % (B, K, len(bones)))
    for a, b in zip(*outs):
        assert a is None or _same(a, b), 'two launches, different bits'
    for t_ in (rows, g):
        assert t_ is None or guarded.unwritten(t_) == 0 or not torch.isfinite(t_).all()
    return outs[0][0].numpy(), None if g is None else outs[0][1].numpy()


def _stats(mi, gpu, kp, w, bones, mean, var, seen, rho):
    """One launch on guarded buffers (the launch updates in place: its second run is another update) -> (mean, var, seen)."""
    B, K, _ = kp.shape
    d = lambda a, n: guarded.place(torch.from_numpy(np.ascontiguousarray(a)).to(gpu), n)
    u, t = d(kp, 'kp'), _table(gpu, bones)
    wt = None if w is None else d(w, 'weight')
    outs = []
    for _ in range(2):
        m, v, s = d(np.asarray(mean, np.float32), 'mean'), d(np.asarray(var, np.float32), 'var'), d(np.asarray(seen, np.int32), 'seen')
        mi.call('mi355_bone_stats_update', mi.ptr(u), mi.ptr(wt), mi.ptr(t), mi.ptr(m), mi.ptr(v), mi.ptr(s), float(rho), B, K, len(bones),
                mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append(tuple(x.cpu().clone() for x in (m, v, s)))
        guarded.check('bone_stats_update B%d K%d E%d' % (B, K, len(bones)))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'two launches, different bits'
    return tuple(x.numpy() for x in outs[0])


def _within(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    exact = bool((got == ref.astype(np.float32)).all())
    assert (err <= bound).all(), '%s: error %.3e over its ceiling %.3e' % (what, (err - bound).max(), bound.max())
    return float(err.max()), exact


@pytest.mark.parametrize('B', [1, 3, 5])
@pytest.mark.parametrize('table', ['hand', 'chain'])
def test_bone_prior_every_case_within_the_ceiling(gpu, B, table):
    mi, _ = _mi()
    n = n_exact = 0
    for case in [c for c in BONE_CASES if c[0] == B and c[1] == table]:
        for collapsed in (False, True):
            y = bone_yardstick(*case, collapsed=collapsed)
            rows, g = _prior(mi, gpu, y['uv'], y['w'], y['bones'], y['mean'], y['var'], y['seen'], y['margin'], y['eps'], y['coef'])
            e_r, x_r = _within(rows, y['ref_rows'], y['bound_rows'], 'loss rows %r' % (case,))
            e_g, x_g = _within(g, y['ref_grad'], y['bound_grad'], 'gradient %r' % (case,))
            skipped = y['ref_rows'] == 0
            assert not rows[skipped].any() and not g[skipped].any() and not np.signbit(g[skipped]).any()      # exactly +0
            n, n_exact = n + 1, n_exact + (x_r and x_g)
            print('%r collapsed %s: rows error %.3e, gradient error %.3e (ceilings %.3e, %.3e), bit for bit: %s'
                  % (case, collapsed, e_r, e_g, y['bound_rows'].max(), y['bound_grad'].max(), x_r and x_g))
            # without the gradient and without weights: the same rows
            if not collapsed and case[2] == 'all':
                rows2, none = _prior(mi, gpu, y['uv'], None, y['bones'], y['mean'], y['var'], y['seen'], y['margin'], y['eps'], y['coef'], want_grad=False)
                assert none is None and rows2.tobytes() == rows.tobytes()
    print('B %d %s: %d of %d cases equal float32(float64 reference) bit for bit' % (B, table, n_exact, n))


@pytest.mark.parametrize('name', R.EXACT)
def test_bone_prior_exact_cases_bit_for_bit(gpu, name):
    mi, _ = _mi()
    e = R.exact_case(name)
    ref_rows, ref_g = R.bone_prior(e['uv'], None, e['bones'], e['mean'], e['var'], e['seen'], e['margin'], e['eps'], 1.0)
    rows, g = _prior(mi, gpu, e['uv'], None, e['bones'], e['mean'], e['var'], e['seen'], e['margin'], e['eps'], 1.0)
    assert rows.tobytes() == np.asarray([e['loss']], np.float32).tobytes()
    assert g.tobytes() == ref_g.astype(np.float32).tobytes()
    assert (name == 'inside') == (not g.any())


def test_bone_prior_nan_stays_in_its_sample_and_selection_is_by_selection(gpu):
    mi, _ = _mi()
    y = bone_yardstick(3, 'hand', 'invisible', 0.0, ())
    clean_rows, clean_g = _prior(mi, gpu, y['uv'], y['w'], y['bones'], y['mean'], y['var'], y['seen'], 0.0, y['eps'], y['coef'])
    uv = y['uv'].copy()
    live = [j for j in range(21) if y['w'][1, j] > 0][3]
    uv[1, live, 0] = np.nan                                   # a present bone of sample 1
    dead = [j for j in range(21) if y['w'][0, j] == 0][0]
    uv[0, dead] = np.nan                                      # an invisible joint of sample 0: selected out
    rows, g = _prior(mi, gpu, uv, y['w'], y['bones'], y['mean'], y['var'], y['seen'], 0.0, y['eps'], y['coef'])
    assert np.isnan(rows[1]) and np.isnan(g[1]).any()
    assert rows[[0, 2]].tobytes() == clean_rows[[0, 2]].tobytes() and g[[0, 2]].tobytes() == clean_g[[0, 2]].tobytes()
    # the statistics of an unseen bone are never read: NaN there changes nothing
    y = bone_yardstick(3, 'hand', 'all', 1.0, (1,))
    a = _prior(mi, gpu, y['uv'], y['w'], y['bones'], y['mean'], y['var'], y['seen'], 1.0, y['eps'], y['coef'])
    mean, var = y['mean'].copy(), y['var'].copy()
    mean[1] = var[1] = np.nan
    b = _prior(mi, gpu, y['uv'], y['w'], y['bones'], mean, var, y['seen'], 1.0, y['eps'], y['coef'])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('table', ['hand', 'chain'])
def test_bone_statistics_first_batch_blend_untouched_bone_and_seen(gpu, table):
    mi, _ = _mi()
    bones, K = TABLES[table]
    E = len(bones)
    state = (np.zeros(E, np.float32), np.zeros(E, np.float32), np.zeros(E, np.int32))
    n_exact = 0
    for it, (B, wcase) in enumerate(((3, 'invisible'), (5, 'all'), (1, 'all'), (5, 'onebone'), (3, 'invisible'))):
        kp = R.hands(B, K, seed=40 + it)
        w = R.weights_case(B, K, bones, wcase)
        if it == 0:
            w[:, bones[-1][1]] = 0.0                          # the last bone is shown by nobody in the first batch
        want = R.bone_stats_update(kp, w, bones, *state, 0.25)
        got = _stats(mi, gpu, kp, w, bones, *state, 0.25)
        touched = want[2] != state[2]
        if it == 0:
            assert state[2].sum() == 0 and got[2][-1] == 0 and got[0][-1] == 0 and got[2][:-1].all()      # seen flips on the device
        if it == 1:
            assert touched[-1] and got[2].all()               # ... and the late bone takes its first batch whole
        assert np.array_equal(got[2], want[2])
        for name, g_, w_ in (('mean', got[0], want[0]), ('var', got[1], want[1])):
            err = np.abs(g_.astype(np.float64) - w_.astype(np.float64))
            bound = 2.0 ** -23 * np.abs(w_.astype(np.float64)) + 2.0 ** -40 * float(np.abs(w_).max())
            assert (err <= bound).all(), (it, name, err.max())
            n_exact += int(g_.tobytes() == w_.tobytes())
        state = got
    print('%s: %d of 10 statistics vectors equal the float64 reference rounded once, bit for bit' % (table, n_exact))
    # a batch whose every sample is skipped touches nothing
    kp = R.hands(2, K, seed=50)
    w = np.zeros((2, K), np.float32)
    same = _stats(mi, gpu, kp, w, bones, *state, 0.25)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(same, state))


def test_bone_refused_arguments(gpu):
    mi, ops = _mi()
    uv = torch.zeros(2, 21, 2, device=gpu)
    bones = torch.tensor(R.HAND, dtype=torch.int32, device=gpu)
    mean, var, seen = torch.zeros(20, device=gpu), torch.zeros(20, device=gpu), torch.zeros(20, dtype=torch.int32, device=gpu)
    for kw in (dict(margin=-1.0), dict(margin=float('inf')), dict(eps=0.0), dict(eps=float('nan')), dict(coef=float('inf'))):
        with pytest.raises(mi.Mi355Error, match='bone_prior'):
            ops.bone_prior(uv, None, bones, mean, var, seen, **kw)
    for rho in (-0.5, 1.5, float('nan')):
        with pytest.raises(mi.Mi355Error, match='rho'):
            ops.bone_stats_update(uv, None, bones, mean, var, seen, rho)
    with pytest.raises(mi.Mi355Error, match='int32'):
        ops.bone_prior(uv, None, bones.long(), mean, var, seen)
    with pytest.raises(mi.Mi355Error, match='mean'):
        ops.bone_prior(uv, None, bones, mean[:5], var, seen)
    with pytest.raises(mi.Mi355Error, match='weights'):
        ops.bone_prior(uv, torch.zeros(2, 20, device=gpu), bones, mean, var, seen)
    with pytest.raises(mi.Mi355Error, match='K=33'):
        ops.bone_prior(torch.zeros(2, 33, 2, device=gpu), None, bones, mean, var, seen)
    big = torch.zeros(33, 2, dtype=torch.int32, device=gpu)
    with pytest.raises(mi.Mi355Error, match='E=33'):
        ops.bone_stats_update(uv, None, big, torch.zeros(33, device=gpu), torch.zeros(33, device=gpu), torch.zeros(33, dtype=torch.int32, device=gpu), 0.1)
    # a table entry outside the joints is no bone: nothing is read or written out of bounds, the sample keeps its other bones
    mi_, _ = _mi()
    y = bone_yardstick(3, 'chain', 'all', 0.0, ())
    wild = ((0, 1), (1, 2), (2, 3), (3, 400), (-7, 2))
    mean5, var5 = np.append(y['mean'], [1.0, 1.0]).astype(np.float32), np.append(y['var'], [0.1, 0.1]).astype(np.float32)
    rows, g = _prior(mi_, gpu, y['uv'], y['w'], wild, mean5, var5, np.ones(5, np.int32), 0.0, y['eps'], y['coef'])
    _within(rows, y['ref_rows'], y['bound_rows'], 'loss rows beside wild table entries')
    _within(g, y['ref_grad'], y['bound_grad'], 'gradient beside wild table entries')
    got = _stats(mi_, gpu, y['uv'], y['w'], wild, np.zeros(5), np.zeros(5), np.zeros(5), 0.5)
    assert got[2].tolist() == [1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------- BonePriorLoss
def _loss_reference(pred, uv32, w, stats, margin, eps, beta, scale):
    """From heat-maps pred (B, K, H, W), the float32 soft-arg-max the kernel gave and the statistics: the float64 loss, its
    ceiling, the float64 heat-map gradient and its elementwise ceiling (the chain of the module docstring)."""
    B, K, H, W = pred.shape
    bones, (mean, var, seen) = stats
    k = R.f32(R.f32(scale) / B)
    rows, g_uv = R.bone_prior(uv32, w, bones, mean, var, seen, margin, eps, k)
    b_rows = bone_bound(rows)
    loss = float(rows.sum()) * k
    b_loss = k * (float(b_rows.sum()) + (B + 1) * 2.0 ** -24 * float(np.abs(rows).sum()))
    p = pred.reshape(B * K, H, W)
    g64 = torch.from_numpy(g_uv.reshape(B * K, 2))
    g32 = g64.float()
    ref = R.softargmax_backward(p, g32, R.f32(beta))
    o32 = R.softargmax_backward(p, g32, R.f32(beta), dtype=torch.float32)
    yard = float((o32.double() - ref).abs().max())
    # what one float32 rounding of g_uv and the bone ceiling let through: the backward is linear in g_uv
    dg = torch.from_numpy(2 * bone_bound(g_uv).reshape(B * K, 2))
    one = torch.ones(B * K, 2, dtype=torch.float64)
    a_u = R.softargmax_backward(p, one * torch.tensor([1.0, 0.0], dtype=torch.float64), R.f32(beta)).abs()
    a_v = R.softargmax_backward(p, one * torch.tensor([0.0, 1.0], dtype=torch.float64), R.f32(beta)).abs()
    bound = 8.0 * yard + 2.0 ** -23 * float(ref.abs().max()) + a_u * dg[:, 0, None, None] + a_v * dg[:, 1, None, None]
    return loss, b_loss, ref, bound, g_uv


@pytest.mark.parametrize('shape,table', [((2, 21, 64, 64), R.HAND), ((2, 3, 16, 16), ((0, 1), (1, 2))), ((1, 21, 6, 10), R.HAND)],
                         ids=['2x21x64x64-hand', '2x3x16x16-chain', '1x21x6x10-hand'])
def test_bone_prior_loss_and_its_gradient(gpu, shape, table):
    mi, ops = _mi()
    from uda.model.loss import BonePriorLoss, BoneStatistics, bone_prior
    B, K, H, W = shape
    pred = C.maps(H, W, B * K, 1.0, seed=5).view(B, K, H, W)
    w = np.ones((B, K), np.float32)
    if K > 3:
        w[0, 7] = 0.0
    mean, var, seen = R.stats_for(table, seed=2, unseen=(1,) if K > 3 else ())
    stats = BoneStatistics(table, 0.1, device=gpu)
    stats.load_state_dict({'mean': torch.from_numpy(mean), 'var': torch.from_numpy(var), 'seen': torch.from_numpy(seen)})
    crit = BonePriorLoss(beta=1.0, margin=0.25, eps=1e-4)
    for scale, up in ((1.0, None), (0.7, None), (0.7, 1.5)):
        out = pred.to(gpu).clone().requires_grad_(True)
        loss = crit(out, torch.from_numpy(w).view(B, K, 1).to(gpu), stats, scale=scale)
        assert loss.dim() == 0 and not crit.uv.requires_grad
        if up is None:
            loss.backward(mi.unit_grad(loss))
        else:
            (loss * up).backward()
        uv32 = crit.uv.cpu()
        assert _same(uv32, ops.softargmax(out.detach(), 1.0, 1.0).cpu())
        uv64 = R.softargmax(pred.view(B * K, H, W), 1.0)
        assert bool(((uv32.double().view(B * K, 2) - uv64).abs() <= 1e-3 + 1e-4 * uv64.abs()).all())
        want, b_loss, ref, bound, g_uv = _loss_reference(pred, uv32.numpy(), w, (table, (mean, var, seen)), 0.25, 1e-4, 1.0, scale)
        u = 1.0 if up is None else up
        err_l = abs(float(loss.detach()) - want)
        err_g = (out.grad.cpu().double().view(B * K, H, W) - u * ref).abs()
        print('%s scale %g upstream %s: loss %.6e, error %.3e (ceiling %.3e); gradient max %.3e, error %.3e (ceiling %.3e)'
              % (shape, scale, up, want, err_l, b_loss, float(ref.abs().max()), float(err_g.max()), float(bound.max())))
        assert want > 0 and float(ref.abs().max()) > 1e-8 and err_l <= b_loss
        assert bool((err_g <= u * bound * (1 + 2.0 ** -22)).all())
        if K > 3:                                             # the invisible joint takes no gradient: its map is +0
            assert int(_bits(out.grad.cpu()[0, 7]).abs().max()) == 0
        # the function on coordinates gives the same loss and the d loss / d uv the chain went through
        pts = crit.uv.clone().requires_grad_(True)
        l2 = bone_prior(pts, torch.from_numpy(w).to(gpu), stats, margin=0.25, eps=1e-4, scale=scale)
        l2.backward(mi.unit_grad(l2))
        assert _same(l2.detach().cpu(), loss.detach().cpu())
        _within(pts.grad.cpu().numpy(), g_uv, bone_bound(g_uv), 'd loss / d uv')
    with torch.no_grad():                                     # no gradient wanted: none is computed
        again = crit(out.detach(), torch.from_numpy(w).view(B, K, 1).to(gpu), stats, scale=0.7)
    assert float(again) == float(loss.detach())
    with pytest.raises(mi.Mi355Error, match='statistics'):
        crit(out.detach(), None, BoneStatistics(table), scale=1.0)


# ------------------------------------------------------------------------------------------------------------------ the step
def _training(gpu, **kw):
    from test_gpu_mixup import _training as base
    return base(gpu, kw.pop('mixup', None), **kw)


def _batches(gpu, n):
    from test_gpu_coord import _batches as base
    return base(gpu, n)


def _host_out(out):
    return {k: v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)}


def _term(ds):
    return ds.KinematicPrior(weight=0.5, margin=0.25, momentum=0.25, beta=1.0, eps=1e-4)


@pytest.fixture(scope='module')
def step_runs(gpu):
    import mi355
    import mi355.da_step as ds
    from test_gpu_mixup import _host, _logged
    runs = {}
    try:
        batches = _batches(gpu, 5)
        for name in ('off', 'off_kw'):
            orig = ds.DAStep
            if name == 'off_kw':
                class WithKeyword(orig):
                    def __init__(self, *a, **k):
                        super().__init__(*a, bone=None, **k)
                ds.DAStep = WithKeyword
            try:
                model, step, scheds = _training(gpu, with_ema=False)
            finally:
                ds.DAStep = orig
            assert step.bone is None
            out = _host_out(step.run(batches[0]))
            for _ in range(2):
                step.run(batches[0])
            torch.cuda.synchronize()
            runs[name] = dict(out=out, log=_logged(step, batches[0]))
        # on: two eager iterations, then the statistics start over and three more run -- eagerly, or as replays of graphs
        # captured at that point, so that the captured launch meets seen == 0
        for name, graph in (('eager', False), ('graph', True)):
            model, step, scheds = _training(gpu, with_ema=False)
            step.bone = _term(ds)
            rec = []
            for i, b in enumerate(batches):
                if i == 2:
                    step.bone.stats.reset()
                    if graph:
                        step.capture(b, warmup=0)
                out = step.run(b)
                for s in scheds.values():
                    s.step()
                torch.cuda.synchronize()
                rec.append(dict(out=_host_out(out), model=_host(model), stats=step.bone.state_dict()))
            assert (step.graphs is not None) == graph
            runs[name] = rec
            if not graph:
                runs['on_log'] = _logged(step, batches[0])
        # beside the source coordinate loss: one kp_s for both
        model, step, scheds = _training(gpu, with_ema=False)
        step.bone = _term(ds)
        step.coord = ds.CoordRegression(weight=0.5)
        rec = []
        for b in batches[:2]:
            out = step.run(b)
            torch.cuda.synchronize()
            rec.append(dict(out=_host_out(out), stats=step.bone.state_dict()))
        runs['with_coord'] = rec
    finally:
        mi355.set_compute_dtype('bf16')
    return runs


def test_step_without_the_term_is_unchanged(step_runs):
    a, b = step_runs['off'], step_runs['off_kw']
    assert set(a['out']) == set(b['out']) and 'loss_bone' not in a['out'] and len(a['out']) > 5
    for k in a['out']:
        assert _same(a['out'][k], b['out'][k]), k
    assert len(a['log']) > 100 and a['log'] == b['log']                 # the same launches, one for one
    names = ('bone_prior', 'bone_stats_update', 'softargmax_backward')
    assert not any(l.startswith(names) for _, l in a['log'])
    on = [l for _, l in step_runs['on_log']]
    assert [sum(l.startswith(n) for l in on) for n in names] == [1, 1, 1]
    # the first iteration's forward passes do not know the term: what step A and step B compute is the same to the bit
    first = step_runs['eager'][0]['out']
    for k in ('loss_s', 'y_s', 'loss_gf', 'y_t', 'loss_gt'):
        assert _same(first[k], a['out'][k]), k


def test_step_loss_bone_is_the_reference_on_the_kept_y_t(gpu, step_runs):
    _, ops = _mi()
    batches = _batches('cpu', 5)
    state = (np.zeros(20, np.float32), np.zeros(20, np.float32), np.zeros(20, np.int32))
    for it, rec in enumerate(step_runs['eager']):
        if it == 2:
            state = (np.zeros(20, np.float32), np.zeros(20, np.float32), np.zeros(20, np.int32))
        w_s = batches[it]['w_s'].numpy().reshape(2, 21)
        want_state = R.bone_stats_update(batches[it]['kp_s'].numpy(), w_s, R.HAND, *state, 0.25)
        got_state = tuple(rec['stats'][k].numpy() for k in ('mean', 'var', 'seen'))
        assert np.array_equal(got_state[2], want_state[2]) and got_state[2].all()
        for g_, w_ in zip(got_state[:2], want_state[:2]):
            assert (np.abs(g_.astype(np.float64) - w_) <= 2.0 ** -23 * np.abs(w_) + 2.0 ** -40 * np.abs(w_).max()).all()
        state = got_state                                     # (the next link starts from what the device holds)
        out = rec['out']
        assert _same(out['bone_uv_t'], ops.softargmax(out['y_t'].to(gpu).float(), 1.0, 1.0).cpu())
        k = R.f32(R.f32(0.5) / 2)
        rows, _ = R.bone_prior(out['bone_uv_t'].numpy(), batches[it]['w_t'].numpy().reshape(2, 21), R.HAND, *got_state, 0.25, 1e-4, k)
        want = float(rows.sum()) * k
        ceiling = k * (float(bone_bound(rows).sum()) + 3 * 2.0 ** -24 * float(np.abs(rows).sum()))
        got = float(out['loss_bone'])
        print('iteration %d: loss_bone %.8e, float64 reference %.8e, error %.3e, ceiling %.3e' % (it, got, want, abs(got - want), ceiling))
        assert want > 0 and abs(got - want) <= ceiling
    assert len({float(r['out']['loss_bone']) for r in step_runs['eager']}) == 5


def test_step_eager_and_replay_agree_bit_for_bit(step_runs):
    a, b = step_runs['eager'], step_runs['graph']
    assert int(a[1]['stats']['seen'].sum()) == 20
    for it in range(5):                                       # iterations 2, 3, 4 of `graph` are replays; 2 meets seen == 0
        for k in ('loss_bone', 'loss_s', 'loss_gt', 'y_s', 'y_t', 'bone_uv_t'):
            assert _same(a[it]['out'][k], b[it]['out'][k]), (it, k)
        for k in ('mean', 'var', 'seen'):
            assert torch.equal(a[it]['stats'][k], b[it]['stats'][k]), (it, k)
        for k in a[it]['model']:
            assert np.array_equal(a[it]['model'][k].view(np.uint8), b[it]['model'][k].view(np.uint8)), (it, k)
    # the first batch after the reset was taken whole: not the blend the iteration before left
    assert not torch.equal(a[2]['stats']['mean'], a[1]['stats']['mean'])


def test_step_runs_beside_the_source_coordinate_loss(step_runs):
    for it, rec in enumerate(step_runs['with_coord']):
        out = rec['out']
        assert float(out['loss_coord']) > 0 and float(out['loss_bone']) > 0 and np.isfinite(float(out['loss_s']))
        for k in ('mean', 'var', 'seen'):                     # the same kp_s, the same statistics
            assert torch.equal(rec['stats'][k], step_runs['eager'][it]['stats'][k]), (it, k)


def test_step_needs_the_key_points(gpu):
    import mi355
    import mi355.da_step as ds
    try:
        model, step, scheds = _training(gpu, with_ema=False)
        step.bone = _term(ds)
        b = _batches(gpu, 1)[0]
        del b['kp_s']
        with pytest.raises(KeyError, match='kp_s'):
            step.run(b)
    finally:
        mi355.set_compute_dtype('bf16')


# --------------------------------------------------------------------------------------------------------------- command line
def test_train_cli_with_the_bone_switch(gpu, tmp_path):
    """train1.py --synthetic with --bone-loss on: the source key points travel from the loader's meta to the step, the meter column
    appears with finite values, the graphs are captured and the checkpoint holds the statistics."""
    env = dict(os.environ, PYTHONPATH=PKG)
    log = str(tmp_path / 'on')
    cmd = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0',
           '--pretrain_epochs', '1', '--epochs', '1', '--pretrain', str(tmp_path / 'none.pth'), '--log', log, '--bone-loss', 'on',
           '--bone-weight', '0.5', '--bone-momentum', '0.1']
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    values = [float(v) for v in re.findall(r'Loss \(bone\) (\S+) \(', r.stdout)]
    assert 'HIP graphs captured' in r.stdout and 'replay six graphs' in r.stdout
    assert len(values) == 3 and all(np.isfinite(v) and v >= 0 for v in values) and any(v > 0 for v in values), values
    ck = torch.load(os.path.join(log, 'checkpoints', '0.pth'), map_location='cpu', weights_only=False)
    assert int(ck['bone_state']['seen'].sum()) == 20 and torch.isfinite(ck['bone_state']['mean']).all()
