"""The references and cases of tests/nonfinite_ref.py, without a GPU.

For every case the GPU modules run (test_gpu_conv_exact.py, test_gpu_bn_exact.py, test_gpu_nonfinite.py): the condition of the
case on its float64 reference (a quarter of the elements finite, every named class present), the reference's agreement with
torch in float64 on the same seeded operands (conv2d, torch.nn.grad, batch_norm, relu, threshold_backward), the indicator rule
of the convolution, and that the seeded positions are where the issue wants them (row tiles, padding, column tail, second K
step, every K group and every slab -- the slabs against csrc/conv_plan.h through tests/conv_dispatch_probe.cpp)."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_exact_ref as B
import conv_exact_ref as C
import heatmap_ref as H
import nonfinite_ref as R
import small_exact_ref as S
from test_conv_dispatch_cpu import probe, _probe          # noqa: F401  (the probe fixture builds the host program)


def _same_classes_and_values(a, b, what):
    assert a.shape == b.shape, what
    ca, cb = R.classes(a), R.classes(b)
    assert torch.equal(ca, cb), '%s: %d elements differ in class' % (what, int((ca != cb).sum()))
    fin = ca == R.FINITE
    assert torch.equal(a[fin], b[fin]), what


# ---------------------------------------------------------------------------------------------- the rules themselves
def test_classes_and_rules():
    t = torch.tensor([0.0, -1.5, R.INF, -R.INF, R.NAN, 3.0])
    assert R.classes(t).tolist() == [0, 0, 1, 2, 3, 0]
    ref = t.double()
    assert R.pointwise_mismatch(t.clone(), ref, torch.float32) is None
    for i, v in ((0, -0.0), (1, -1.25), (2, R.NAN), (3, R.INF), (4, 0.0), (4, R.INF)):          # one element wrong: a sign of zero, a value, every class
        bad = t.clone()
        bad[i] = v
        assert R.pointwise_mismatch(bad, ref, torch.float32) is not None, (i, v)
    assert R.pointwise_mismatch(t.to(torch.bfloat16), ref, torch.bfloat16) is None
    assert R.pointwise_mismatch(t, ref, torch.bfloat16) is not None
    # reduced: any non-finite value where the reference is non-finite, nothing else
    got = torch.tensor([0.0, -1.5, R.NAN, R.NAN, R.INF, 3.0])
    assert R.reduced_mismatch(got, ref) is None
    assert R.reduced_mismatch(torch.tensor([0.0, -1.5, 1.0, R.NAN, R.INF, 3.0]), ref) is not None       # swallowed
    assert R.reduced_mismatch(torch.tensor([R.NAN, -1.5, R.NAN, R.NAN, R.INF, 3.0]), ref) is not None    # invented
    assert R.reduced_mismatch(torch.tensor([0.0, -1.5, R.NAN, R.NAN, R.INF, 3.5]), ref) is not None
    assert R.reduced_mismatch(torch.tensor([0.0, -1.5, R.NAN, R.NAN, R.INF, 3.00001]), ref, rtol=1e-5) is None
    with pytest.raises(AssertionError):
        R.case_condition(torch.tensor([R.NAN, R.NAN, R.NAN, R.NAN, 1.0]), ('nan',))
    with pytest.raises(AssertionError):
        R.case_condition(torch.tensor([R.NAN, 1.0, 1.0, 1.0]), ('nan', '+inf'))
    R.case_condition(torch.tensor([R.NAN, R.INF, 1.0, 1.0]), ('nan', '+inf'))


def test_where_variants_against_aten():
    g = torch.tensor([1.0, R.NAN, R.INF, -2.0, R.NAN, -R.INF], dtype=torch.float64)
    y = torch.tensor([1.0, 0.0, -1.0, 2.0, 3.0, 0.0], dtype=torch.float64)
    sel = R.relu_bwd_select(g, y > 0)
    assert R.classes(sel).tolist() == [0, 0, 0, 0, 3, 0]
    _same_classes_and_values(sel, torch.ops.aten.threshold_backward(g, y, 0.0), 'threshold_backward')
    assert R.classes(g * (y > 0)).tolist() == [0, 3, 3, 0, 3, 3]          # what multiplying by the mask keeps: wrong here
    v = torch.tensor([-1.0, R.NAN, R.INF, -R.INF, 2.0, -0.0], dtype=torch.float64)
    _same_classes_and_values(R.relu_keep_nan(v), torch.relu(v), 'relu')
    assert R.classes(R.relu_keep_nan(v)).tolist() == [0, 3, 1, 0, 0, 0]
    base, bits = torch.tensor([R.NAN, R.NAN, 4.0, R.INF]), torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64)
    out = R.dgrad_epilogue_where(torch.ones(4, dtype=torch.float64), 1.0, base, bits)
    assert out.tolist()[0] == 1.0 and out.tolist()[2:] == [5.0, 1.0] and bool(out[1] != out[1])
    assert R.classes(C.dgrad_epilogue(torch.ones(4, dtype=torch.float64), 1.0, base, bits)).tolist() == [3, 3, 0, 3]


# ---------------------------------------------------------------------------------------------- conv cases
def _torch_conv(sp, what):
    c, o = sp['case'], sp['ops']
    N, Ci, Hh, W, Co, k, s, p = c.shape
    x, w, dy = o['x'].double(), o['w'].double(), o['dy'].double()
    if sp['mode'] == 'fwd':
        y = F.conv2d(x, w, None, s, p) + o['bias'].double().view(1, -1, 1, 1) + o['res'].double()
        return torch.relu(y) if what.endswith('relu') else y
    if sp['mode'] in ('dgrad', 'macc'):
        dx = torch.nn.grad.conv2d_input((N, Ci, Hh, W), w, dy, s, p)
        if what == 'dgrad':
            return dx
        if what == 'dgrad*scale':
            return dx * 0.25
        if what == 'dgrad*scale+acc':
            return dx * 0.25 + o['base'].double()
        per = int(what.split('/')[1])
        bits = C.mask_bits(c.mask[per], N, Ci, Hh, W, per)
        return dx + torch.ops.aten.threshold_backward(o['base'].double(), bits, 0.0)
    dw = torch.nn.grad.conv2d_weight(x, (Co, Ci, k, k), dy, s, p).permute(0, 2, 3, 1)
    return dw if what == 'wgrad' else dw + o['dw0'].double()


@pytest.mark.parametrize('spec', R.CONV_SPECIALS, ids=R.special_id)
def test_conv_case(spec):
    sp = R.conv_special(*spec)
    c = sp['case']
    assert sp['refs']
    for what, ref in sp['refs'].items():
        n = R.case_condition(ref, sp['expect'][what], '%s %s' % (R.special_id(spec), what))
        print('\nCLASSES %s %s: %s' % (R.special_id(spec), what, {R.CLASS_NAME[k]: v for k, v in n.items()}))
        _same_classes_and_values(ref, _torch_conv(sp, what), what)
    N, Ci, Hh, W, Co, k, s, p = c.shape
    mode, name, operand = spec
    pos = sp['positions']
    assert set(kd for _, kd in pos) == set(sp['kinds'])
    if mode == 'fwd' and operand == 'x':
        y = C.conv_fwd(sp['ops']['x'], c.w, s, p, c.out_hw)
        assert torch.equal(R.classes(y), R.conv_class_rule(sp['ops']['x'], c.w, s, p, c.out_hw)), 'indicator rule'
        if p > 0:
            assert any(iy == 0 or ix == 0 or iy == Hh - 1 or ix == W - 1 for (n, ch, iy, ix), _ in pos), 'no window touches the padding'
        assert any(ch == Ci - 1 for (n, ch, iy, ix), _ in pos)
        # a contracted index >= 64 (the second K step): any tap but the first, or a channel >= 64
        assert k > 1 or Ci <= 64 or any(ch >= 64 for (n, ch, iy, ix), _ in pos)
        # the first and the last row of a full row tile and a row of the ragged one, in output rows, for both formats' tiles
        M = N * c.Ho * c.Wo
        rows = set((n * c.Ho + min(iy // s, c.Ho - 1)) * c.Wo + min(ix // s, c.Wo - 1) for (n, ch, iy, ix), _ in pos)
        for bm in R._bms(name, 0):
            if M // bm:
                assert {0, bm - 1} <= rows, (bm, sorted(rows))
            if M % bm:
                assert any(r >= M // bm * bm for r in rows), (bm, sorted(rows))
    if mode == 'fwd' and operand in ('bias', 'w'):
        assert any(idx[0] == Co - 1 for idx, _ in pos), 'the last live column'
    if mode == 'macc':
        for per in (4, 8):
            bits = C.mask_bits(c.mask[per], N, Ci, Hh, W, per)
            got = [float(bits[idx]) for idx, _ in pos]
            assert 0.0 in got and 1.0 in got, got
            ref, clean = sp['refs']['dgrad+macc/%d' % per], sp['clean']['dgrad+macc/%d' % per]
            for idx, _ in pos:          # a NaN base under a cleared bit: the clean result, exactly; under a set bit: NaN
                assert (float(ref[idx]) == float(clean[idx])) if float(bits[idx]) == 0.0 else bool(ref[idx] != ref[idx])
            assert int((ref != ref).sum()) == got.count(1.0)
    if 'kg2' in C.EXPECT[name][0][0] and mode == 'fwd':
        K = k * k * Ci
        for ktile in (64, 32):
            if operand == 'w':
                ks = [(i * k + j) * Ci + ci for (o, ci, i, j), _ in pos]
            else:           # an x element meets tap (i, j) in the output pixel (iy + p - i, ix + p - j)
                ks = [(i * k + j) * Ci + ch for (n, ch, iy, ix), _ in pos for i in range(k) for j in range(k)
                      if 0 <= iy + p - i < c.Ho and 0 <= ix + p - j < c.Wo]
            assert R.k_groups_hit(K, ktile, ks) == {0, 1}


def test_weight_gradient_specials_sit_in_every_slab(probe):
    """The slab of a reduction row, from plan_wgrad / wgrad_split of csrc/conv_plan.h (the probe prints rows per split)."""
    specs = [s for s in R.CONV_SPECIALS if s[0] == 'wgrad' and s[2] in ('x', 'dy')]
    keys, lines = [], []
    for mode, name, operand in specs:
        g, N, Ci, Hh, W, Co, k, s, p, out_hw, dgrad = C.CASES[name]
        Ho, Wo = C.out_size(Hh, W, k, k, s, p)
        for dt in ('bf16', 'f32'):
            keys.append((mode, name, operand, dt))
            lines.append('wplan %s %d %d %d %d %d %d %d %d %d %d' % (dt, N, Hh, W, Ci, Co, k, s, p, Ho, Wo))
    got = _probe(probe, lines)
    for i, (mode, name, operand, dt) in enumerate(keys):
        m = re.match(r'(\w+) S(\d+) rows(\d+) M(\d+) ws(\d+)$', got[i + 1][0])
        S_, rps, M = int(m.group(2)), int(m.group(3)), int(m.group(4))
        assert '%s S%d' % (m.group(1), S_) == C.EXPECT[name][0 if dt == 'bf16' else 1][4]
        assert rps == R.wgrad_slab_rows(M, 64 if dt == 'bf16' else 32, S_)
        sp = R.conv_special(mode, name, operand)
        c = sp['case']
        N, Ci, Hh, W, Co, k, s, p = c.shape
        if operand == 'dy':
            rows = [(n * c.Ho + oy) * c.Wo + ox for (n, ch, oy, ox), _ in sp['positions']]
        else:
            rows = [(n * c.Ho + iy // s) * c.Wo + ix // s for (n, ch, iy, ix), _ in sp['positions']]
        assert set(r // rps for r in rows) == set(range(S_)), (name, operand, dt, rows, rps, S_)


@pytest.mark.parametrize('dt_index', [0, 1])
def test_concat_heatmap_and_pgemm_cases(dt_index):
    name = 'cat_64x64'
    c = C.build_cat_case(name)
    N, Ci, Hh, W, Co, k, s, p = c.shape
    for n2 in C.CAT_C2[(torch.bfloat16, torch.float32)[dt_index]]:
        sp = R.cat_special(name, n2, dt_index)
        for what, ref in sp['refs'].items():
            R.case_condition(ref, sp['kinds'], '%s c2=%d %s' % (name, n2, what))
        t = F.conv2d(c.x.double(), c.w.double(), None, s, p) + F.conv2d(sp['x2'].double(), c.w2[n2].double().view(Co, n2, 1, 1))
        _same_classes_and_values(sp['refs']['cat'], t, 'cat')
        assert any(ch == n2 - 1 for (n, ch, oy, ox), _ in sp['positions'])
    if dt_index:
        return
    sp = R.hm_special()
    R.case_condition(sp['refs']['hm'], sp['kinds'], 'hm_120')
    hc = sp['case']
    _same_classes_and_values(sp['refs']['hm'], F.conv2d(sp['x'].double(), hc.w.double(), hc.b.double()), 'hm')
    assert torch.equal(R.classes(C.conv_fwd(sp['x'], hc.w, 1, 0)), R.conv_class_rule(sp['x'], hc.w, 1, 0))
    for name, operand in R.PGEMM_SPECIALS:
        sp = R.pgemm_special(name, operand)
        pc = sp['case']
        for what, ref in sp['refs'].items():
            R.case_condition(ref, sp['expect'][what], '%s %s %s' % (name, operand, what))
        y = F.conv2d(sp['ops']['x'].double(), pc.w.double())
        _same_classes_and_values(sp['refs']['fwd+bias+res+relu'], torch.relu(y + pc.bias.double().view(1, -1, 1, 1) + sp['ops']['res'].double()), name)
        if operand == 'x':
            _same_classes_and_values(sp['refs']['fwd'], y, name)
            if pc.shape[1] > 64:
                assert any(ch >= 64 for (n, ch, iy, ix), _ in sp['positions'])


def test_grouped_weight_gradient_case():
    items, refs = R.grouped_special('wgrad_group')
    clean_items, clean = C.build_grouped_case('wgrad_group')
    for i, ((shape, x, dy, dw0), ref) in enumerate(zip(items, refs)):
        N, Hh, W, Ci, Co, k, s, p, acc, share = shape
        if ref is None:
            continue
        t = torch.nn.grad.conv2d_weight(x.double(), (Co, Ci, k, k), dy.double(), s, p).permute(0, 2, 3, 1)
        for j, (sh2, x2, dy2, _) in enumerate(items):          # the items that accumulate onto this one's gradient
            if sh2[9] == i:
                t = t + torch.nn.grad.conv2d_weight(x2.double(), (sh2[4], sh2[3], sh2[5], sh2[5]), dy2.double(), sh2[6], sh2[7]).permute(0, 2, 3, 1)
        t = t + dw0.double() if (acc and dw0 is not None) else t
        _same_classes_and_values(ref, t, 'item %d' % i)
        if i in (0, 2):
            R.case_condition(ref, R.KINDS, 'wgrad_group item %d' % i)
        else:
            assert torch.equal(ref, clean[i])


def test_store_overflow_case():
    c = R.store_overflow_case()
    e = C.to_dtype(c['ref'], torch.bfloat16)
    n = R.class_counts(e)
    assert n[R.POS_INF] and n[R.NEG_INF] and not n[R.IS_NAN] and 4 * n[R.FINITE] >= e.numel()
    assert torch.equal(e[0, :, 0, 0], c['bias'].to(torch.bfloat16))
    assert bool((e[0, 4, 0, 0] != 0)) and float(e[0, 2, 0, 0]) == S.BF16_MAX


# ---------------------------------------------------------------------------------------------- 21-channel 1x1 kernels
@pytest.mark.parametrize('dt', S.DTS)
def test_pw_cases(dt):
    for kernel, operands in R.PW_OPERANDS.items():
        for operand in operands:
            c = R.pw_special(dt, operand, R.PW_WGRAD_HW if kernel == 'wgrad' else None)
            assert set(kd for _, kd in c['positions']) == set(R.KINDS)
            x, y = c['x'], c['y']
            if kernel == 'c2k':
                ref = S.pw_c2k(x, c['wkc'], c['bias_k'])
                t = F.conv2d(x, c['wkc'].view(c['K'], c['C'], 1, 1), c['bias_k'])
            elif kernel == 'k2c':
                ref = S.pw_k2c(y, c['wck'], c['bias_c'], c['res'])
                t = F.conv2d(y, c['wck'].view(c['C'], c['K'], 1, 1), c['bias_c']) + c['res']
                st = S.slice_stats(S.rne(ref, dt), c['HW'])
                fin = torch.isfinite(st[:, :, 1])
                assert bool(fin.any()) and not bool(fin.all()) and 4 * int(fin.sum()) >= fin.numel()
            elif kernel == 'wgrad':
                ref = S.pw_wgrad(x, y, c['prior_w'])
                t = torch.nn.grad.conv2d_weight(x, (c['K'], c['C'], 1, 1), y).view(c['K'], c['C']) + c['prior_w']
            else:
                ref = S.hm_rowsum(y, c['bias_k'])
                t = sum(y[n, :, i, j] for n in range(y.shape[0]) for i in range(y.shape[2]) for j in range(y.shape[3])) + c['bias_k']
                assert int((~torch.isfinite(ref)).sum()) == 3 and torch.equal(torch.isfinite(ref), torch.isfinite(t))
                continue
            R.case_condition(ref, R.KINDS, '%s %s %s' % (kernel, dt, operand))
            _same_classes_and_values(ref, t, '%s %s' % (kernel, operand))
            if c[operand].dim() == 4:          # the first and the last pixel of a full 64-pixel tile, one of the ragged tile
                px = sorted(i * c['W'] + j for (n, ch, i, j), _ in c['positions'])
                assert px[0] == 0 and 63 in px and any(p_ >= 64 for p_ in px) and (c['HW'] % 64 != 0 or kernel == 'wgrad')


# ---------------------------------------------------------------------------------------------- heat-map kernels
def test_heatmap_references_with_specials():
    bad = R.hm_poisoned_maps()
    B, K = R.HM_SHAPE[:2]
    clean = [(b, k) for b in range(B) for k in range(K) if (b, k) not in bad]
    pred, target = R.hm_inputs('kl pred', 3.0), R.hm_inputs('kl target', 1.0, positive=True)
    for eps in (0.0, 1e-7):
        for p2, t2 in ((R.hm_seed(pred), target), (pred, R.hm_seed(target))):
            rows, grad = H.kl(p2, t2, None, eps, 1.0)
            assert all(bool(torch.isfinite(rows[b, k])) and bool(torch.isfinite(grad[b, k]).all()) for b, k in clean)
            assert any(not bool(torch.isfinite(rows[b, k])) for b, k in bad)
            o_rows, o_grad = H.kl(p2, t2, None, eps, 1.0, dtype=torch.float32)          # the float32 oracle: the same finiteness
            assert torch.equal(torch.isfinite(o_rows), torch.isfinite(rows)) and torch.equal(torch.isfinite(o_grad), torch.isfinite(grad))
    hm = R.hm_seed(R.hm_inputs('decode', 0.05))
    uv = H.soft_argmax(hm)
    assert not bool(torch.isfinite(uv[0, 3]).any()) and not bool(torch.isfinite(uv[0, 20]).any()) and bool(torch.isfinite(uv[1, 5]).all())
    assert all(bool(torch.isfinite(uv[b, k]).all()) for b, k in clean)
    x2 = R.hm_seed(R.hm_inputs('bilinear'))
    for size in (32, 64):
        ref = H.bilinear(x2, size)
        R.case_condition(ref, R.KINDS, 'bilinear %d' % size)
        nf = (~torch.isfinite(ref)).view(B, K, -1).any(2)
        assert sorted((int(b), int(k)) for b, k in nf.nonzero()) == sorted(bad)
    # pseudo labels: numpy's clip and max keep a NaN (the rule mi355_pseudo_label follows)
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 64, (B, K, 2)).astype(np.float32)
    extra = (rng.standard_normal((B, K, 16, 16)) * 0.3).astype(np.float32)
    for b, k, i, j, kd in R.HM_SPECIALS:
        extra[b, k, i, j] = R.SPECIAL[kd]
    for norm, count in ((0, 1), (1, 256), (2, 1)):
        _, gf = H.labels(xy, 3.0, 2, 4, 16, 1, extra, norm)
        assert np.isnan(gf[0, 3]).sum() == count and np.isfinite(gf[0, 20]).all() and np.isfinite(gf[1, 5]).all()
    _, gf = H.labels(xy, 3.0, 2, 4, 16, 1, extra, 0)
    assert gf[0, 20, 15, 15] == 1.0 and gf[1, 5, 0, 0] == 0.0
    # and torch agrees with numpy there (the reference model's own operations)
    t = torch.tensor([float('nan'), float('inf'), -float('inf'), 0.5])
    assert np.array_equal(np.isnan(t.clip(min=0., max=1.).numpy()), [True, False, False, False]) and bool(torch.isnan(torch.max(t)))


# ---------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize('rows,C', [(3, 64), (315, 64), (315, 192)])
def test_batchnorm_training_forward_against_torch(rows, C):
    """An Inf in one channel and a NaN in another: torch's batch_norm in float64 gives those channels entirely NaN and their
    running statistics non-finite, as bn_exact_ref.train_fwd does; every other channel is untouched."""
    s = B.stats_case(rows, C)
    x2 = R.seed_specials(s['x'], [((rows - 1, C - 1), '+inf'), ((rows // 2, 0), 'nan')])
    rm0, rv0 = B.int_prior(C, 'rm'), B.int_prior(C, 'rv').abs() + 1
    for updates in (1, 2):
        ref = B.train_fwd(x2, s['gamma'], s['beta'], rm0=rm0, rv0=rv0, repeats=updates)
        clean = B.train_fwd(s['x'], s['gamma'], s['beta'], rm0=rm0, rv0=rv0, repeats=updates)
        rm, rv = rm0.clone(), rv0.clone()
        for _ in range(updates):
            y = F.batch_norm(B.nchw(x2), rm, rv, s['gamma'], s['beta'], True, B.MOMENTUM, B.EPS)
        y = B.rows_of(y)
        bad = [0, C - 1]
        ok = [ch for ch in range(C) if ch not in bad]
        assert bool((y[:, bad] != y[:, bad]).all()) and bool((ref['y'][:, bad] != ref['y'][:, bad]).all())
        assert 4 * int(torch.isfinite(ref['y']).sum()) >= ref['y'].numel()
        assert torch.allclose(y[:, ok], ref['y'][:, ok], rtol=1e-12, atol=1e-12) and torch.equal(ref['y'][:, ok], clean['y'][:, ok])
        for got, mine in ((rm, ref['rm']), (rv, ref['rv'])):
            assert torch.equal(torch.isfinite(got), torch.isfinite(mine)) and not bool(torch.isfinite(mine[bad]).any())
            assert torch.allclose(got[ok], mine[ok], rtol=1e-12, atol=1e-12)
        for k in ('mean', 'invstd'):
            assert not bool(torch.isfinite(ref[k][bad]).any()) and torch.equal(ref[k][ok], clean[k][ok])


@pytest.mark.parametrize('relu', [0, 1, 2])
@pytest.mark.parametrize('rows,C', [(315, 64), (256, 64)])
def test_batchnorm_backward_reference_with_specials(rows, C, relu):
    c = B.make_case(rows, C)
    keep = None if relu == 0 else (c['ypre'] > 0 if relu == 2 else B.fwd_y(c, True, True) > 0)
    clean = R.bn_bwd_select(c, keep)
    old = B.bn_bwd(c, keep)
    for k in ('dx', 'dres', 'dgamma', 'dbeta'):
        assert torch.equal(clean[k], old[k])          # on the integers the select and the product are one function
    (r, ch), _ = R.bn_positions(rows, C, keep, True)
    assert ch == C - 1 and (keep is None or bool(keep[r, ch]))
    a = R.bn_bwd_select(dict(c, dy=R.seed_specials(c['dy'], [((r, ch), 'nan')])), keep)
    assert bool((a['dx'][:, ch] != a['dx'][:, ch]).all()) and not bool(torch.isfinite(a['dgamma'][ch])) and not bool(torch.isfinite(a['dbeta'][ch]))
    ok = [q for q in range(C) if q != ch]
    assert torch.equal(a['dx'][:, ok], clean['dx'][:, ok]) and torch.equal(a['dgamma'][ok], clean['dgamma'][ok])
    assert 4 * int(torch.isfinite(a['dx']).sum()) >= a['dx'].numel()
    # the same through autograd's threshold_backward: the masked gradient torch hands the BatchNorm backward
    if keep is not None:
        masked = R.bn_positions(rows, C, keep, False)
        assert all(not bool(keep[p]) for p in masked) and sorted(p[1] for p in masked) == [0, C - 1]
        dy2 = R.seed_specials(c['dy'], [(p, 'nan') for p in masked])
        b = R.bn_bwd_select(dict(c, dy=dy2), keep)
        for k in ('dx', 'dres', 'dgamma', 'dbeta'):
            assert torch.equal(b[k], clean[k]), k
        assert torch.equal(b['dres'], torch.ops.aten.threshold_backward(dy2, keep.double(), 0.0))
        assert not bool(torch.isfinite(B.bn_bwd(dict(c, dy=dy2), keep)['dbeta']).all())          # what the multiplying reference would say
    x2 = R.seed_specials(c['x'], [((rows // 2, C - 1), '+inf')])
    keep2 = keep if relu != 2 else ((x2 - c['mean']) * c['invstd'] * c['gamma'] + c['beta']) > 0
    e = R.bn_bwd_select(dict(c, x=x2), keep2)
    assert not bool(torch.isfinite(e['dgamma'][C - 1])) and not bool(torch.isfinite(e['dx'][:, C - 1]).any())
    assert bool(torch.isfinite(e['dbeta']).all()) and torch.equal(e['dx'][:, :C - 1], clean['dx'][:, :C - 1])


def test_maxpool_case_of_the_fused_batchnorm():
    """The specials of test_gpu_bn_exact.test_bn_relu_maxpool_with_specials survive BatchNorm + ReLU as the test assumes."""
    s = B.stats_case(256, 64)
    g = s['gamma']
    # +Inf under a positive gamma or -Inf under a negative one leaves the ReLU as +Inf: channels 45 and 9 (+Inf), 18 and 0 (-Inf)
    assert bool(g[45] > 0) or bool(g[9] > 0) or bool(g[18] < 0) or bool(g[0] < 0)
    x = torch.tensor([[R.NAN, 1.0, R.INF], [2.0, R.NAN, -R.INF], [0.0, 0.0, 0.0]], dtype=torch.float64).view(1, 1, 3, 3)
    y, code = S.maxpool_fwd(x)
    assert bool(y[0, 0, 0, 0] != y[0, 0, 0, 0]) and int(code[0, 0, 0, 0]) == 8 and int(code[0, 0, 1, 1]) == 0          # the last NaN of a window is kept: (1, 1), not (0, 0)
    assert float(y[0, 0, 0, 1]) != float(y[0, 0, 0, 1]) and int(code[0, 0, 0, 1]) == 6         # a NaN beats the +Inf beside it
