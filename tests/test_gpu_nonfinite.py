"""NaN, +Inf and -Inf through the 21-channel 1x1 kernels (csrc/pw21.hip) and the heat-map decode, loss and label kernels
(csrc/heatmap.hip, the masked MSE of csrc/teacher.hip), by the rules of tests/nonfinite_ref.py.

pw21: one operand at a time carries one NaN, one +Inf and one -Inf; every other value is the exact integer of
small_exact_ref.pw_case.  Outputs that are one sum per element (C -> K, K -> C, the weight gradient) follow the pointwise rule
against float64 matmuls, the bias gradient (hm_rowsum) and the statistics partials of pw_k2c_stats the reduced one.

Heat maps: B = 2, K = 21, 16 x 16, one map per special (nonfinite_ref.HM_SPECIALS).  The references are the float64
restatements of tests/heatmap_ref.py (the CPU oracle's JointsKLLoss under autograd for the KL loss) and tests/mt_ref.py (the
reference's mt_loss) -- uda/model/loss.py itself is the module under test: it launches these kernels.  The loss rows and the
gradient of a poisoned map are non-finite wherever the reference's are, and every clean map has the bits of the run without the
special: a special may not leak into another map's row.

pseudo_label with a non-finite `extra`.  The kernel used to clip and to take the per-map maximum with fminf / fmaxf, which return
the other operand for a NaN: a NaN pixel of `extra` came out as 0 and the map was normalised as if nothing had happened, where
the reference (torch.clip, torch.max: regda_7.py) keeps the NaN in its pixel and, dividing by a NaN maximum, makes the whole
map NaN.  CHOSEN: the kernel follows the reference (selects instead of fminf / fmaxf; test_pseudo_label_with_a_non_finite_extra).
Not the refusal in the wrapper: `extra` is an activation of the model itself, it is non-finite exactly when the run is already
going wrong, the step guard needs that to reach the gradients, and a check in the wrapper would cost a device synchronisation
inside a captured graph.  The reference's behaviour is no accident either: it is what every torch operation in that path does."""
import numpy as np
import pytest
import torch

import heatmap_ref as HR
import mt_ref
import nonfinite_ref as NF
import small_exact_ref as S

pytestmark = pytest.mark.gpu


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def _feat(v64, dt, gpu):
    return S.nhwc(v64, S.TDT[dt]).to(gpu)


def _f32(v64, gpu):
    return v64.float().contiguous().to(gpu)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pointwise(what, got, ref, dtype):
    bad = NF.pointwise_mismatch(got, ref, dtype)
    assert bad is None, '%s: %s' % (what, bad)


def _reduced(what, got, ref, **tol):
    bad = NF.reduced_mismatch(got, ref, **tol)
    assert bad is None, '%s: %s' % (what, bad)


# ================================================================ pw21
@pytest.mark.parametrize('operand', NF.PW_OPERANDS['c2k'])
@pytest.mark.parametrize('dt', S.DTS)
def test_pw_c2k(gpu, dt, operand):
    _, ops = _mi()
    c = NF.pw_special(dt, operand)
    K = c['K']
    ref = S.pw_c2k(c['x'], c['wkc'], c['bias_k'])
    NF.case_condition(ref, NF.KINDS, 'pw_c2k %s' % operand)
    x, b = _feat(c['x'], dt, gpu), _f32(c['bias_k'], gpu)
    y = ops.pw_c2k(x, _f32(c['wkc'], gpu), b, K)
    _pointwise('[K][C]', y, ref, torch.float32)
    y = ops.pw_c2k(x, _f32(c['wkc'].t().contiguous(), gpu), b, K, w_transposed=True)
    _pointwise('[C][K]', y, ref, torch.float32)


@pytest.mark.parametrize('operand', NF.PW_OPERANDS['k2c'])
@pytest.mark.parametrize('dt', S.DTS)
def test_pw_k2c_and_its_statistics(gpu, dt, operand):
    _, ops = _mi()
    c = NF.pw_special(dt, operand)
    C, HW, dtype = c['C'], c['HW'], S.TDT[dt]
    half = torch.tensor(0.5, device=gpu)
    y, w, b, r = _f32(c['y'], gpu), _f32(c['wck'], gpu), _f32(c['bias_c'], gpu), _feat(c['res'], dt, gpu)
    ref = S.pw_k2c(c['y'], c['wck'], c['bias_c'], c['res'])
    NF.case_condition(ref, NF.KINDS, 'pw_k2c %s' % operand)
    _pointwise('bias+res', ops.pw_k2c(y, w, b, C, dtype, residual=r), ref, dtype)
    _pointwise('bias+res*0.5', ops.pw_k2c(y, w, b, C, dtype, residual=r, scale_dev=half), S.pw_k2c(c['y'], c['wck'], c['bias_c'], c['res'], 0.5), dtype)
    _pointwise('[K][C]', ops.pw_k2c(y, _f32(c['wck'].t().contiguous(), gpu), b, C, dtype, residual=r, w_transposed=True), ref, dtype)
    if operand != 'res':
        _pointwise('plain', ops.pw_k2c(y, w, None if operand != 'bias_c' else b, C, dtype),
                   S.pw_k2c(c['y'], c['wck'], None if operand != 'bias_c' else c['bias_c']), dtype)
    out, (partial, ns) = ops.pw_k2c_stats(y, w, b, C, dtype, residual=r)
    _pointwise('stats: out', out, ref, dtype)
    assert ns == c['N'] * ((HW + 63) // 64)
    p = partial[:ns * C * 3].view(ns, C, 3).double().cpu()
    st = S.slice_stats(S.rne(ref, dt), HW)                 # of the STORED values; non-finite where a slice holds a special
    fin = torch.isfinite(st[:, :, 1])
    assert bool(fin.any()) and not bool(fin.all())
    assert torch.equal(p[:, :, 0], st[:, :, 0])            # the counts stay counts
    # [stats] of test_gpu_small_exact.test_pw_k2c_stats, on the finite slices; a slice and channel with a special: non-finite
    _reduced('stats: mean', p[:, :, 1], st[:, :, 1], atol=1e-5 * float(st[:, :, 1][fin].abs().max() + 1))
    _reduced('stats: M2', p[:, :, 2], st[:, :, 2], atol=1e-4 * float(st[:, :, 2][torch.isfinite(st[:, :, 2])].abs().max() + 1))


@pytest.mark.parametrize('operand', NF.PW_OPERANDS['wgrad'])
@pytest.mark.parametrize('dt', S.DTS)
def test_pw_wgrad(gpu, dt, operand):
    _, ops = _mi()
    c = NF.pw_special(dt, operand, NF.PW_WGRAD_HW)          # (whole 64-pixel groups: the kernel's contract)
    x, y = _feat(c['x'], dt, gpu), _f32(c['y'], gpu)
    for acc in ((True,) if operand == 'prior_w' else (False, True)):
        ref = S.pw_wgrad(c['x'], c['y'], c['prior_w'] if acc else None)
        NF.case_condition(ref, NF.KINDS, 'pw_wgrad %s' % operand)
        for kc in (True, False):
            prior = c['prior_w'] if kc else c['prior_w'].t().contiguous()
            dw = _f32(prior, gpu) if acc else torch.full(prior.shape, 777.0, device=gpu)
            ops.pw_wgrad(x, y, dw, kc, acc)
            _pointwise('acc=%d kc=%d' % (acc, kc), dw if kc else dw.t(), ref, torch.float32)


@pytest.mark.parametrize('operand', NF.PW_OPERANDS['rowsum'])
def test_hm_rowsum(gpu, operand):
    """The bias gradient of the 21-channel head: the reduced rule, the finite sums exact (integers)."""
    _, ops = _mi()
    c = NF.pw_special('f32', operand)
    y = _f32(c['y'], gpu)
    for acc in ((True,) if operand == 'bias_k' else (False, True)):
        ref = S.hm_rowsum(c['y'], c['bias_k'] if acc else None)
        assert bool(torch.isfinite(ref).any()) and int((~torch.isfinite(ref)).sum()) == 3
        out = _f32(c['bias_k'], gpu) if acc else torch.full((c['K'],), 777.0, device=gpu)
        ops.hm_rowsum(y, out, acc)
        _reduced('acc=%d' % acc, out, ref)


# ================================================================ heat-map kernels
def _clean_rows_equal(what, got, clean, rows_shape):
    """Every map that holds no special: the bits of the run without specials."""
    B, K = NF.HM_SHAPE[:2]
    g, c = _bits(got).view(B, K, -1), _bits(clean).view(B, K, -1)
    bad = set(NF.hm_poisoned_maps())
    for b in range(B):
        for k in range(K):
            if (b, k) not in bad:
                assert torch.equal(g[b, k], c[b, k]), '%s: the clean map (%d, %d) changed' % (what, b, k)


def _nonfinite_where_ref(what, got, ref):
    """A poisoned map: non-finite wherever the float64 reference is (nothing swallowed) and nowhere else (nothing invented)."""
    g, r = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    miss = (~torch.isfinite(r)) & torch.isfinite(g)
    assert not bool(miss.any()), '%s: %d values are finite where the float64 reference is not (first at %d: %r)' % (
        what, int(miss.sum()), int(miss.nonzero()[0]), float(g[miss.nonzero()[0]]))
    extra = torch.isfinite(r) & ~torch.isfinite(g)
    print('\nMEASURE %s: %d of %d non-finite in the reference, %d more in the kernel' % (what, int((~torch.isfinite(r)).sum()), r.numel(), int(extra.sum())))
    assert not bool(extra.any()), '%s: %d values are non-finite where the float64 reference is finite' % (what, int(extra.sum()))


@pytest.mark.parametrize('side', ['pred', 'target'])
@pytest.mark.parametrize('eps', [0.0, 1e-7])
def test_kl_heatmap(gpu, side, eps):
    _, ops = _mi()
    pred, target = NF.hm_inputs('kl pred', 3.0), NF.hm_inputs('kl target', 1.0, positive=True)
    p2, t2 = (NF.hm_seed(pred), target) if side == 'pred' else (pred, NF.hm_seed(target))
    ref_rows, ref_grad = HR.kl(p2, t2, None, eps, 1.0)
    clean_rows, clean_grad = ops.kl_heatmap(pred.to(gpu), target.to(gpu), None, eps, True)
    assert bool(torch.isfinite(clean_rows).all()) and bool(torch.isfinite(clean_grad).all())
    rows, grad = ops.kl_heatmap(p2.to(gpu), t2.to(gpu), None, eps, True)
    bad = NF.hm_poisoned_maps()
    assert any(not bool(torch.isfinite(ref_rows[b, k])) for b, k in bad)
    for b, k in bad:
        _nonfinite_where_ref('kl %s eps=%g rows (%d, %d)' % (side, eps, b, k), rows[b, k], ref_rows[b, k])
        _nonfinite_where_ref('kl %s eps=%g grad (%d, %d)' % (side, eps, b, k), grad[b, k], ref_grad[b, k])
    _clean_rows_equal('kl rows', rows, clean_rows, None)
    _clean_rows_equal('kl grad', grad, clean_grad, None)
    # the scalar the step logs and differentiates: non-finite iff a row is
    total = ops.reduce_sum(rows.view(-1), 1.0 / rows.numel())
    assert bool(torch.isfinite(total)) == bool(torch.isfinite(ref_rows).all())


@pytest.mark.parametrize('side', ['pred', 'target'])
def test_mse_heatmap(gpu, side):
    """All joints (k = 400) and the six-joint subset (k = 100: joints 3 and 20 are outside the mask -- their specials must leave
    exact zeros, rows and gradient, as the reference never reads a joint it does not select)."""
    _, ops = _mi()
    pred, target = NF.hm_inputs('mse pred'), NF.hm_inputs('mse target', 1.0, positive=True)
    p2, t2 = (NF.hm_seed(pred), target) if side == 'pred' else (pred, NF.hm_seed(target))
    B, K, Hh, W = NF.HM_SHAPE
    for k in (400, 100):
        mask, gs = mt_ref.mask(k), mt_ref.grad_scale(1.0, NF.HM_SHAPE, k)
        rec = ops.mse_record(mask, gs, gpu)
        clean_rows, clean_grad = ops.mse_heatmap(pred.to(gpu), target.to(gpu), rec, True)
        rows, grad = ops.mse_heatmap(p2.to(gpu), t2.to(gpu), rec, True)
        on = torch.tensor([(mask >> j) & 1 for j in range(K)], dtype=torch.bool)
        d = p2.double() - t2.double()
        ref_rows = torch.where(on.view(1, K), (d * d).sum((2, 3)), torch.zeros(B, K, dtype=torch.float64))
        ref_grad = torch.where(on.view(1, K, 1, 1), d * float(gs), torch.zeros_like(d))
        assert np.isfinite(mt_ref.mt_loss64(p2.numpy(), t2.numpy(), k)) == bool(torch.isfinite(ref_rows).all())      # the reference's own scalar
        live = [(b, j) for b, j in NF.hm_poisoned_maps() if bool(on[j])]
        assert len(live) == (3 if k == 400 else 1)
        # rows: reduced rule (finite: the tolerance of test_gpu_mt: another lane order, rtol 1e-6 is its looser comparison)
        _reduced('mse rows k=%d' % k, rows, ref_rows, rtol=1e-5)
        # gradient: one product per element: the class of every element, and the finite ones the fp32 expression's bits
        want = torch.from_numpy(mt_ref.unit_grad(p2.numpy(), t2.numpy(), mask, gs))
        assert torch.equal(NF.classes(grad.cpu()), NF.classes(ref_grad)), 'mse gradient classes k=%d' % k
        fin = torch.isfinite(want)
        assert torch.equal(_bits(grad)[fin], _bits(want)[fin])
        for b, j in NF.hm_poisoned_maps():
            if not bool(on[j]):
                assert float(rows[b, j]) == 0.0 and not bool(grad[b, j].ne(0).any()), 'a special in the unselected joint %d leaked' % j
        _clean_rows_equal('mse rows', rows, clean_rows, None)
        _clean_rows_equal('mse grad', grad, clean_grad, None)
        total = ops.scale_by_dev(ops.reduce_sum(rows.view(-1)), torch.tensor(float(mt_ref.loss_scale(1.0, NF.HM_SHAPE, k)), device=gpu))
        assert bool(torch.isfinite(total)) == (len(live) == 0)


def test_softargmax_and_argmax(gpu):
    _, ops = _mi()
    hm = NF.hm_inputs('decode', 0.05)
    hm[:, :, 4, 9] += 1.0
    h2 = NF.hm_seed(hm)
    ref = HR.soft_argmax(h2)
    clean = ops.softargmax(hm.to(gpu))
    uv = ops.softargmax(h2.to(gpu))
    for b, k in NF.hm_poisoned_maps():
        _nonfinite_where_ref('softargmax (%d, %d)' % (b, k), uv[b, k], ref[b, k])
        r = ref[b, k]
        if bool(torch.isfinite(r).all()):          # (-inf: a pixel of weight zero) the tolerance of test_softargmax_every_form's ceiling
            assert torch.allclose(uv[b, k].double().cpu(), r, rtol=1e-4, atol=1e-3)
    assert not bool(torch.isfinite(ref[0, 3]).any()) and not bool(torch.isfinite(ref[0, 20]).any())
    _clean_rows_equal('softargmax', uv, clean, None)
    # hard arg-max: numpy's rules are the specification (a NaN is the maximum, the first one wins), bit for bit
    r_idx, r_xy, r_mv = HR.argmax(h2.numpy())
    idx, xy, mv = ops.argmax2d(h2.to(gpu))
    assert np.array_equal(idx.cpu().numpy(), r_idx)
    assert np.array_equal(xy.cpu().numpy().view(np.int32), r_xy.view(np.int32))
    assert np.array_equal(mv.cpu().numpy().view(np.int32) & 0x7fffffff, r_mv.astype(np.float32).view(np.int32) & 0x7fffffff)      # (the sign of a NaN is no promise)
    assert np.isnan(r_mv[0, 3, 0]) and r_mv[0, 20, 0] == np.inf and np.isfinite(r_mv[1, 5, 0])


@pytest.mark.parametrize('size', [32, 64])
def test_bilinear_up(gpu, size):
    """A special spreads over the footprint of its pixel and nowhere else: the class of every output element is the float64
    interpolation's, the finite ones within the tolerance of test_gpu_heatmap_rows.test_bilinear_up."""
    _, ops = _mi()
    x = NF.hm_inputs('bilinear')
    x2 = NF.hm_seed(x)
    acc = NF.hm_inputs('bilinear acc %d' % size)[:, :, :1, :1].expand(2, 21, size, size).contiguous()
    for alpha, out0 in ((1.0, None), (0.5, acc)):
        ref = HR.bilinear(x2, size, alpha, out=out0)
        NF.case_condition(ref, NF.KINDS, 'bilinear %d' % size)
        clean = ops.bilinear_up(x.to(gpu), size, alpha, out=None if out0 is None else out0.clone().to(gpu))
        got = ops.bilinear_up(x2.to(gpu), size, alpha, out=None if out0 is None else out0.clone().to(gpu))
        cg, cr = NF.classes(got.cpu()), NF.classes(ref)
        assert torch.equal(cg, cr), '%d elements differ in class' % int((cg != cr).sum())
        fin = cr == NF.FINITE
        assert torch.allclose(got.cpu().double()[fin], ref[fin], rtol=1e-5, atol=1e-5)
        _clean_rows_equal('bilinear', got, clean, None)


LABEL_SIZES = [(16, 3.0, 4), (32, 4, 2), (64, 6, 1)]          # (S, radius, div): the loop kernel and both register forms


@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('case', LABEL_SIZES, ids=lambda c: 'S%d' % c[0])
def test_pseudo_label_with_a_non_finite_extra(gpu, case, kind):
    """The kernel follows the reference (module docstring): +Inf clips to 1 and -Inf to 0, a NaN stays in its pixel without
    normalisation and under normalise = 2 (np.where(max > 0, ...) leaves the map unscaled), and makes its whole map NaN under
    normalise = 1.  Every map without a special keeps the bits of the run with the finite `extra`."""
    _, ops = _mi()
    S_, tmp, div = case
    B, K = NF.HM_SHAPE[:2]
    rng = np.random.default_rng([59, S_, kind])
    xy = rng.integers(0, S_ * div, (B, K, 2)).astype(np.float32)
    extra = (rng.standard_normal((B, K, S_, S_)) * 0.3).astype(np.float32)
    poisoned = extra.copy()
    for b, k, i, j, kd in NF.HM_SPECIALS:
        # away from the key point's own patch, where - 100 gt would clip anything finite (a NaN survives there too)
        poisoned[b, k, (i * S_) // 16, (j * S_) // 16] = NF.SPECIAL[kd]
    xy_d = torch.from_numpy(xy).to(gpu)
    patch_d = torch.from_numpy(HR.patch(tmp, 2).reshape(-1)).to(gpu)
    for norm in (0, 1, 2):
        _, r_gf = HR.labels(xy, tmp, 2, div, S_, kind, poisoned, norm)
        _, c_gf = HR.labels(xy, tmp, 2, div, S_, kind, extra, norm)
        nan = np.isnan(r_gf)
        # the reference: the NaN map is NaN in one pixel (normalise 0, 2) or throughout (1); the infinities clip
        assert nan[0, 3].sum() == (S_ * S_ if norm == 1 else 1)
        only = nan.copy()
        only[0, 3] = False
        if norm != 1:
            assert not only.any()
        _, gf = ops.pseudo_label(xy_d, patch_d, int(tmp), div, S_, kind, extra=torch.from_numpy(poisoned).to(gpu), normalise=norm)
        _, gf_clean = ops.pseudo_label(xy_d, patch_d, int(tmp), div, S_, kind, extra=torch.from_numpy(extra).to(gpu), normalise=norm)
        g = gf.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(g), nan), 'kind %d normalise %d: NaN pattern (%d in the kernel, %d in the reference)' % (kind, norm, np.isnan(g).sum(), nan.sum())
        assert np.isfinite(g[~nan]).all()
        np.testing.assert_allclose(g[~nan], r_gf[~nan], rtol=1e-5, atol=1e-6)          # the tolerance of test_pseudo_labels_every_form
        for b, k, i, j, kd in NF.HM_SPECIALS[1:]:          # the infinities, before the normalisation: exactly the clip's ends
            if norm == 0:
                assert g[b, k, (i * S_) // 16, (j * S_) // 16] == (1.0 if kd == '+inf' else 0.0)
        _clean_rows_equal('pseudo_label', gf, gf_clean, None)
