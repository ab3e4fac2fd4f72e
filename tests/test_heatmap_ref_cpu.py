"""The float64 references of tests/heatmap_ref.py are themselves pinned here, on the CPU, so that a wrong reference cannot
pass a wrong kernel: against the oracle's S^4 label table, the reference-captured goldens (g3 / g4 / g5), the oracle's
disparity classes, and the float32 oracle.

This module also owns the yardstick of tests/test_gpu_heatmap_rows.py: `softargmax_yardstick` / `kl_yardstick` return, for
one case of the GPU matrix, the float64 reference together with the error of the float32 CPU oracle against it on that very
input -- what float32 arithmetic with an unspecified summation order costs there, measured without the code under test."""
import numpy as np
import pytest
import torch
from conftest import golden
from seeded import randn, rand, peaky_heatmaps, weights_bk

import heatmap_ref as R
from oracle import losses as ol

torch.set_num_threads(8)

ULP16 = 2.0 ** -20          # 16 float32 ulps of a quantity's scale


# ------------------------------------------------------------------------------------------------------------------ yardstick
def _finite_max(t):
    t = t[torch.isfinite(t)]
    return float(t.abs().max()) if t.numel() else 0.0


def bound(yard, scale, ceiling):
    """Kernel tolerance: 16 x the float32 oracle's own error, at least 16 float32 ulps of the quantity's scale, never more
    than the tolerance tests/test_gpu_kernels.py already asks of the same kernel."""
    return min(max(16.0 * yard, ULP16 * scale), ceiling)


def softargmax_yardstick(H, W, rows, beta, out_scale):
    """-> dict(hm, ref [rows, 1, 2] float64, yard, scale, bound (per coordinate, [rows, 1, 2]))."""
    hm = R.softargmax_maps(H, W, rows)
    ref = R.soft_argmax(hm, beta, out_scale)
    o32 = R.soft_argmax(hm, beta, out_scale, dtype=torch.float32)
    assert torch.isfinite(ref).all() and torch.isfinite(o32).all()
    yard = float((o32.double() - ref).abs().max())
    scale = out_scale * max(H, W)
    ceiling = 1e-3 + 1e-4 * ref.abs()                  # rtol 1e-4, atol 1e-3 of test_softargmax
    assert bool(((o32.double() - ref).abs() <= ceiling).all())
    return dict(hm=hm, ref=ref, yard=yard, scale=scale, bound=torch.clamp(ceiling, max=bound(yard, scale, float('inf'))))


def kl_yardstick(H, W, rows, eps, wmode, coeff):
    """-> dict(pred, target, weight, ref_rows / ref_grad float64 (NaN where the oracle gives NaN), nan_rows (bool [rows]),
    yard_* / scale_* / bound_* for `rows` and `grad`).  Errors and scales are taken over the rows the reference keeps finite."""
    pred, target = R.kl_inputs(H, W, rows)
    weight = R.kl_weight(wmode, rows)
    ref_rows, ref_grad = R.kl(pred, target, weight, eps, coeff)
    o_rows, o_grad = R.kl(pred, target, weight, eps, coeff, dtype=torch.float32)
    ref_rows, o_rows = ref_rows.view(rows), o_rows.view(rows)
    nan_rows = ~torch.isfinite(ref_rows)
    # the float32 oracle is NaN in the same rows, and a NaN row is NaN in its whole gradient map
    assert torch.equal(~torch.isfinite(o_rows), nan_rows)
    gnan = ~torch.isfinite(ref_grad.view(rows, -1))
    assert torch.equal(gnan.all(1), nan_rows) and torch.equal(gnan.any(1), nan_rows)
    assert torch.equal(~torch.isfinite(o_grad.view(rows, -1)), gnan)
    ok = ~nan_rows
    out = dict(pred=pred, target=target, weight=weight, ref_rows=ref_rows, ref_grad=ref_grad, nan_rows=nan_rows)
    for name, o, r, ceil in (('rows', o_rows[ok], ref_rows[ok], 1e-4), ('grad', o_grad.view(rows, -1)[ok], ref_grad.view(rows, -1)[ok], 1e-3)):
        yard = float((o.double() - r).abs().max()) if r.numel() else 0.0
        scale = _finite_max(r)
        out['yard_' + name], out['scale_' + name] = yard, scale
        out['bound_' + name] = bound(yard, scale, ceil * scale)      # ceilings of test_kl_heatmap_vs_oracle, on the same scales
    return out


# ------------------------------------------------------------------------------------------------------------------- pins
@pytest.mark.parametrize('S,tmp', [(16, 3.0), (32, 4), (24, 6)])
def test_per_centre_label_builder_equals_the_oracle_table(S, tmp):
    table = ol._table(S, S, tmp, 2)
    g = R.patch(tmp, 2)
    assert g.dtype == np.float32 and np.array_equal(g, ol._gauss_patch(tmp, 2).astype(np.float32))
    for mx in range(S):
        for my in range(S):
            assert np.array_equal(R.centre_map(mx, my, S, tmp, g), table[mx][my]), (mx, my)


def test_labels_reproduce_the_pseudo_label_goldens():
    g = golden('g3_pseudo_labels')
    y = peaky_heatmaps(301, 2, 21, 64, 64)
    _, xy, _ = R.argmax(y.numpy())
    for (tmp, div, S, kind), a, b in [((6, 1, 64, 0), 'gt', 'gf'), ((3.0, 4, 16, 1), 'gt01', 'gf01'), ((4, 2, 32, 1), 'gt03', 'gf03')]:
        gt, gf = R.labels(xy, tmp, 2, div, S, kind)
        assert gt.dtype == np.float32 and np.array_equal(gt, g[a]), a
        # gf is float64 here; the golden went through float32 (and, for kind 0, a BLAS dot)
        np.testing.assert_allclose(gf, g[b], rtol=0, atol=2e-7, err_msg=b)


def test_labels_reproduce_the_oracle_disparity_ground_false():
    import torch.nn as nn
    B, K = 2, 21
    y = peaky_heatmaps(201, B, K, 64, 64)
    y_adv2, y_adv3 = randn(203, B, K, 32, 32), randn(204, B, K, 16, 16)
    up = lambda t, s: nn.Upsample(size=s, mode='bilinear')(t)
    t5, t0 = 0.5 * up(y_adv3, 64) + up(y_adv2, 64), up(y_adv3, 32)
    np.testing.assert_allclose(R.bilinear(y_adv2, 64, 1.0, out=R.bilinear(y_adv3, 64, 0.5)).numpy(), t5.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(R.bilinear(y_adv3, 32).numpy(), t0.numpy(), rtol=1e-5, atol=1e-5)
    _, xy, _ = R.argmax(y.numpy())
    w = weights_bk(207, B, K)
    rd6 = ol.RegressionDisparityx6(ol.PseudoLabelGenerator(K, 64, 64), ol.JointsKLLoss(epsilon=1e-7))
    rd5 = ol.RegressionDisparityx5(ol.PseudoLabelGenerator03(K), ol.JointsKLLoss(epsilon=1e-7))
    rd1 = ol.RegressionDisparityx1(ol.PseudoLabelGenerator01(K), ol.JointsKLLoss(epsilon=1e-7))
    for extra in (None, t5):
        rd6(y, randn(1, B, K, 64, 64), extra, w, mode='max')
        gt, gf = R.labels(xy, 6, 2, 1, 64, 2, extra=None if extra is None else extra.numpy(), normalise=1)
        assert np.array_equal(gt, rd6.ground_truth.numpy())
        np.testing.assert_allclose(gf, rd6.ground_false.numpy(), rtol=1e-5, atol=1e-6)
    for extra in (None, t0):
        rd5(y, randn(1, B, K, 32, 32), extra, w, mode='max')
        gt, gf = R.labels(xy, 4, 2, 2, 32, 1, extra=None if extra is None else extra.numpy(), normalise=1)
        assert np.array_equal(gt, rd5.ground_truth.numpy())
        np.testing.assert_allclose(gf, rd5.ground_false.numpy(), rtol=1e-5, atol=1e-6)
    rd1(y, randn(1, B, K, 16, 16), w, mode='max')
    gt, gf = R.labels(xy, 3.0, 2, 4, 16, 1)
    assert np.array_equal(gt, rd1.ground_truth.numpy())
    np.testing.assert_allclose(gf, rd1.ground_false.numpy(), rtol=0, atol=2e-7)


def test_labels_empty_maps_nan_or_zero():
    """An `extra` negative enough to empty a map: normalise 1 -> NaN as the oracle's 0 / 0, 2 -> the map stays zero; a map
    with a positive maximum is the same under both."""
    B, K, S = 2, 5, 16
    xy = np.zeros((B, K, 2), np.float32)
    xy[..., 0] = np.arange(K)[None] * 3
    xy[..., 1] = 4
    extra = np.zeros((B, K, S, S), np.float32)
    extra[0] = -3.0
    gf1 = R.labels(xy, 3.0, 2, 1, S, 2, extra, 1)[1]
    gf2 = R.labels(xy, 3.0, 2, 1, S, 2, extra, 2)[1]
    assert np.isnan(gf1[0]).all() and np.isfinite(gf1[1]).all()
    assert (gf2[0] == 0).all() and np.array_equal(gf1[1], gf2[1])
    ref = ol._max_normalise(torch.from_numpy(R.labels(xy, 3.0, 2, 1, S, 2, extra, 0)[1]))
    assert np.array_equal(np.isnan(ref.numpy()), np.isnan(gf1))
    np.testing.assert_array_equal(ref.numpy()[1], gf1[1])


def test_soft_argmax_reproduces_the_golden_and_the_oracle():
    hm = randn(501, 2, 21, 64, 64, scale=0.05)
    hm[0, 0, 20, 33] += 1.0
    assert torch.equal(R.soft_argmax(hm, 100.0, 4.0, dtype=torch.float32), ol.soft_argmax(hm))     # the oracle's own ops
    np.testing.assert_allclose(R.soft_argmax(hm).numpy(), golden('g5_softargmax')['uv'], rtol=1e-5, atol=1e-6)
    # u = column, v = row on a non-square map; a flat map's centroid is the map centre
    one = torch.full((1, 1, 5, 7), -1.0)
    one[0, 0, 3, 6] = 1.0
    assert torch.allclose(R.soft_argmax(one, 100.0, 1.0), torch.tensor([[[6.0, 3.0]]], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(R.soft_argmax(torch.zeros(1, 1, 5, 7), 1.0, 2.0), torch.tensor([[[6.0, 4.0]]], dtype=torch.float64), atol=1e-12)


def test_argmax_reproduces_the_golden():
    g = golden('g4_argmax_accuracy')
    hm = peaky_heatmaps(401, 3, 21, 64, 64).numpy()
    hm[1, 0] = 0.5
    hm[1, 1, 10, 7] = hm[1, 1, 40, 3] = 9.0
    hm[2, 2, 63, 63] = 11.0
    idx, preds, maxvals = R.argmax(hm)
    assert np.array_equal(preds, g['preds']) and np.array_equal(maxvals, g['maxvals'])
    assert idx.dtype == np.int32 and idx[1, 0] == 0 and idx[1, 1] == 10 * 64 + 7 and idx[2, 2] == 4095


@pytest.mark.parametrize('eps', [0.0, 1e-7])
def test_kl_float64_agrees_with_the_float32_oracle(eps):
    """Rows and gradient of R.kl against oracle.losses.JointsKLLoss used the way the training step uses it (mean over B*K,
    float32), on the recipe of test_kl_heatmap_vs_oracle and over 5x7 ... 128x128 maps: within the float32 figures the
    tolerances of the GPU module start from (2.1e-7 of the loss, 2.3e-6 of the gradient's maximum)."""
    for (B, K, H, W) in [(2, 21, 64, 64), (3, 4, 5, 7), (2, 3, 128, 128), (2, 5, 16, 16)]:
        pred = randn(202, B, K, H, W)
        label = rand(205, B, K, H, W) * (rand(206, B, K, H, W) > 0.9)
        label[..., 0, 0] += 0.5                           # (no all-zero map at the small sizes)
        w = weights_bk(207, B, K)
        p = pred.clone().requires_grad_(True)
        ref = ol.JointsKLLoss(epsilon=eps)(p, label, w)
        ref.backward()
        rows, grad = R.kl(pred, label, w, eps)
        assert abs(float(rows.mean()) - float(ref.detach())) <= 2.1e-7 * abs(float(ref.detach()))
        assert float((grad - p.grad.double()).abs().max()) <= 2.3e-6 * float(p.grad.abs().max())
        r2, g2 = R.kl(pred, label, w, eps, coeff=0.25)
        assert torch.equal(r2, rows) and torch.allclose(g2, 0.25 * grad, rtol=1e-14, atol=0)


def test_pck_reference_is_calc_dists():
    pred = np.array([[[3.0, 4.0], [10.0, 2.0]], [[5.0, 5.0], [7.0, 9.0]]], np.float32)
    tgt = np.array([[[0.0, 0.0], [1.0, 5.0]], [[2.0, 1.5], [7.0, 3.0]]], np.float32)
    d = R.pck(pred, tgt, 6.4, 3.2)
    assert d.shape == (2, 2) and d[0, 0] == -1 and d[0, 1] == -1
    nx, ny = float(np.float32(6.4)), float(np.float32(3.2))
    assert abs(d[1, 0] - np.hypot(3.0 / nx, 3.5 / ny)) < 1e-15
    assert abs(d[1, 1] - 6.0 / ny) < 1e-15


@pytest.mark.parametrize('hw', R.SIZES, ids=R.size_id)
def test_yardsticks_of_the_gpu_matrix(hw):
    """Every soft-arg-max / KL case of the GPU module has a finite float64 reference and a finite float32-oracle error; NaN
    appears in the reference only where the inputs ask for it (eps = 0 with an all-zero target map; a +inf target pixel)."""
    H, W = hw
    for rows in R.ROWS:
        for beta, out_scale in R.configs_for(R.SOFT_CONFIGS, rows):
            y = softargmax_yardstick(H, W, rows, beta, out_scale)
            assert np.isfinite(y['yard']) and bool((y['bound'] > 0).all()) and bool((y['bound'] <= 1e-3 + 1e-4 * y['ref'].abs()).all())
        for eps, wmode, coeff in R.configs_for(R.KL_CONFIGS, rows):
            y = kl_yardstick(H, W, rows, eps, wmode, coeff)
            t = y['target'].view(rows, -1)
            expect_nan = torch.isinf(t).any(1) | ((t == 0).all(1) if eps == 0.0 else torch.zeros(rows, dtype=torch.bool))
            assert torch.equal(y['nan_rows'], expect_nan)
            assert np.isfinite(y['yard_rows']) and np.isfinite(y['yard_grad'])
            assert y['bound_rows'] <= 1e-4 * y['scale_rows'] and y['bound_grad'] <= 1e-3 * y['scale_grad']
            # the inputs are well conditioned: the float32 oracle itself stays inside the ceilings the kernels are held to
            assert y['yard_rows'] <= 1e-4 * y['scale_rows'] and y['yard_grad'] <= 1e-3 * y['scale_grad'], (rows, eps, wmode, coeff, y['yard_rows'], y['scale_rows'])
