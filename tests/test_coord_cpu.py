"""The float64 reference of the coordinate loss (tests/coord_ref.py) is pinned here, on the CPU, so that a wrong reference cannot
pass a wrong kernel: its closed-form gradient against torch.autograd, its soft-arg-max against the reference-captured golden g5,
and the exact cases of the specification bit for bit in float32.

This module also owns the yardstick of tests/test_gpu_coord.py: `coord_yardstick` returns, for one case of the GPU matrix, the
inputs, the float64 reference and the ceilings.  uv: the project's 1e-3 + 1e-4 |ref|.  loss rows and gradient: 8 x the largest
error of the float32 CPU torch expression against the float64 reference on those very inputs, plus 2^-23 x max |ref|.  The
factor 8 is a margin over a measured quantity (the kernel folds up to 4096 terms in another fixed order and uses expf), not a
measured bound; the GPU test prints the kernel's error beside it.

Also here: utils.synthetic.make_batch(with_keypoints=True) and the --coord-* command line."""
import functools
import inspect

import numpy as np
import pytest
import torch
from conftest import golden
from seeded import randn

import coord_ref as C

torch.set_num_threads(8)

SIDES = ((16, 16), (32, 32), (64, 64), (24, 20), (6, 10))      # the last two take the loop form: H != W, W no multiple of 4
ROWS = (1, 4, 5)
CASES = [(H, W, rows, beta, delta, wmode) for (H, W) in SIDES for rows in ROWS for beta in (1.0, 100.0) for delta in (0.0, 1.0)
         for wmode in ('none', 'mixed')]


@functools.lru_cache(maxsize=None)
def coord_yardstick(H, W, rows, beta, delta, wmode, coef=1.0):
    """-> dict(pred [rows, H, W], coord [rows, 2], weight [rows] or None (float32 inputs), coef (the kernel's: coef / rows),
    ref_rows / ref_grad / ref_uv (float64), bound_uv (per coordinate), yard_* and bound_* for `rows` and `grad`).  The kink
    condition of coord_ref.kink_clear is asserted for every case."""
    pred = C.maps(H, W, rows, beta)
    weight = None if wmode == 'none' else C.weights(rows)
    k = C.f32(C.f32(coef) / rows)
    b32, d32 = C.f32(beta), C.f32(delta)
    uv_ref = C.coord(pred, torch.zeros(rows, 2), weight, b32, d32, k)[2]
    coord = C.coords_for(uv_ref, delta, shift=H + rows)
    assert C.kink_clear(uv_ref, coord, d32), (H, W, rows, beta, delta, wmode)
    ref_rows, ref_grad, ref_uv = C.coord(pred, coord, weight, b32, d32, k)
    o_rows, o_grad, o_uv = C.coord(pred, coord, weight, b32, d32, k, dtype=torch.float32)
    assert torch.isfinite(ref_rows).all() and torch.isfinite(ref_grad).all() and torch.isfinite(o_grad).all()
    out = dict(pred=pred, coord=coord, weight=weight, coef=k, ref_rows=ref_rows, ref_grad=ref_grad, ref_uv=ref_uv,
               bound_uv=1e-3 + 1e-4 * ref_uv.abs())
    assert bool(((o_uv.double() - ref_uv).abs() <= out['bound_uv']).all())
    for name, o, r in (('rows', o_rows, ref_rows), ('grad', o_grad, ref_grad)):
        yard = float((o.double() - r).abs().max())
        out['yard_' + name] = yard
        out['bound_' + name] = 8.0 * yard + 2.0 ** -23 * float(r.abs().max())
    return out


# ------------------------------------------------------------------------------------------------------------------- pins
@pytest.mark.parametrize('delta', [0.0, 1.0])
def test_closed_form_gradient_equals_autograd(delta):
    for (H, W, rows, beta, wmode) in [(16, 16, 5, 1.0, 'mixed'), (24, 20, 4, 1.0, 'none'), (6, 10, 5, 100.0, 'mixed'), (64, 64, 2, 1.0, 'none')]:
        pred = C.maps(H, W, rows, beta)
        weight = None if wmode == 'none' else C.weights(rows)
        uv = C.coord(pred, torch.zeros(rows, 2), weight, beta, delta, 1.0)[2]
        coord = C.coords_for(uv, delta)
        assert C.kink_clear(uv, coord, delta)
        rows_c, grad_c, uv_c = C.coord(pred, coord, weight, beta, delta, 0.37)
        rows_a, grad_a, uv_a = C.coord_autograd(pred, coord, weight, beta, delta, 0.37)
        assert float(grad_a.abs().max()) > 1e-4                      # (not a comparison of zeros)
        for a, c in ((rows_a, rows_c), (grad_a, grad_c), (uv_a, uv_c)):
            assert float((a - c).abs().max()) <= 1e-10 * float(a.abs().max()), (H, W, delta)


def test_soft_argmax_of_the_reference_reproduces_the_golden():
    hm = randn(501, 2, 21, 64, 64, scale=0.05)
    hm[0, 0, 20, 33] += 1.0
    uv = C.coord(hm.reshape(42, 64, 64), torch.zeros(42, 2), None, 100.0, 1.0, 1.0)[2]
    np.testing.assert_allclose((uv * 4).reshape(2, 21, 2).numpy(), golden('g5_softargmax')['uv'], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('name', C.EXACT)
@pytest.mark.parametrize('embed', [(4, 8, 0, 0), (16, 16, 9, 7)])
def test_exact_cases_hold_bit_for_bit_in_float32(name, embed):
    e = C.exact_case(name, *embed)
    for dtype in (torch.float32, torch.float64):
        rows, grad, uv = C.coord(e['pred'], e['coord'], None, e['beta'], e['delta'], e['coef'], dtype=dtype)
        assert torch.equal(uv.float(), e['uv']) and torch.equal(rows.float(), e['loss']) and torch.equal(grad.float(), e['grad'])
    if name == 'two':
        assert e['uv'].tolist() == [[embed[3] + 2.5, embed[2] + 1.0]] and e['loss'].item() == 0.03125
        assert sorted(e['grad'][e['grad'] != 0].tolist()) == [-0.0625, 0.0625]


def test_zero_weight_row_is_selected_out_of_the_reference():
    pred = C.maps(6, 10, 3, 1.0)
    coord = torch.tensor([[1.0, 2.0], [float('nan'), 3.0], [4.0, 4.0]])
    pred[1, 0, 0] = float('nan')
    rows, grad, uv = C.coord(pred, coord, torch.tensor([1.0, 0.0, 1.0]), 1.0, 1.0, 1.0)
    assert rows[1] == 0 and bool((grad[1] == 0).all()) and torch.isfinite(rows).all() and torch.isfinite(grad).all()
    rows, grad, uv = C.coord(pred, coord, torch.tensor([1.0, 1.0, 1.0]), 1.0, 1.0, 1.0)
    assert torch.isnan(rows[1]) and bool(torch.isnan(grad[1]).all()) and torch.isfinite(grad[[0, 2]]).all()


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d-r%d-b%g-d%g-%s' % c)
def test_yardstick_of_every_gpu_case(case):
    y = coord_yardstick(*case)
    assert y['bound_rows'] > 0 and y['bound_grad'] > 0 and float(y['ref_grad'].abs().max()) > 1e-6
    # the margin stays a float32 matter: far below the quantities themselves
    assert y['bound_rows'] < 1e-3 * max(float(y['ref_rows'].abs().max()), 1.0) and y['bound_grad'] < 1e-3 * float(y['ref_grad'].abs().max())


# ------------------------------------------------------------------------------------------------------------ make_batch
def test_make_batch_with_keypoints_leaves_the_other_tensors_bit_identical():
    from utils.synthetic import make_batch
    a = make_batch(3, 64, 16, 21, seed=5, p_visible=0.8)
    b = make_batch(3, 64, 16, 21, seed=5, p_visible=0.8, with_keypoints=True)
    assert set(b) == set(a) | {'kp_s', 'kp_t'} and 'kp_s' not in a
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert b['kp_s'].dtype == torch.float32 and tuple(b['kp_s'].shape) == (3, 21, 2) and tuple(b['kp_t'].shape) == (3, 21, 2)


def test_make_batch_keypoints_are_the_draws_the_labels_are_made_of():
    from utils.synthetic import make_batch
    b = make_batch(4, 256, 64, 21, seed=9, p_visible=0.7, with_keypoints=True)
    seen = 0
    for kp, lab, w in ((b['kp_s'], b['label_s'], b['w_s']), (b['kp_t'], b['label_t'], b['w_t'])):
        centre = (kp + 0.5).to(torch.int64)                           # int(kp + 0.5), coordinates are positive
        idx = lab.reshape(4, 21, -1).argmax(2)
        vis = w.reshape(4, 21) > 0
        assert torch.equal(idx[vis] % 64, centre[..., 0][vis]) and torch.equal(idx[vis] // 64, centre[..., 1][vis])
        assert float((kp - centre).abs().max()) <= 0.5 and float((kp - centre).abs().mean()) > 0.1      # un-quantised
        seen += int(vis.sum())
    assert 0 < seen < 2 * 4 * 21


def test_source_keypoints_come_from_the_loader_meta_unquantised():
    """train(): batch['kp_s'] = meta['keypoint2d'] / stride as fp32 (B, K, 2); on the synthetic data set int(kp_s + 0.5) is the
    label's arg-max, and float64 meta (the collated key points of the real data sets) is accepted."""
    import train1
    from utils.synthetic_dataset import SyntheticHand21
    ds = SyntheticHand21(8, (128, 128), (32, 32))
    items = [ds[i] for i in range(3)]
    meta = {'keypoint2d': torch.stack([m['keypoint2d'] for _, _, _, m in items])}
    kp = train1.source_keypoints(meta, 128, 32, 'cpu')
    assert kp.dtype == torch.float32 and tuple(kp.shape) == (3, 21, 2) and kp.is_contiguous()
    assert torch.equal(kp, meta['keypoint2d'] / 4.0)
    idx = torch.stack([t for _, t, _, _ in items]).reshape(3, 21, -1).argmax(2)
    centre = (kp + 0.5).to(torch.int64)
    assert torch.equal(idx % 32, centre[..., 0]) and torch.equal(idx // 32, centre[..., 1])
    kp64 = train1.source_keypoints({'keypoint2d': meta['keypoint2d'].double().numpy()}, 128, 32, 'cpu')
    assert kp64.dtype == torch.float32 and torch.equal(kp64, kp)


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_coord_flags_parse_and_default_to_off():
    import train1
    from mi355.da_step import CoordRegression, DAStep
    a = train1.build_parser().parse_args(['d'])
    assert (a.coord_loss, a.coord_weight, a.coord_target_weight, a.coord_beta, a.coord_delta) == ('off', 1.0, 1.0, 1.0, 1.0)
    assert train1.coord_term(a, None) is None                        # the defaults build no CoordRegression
    params = list(inspect.signature(DAStep.__init__).parameters.values())
    assert params[-1].name == 'coord' and params[-1].default is None
    b = train1.build_parser().parse_args(['d', '--coord-loss', 'source', '--coord-weight', '0.5', '--coord-beta', '2', '--coord-delta', '0'])
    t = train1.coord_term(b, None)
    assert isinstance(t, CoordRegression) and (t.weight, t.beta, t.crit.delta, t.target) == (0.5, 2.0, 0.0, 'off')
    c = train1.build_parser().parse_args(['d', '--coord-loss', 'both', '--ema-update', 'const', '--coord-target-weight', '3'])
    t = train1.coord_term(c, object())
    assert (t.target, t.target_weight) == ('teacher', 3.0)
    for flag in ('--coord-weight', '--coord-target-weight'):         # placeholders, and said so
        assert 'placeholder' in [kw for flags, kw in train1._OPTIONS if flag in flags][0]['help']


def test_coord_both_needs_a_moving_teacher(capsys):
    import train1
    from mi355.da_step import CoordRegression
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--coord-loss', 'both'])
    err = capsys.readouterr().err
    assert '--coord-loss' in err and '--ema-update' in err
    with pytest.raises(ValueError, match='--ema-update'):
        CoordRegression(target='teacher', ema=None)
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--coord-loss', 'source', '--coord-delta', '-1'])
