"""The flip test and the sub-pixel decodes on the CPU: the properties of the reference (tests/tta_ref.py) that the GPU tests
rest on -- what each decode costs on the Gaussian labels the network is trained on, the geometry behind --flip-shift, every
border and degenerate rule -- plus the command line and the C interface of the feature.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import tta_ref as T
from conftest import PKG, ROOT


def _err(xy, centres):
    return np.sqrt(((xy.astype(np.float64) - centres) ** 2).sum(1))


# ------------------------------------------------------------------------------------------------------------------ accuracy
def test_decode_errors_on_gaussian_labels():
    """300 sigma = 2 unit Gaussians on 64 x 64 maps, centres uniform in [8, 55]^2, distance from the true centre in heat-map
    pixels: argmax 0.40 mean / 0.70 max, quarter 0.19 / 0.35, taylor 0.0002 / 0.0005."""
    maps, c = T.gaussians(300)
    e = {}
    for mode in ('argmax', 'quarter', 'taylor'):
        idx, xy, mv, det = T.decode(maps, mode)
        e[mode] = _err(xy, c)
        print('MEASURE %s: mean %.4f max %.4f' % (mode, e[mode].mean(), e[mode].max()))
    assert np.isfinite(det).all() and (np.abs(det) >= T.DET_MIN).all()       # 1/64 for sigma^2 + sigma^2 = 8
    assert abs(np.abs(det).min() - 1 / 64) < 1e-3
    assert e['taylor'].max() <= 0.001
    assert e['taylor'].mean() < e['quarter'].mean() < e['argmax'].mean()
    assert e['argmax'].max() <= 0.5 * np.sqrt(2) + 1e-6 and e['quarter'].max() <= 0.36


def test_taylor_under_label_noise():
    maps, c = T.gaussians(300, noise=0.02)
    idx, xy, mv, det = T.decode(maps, 'taylor')
    e = _err(xy, c)
    print('MEASURE taylor, N(0, 0.02^2) noise: mean %.4f max %.4f' % (e.mean(), e.max()))
    assert (np.abs(det) >= T.DET_MIN).all() and e.mean() < 0.03 and e.max() < 0.1


def test_gpu_taylor_inputs_meet_the_determinant_condition():
    """The one-ulp comparison of test_gpu_tta.py is made where |det| >= 0.01: none of its inputs falls below."""
    for name, maps in T.taylor_cases().items():
        det = T.decode(maps, 'taylor')[3]
        applied = np.isfinite(det)
        assert applied.sum() >= len(maps) // 2, name
        assert (np.abs(det[applied]) >= T.DET_MIN).all(), (name, np.abs(det[applied]).min())


def test_scale_invariance_makes_the_renormalisation_unnecessary():
    """DARK rescales the smoothed map to the maximum of the original one: a factor on the map, a constant on every log, nothing
    on the differences.  A power of two is exact in fp32, so the result is the same to the last bit."""
    maps, _ = T.gaussians(64, seed=8)
    a, b = T.decode(maps, 'taylor')[1], T.decode(maps * np.float32(4), 'taylor')[1]
    assert np.abs(a.astype(np.float64) - b).max() <= 1e-6
    idx = T.decode(maps, 'argmax')[0].astype(np.int64)
    at = (maps, idx % 64, idx // 64) + T.gaussian_taps(2.0)
    S = T.smoothed_points(*at)
    assert np.array_equal(T.smoothed_points(maps * np.float32(4), *at[1:]), S * np.float32(4)) and S.min() > 0.01
    assert np.array_equal(a, b)


def test_taps_are_darks_kernel():
    g, r = T.gaussian_taps(2.0)
    assert r == 5 and len(g) == 11 and g.dtype == np.float32 and abs(float(g.astype(np.float64).sum()) - 1) < 1e-6
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert T.gaussian_taps(1.0)[1] == 3 and T.gaussian_taps(6.4)[1] == 16
    from mi355 import ops
    for s in (1.0, 2.0, 3.5):
        mine, want = ops.gaussian_taps(s), T.gaussian_taps(s)
        assert mine[1] == want[1] and mine[0].tobytes() == want[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ flip geometry
def _peak_x(row):
    """Sub-pixel peak of a sampled 1-D Gaussian (three-point log-parabola: exact for a Gaussian)."""
    i = int(row.argmax())
    l = np.log(row[i - 1:i + 2].astype(np.float64))
    return i + .5 * (l[0] - l[2]) / (l[0] - 2 * l[1] + l[2])


@pytest.mark.parametrize('x_img', [100.0, 101.0, 102.5, 131.0])
def test_shift_geometry(x_img):
    """A key point at image column x has its label peak at x / 4.  The mirror image (x -> 255 - x) has it at (255 - x) / 4, and
    mirrored back on the 64-pixel map (u -> 63 - u) at x / 4 - 0.75; one column to the right is x / 4 + 0.25."""
    g = np.arange(64, dtype=np.float64)
    hm_flip = np.exp(-(g - (255.0 - x_img) / 4) ** 2 / 8.0).astype(np.float32)[None, None, :].repeat(3, 1)
    plain, shifted = T.flip_back(hm_flip, 0)[0, 1], T.flip_back(hm_flip, 1)[0, 1]
    assert abs(_peak_x(plain) - (x_img / 4 - 0.75)) < 1e-4
    assert abs(_peak_x(shifted) - (x_img / 4 + 0.25)) < 1e-4
    assert shifted[0] == plain[0] and np.array_equal(shifted[1:], plain[:-1])
    # the average of the label and the shifted copy peaks a quarter pixel / 2 from the truth; unshifted, three eighths
    hm = np.exp(-(g - x_img / 4) ** 2 / 8.0).astype(np.float32)[None, None, :].repeat(3, 1)
    e1 = abs(_peak_x(T.working_map(hm, hm_flip, 1)[0, 1]) - x_img / 4)
    e0 = abs(_peak_x(T.working_map(hm, hm_flip, 0)[0, 1]) - x_img / 4)
    assert e1 < 0.13 and 0.36 < e0 < 0.39


def test_flip_back_and_average_definitions():
    rng = np.random.default_rng(3)
    a, f = rng.integers(-9, 9, (2, 3, 5)).astype(np.float32), rng.integers(-9, 9, (2, 3, 5)).astype(np.float32)
    m0, m1 = T.working_map(a, f, 0), T.working_map(a, f, 1)
    for y in range(3):
        for x in range(5):
            assert m0[1, y, x] == 0.5 * (a[1, y, x] + f[1, y, 4 - x])
            assert m1[1, y, x] == 0.5 * (a[1, y, x] + (f[1, y, 5 - x] if x >= 1 else f[1, y, 4]))
    assert T.working_map(a) is not None and np.array_equal(T.working_map(a), a)
    one = np.float32([[[1, 2, 3]]])
    assert np.array_equal(T.flip_back(one[..., :1], 1), one[..., :1])        # w = 1: the column is its own mirror
    x = rng.standard_normal((2, 3, 4, 7)).astype(np.float32)
    mb = T.mirror_batch(x)
    assert mb.shape == (4, 3, 4, 7) and np.array_equal(mb[:2], x) and np.array_equal(mb[2:, :, :, ::-1], x)
    assert mb[3, 2, 1, 0] == x[1, 2, 1, 6]


# ------------------------------------------------------------------------------------------------------------------ borders
def test_border_rules():
    """quarter moves only where both neighbours exist (1 <= p <= size - 2), taylor only two pixels inside in both directions."""
    maps, spots = T.border_maps()
    n, h, w = maps.shape
    for mode in ('argmax', 'quarter', 'taylor'):
        idx, xy, mv, det = T.decode(maps, mode)
        assert (mv == 512).all() and np.array_equal(idx, [y * w + x for x, y in spots])
        for i, (x, y) in enumerate(spots):
            if mode == 'argmax':
                assert tuple(xy[i]) == (x, y)
            elif mode == 'quarter':         # the background rises with x and y: +0.25 wherever an offset applies
                assert xy[i, 0] == x + (.25 if 1 <= x <= w - 2 else 0) and xy[i, 1] == y + (.25 if 1 <= y <= h - 2 else 0)
            else:
                inside = 2 <= x <= w - 3 and 2 <= y <= h - 3
                assert np.isfinite(det[i]) == inside
                if not inside:
                    assert tuple(xy[i]) == (x, y)
                else:
                    assert abs(xy[i, 0] - x) < 1 and abs(xy[i, 1] - y) < 1 and tuple(xy[i]) != (x, y)
    assert [s for s in spots if 2 <= s[0] <= w - 3 and 2 <= s[1] <= h - 3] and len(spots) == 18


def test_degenerate_maps():
    flat = np.zeros((1, 9, 9), np.float32)
    flat[0, 4, 4] = 2.0
    flat[0, 3:6, 3:6] = np.maximum(flat[0, 3:6, 3:6], 1.0)                   # equal neighbours on both sides: sign(0) = 0
    assert tuple(T.decode(flat, 'quarter')[1][0]) == (4, 4)
    nanmap = flat.copy()
    nanmap[0, 4, 5] = -np.inf; nanmap[0, 4, 3] = -np.inf                     # (-inf) - (-inf) = NaN: no offset
    assert tuple(T.decode(nanmap, 'quarter')[1][0]) == (4, 4)
    S = T.smoothed_points(np.full((1, 40, 40), 3.0, np.float32), np.array([20]), np.array([20]), *T.gaussian_taps(2.0))
    assert (S == S[0, 0]).all()                                              # a constant neighbourhood smooths to one value:
    ox, oy, det = T.taylor_offsets(S)
    assert det[0] == 0 and ox[0] == 0 and oy[0] == 0                         # det == 0, no offset
    idx, xy, mv, det = T.decode(np.full((1, 40, 40), 3.0, np.float32), 'taylor')
    assert idx[0] == 0 and tuple(xy[0]) == (0, 0) and np.isnan(det[0])       # a constant map: first maximum in the corner
    idx, xy, mv, det = T.decode(T.faint_maps(), 'taylor')                    # every smoothed value below the 1e-10 clamp
    assert det.tolist() == [0, 0] and xy.tolist() == [[20, 13], [2, 37]] and (mv > 0).all()
    for maps in (np.full((1, 9, 9), -1.0, np.float32), np.zeros((1, 9, 9), np.float32)):
        for mode in T.MODES:
            idx, xy, mv, det = T.decode(maps, mode)
            assert not xy.any() and idx[0] == 0 and mv[0] == maps[0, 0, 0]
    neg = -np.ones((1, 9, 9), np.float32)
    neg[0, 4, 5] = -0.5
    assert T.decode(neg, 'taylor')[0][0] == 4 * 9 + 5 and not T.decode(neg, 'quarter')[1].any()


def test_mode_0_without_flip_is_first_argmax_times_scale():
    import eval_ref as E
    maps = E.integer_maps(5, 7, 9, seed=4)
    ridx, rxy, rmv = E.first_argmax(maps)
    idx, xy, mv, det, m = T.flip_decode(maps, scale=(3., 2.))
    assert np.array_equal(idx, ridx) and np.array_equal(xy, rxy * np.float32([3, 2])) and np.array_equal(mv, rmv) and m is not None


# ------------------------------------------------------------------------------------------------------------------ interface
def _parser():
    import train1
    return train1.build_parser()


@pytest.mark.parametrize('mode', ['quarter', 'taylor', 'upsample'])
def test_sub_pixel_decodes_need_full_metrics(mode, capsys):
    p = _parser()
    with pytest.raises(SystemExit):
        p.parse_args(['data/none', '--decode', mode])
    assert '--decode %s decodes the key points of --metrics full: add --metrics full' % mode in capsys.readouterr().err
    a = p.parse_args(['data/none', '--decode', mode, '--metrics', 'full'])
    assert a.decode == mode and a.flip_test is False and a.flip_shift == 1 and a.decode_sigma is None


def test_flip_flags():
    p = _parser()
    a = p.parse_args(['data/none'])
    assert a.flip_test is False and a.flip_shift == 1 and a.decode == 'argmax' and a.metrics == 'pck'
    a = p.parse_args(['data/none', '--flip-test', '--flip-shift', '0', '--decode-sigma', '1.5'])           # either metrics setting
    assert a.flip_test is True and a.flip_shift == 0 and a.decode_sigma == 1.5 and a.metrics == 'pck'
    with pytest.raises(SystemExit):
        p.parse_args(['data/none', '--flip-shift', '2'])


def test_symbols_are_declared_and_bound():
    import ctypes
    import mi355
    txt = open(os.path.join(ROOT, 'include', 'mi355pose.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name, nargs in (('mi355_mirror_batch', 7), ('mi355_flip_decode', 16)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, code)
        assert m, name + ' is not declared in include/mi355pose.h'
        assert len(m.group(1).split(',')) == nargs == len(mi355.SIGNATURES[name][1])
        assert mi355.SIGNATURES[name][0] is ctypes.c_int
    # each declaration cites what it implements
    for name, cited in (('mirror_batch', 'function.py'), ('flip_decode', 'DARK')):
        comment = [c for c in re.findall(r'/\*.*?\*/', txt, flags=re.S) if re.match(r'/\*\s*%s:' % name, c)]
        assert len(comment) == 1 and cited in comment[0], name


def test_python_surface_refuses_bad_arguments_before_any_launch():
    import torch
    import mi355
    from mi355 import ops
    from utils.keypoint_detection import decode_keypoints
    with pytest.raises(mi355.Mi355Error):                   # no CPU fall-back
        ops.flip_decode(torch.zeros(1, 2, 8, 8))
    with pytest.raises(mi355.Mi355Error):
        ops.mirror_batch(torch.zeros(1, 3, 8, 8))
    with pytest.raises(mi355.Mi355Error):
        ops.gaussian_taps(7.0)                               # radius 18
    with pytest.raises(mi355.Mi355Error):
        ops.gaussian_taps(0.0)
    with pytest.raises(ValueError):
        decode_keypoints(torch.zeros(1, 2, 8, 8), 32, 'soft')
    from mi355.infer import PosePredictor
    with pytest.raises(ValueError):
        PosePredictor(torch.nn.Identity(), 64, decode='soft')
