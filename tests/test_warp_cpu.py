"""The geometric teacher view without a GPU: the fp32 restatement of tests/warp_ref.py on its exact cases, against
torch.nn.functional.grid_sample in float64 and on the round trip of a Gaussian; the records; the flag; the command line; the
state of mi355.teacher.GeometricView."""
import numpy as np
import pytest
import torch

import warp_ref as R


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def _plane(h, w, seed, special=False):
    x = np.random.default_rng(seed).standard_normal((h, w)).astype(np.float32)
    if special:
        x.reshape(-1)[::5] = -0.0
        x.reshape(-1)[2::7] = np.inf
        x.reshape(-1)[3::11] = np.nan
    return x


# ---------------------------------------------------------------- exact cases (records given as matrices, no cos / sin)
def test_identity_is_a_copy_bit_for_bit():
    for h, w in ((16, 16), (17, 19)):
        x = _plane(h, w, 1, special=True)
        assert _bits(R.sample32(x, R.IDENTITY)) == _bits(x)


def test_integer_shift_copies_and_fills_with_positive_zero():
    x = _plane(17, 19, 2, special=True)
    got = R.sample32(x, R.shift_matrix(3, -2))
    want = np.zeros_like(x)
    want[2:, :-3] = x[:-2, 3:]
    assert _bits(got) == _bits(want)
    assert not np.signbit(got[:2]).any() and not np.signbit(got[:, -3:]).any()
    assert _bits(R.sample32(x, R.shift_matrix(2 * 19, 0))) == _bits(np.zeros_like(x))


def test_quarter_turn_of_a_square_plane_is_a_permutation():
    side = 16
    x = _plane(side, side, 3, special=True)
    got = R.sample32(x, R.quarter_matrix(side))
    j, i = np.meshgrid(np.arange(side), np.arange(side))
    assert _bits(got) == _bits(x[j, side - 1 - i])
    four = x
    for _ in range(4):
        four = R.sample32(four, R.quarter_matrix(side))
    assert _bits(four) == _bits(x)


def test_non_finite_coordinates_give_zeros():
    x = _plane(8, 8, 4)
    for idx in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            m = R.IDENTITY.copy().reshape(-1)
            m[idx] = bad
            got = R.sample32(x, m.reshape(2, 3))
            # (inf * 0 is NaN and the whole row / column of coordinates is out of range; a finite coordinate may remain at j or i = 0)
            assert np.isfinite(got).all()


# ---------------------------------------------------------------- against grid_sample
def test_restatement_against_grid_sample_in_float64():
    """The fp32 sampler against torch's grid_sample (bilinear, align_corners=True, zero padding) in float64, both fed the same
    fp32 matrix.  The bound is derived, not tuned.  u = one ulp of 2 * side in fp32 (2^-16 at side 64), D = the largest
    difference between horizontally or vertically neighbouring taps (the zero border included), M = max |tap|.
      * Coordinates: three roundings of at most u, 3 u in all.  In detail, at these scales (<= 1.33) and shifts the two products
        stay below 2 * side (half an ulp there: u / 4 each), their sum below 4 * side (u / 2), and a coordinate that matters lies
        in (-1, side) (u / 4): 1.25 u per axis, 2.5 u over both.  Bilinear interpolation with zero padding is continuous and
        piecewise linear with slope at most D along each axis, so a value moves by at most 3 u D.
      * Blend: four roundings (1 - f, two products, one sum), each at most 2^-24 M, for the horizontal and again for the
        vertical blend, the first level's errors carried through weights that sum to one: 8 * 2^-24 M.
    grid_sample's own float64 rounding (normalising the coordinates and back) is below 1e-12 M."""
    side = 64
    rng = np.random.default_rng(5)
    u = float(np.spacing(np.float32(2 * side)))
    for trial in range(12):
        x = rng.standard_normal((side, side)).astype(np.float32)
        rec = R.records([rng.uniform(-45, 45)], [rng.uniform(0.75, 1.33)], [rng.uniform(-8, 8, 2)], side, side)[0]
        for m in (rec[0:6], rec[6:12], rec[12:18]):
            m64 = m.astype(np.float64).reshape(2, 3)
            j, i = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
            xs = m64[0, 0] * j + m64[0, 1] * i + m64[0, 2]
            ys = m64[1, 0] * j + m64[1, 1] * i + m64[1, 2]
            grid = torch.from_numpy(np.stack([2 * xs / (side - 1) - 1, 2 * ys / (side - 1) - 1], axis=-1))[None]
            want = torch.nn.functional.grid_sample(torch.from_numpy(x.astype(np.float64))[None, None], grid, mode='bilinear',
                                                   padding_mode='zeros', align_corners=True)[0, 0].numpy()
            padded = np.pad(x.astype(np.float64), 1)
            D = max(np.abs(np.diff(padded, axis=0)).max(), np.abs(np.diff(padded, axis=1)).max())
            M = np.abs(x).max()
            tol = 3 * u * D + 8 * 2.0 ** -24 * M + 1e-12 * M
            got = R.sample32(x, m)
            assert np.abs(got.astype(np.float64) - want).max() <= tol, (trial, np.abs(got - want).max(), tol)
            assert np.abs(R.sample64(x, m64) - want).max() <= 1e-12 * M          # the float64 oracle is grid_sample's sampler


# ---------------------------------------------------------------- records
def test_records_invert_each_other_and_follow_the_stride():
    rng = np.random.default_rng(6)
    for _ in range(50):
        a, s, t = rng.uniform(-45, 45), rng.uniform(0.75, 1.33), rng.uniform(-32, 32, 2)
        rec = R.records([a], [s], [t], 256, 64)[0].astype(np.float64)
        img, hm, inv = (np.vstack([rec[o:o + 6].reshape(2, 3), [0, 0, 1]]) for o in (0, 6, 12))
        # entries of magnitude <= 64 rounded to fp32 (relative 2^-24), products of two such matrices: a few 1e-5 at the most
        assert np.abs(inv @ hm - np.eye(3)).max() < 64 * 2 * 2.0 ** -24 * 3
        i64, h64, v64 = R.compose64(a, s, t, 256, 64)
        assert np.abs(h64[:, :2] - np.linalg.inv(i64[:, :2])).max() < 1e-12          # the same linear part as A
        c = np.array([127.5, 127.5])
        L = h64[:, :2]
        assert np.abs(h64[:, 2] - (c + t - L @ c) / 4).max() < 1e-12                # the translation over the stride
        # a point of the loader's frame, mapped into the view in image pixels and divided by the stride, is hm of the point / stride
        p = rng.uniform(0, 255, 2)
        q = np.linalg.inv(np.vstack([i64, [0, 0, 1]]))[:2] @ np.append(p, 1)
        assert np.abs(h64 @ np.append(p / 4, 1) - q / 4).max() < 1e-10
    with pytest.raises(ValueError):
        R.records([0], [1], [[0, 0]], (256, 128), 64)


def test_ops_view_records_equal_the_restatement():
    import mi355
    from mi355 import ops
    rng = np.random.default_rng(7)
    a, s, t = rng.uniform(-30, 30, 5), rng.uniform(0.75, 1.25, 5), rng.uniform(-25, 25, (5, 2))
    assert _bits(ops.view_records(a, s, t, 256, 64)) == _bits(R.records(a, s, t, 256, 64))
    ident = ops.view_records([0.0], [1.0], [[0.0, 0.0]], 64, 16)[0]
    assert np.array_equal(ident, np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), 3))
    for bad in (dict(angle=[np.nan]), dict(scale=[0.0]), dict(scale=[-1.0]), dict(shift=[[np.inf, 0]]), dict(image_size=(64, 32)),
                dict(heatmap_size=24), dict(scale=[1.0, 1.0])):
        with pytest.raises(mi355.Mi355Error):
            ops.view_records(**dict(dict(angle=[0.0], scale=[1.0], shift=[[0, 0]], image_size=64, heatmap_size=16), **bad))


# ---------------------------------------------------------------- round trip
def test_back_warped_gaussian_peaks_exactly_where_it_was_drawn():
    """A sigma = 2 Gaussian drawn in the teacher's frame at A_hm p0, p0 an integer point with p0 and A_hm p0 at least 6 pixels
    inside a 64 x 64 map; angles in +-45 degrees, scales in 0.75 .. 1.33, shifts in +-8 heat-map pixels.  After the back-warp the
    arg-max is exactly p0 (the float64 form of this sampler met this in 3283 of 3283 draws of the family)."""
    rng = np.random.default_rng(8)
    done = 0
    while done < 120:
        a, s, t = rng.uniform(-45, 45), rng.uniform(0.75, 1.33), rng.uniform(-8, 8, 2) * 4
        rec = R.records([a], [s], [t], 256, 64)[0]
        p0 = rng.integers(6, 58, 2)
        u = rec[6:12].astype(np.float64).reshape(2, 3) @ np.append(p0, 1)
        if not (6 <= u[0] <= 57 and 6 <= u[1] <= 57):
            continue
        done += 1
        y_v = R.gaussian(64, 64, u[0], u[1], 2.0)
        back = R.sample32(y_v, rec[6:12])
        i = R.argmax2d(back)
        assert (i % 64, i // 64) == (int(p0[0]), int(p0[1])), (a, s, t, p0)
        i64 = int(np.argmax(R.sample64(y_v, rec[6:12])))
        assert (i64 % 64, i64 // 64) == (int(p0[0]), int(p0[1]))


# ---------------------------------------------------------------- the flag
def _one_hot(h, w, *points):
    y = np.zeros((h, w), dtype=np.float32)
    for px, py in points:
        y[py, px] = 1.0
    return y


def test_flag_at_the_margin_on_ties_and_for_a_pre_image_outside():
    ident = R.from_matrices()
    w = h = 16
    for px, want in ((1, 0), (2, 1), (13, 1), (14, 0)):                         # margin - 1, margin, w-1-margin, w-margin
        assert R.valid_flag(_one_hot(h, w, (px, 8)), ident, 2) == want
        assert R.valid_flag(_one_hot(h, w, (8, px)), ident, 2) == want
    assert R.valid_flag(_one_hot(h, w, (5, 5), (1, 9)), ident, 2) == 1           # a tie: the first index in row-major order decides
    assert R.valid_flag(_one_hot(h, w, (9, 1), (5, 5)), ident, 2) == 0
    assert R.valid_flag(np.full((h, w), 0.25, np.float32), ident, 0) == 1         # flat: index 0; margin 0 accepts the corner
    assert R.valid_flag(np.full((h, w), 0.25, np.float32), ident, 0.5) == 0
    moved = R.from_matrices(R.shift_matrix(-6, 0), R.shift_matrix(-6, 0))        # the teacher's frame is 6 pixels to the side
    assert R.valid_flag(_one_hot(h, w, (12, 8)), moved, 2) == 0                   # its pre-image is column 18
    assert R.valid_flag(_one_hot(h, w, (9, 8)), moved, 2) == 1                    # column 15: the last one inside
    y = _one_hot(h, w, (8, 8)) * 1e-30                                            # the location decides, not the value
    assert R.valid_flag(y, ident, 2) == 1 and R.valid_flag(-_one_hot(h, w, (0, 0)) + 0, ident, 2) == 0
    y = _one_hot(h, w, (8, 8))
    y[0, 0] = np.nan                                                              # a NaN counts as the maximum
    assert R.valid_flag(y, ident, 2) == 0
    nan_rec = ident.copy()
    nan_rec[12] = np.nan
    assert R.valid_flag(_one_hot(h, w, (8, 8)), nan_rec, 2) == 0
    out, valid, w_out = R.unwarp_heatmaps(np.stack([_one_hot(h, w, (8, 8)), _one_hot(h, w, (1, 1))])[None], ident[None], 2,
                                          np.array([[[0.5], [1.0]]], np.float32))
    assert valid.tolist() == [[1.0, 0.0]] and w_out.tolist() == [[[0.5], [0.0]]]


def test_weighted_mse_restatement_is_the_unweighted_one_under_unit_weights():
    import mt_ref
    rng = np.random.default_rng(9)
    pred, target = rng.standard_normal((2, 5, 7, 9)).astype(np.float32), rng.random((2, 5, 7, 9)).astype(np.float32)
    rows, grad = R.mse_heatmap_w(pred, target, 0b10111, 0.01, np.ones((2, 5), np.float32))
    assert _bits(grad) == _bits(mt_ref.unit_grad(pred, target, 0b10111, 0.01))
    d = (pred.astype(np.float64) - target) ** 2
    assert np.allclose(rows, d.sum(axis=(2, 3)) * np.array([1, 1, 1, 0, 1]), rtol=1e-5)
    rows_w, grad_w = R.mse_heatmap_w(pred, target, 0b10111, 0.01, np.array([[0.5, 0, 1, 1, 0.25]] * 2, np.float32))
    assert _bits(rows_w[:, 0]) == _bits((rows[:, 0] * np.float32(0.5)).astype(np.float32)) and not rows_w[:, 1].any() and not rows_w[:, 3].any()
    assert _bits(grad_w[:, 4]) == _bits((grad[:, 4] * np.float32(0.25)).astype(np.float32)) and not grad_w[:, 1].any()


# ---------------------------------------------------------------- the command line
BASE = ['data/none', '--synthetic']


def _error(capsys, argv):
    import train1
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(BASE + argv)
    return capsys.readouterr().err


def test_parser_defaults_and_errors(capsys):
    import train1
    a = train1.build_parser().parse_args(BASE)
    assert (a.mt_view, a.view_rot, list(a.view_scale), a.view_shift, a.view_margin) == ('same', 30.0, [0.75, 1.25], 0.1, 2.0)
    ok = train1.build_parser().parse_args(BASE + ['--mt-view', 'geom', '--ema-update', 'const', '--mt-loss', 'on', '--view-rot', '15',
                                                  '--view-scale', '0.9', '1.1', '--view-shift', '0.05', '--view-margin', '3'])
    assert (ok.mt_view, ok.view_rot, list(ok.view_scale), ok.view_shift, ok.view_margin) == ('geom', 15.0, [0.9, 1.1], 0.05, 3.0)
    for consumer in (['--coord-loss', 'both'], ['--mixup', 'on', '--mixup-labels', 'teacher']):
        train1.build_parser().parse_args(BASE + ['--mt-view', 'geom', '--ema-update', 'warmup'] + consumer)
    err = _error(capsys, ['--mt-view', 'geom', '--ema-update', 'const'])
    assert '--mt-loss on' in err and '--coord-loss both' in err and '--mixup-labels teacher' in err
    err = _error(capsys, ['--mt-view', 'geom', '--ema-update', 'const', '--mixup', 'on'])          # student labels: no teacher forward
    assert '--mixup-labels teacher' in err
    err = _error(capsys, ['--mt-view', 'geom', '--mt-loss', 'on'])
    assert '--ema-update' in err
    geom = ['--mt-view', 'geom', '--ema-update', 'const', '--mt-loss', 'on']
    for bad in (['--view-rot', '-1'], ['--view-rot', 'nan'], ['--view-rot', '181'], ['--view-scale', '0', '1'], ['--view-scale', '1.2', '0.8'],
                ['--view-scale', '0.5', 'inf'], ['--view-shift', '-0.1'], ['--view-shift', '1.5'], ['--view-shift', 'nan'],
                ['--view-margin', '-1'], ['--view-margin', 'inf'], ['--view-margin', '40']):
        assert '--view-' in _error(capsys, geom + bad), bad


# ---------------------------------------------------------------- GeometricView's state
def _view(**kw):
    from mi355.teacher import GeometricView
    return GeometricView(**dict(dict(rot_deg=30.0, scale=(0.75, 1.25), shift=0.1, margin=2, seed=3, rank=0, image_size=64, heatmap_size=16), **kw))


def test_view_draws_inside_its_ranges_and_leaves_the_global_generator_alone():
    v = _view()
    torch.manual_seed(11)
    before = torch.get_rng_state().clone()
    for _ in range(20):
        p = v.draw(4, 'cpu')
        assert p.shape == (4, 4) and (np.abs(p[:, 0]) <= 30).all() and (p[:, 1] >= 0.75).all() and (p[:, 1] <= 1.25).all()
        assert (np.abs(p[:, 2:]) <= 0.1 * 64).all()
        assert _bits(v.recs_host) == _bits(R.records(p[:, 0], p[:, 1], p[:, 2:], 64, 16))
        assert _bits(v.recs.numpy().reshape(4, 18)) == _bits(v.recs_host)
    assert torch.equal(torch.get_rng_state(), before)
    pinned = _view(rot_deg=0.0, scale=(1.0, 1.0), shift=0.0, margin=0)
    pinned.draw(3, 'cpu')
    assert np.array_equal(pinned.recs_host, np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (3, 3)))


def test_view_state_round_trip_and_ranks():
    a = _view()
    for _ in range(3):
        a.draw(4, 'cpu')
    state = a.state_dict()
    want = [a.draw(4, 'cpu').copy() for _ in range(3)]
    b = _view()
    b.load_state_dict(state)
    assert b.draws == 3
    assert all(_bits(b.draw(4, 'cpu')) == _bits(w) for w in want)
    other = _view(rank=1)
    assert _bits(other.draw(4, 'cpu')) != _bits(_view().draw(4, 'cpu'))           # ranks draw different views from the start
    other = _view(rank=1)
    other.load_state_dict(state)                                                   # rank 0's checkpoint: the count, a state of its own
    assert other.draws == 3
    got = [other.draw(4, 'cpu').copy() for _ in range(3)]
    assert all(_bits(g) != _bits(w) for g, w in zip(got, want))
    again = _view(rank=1)
    again.load_state_dict(state)
    assert all(_bits(again.draw(4, 'cpu')) == _bits(g) for g in got)


def test_view_refuses_bad_ranges():
    for bad in (dict(rot_deg=-1), dict(rot_deg=float('nan')), dict(scale=(0.0, 1.0)), dict(scale=(1.2, 0.8)), dict(scale=(0.5, float('inf'))),
                dict(shift=-0.1), dict(shift=float('nan')), dict(margin=-1), dict(margin=float('inf'))):
        with pytest.raises(ValueError):
            _view(**bad)
