"""The geometric teacher view on the GPU: mi355_affine_warp_images, mi355_affine_unwarp_heatmaps and mi355_mse_heatmap_w bit for
bit against the fp32 restatement of tests/warp_ref.py, inside the poisoned guard buffers of tests/guarded.py: every output
element written, no flank byte changed, the inputs unchanged."""
import numpy as np
import pytest
import torch

import guarded
import warp_ref as R

pytestmark = pytest.mark.gpu

IMAGES = [(1, 3, 16, 16), (3, 3, 17, 19), (2, 1, 24, 40), (2, 3, 64, 64), (2, 3, 256, 256)]
MAPS = [(1, 1, 4, 4), (3, 21, 16, 16), (2, 5, 17, 19), (2, 21, 64, 64), (1, 3, 128, 128), (1, 2, 130, 127)]
KINDS = ('identity', 'shift', 'quarter', 'random', 'outside', 'nan')


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _records(kind, B, H, W, stride, seed):
    """(B, 18) records for planes of H x W pixels; `stride` = image pixels per heat-map pixel of the random draws (1: the plane is
    an image, 4: the plane is a heat-map of a 4H x 4W image)."""
    if kind == 'identity':
        one = R.from_matrices()
    elif kind == 'shift':
        one = R.from_matrices(R.shift_matrix(3, -2), R.shift_matrix(3, -2))
    elif kind == 'quarter':
        one = R.from_matrices(R.quarter_matrix(min(H, W)), R.quarter_matrix(min(H, W)))
    elif kind == 'outside':
        one = R.from_matrices(R.shift_matrix(2 * W, 0), R.shift_matrix(2 * W, 0))
    elif kind == 'nan':
        one = R.from_matrices().copy()
        one[[0, 6, 12]] = np.nan                      # a hand-built record: one NaN entry in each matrix
    else:
        rng = np.random.default_rng(seed)             # the default ranges of the view: 30 degrees, 0.75 .. 1.25, a tenth of the side
        side = stride * max(H, W)
        return R.records(rng.uniform(-30, 30, B), rng.uniform(0.75, 1.25, B), rng.uniform(-0.1, 0.1, (B, 2)) * side,
                         (stride * H, stride * W), (H, W))
    return np.tile(one[None], (B, 1)).astype(np.float32)


# ---------------------------------------------------------------- images
def _check_images(gpu, shape, kind, x=None, in_start=guarded.START, out_start=guarded.START, seed=0):
    from mi355 import ops
    B, C, H, W = shape
    if x is None:
        x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    recs = _records(kind, B, H, W, 1, seed + 1)
    x_d = guarded.place(torch.from_numpy(x).to(gpu), 'x', start=in_start)
    r_d = guarded.place(torch.from_numpy(recs).to(gpu), 'recs', start=in_start)
    out = guarded.empty(shape, torch.float32, gpu, 'out', start=out_start)
    assert x_d.data_ptr() % 16 == in_start % 16 and out.data_ptr() % 16 == out_start % 16
    got = ops.affine_warp_images(x_d, r_d, out=out)
    torch.cuda.synchronize()
    guarded.check('affine_warp_images %s %s' % (shape, kind))
    assert got.data_ptr() == out.data_ptr()
    want = R.warp_images(x, recs)
    assert guarded.unwritten(got) == 0 or np.isnan(want).any(), (shape, kind)
    assert _same(got, want), (shape, kind)
    assert _same(x_d, x) and _same(r_d, recs)                      # the inputs are only read
    return got, want


@pytest.mark.parametrize('shape', IMAGES, ids=lambda s: 'x'.join(map(str, s)))
def test_image_warp_bit_exact_inside_guard_buffers(gpu, shape):
    try:
        for kind in KINDS:
            got, want = _check_images(gpu, shape, kind, seed=sum(shape))
            if kind in ('outside', 'nan'):
                assert not want.any() and not np.signbit(want).any()       # all +0
            if kind == 'random':
                assert np.count_nonzero(want) > want.size // 2
    finally:
        guarded.reset()


def _special_planes(shape, seed):
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = -0.0
    flat[3::11] = np.inf
    flat[5::13] = -np.inf
    flat[1::17] = np.nan
    return x


def test_exact_records_copy_negative_zero_inf_and_nan(gpu):
    try:
        for shape in ((2, 3, 16, 16), (1, 2, 17, 17)):
            x = _special_planes(shape, 3)
            got, _ = _check_images(gpu, shape, 'identity', x=x)
            assert _same(got, x)
            got, _ = _check_images(gpu, shape, 'quarter', x=x)
            side = shape[-1]
            j, i = np.meshgrid(np.arange(side), np.arange(side))
            assert _same(got, x[:, :, j, side - 1 - i])                 # output (row i, column j) = input (row j, column side-1-i)
            got, _ = _check_images(gpu, shape, 'shift', x=x)
            want = np.zeros_like(x)
            want[:, :, 2:, :-3] = x[:, :, :-2, 3:]                      # output (i, j) = input (i - 2, j + 3), +0 where that runs out
            assert _same(got, want)
    finally:
        guarded.reset()


@pytest.mark.parametrize('which', ['all', 'inputs', 'outputs'])
def test_scalar_paths_on_views_4_bytes_off_a_16_byte_boundary(gpu, which):
    off = guarded.START + 4
    ins = off if which != 'outputs' else guarded.START
    outs = off if which != 'inputs' else guarded.START
    try:
        for shape in ((2, 3, 16, 16), (3, 3, 17, 19)):
            for kind in ('identity', 'random'):
                _check_images(gpu, shape, kind, in_start=ins, out_start=outs, seed=9)
        for shape in ((3, 21, 16, 16), (2, 5, 17, 19)):
            for kind in ('quarter', 'random'):
                _check_maps(gpu, shape, kind, in_start=ins, out_start=outs, seed=9)
        _check_mse(gpu, (2, 21, 8, 8), in_start=ins, out_start=outs, seed=9)
    finally:
        guarded.reset()


# ---------------------------------------------------------------- heat-maps
def _maps(shape, seed):
    """Gaussians at random centres, some of them close to or on the border, on a floor of small noise; every third map flat (a
    tie over the whole map: index 0 wins)."""
    B, K, h, w = shape
    rng = np.random.default_rng(seed)
    y = (rng.random(shape) * 0.01).astype(np.float32)
    for b in range(B):
        for k in range(K):
            if (b * K + k) % 3 == 2:
                y[b, k] = 0.25
            else:
                y[b, k] += R.gaussian(h, w, rng.integers(0, w), rng.integers(0, h), 1.5)
    return y


def _check_maps(gpu, shape, kind, y=None, margin=None, with_w=True, in_start=guarded.START, out_start=guarded.START, seed=0):
    from mi355 import ops
    B, K, h, w = shape
    margin = (1 if min(h, w) < 8 else 2) if margin is None else margin
    if y is None:
        y = _maps(shape, seed)
    recs = _records(kind, B, h, w, 4, seed + 1)
    w_in = (np.random.default_rng(seed + 2).integers(0, 3, (B, K, 1)) * 0.5).astype(np.float32) if with_w else None
    y_d = guarded.place(torch.from_numpy(y).to(gpu), 'y', start=in_start)
    r_d = guarded.place(torch.from_numpy(recs).to(gpu), 'recs', start=in_start)
    w_d = guarded.place(torch.from_numpy(w_in).to(gpu), 'w_in', start=in_start) if with_w else None
    out = (guarded.empty(shape, torch.float32, gpu, 'y_hat', start=out_start), guarded.empty((B, K), torch.float32, gpu, 'valid', start=out_start),
           guarded.empty((B, K, 1), torch.float32, gpu, 'w_out', start=out_start) if with_w else None)
    got = ops.affine_unwarp_heatmaps(y_d, r_d, margin, w_in=w_d, out=out)
    torch.cuda.synchronize()
    guarded.check('affine_unwarp_heatmaps %s %s' % (shape, kind))
    want = R.unwarp_heatmaps(y, recs, margin, w_in)
    for g, o, wt, name in zip(got, out, want, ('y_hat', 'valid', 'w_out')):
        if o is None:
            assert g is None and wt is None
            continue
        assert g.data_ptr() == o.data_ptr()
        assert guarded.unwritten(g) == 0 or np.isnan(wt).any(), (name, shape, kind)
        assert _same(g, wt), (name, shape, kind)
    assert _same(y_d, y) and _same(r_d, recs) and (not with_w or _same(w_d, w_in))
    return got, want


@pytest.mark.parametrize('shape', MAPS, ids=lambda s: 'x'.join(map(str, s)))
def test_heatmap_unwarp_bit_exact_inside_guard_buffers(gpu, shape):
    """(1,3,128,128) is the largest map staged in LDS (64 KB, 1024 threads), (1,2,130,127) the global-memory form."""
    try:
        seen = set()
        for kind in KINDS:
            got, want = _check_maps(gpu, shape, kind, seed=sum(shape))
            seen.update(want[1].reshape(-1).tolist())
            if kind in ('outside', 'nan'):
                assert not want[0].any() and not want[1].any() and not want[2].any()
            if kind == 'identity':
                assert _same(got[0], _maps(shape, sum(shape)))
        assert seen == {0.0, 1.0} or shape[2] < 8
        _check_maps(gpu, shape, 'random', with_w=False, seed=5)
    finally:
        guarded.reset()


def test_flag_at_the_margin_on_ties_and_for_a_peak_seen_from_outside(gpu):
    h = w = 16
    peaks = [(1, 8), (2, 8), (13, 8), (14, 8), (8, 1), (8, 2), (8, 13), (8, 14)]      # margin - 1, margin, w-1-margin, w-margin
    y = np.zeros((1, len(peaks) + 2, h, w), dtype=np.float32)
    for k, (px, py) in enumerate(peaks):
        y[0, k, py, px] = 1.0
    y[0, -2, 5, 5] = y[0, -2, 9, 1] = 2.0                                             # a tie: the first index (5, 5) decides
    y[0, -1, 1, 9] = y[0, -1, 5, 5] = 2.0                                             # a tie whose first index is cut by the frame
    try:
        got, want = _check_maps(gpu, y.shape, 'identity', y=y, margin=2)
        assert want[1].reshape(-1).tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 1, 0]
        # the teacher's frame is shifted by 6 pixels: a peak at column 12 of it has its pre-image at column 18, outside the map
        y2 = np.zeros((1, 2, h, w), dtype=np.float32)
        y2[0, 0, 8, 12] = y2[0, 1, 8, 9] = 1.0
        recs = np.tile(R.from_matrices(R.shift_matrix(-6, 0), R.shift_matrix(-6, 0))[None], (1, 1))
        from mi355 import ops
        out = ops.affine_unwarp_heatmaps(torch.from_numpy(y2).to(gpu), torch.from_numpy(recs).to(gpu), 2)
        assert out[1].cpu().reshape(-1).tolist() == [0.0, 1.0] and out[2] is None
        assert R.unwarp_heatmaps(y2, recs, 2)[1].reshape(-1).tolist() == [0.0, 1.0]
        # a NaN counts as the maximum: its location decides
        y3 = y2.copy()
        y3[0, 1, 0, 0] = np.nan
        out = ops.affine_unwarp_heatmaps(torch.from_numpy(y3).to(gpu), torch.from_numpy(recs).to(gpu), 2)
        assert out[1].cpu().reshape(-1).tolist() == [0.0, 0.0]
    finally:
        guarded.reset()


# ---------------------------------------------------------------- weighted MSE
def _check_mse(gpu, shape, wmap=None, k=400, poison=False, in_start=guarded.START, out_start=guarded.START, seed=0):
    from mi355 import ops
    import mt_ref
    B, K, H, W = shape
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal(shape).astype(np.float32)
    target = rng.random(shape).astype(np.float32)
    if wmap is None:
        wmap = rng.choice(np.array([0.0, 1.0, 0.5, 0.3], dtype=np.float32), (B, K))
    mask = mt_ref.mask(k, K) & ((1 << K) - 1)
    if poison:                                              # rows that must not be read hold NaN
        for b in range(B):
            for j in range(K):
                if wmap[b, j] == 0 or not (mask >> j) & 1:
                    pred[b, j] = np.nan
                    target[b, j] = np.nan
    gs = np.float32(2.0 * 0.3 / pred.size)
    p_d, t_d, w_d = (guarded.place(torch.from_numpy(a).to(gpu), n, start=in_start) for a, n in ((pred, 'pred'), (target, 'target'), (wmap, 'wmap')))
    rec = guarded.place(ops.mse_record(mask, gs, device=gpu), 'rec')
    rows, grad = guarded.empty((B, K), torch.float32, gpu, 'rows'), guarded.empty(shape, torch.float32, gpu, 'grad', start=out_start)
    got = ops.mse_heatmap_w(p_d, t_d, rec, w_d, True, rows=rows, grad=grad)
    torch.cuda.synchronize()
    guarded.check('mse_heatmap_w %s' % (shape,))
    vec = (H * W) % 4 == 0 and in_start % 16 == 0 and out_start % 16 == 0
    want = R.mse_heatmap_w(pred, target, mask, gs, wmap, vec=vec)
    for g, wt, n in zip(got, want, ('rows', 'grad')):
        assert guarded.unwritten(g) == 0, n
        assert _same(g, wt), (n, shape)
    assert _same(p_d, pred) and _same(t_d, target) and _same(w_d, wmap)
    return got, (pred, target, mask, gs)


@pytest.mark.parametrize('shape', [(2, 21, 8, 8), (3, 5, 7, 9), (1, 21, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_weighted_mse_against_the_restatement(gpu, shape):
    try:
        _check_mse(gpu, shape, seed=1)
        _check_mse(gpu, shape, k=250, poison=True, seed=2)           # a NaN-poisoned row under w == 0 or outside the mask is not read
    finally:
        guarded.reset()


@pytest.mark.parametrize('shape', [(2, 21, 8, 8), (3, 5, 7, 9), (2, 21, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_weighted_mse_with_unit_weights_is_mse_heatmap(gpu, shape):
    from mi355 import ops
    try:
        ones = np.ones(shape[:2], dtype=np.float32)
        for k in (400, 150):
            (rows, grad), (pred, target, mask, gs) = _check_mse(gpu, shape, wmap=ones, k=k, seed=4)
            rec = ops.mse_record(mask, gs, device=gpu)
            rows0, grad0 = ops.mse_heatmap(torch.from_numpy(pred).to(gpu), torch.from_numpy(target).to(gpu), rec, True)
            assert _same(rows, rows0) and _same(grad, grad0)
    finally:
        guarded.reset()


# ---------------------------------------------------------------- determinism, the log, refusals
def test_two_eager_runs_and_a_graph_replay_give_the_same_bits(gpu):
    from mi355 import ops
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((2, 3, 64, 64)).astype(np.float32)).to(gpu)
    y = torch.from_numpy(_maps((2, 21, 16, 16), 12)).to(gpu)
    w_in = torch.ones(2, 21, 1, device=gpu)
    recs = torch.from_numpy(_records('random', 2, 16, 16, 4, 13)).to(gpu)
    rec = ops.mse_record(0x1fffff, 1e-3, device=gpu)
    bufs = dict(v=torch.empty_like(x), u=(torch.empty_like(y), torch.empty(2, 21, device=gpu), torch.empty(2, 21, 1, device=gpu)),
                rows=torch.empty(2, 21, device=gpu), grad=torch.empty_like(y))

    def run():
        ops.affine_warp_images(x, recs, out=bufs['v'])
        y_hat, valid, _ = ops.affine_unwarp_heatmaps(y, recs, 2, w_in=w_in, out=bufs['u'])
        ops.mse_heatmap_w(y, y_hat, rec, valid, True, rows=bufs['rows'], grad=bufs['grad'])

    def snap():
        torch.cuda.synchronize()
        return [_bits(t) for t in (bufs['v'],) + bufs['u'] + (bufs['rows'], bufs['grad'])]

    run(); first = snap()
    run(); assert snap() == first
    import mi355
    g = torch.cuda.CUDAGraph()
    with mi355.no_gc_in_capture():
        with torch.cuda.graph(g):
            run()
    for t in (bufs['v'],) + bufs['u'] + (bufs['rows'], bufs['grad']):
        t.fill_(-7.0)
    g.replay()
    assert snap() == first


def test_launches_are_logged_under_their_labels(gpu):
    from mi355 import ops
    x, y = torch.zeros(2, 3, 16, 16, device=gpu), torch.zeros(2, 5, 8, 8, device=gpu)
    recs = torch.from_numpy(_records('identity', 2, 8, 8, 4, 0)).to(gpu)
    rec = ops.mse_record(0x1f, 1.0, device=gpu)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        ops.affine_warp_images(x, recs)
        y_hat, valid, _ = ops.affine_unwarp_heatmaps(y, recs, 2)
        ops.mse_heatmap_w(y, y_hat, rec, valid, True)
        torch.cuda.synchronize()
        log = ops.prof_launches()
    finally:
        ops.prof_enable(0); ops.prof_reset()
    assert [e['label'].split()[0] for e in log] == ['affine_warp', 'affine_unwarp', 'mse_heatmap_w']
    assert all(e['family'] == 2 for e in log)
    assert log[0]['bytes'] == 8.0 * x.numel() + 72 * 2 and log[1]['bytes'] == 8.0 * y.numel() + 72 * 2 + 4 * 10
    assert log[2]['bytes'] == 12.0 * y.numel() + 4 * 10


def test_wrappers_refuse_what_the_kernels_cannot_index(gpu, monkeypatch):
    import mi355
    from mi355 import ops
    z = lambda *s: torch.zeros(s, device=gpu)
    recs = torch.from_numpy(_records('identity', 2, 8, 8, 4, 0)).to(gpu)
    x, y, w_in = z(2, 3, 8, 8), z(2, 5, 8, 8), z(2, 5, 1)
    ops.affine_warp_images(x, recs)
    ops.affine_unwarp_heatmaps(y, recs, 0, w_in=w_in)
    bad_warp = [dict(x=z(2, 3, 8, 16)[..., ::2]), dict(x=x.double()), dict(x=x.cpu()), dict(x=z(3, 3, 8, 8)), dict(x=z(3, 8, 8)),
                dict(recs=recs[:1]), dict(recs=recs.double()), dict(recs=recs.cpu()), dict(out=z(2, 3, 8, 9)), dict(out=z(2, 3, 8, 8).half()),
                dict(out=z(2, 3, 8, 16)[..., ::2])]
    for change in bad_warp:
        with pytest.raises(mi355.Mi355Error):
            ops.affine_warp_images(**dict(dict(x=x, recs=recs), **change))
    with pytest.raises(mi355.Mi355Error, match='overlap'):
        ops.affine_warp_images(x, recs, out=x)
    for margin in (-1, float('nan'), float('inf'), None, '2'):
        with pytest.raises(mi355.Mi355Error):
            ops.affine_unwarp_heatmaps(y, recs, margin)
    bad_unwarp = [dict(y=z(2, 5, 8, 16)[..., ::2]), dict(y=y.half()), dict(y=z(3, 5, 8, 8)), dict(recs=recs.reshape(-1)[:35]),
                  dict(w_in=z(2, 4, 1)), dict(w_in=w_in.double()), dict(w_in=w_in.cpu()),
                  dict(out=(z(2, 5, 8, 8), z(2, 5), None), w_in=w_in), dict(out=(z(2, 5, 8, 8), z(2, 5), z(2, 5, 1))),
                  dict(out=(z(2, 5, 8, 9), z(2, 5), None)), dict(out=(z(2, 5, 8, 8), z(2, 4), None)), dict(out=(y, z(2, 5), None))]
    for change in bad_unwarp:
        with pytest.raises(mi355.Mi355Error):
            ops.affine_unwarp_heatmaps(**dict(dict(y=y, recs=recs, margin=2), **change))
    rec = ops.mse_record(0x1f, 1.0, device=gpu)
    ops.mse_heatmap_w(y, y, rec, z(2, 5), True)
    for change in (dict(target=z(2, 5, 8, 9)), dict(wmap=z(2, 4)), dict(wmap=z(2, 5).double()), dict(wmap=z(2, 5).cpu()),
                   dict(pred=y.half()), dict(rec=rec.float()), dict(rows=z(2, 4)), dict(grad=z(2, 5, 8, 4)),
                   dict(pred=z(2, 5, 8, 16)[..., ::2])):
        with pytest.raises(mi355.Mi355Error):
            ops.mse_heatmap_w(**dict(dict(pred=y, target=y, rec=rec, wmap=z(2, 5), want_grad=True), **change))
    # no allocation during graph capture
    wmap = z(2, 5)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    for call in (lambda: ops.affine_warp_images(x, recs), lambda: ops.affine_unwarp_heatmaps(y, recs, 2),
                 lambda: ops.mse_heatmap_w(y, y, rec, wmap, True), lambda: ops.mse_heatmap_w(y, y, rec, wmap, True, rows=z(2, 5))):
        with pytest.raises(mi355.Mi355Error, match='during graph capture'):
            call()


def test_view_records_refuse_bad_draws():
    import mi355
    from mi355 import ops
    r = ops.view_records([10.0, -20.0], [1.0, 0.8], [[3, 0], [0, -5]], 64, 16)
    assert r.shape == (2, 18) and r.dtype == np.float32
    assert _same(r, R.records([10.0, -20.0], [1.0, 0.8], [[3, 0], [0, -5]], 64, 16))
    for a, s, t, im, hm in (([np.nan], [1.0], [[0, 0]], 64, 16), ([0.0], [0.0], [[0, 0]], 64, 16), ([0.0], [-1.0], [[0, 0]], 64, 16),
                            ([0.0], [np.inf], [[0, 0]], 64, 16), ([0.0], [1.0], [[np.inf, 0]], 64, 16), ([0.0], [1.0], [[0, 0]], (64, 32), 16),
                            ([0.0], [1.0], [[0, 0]], 64, 24), ([0.0, 1.0], [1.0], [[0, 0]], 64, 16)):
        with pytest.raises(mi355.Mi355Error):
            ops.view_records(a, s, t, im, hm)
