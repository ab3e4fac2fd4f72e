"""mi355_peak_prob, mi355_teacher_select and mi355_occlude_images (csrc/occlude.hip) through the C ABI, against the restatement of
tests/occlude_ref.py.

Forms of peak_prob.  `row_form()` picks the register-resident kernel of the map size (64 x 64: block per map; 32 x 32 and 16 x 16:
wave per map) for a 16-byte-aligned `hm`, and the loop kernel for any other size (24 x 40) or pointer.  Every case runs from an
aligned buffer and with `hm` one float past a 16-byte boundary; rows 1, 4, 5 and 21 give the wave-per-map forms a partial
workgroup.  idx and xy must equal mi355_argmax2d's on the same buffer bit for bit; p is held to the ceiling of
tests/test_occlude_cpu.py (8 x the float32 CPU expression's error + 2^-23 max |ref|), the worst error / ceiling is printed.

teacher_select and occlude_images are integer work behind one comparison: bit for bit with the restatement.

Operands and outputs live in the 0xFF-filled guard buffers of tests/guarded.py: the flanks must survive and every output word
must be written.  Every call is made twice and must give the same bits."""
import numpy as np
import pytest
import torch

import guarded
import occlude_ref as R
from test_occlude_cpu import PEAK_CASES, PEAK_SIDES, peak_yardstick

pytestmark = pytest.mark.gpu

HM_ALIGN = {'aligned': guarded.START, 'hm+4': guarded.START + 4}
SENTINEL = -7.0                    # no p is negative


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(a, gpu, name, start=guarded.START):
    return guarded.place(torch.from_numpy(np.ascontiguousarray(a)).to(gpu), name, start=start)


def _peak(mi, gpu, hm, beta, align='aligned', nan_ok=False):
    """Two launches on the same guarded buffers, and mi355_argmax2d on the same hm -> (idx, xy, p, idx_ref, xy_ref) on the CPU."""
    rows, H, W = hm.shape
    h = _dev(hm, gpu, 'hm', HM_ALIGN[align])
    assert h.data_ptr() % 16 == HM_ALIGN[align] % 16
    idx = guarded.empty((rows,), torch.int32, gpu, 'idx')
    xy = guarded.empty((rows, 2), torch.float32, gpu, 'xy')
    p = guarded.empty((rows,), torch.float32, gpu, 'p')
    if nan_ok:
        p.fill_(SENTINEL)                                     # (the guard fill 0xFF.. is itself a NaN: a finite word shows an unwritten p)
    outs = []
    for _ in range(2):
        mi.call('mi355_peak_prob', mi.ptr(h), float(beta), mi.ptr(idx), mi.ptr(xy), mi.ptr(p), rows, H, W, mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append((idx.cpu().clone(), xy.cpu().clone(), p.cpu().clone()))
    idx2 = guarded.empty((rows,), torch.int32, gpu, 'idx_argmax')
    xy2 = guarded.empty((rows, 2), torch.float32, gpu, 'xy_argmax')
    mi.call('mi355_argmax2d', mi.ptr(h), mi.ptr(idx2), mi.ptr(xy2), 0, rows, H, W, mi.stream_ptr())
    torch.cuda.synchronize()
    guarded.check('peak_prob %dx%d rows %d %s' % (H, W, rows, align))
    assert guarded.unwritten(idx) == 0 and guarded.unwritten(xy) == 0
    assert guarded.unwritten(p) == 0 and not bool((p == SENTINEL).any())      # every p written, the NaN ones too
    for a, b in zip(*outs):
        assert _same(a, b), 'two launches, different bits'
    assert torch.equal(h.cpu(), torch.from_numpy(hm)) or nan_ok
    return outs[0] + (idx2.cpu(), xy2.cpu())


# ------------------------------------------------------------------------------------------------------------- peak_prob
@pytest.mark.parametrize('side', PEAK_SIDES, ids=lambda s: '%dx%d' % s)
def test_peak_prob_every_form_within_the_yardstick_ceiling(gpu, side):
    mi, _ = _mi()
    worst = 0.0
    for case in [c for c in PEAK_CASES if (c[0], c[1]) == side]:
        H, W, rows, beta = case
        y = peak_yardstick(*case)
        for align in HM_ALIGN:
            idx, xy, p, idx2, xy2 = _peak(mi, gpu, y['hm'], y['beta'], align)
            assert torch.equal(idx, idx2) and _same(xy, xy2)                      # mi355_argmax2d's, bit for bit
            assert np.array_equal(idx.numpy(), y['idx']) and np.array_equal(xy.numpy(), y['xy'])
            err = float(np.abs(p.numpy().astype(np.float64) - y['ref']).max())
            print('%dx%d rows %d beta %g %s: error %.3e, ceiling %.3e (float32 CPU expression %.3e)' % (H, W, rows, beta, align, err, y['bound'], y['yard']))
            assert err <= y['bound']
            worst = max(worst, err / y['bound'])
            # the gate the chain takes of these p is the reference's: no map sits on the threshold
            assert np.array_equal(p.numpy() >= np.float32(y['tau']), y['ref'] >= y['tau'])
    print('%dx%d: worst error %.2f of its ceiling' % (side + (worst,)))


@pytest.mark.parametrize('side', PEAK_SIDES, ids=lambda s: '%dx%d' % s)
def test_peak_prob_nan_infinities_flat_maps_and_ties(gpu, side):
    mi, _ = _mi()
    H, W = side
    for align in HM_ALIGN:
        hm = R.maps(H, W, 9, seed=3)
        hm[0, H // 3, W // 4] = hm[0, H - 1, W - 1] = 40.0         # a tie: the first index
        hm[1, H // 2, 1] = np.nan
        hm[2, 0, W - 1] = np.inf
        hm[3, H - 1, W - 1] = -np.inf
        hm[4, 2, 2] = np.nan; hm[4, 1, 1] = np.nan                 # two NaNs: the first
        hm[5] = -3.25                                              # all equal: p = 1 / HW, idx 0
        hm[6] = 0.0; hm[6, H - 1, 0] = -0.0
        hm[7, 0, 0] = np.inf; hm[7, 0, 1] = np.nan                 # a NaN beats an inf
        idx, xy, p, idx2, xy2 = _peak(mi, gpu, hm, 1.0, align, nan_ok=True)
        want_idx, want_xy, ref = R.peak_prob(hm, 1.0)
        assert torch.equal(idx, idx2) and _same(xy, xy2)
        assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(xy.numpy(), want_xy)
        got = p.numpy()
        assert np.isnan(got[[1, 2, 3, 4, 7]]).all() and np.isfinite(got[[0, 5, 6, 8]]).all()
        assert got[5] == np.float32(1.0 / (H * W)) and got[6] == np.float32(1.0 / (H * W))
        assert abs(float(got[0]) - ref[0]) <= 1e-5 * ref[0] and abs(float(got[8]) - ref[8]) <= 1e-5 * ref[8]
        assert idx[0] == (H // 3) * W + W // 4 and idx[4] == W + 1 and idx[5] == 0 and idx[7] == 1
        # a NaN fails every >=: no non-finite map is ever confident
        assert not (got[[1, 2, 3, 4, 7]] >= np.float32(0.0)).any()


def test_peak_confidence_and_the_wrapper_outputs(gpu):
    mi, ops = _mi()
    from uda.model.loss import peak_confidence
    y = peak_yardstick(64, 64, 21, 1.0)
    hm = torch.from_numpy(y['hm']).view(1, 21, 64, 64).to(gpu)
    idx, xy, p = ops.peak_prob(hm, 1.0)
    assert idx.shape == (1, 21) and xy.shape == (1, 21, 2) and p.shape == (1, 21)
    xy2, p2 = peak_confidence(hm.requires_grad_(True), 1.0)
    assert _same(xy.cpu(), xy2.cpu()) and _same(p.cpu(), p2.cpu()) and not p2.requires_grad
    assert _same(xy.cpu(), ops.argmax2d(hm.detach())[1].cpu())
    out = (torch.empty_like(idx), torch.empty_like(xy), torch.empty_like(p))
    got = ops.peak_prob(hm.detach(), 1.0, out=out)
    assert all(a is b for a, b in zip(got, out)) and _same(out[2].cpu(), p.cpu())
    with pytest.raises(mi.Mi355Error, match='hm'):
        ops.peak_prob(hm.detach()[:, :, :, ::2], 1.0)
    with pytest.raises(mi.Mi355Error, match=' p '):
        ops.peak_prob(hm.detach(), 1.0, out=(out[0], out[1], torch.empty(1, 20, device=gpu)))
    for beta in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(mi.Mi355Error, match='beta'):
            ops.peak_prob(hm.detach(), beta)


# ---------------------------------------------------------------------------------------------------------- teacher_select
def _select(mi, gpu, c):
    """Two launches on guarded buffers -> (conf, w_out, boxes, count, stats) as numpy arrays (None where the call has none)."""
    B, K = c['p'].shape
    N = c['N']
    d = lambda a, n: None if a is None else _dev(a, gpu, n)
    p, xy, g, w, u = d(c['p'], 'p'), d(c['xy'], 'xy'), d(c['gate_in'], 'gate_in'), d(c['w_in'], 'w_in'), d(c['u'], 'u')
    conf = guarded.empty((B, K), torch.float32, gpu, 'conf')
    w_out = None if w is None else guarded.empty(tuple(w.shape), torch.float32, gpu, 'w_out')
    boxes = guarded.empty((B, N, 4), torch.int32, gpu, 'boxes') if N else None
    count = guarded.empty((B,), torch.int32, gpu, 'count') if N else None
    stats = guarded.empty((2,), torch.float32, gpu, 'stats')
    outs = []
    for _ in range(2):
        mi.call('mi355_teacher_select', mi.ptr(p), mi.ptr(xy) if N else 0, mi.ptr(g), mi.ptr(w), mi.ptr(u) if N else 0, float(c['tau']),
                float(c['prob']), N, c['lo'], c['hi'], c['S'], c['H'], c['W'], mi.ptr(conf), mi.ptr(w_out), mi.ptr(boxes), mi.ptr(count),
                mi.ptr(stats), B, K, mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append(tuple(None if t is None else t.cpu().clone() for t in (conf, w_out, boxes, count, stats)))
    guarded.check('teacher_select B%d K%d N%d' % (B, K, N))
    for t in (conf, w_out, boxes, count, stats):
        assert t is None or guarded.unwritten(t) == 0
    for a, b in zip(*outs):
        assert a is None or _same(a, b), 'two launches, different bits'
    return tuple(None if t is None else t.numpy() for t in outs[0])


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('K', [21, 1])
def test_teacher_select_bit_for_bit(gpu, B, K):
    mi, _ = _mi()
    n = boxes_seen = 0
    for case in [c for c in R.SELECT_CASES if c[0] == B and c[1] == K]:
        c = R.select_case(*case)
        want = R.teacher_select(c['p'], c['xy'], c['gate_in'], c['w_in'], c['u'], c['tau'], c['prob'], c['N'], c['lo'], c['hi'], c['S'], c['H'], c['W'])
        got = _select(mi, gpu, c)
        for name, g, w in zip(('conf', 'w_out', 'boxes', 'count', 'stats'), got, want):
            assert (g is None) == (w is None), (case, name)
            assert g is None or (g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()), (case, name, g, w)
        n += 1
        boxes_seen += 0 if want[3] is None else int(want[3].sum())
    print('B %d K %d: %d cases bit for bit, %d boxes among them' % (B, K, n, boxes_seen))
    assert n == 24 and boxes_seen > 0


def test_teacher_select_on_the_peaks_the_kernel_gave(gpu):
    """The chain: p and xy of mi355_peak_prob feed mi355_teacher_select; flags and boxes equal the restatement on the float64 p."""
    mi, ops = _mi()
    y = peak_yardstick(64, 64, 21, 1.0)
    hm = torch.from_numpy(y['hm']).view(1, 21, 64, 64).to(gpu)
    _, xy, p = ops.peak_prob(hm, 1.0)
    u = np.array([[0.0, 0.3, 0.7, 0.9, 0.1, 0.5, 0.5]], np.float32)
    stats = torch.empty(2, device=gpu)
    conf, w_out, boxes, count = ops.teacher_select(p, xy, torch.from_numpy(u).to(gpu), y['tau'], 1.0, 3, 20, 41, 256, (64, 64), stats=stats)
    want = R.teacher_select(y['ref'].astype(np.float32).reshape(1, 21), y['xy'].reshape(1, 21, 2), None, None, u, y['tau'], 1.0, 3, 20, 41, 256, 64, 64)
    assert w_out is None and conf.cpu().numpy().tobytes() == want[0].tobytes()
    assert boxes.cpu().numpy().tobytes() == want[2].tobytes() and count.cpu().tolist() == [3]
    assert stats.cpu().numpy().tobytes() == want[4].tobytes()


# ---------------------------------------------------------------------------------------------------------- occlude_images
IMG_ALIGN = {'aligned': (guarded.START, guarded.START), 'x+4': (guarded.START + 4, guarded.START), 'out+4': (guarded.START, guarded.START + 4)}


def _occlude(mi, gpu, x, boxes, align='aligned'):
    B, C, H, W = x.shape
    N = boxes.shape[1]
    sx, so = IMG_ALIGN[align]
    xd = guarded.place(torch.from_numpy(x.view(np.int32)).to(gpu), 'x', start=sx)
    bd = _dev(boxes, gpu, 'boxes')
    out = guarded.empty((B, C, H, W), torch.int32, gpu, 'out', start=so)
    assert xd.data_ptr() % 16 == sx % 16 and out.data_ptr() % 16 == so % 16
    outs = []
    for _ in range(2):
        mi.call('mi355_occlude_images', mi.ptr(xd), mi.ptr(bd), N, mi.ptr(out), B, C, H, W, mi.stream_ptr())
        torch.cuda.synchronize()
        outs.append(out.cpu().clone())
    guarded.check('occlude_images %s N%d %s' % ((B, C, H, W), N, align))
    assert torch.equal(outs[0], outs[1]), 'two launches, different bits'
    assert torch.equal(xd.cpu(), torch.from_numpy(x.view(np.int32))), 'the input changed'
    return outs[0].numpy().view(np.uint32), out


@pytest.mark.parametrize('shape', [(1, 3, 16, 16), (3, 3, 48, 48), (2, 1, 16, 20)], ids=str)
@pytest.mark.parametrize('align', list(IMG_ALIGN))
def test_occlude_images_bit_for_bit(gpu, shape, align):
    mi, _ = _mi()
    B, C, H, W = shape
    x = R.random_words(shape, seed=H + W)
    for kind in ('empty', 'pixel', 'full', 'overlap', 'eight', 'wild'):
        boxes = R.image_boxes(B, H, W, kind)
        got, out = _occlude(mi, gpu, x, boxes, align)
        want = R.occlude_images(x, boxes)
        assert got.tobytes() == want.tobytes(), (kind, int((got != want).sum()))
    # every output word is written: a source with no all-ones word and one box leaves none of the fill behind
    clean = x.copy()
    clean[clean == 0xFFFFFFFF] = 1
    got, out = _occlude(mi, gpu, clean, R.image_boxes(B, H, W, 'overlap'), align)
    assert guarded.unwritten(out) == 0
    # N == 0: a copy
    got, _ = _occlude(mi, gpu, x, np.zeros((B, 0, 4), np.int32), align)
    assert got.tobytes() == x.tobytes()


def test_occlude_images_wrapper_and_more_blocks_than_one(gpu):
    mi, ops = _mi()
    x = torch.from_numpy(R.random_words((5, 3, 64, 64), seed=1).view(np.float32)).to(gpu)       # several blocks per sample
    boxes = R.image_boxes(5, 64, 64, 'eight')
    out = ops.occlude_images(x, torch.from_numpy(boxes).to(gpu))
    want = R.occlude_images(x.cpu().numpy(), boxes)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    buf = torch.empty_like(x)
    assert ops.occlude_images(x, torch.from_numpy(boxes).to(gpu), out=buf) is buf and _same(buf.cpu(), out.cpu())


# ------------------------------------------------------------------------------------------------------ refused arguments
def test_refused_arguments_name_the_argument_and_launch_nothing(gpu):
    mi, ops = _mi()
    ops.prof_enable(2)
    ops.prof_reset()
    try:
        p = torch.full((2, 3), 0.5, device=gpu)
        xy = torch.zeros(2, 3, 2, device=gpu)
        u = torch.zeros(2, 3, device=gpu)
        kw = dict(tau=0.1, prob=0.5, n=1, lo=2, hi=4, image_side=16, heatmap_size=(4, 4))
        for change, word in ((dict(n=9), 'N=9'), (dict(lo=5), 'lo=5'), (dict(lo=0), 'lo=0'), (dict(hi=17), 'hi=17'), (dict(prob=1.5), 'prob'),
                             (dict(prob=-0.5), 'prob'), (dict(tau=float('nan')), 'tau'), (dict(tau=float('inf')), 'tau'),
                             (dict(image_side=18), 'multiple'), (dict(heatmap_size=(5, 4)), 'multiple')):
            with pytest.raises(mi.Mi355Error, match=word):
                ops.teacher_select(p, xy, u if change.get('n', 1) == 1 else torch.zeros(2, 19, device=gpu), **dict(kw, **change))
        with pytest.raises(mi.Mi355Error, match='xy'):
            ops.teacher_select(p, None, u, **kw)
        with pytest.raises(mi.Mi355Error, match=' u '):
            ops.teacher_select(p, xy, torch.zeros(2, 5, device=gpu), **kw)
        with pytest.raises(mi.Mi355Error, match='gate_in'):
            ops.teacher_select(p, xy, u, gate_in=torch.zeros(2, 4, device=gpu), **kw)
        with pytest.raises(mi.Mi355Error, match='w_in'):
            ops.teacher_select(p, xy, u, w_in=torch.zeros(2, 4, device=gpu), **kw)
        with pytest.raises(mi.Mi355Error, match=' p '):
            ops.teacher_select(p.t(), xy, u, **kw)
        with pytest.raises(mi.Mi355Error, match='conf'):
            ops.teacher_select(p, xy, u, out=(torch.empty(2, 4, device=gpu), None, torch.empty(2, 1, 4, dtype=torch.int32, device=gpu),
                                              torch.empty(2, dtype=torch.int32, device=gpu)), **kw)
        x = torch.zeros(2, 3, 8, 8, device=gpu)
        b = torch.zeros(2, 1, 4, dtype=torch.int32, device=gpu)
        with pytest.raises(mi.Mi355Error, match='boxes'):
            ops.occlude_images(x, b.long())
        with pytest.raises(mi.Mi355Error, match='boxes'):
            ops.occlude_images(x, b[:1])
        with pytest.raises(mi.Mi355Error, match='N=9'):
            ops.occlude_images(x, torch.zeros(2, 9, 4, dtype=torch.int32, device=gpu))
        with pytest.raises(mi.Mi355Error, match=' x '):
            ops.occlude_images(x[:, :, :, ::2], b)
        with pytest.raises(mi.Mi355Error, match='out'):
            ops.occlude_images(x, b, out=torch.zeros(2, 3, 8, 4, device=gpu))
        with pytest.raises(mi.Mi355Error, match='overlap'):
            mi.call('mi355_occlude_images', mi.ptr(x), mi.ptr(b), 1, mi.ptr(x), 2, 3, 8, 8, mi.stream_ptr())
        for a, word in (((0, 1.0, mi.ptr(b), mi.ptr(xy), mi.ptr(p)), 'hm'), ((mi.ptr(x), 1.0, 0, mi.ptr(xy), mi.ptr(p)), 'idx'),
                        ((mi.ptr(x), 1.0, mi.ptr(b), 0, mi.ptr(p)), 'xy'), ((mi.ptr(x), 1.0, mi.ptr(b), mi.ptr(xy), 0), 'null p')):
            with pytest.raises(mi.Mi355Error, match=word):
                mi.call('mi355_peak_prob', *a, 6, 8, 8, mi.stream_ptr())
        torch.cuda.synchronize()
        assert not [e['label'] for e in ops.prof_launches() if e['label'].startswith(('peak_prob', 'teacher_select', 'occlude_images'))]
        # ... and a good call is logged: the check above looks at a list that would show a launch
        ops.teacher_select(p, xy, u, **kw)
        torch.cuda.synchronize()
        assert [e['label'] for e in ops.prof_launches() if e['label'].startswith('teacher_select')]
    finally:
        ops.prof_enable(0)
        ops.prof_reset()
