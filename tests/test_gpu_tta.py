"""Flip test and sub-pixel decode on the MI355X: mi355_mirror_batch and mi355_flip_decode (csrc/eval.hip) against tests/tta_ref.py.

As in test_gpu_eval.py / test_gpu_heatmap_rows.py: outputs sit inside sentinel-filled buffers whose guard words must survive,
every call is made twice and must give the same bits, and the inputs are read once from a 16-byte-aligned pointer and once from
one float past it.

What is compared how:
  * the mirror, the average (on integer maps, where sum and half are exact), the arg-max index, maxval and the argmax / quarter
    coordinates: bit for bit;
  * the taylor coordinates: the smoothed values are specified bit for bit (fp32, fixed order), everything after them is float64
    and can differ from numpy only through the two `log` implementations -- about 1e-13 pixels after the division by
    det >= 0.01 -- so only the final rounding to fp32 can fall on the other side: within one fp32 unit in the last place of the
    reference (np.spacing).  The check applies where the reference's |det| >= 0.01 (tta_ref.DET_MIN); at most 1 % of the cases
    may be left out for that reason (test_tta_cpu.py: with these inputs none is).  Where the step is not applied (border,
    det == 0) the coordinates are the arg-max's, exactly.  The end-to-end test cannot choose its heat-maps (a seeded random
    network's are nearly flat: |det| < 0.01 on 56 of the 59 refined maps of a split); it leaves none out and holds those to the
    reference's propagated float64 error bound (tta_ref.taylor_offsets, below 2e-9 px there) on top of the final rounding.
    Measured on an MI355X: every compared coordinate, kernel cases and end to end, is bit-identical."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_ref as E
import tta_ref as T
from conftest import PKG
from test_gpu_heatmap_rows import Slot, _place, _twice

pytestmark = pytest.mark.gpu
EINVAL = -1


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ mirror_batch
@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('shape', [(1, 3, 16, 16), (2, 3, 16, 48), (3, 1, 5, 7), (2, 3, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_mirror_batch_bits(gpu, shape, off):
    mi355, ops = _mi()
    x = np.random.default_rng([41] + list(shape)).standard_normal(shape).astype(np.float32)
    want = T.mirror_batch(x)
    xd = _place(torch.from_numpy(x), gpu, off)
    for out_off in (0, 1):
        s = Slot(want.size, gpu, off=out_off)
        b = _twice(lambda: mi355.call('mi355_mirror_batch', xd.data_ptr(), s.out.data_ptr(), *shape, mi355.stream_ptr()), [s])
        assert np.array_equal(b[0], _bits(want).reshape(-1)), (shape, off, out_off)
    y = ops.mirror_batch(xd)
    assert tuple(y.shape) == (2 * shape[0],) + shape[1:] and y.dtype == torch.float32 and np.array_equal(_bits(y.cpu().numpy()), _bits(want))


# ------------------------------------------------------------------------------------------------------------------ flip_decode
@functools.lru_cache(maxsize=None)
def taps_on(sigma, dev):
    g, r = T.gaussian_taps(sigma)
    return torch.from_numpy(g).to(dev), r


def run_flip_decode(hm, hf, shift, mode, scale, dev, off, want_avg, sigma=2.0):
    """mi355_flip_decode on (rows, h, w) maps placed `off` floats past a 16-byte boundary (avg_out likewise): (idx, xy, maxval,
    avg or None) as numpy after the twice-the-same-bits and guard-word checks."""
    mi355, _ = _mi()
    rows, h, w = hm.shape
    d_hm = _place(torch.from_numpy(np.ascontiguousarray(hm)), dev, off)
    d_hf = _place(torch.from_numpy(np.ascontiguousarray(hf)), dev, off) if hf is not None else None
    s_idx, s_xy, s_mv, s_avg = Slot(rows, dev, torch.int32), Slot(2 * rows, dev), Slot(rows, dev), Slot(rows * h * w, dev, off=off)
    taps, r = taps_on(sigma, dev) if mode == 2 else (None, 0)
    fn = lambda: mi355.call('mi355_flip_decode', d_hm.data_ptr(), mi355.ptr(d_hf), shift, s_avg.out.data_ptr() if want_avg else 0, mode,
                            mi355.ptr(taps), r, float(scale[0]), float(scale[1]), s_idx.out.data_ptr(), s_xy.out.data_ptr(),
                            s_mv.out.data_ptr(), rows, h, w, mi355.stream_ptr())
    b = _twice(fn, [s_idx, s_xy, s_mv] + ([s_avg] if want_avg else []))
    if not want_avg:
        assert s_avg.untouched()
    return b[0].copy(), b[1].view(np.float32).reshape(rows, 2).copy(), b[2].view(np.float32).copy(), (b[3].view(np.float32).reshape(hm.shape) if want_avg else None)


CASES = [(1, 1, 1), (3, 5, 7), (21, 8, 8), (42, 16, 16), (42, 64, 64), (2, 128, 128), (1, 130, 130)]


@functools.lru_cache(maxsize=None)
def exact_inputs(case):
    rows, h, w = case
    return E.integer_maps(rows, h, w, seed=[1711, rows, h, w]), E.integer_maps(rows, h, w, seed=[1712, rows, h, w])


@functools.lru_cache(maxsize=None)
def exact_reference(case, flip, mode, scale):
    hm, hf = exact_inputs(case)
    return T.flip_decode(hm, None if flip is None else hf, flip or 0, ('argmax', 'quarter')[mode], scale=scale)


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d' % c)
def test_average_argmax_quarter_bit_exact(gpu, case, off):
    """Integer maps in [-512, 512]: hm + f and its half are exact, so the average has one value whatever the evaluation."""
    rows, h, w = case
    hm, hf = exact_inputs(case)
    n = 0
    for flip in (None, 0, 1):
        for scale in ((4., 4.), (3., 2.)):
            for mode in (0, 1):
                want_avg = bool((n := n + 1) % 2) or (flip is not None and scale[0] == 4. and mode == 0)
                ridx, rxy, rmv, _, rm = exact_reference(case, flip, mode, scale)
                idx, xy, mv, avg = run_flip_decode(hm, None if flip is None else hf, flip or 0, mode, scale, gpu, off, want_avg)
                tag = (case, flip, scale, mode)
                assert np.array_equal(idx, ridx), tag
                assert np.array_equal(_bits(mv), _bits(rmv)) and np.array_equal(_bits(xy), _bits(rxy)), tag
                if want_avg:
                    assert np.array_equal(_bits(avg), _bits(rm)), tag
    # without hm_flip, mode 0, scale 1: mi355_argmax2d's bits
    _, ops = _mi()
    idx, xy, mv, _ = run_flip_decode(hm, None, 0, 0, (1., 1.), gpu, off, False)
    aidx, axy, amv = ops.argmax2d(_place(torch.from_numpy(hm), gpu, off).view(1, rows, h, w))
    assert np.array_equal(aidx.cpu().numpy().reshape(-1), idx)
    assert np.array_equal(_bits(axy.cpu().numpy().reshape(rows, 2)), _bits(xy)) and np.array_equal(_bits(amv.cpu().numpy().reshape(-1)), _bits(mv))


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
def test_special_maps_every_mode(gpu, off):
    for name, maps in E.special_maps().items():
        for mode, mname in enumerate(('argmax', 'quarter', 'taylor')):
            ridx, rxy, rmv, det = T.decode(maps, mname, scale=(4., 4.))
            idx, xy, mv, _ = run_flip_decode(maps, None, 0, mode, (4., 4.), gpu, off, False)
            assert np.array_equal(idx, ridx), (name, mname)
            if name == 'nan':                          # NaN counts as the maximum; its payload is not compared
                assert np.isnan(mv).all() and np.isnan(rmv).all() and not xy.any()
                assert np.array_equal(idx, [int(np.flatnonzero(np.isnan(m.reshape(-1)))[0]) for m in maps])
            else:
                assert np.array_equal(_bits(mv), _bits(rmv)), (name, mname)
            if name in ('negative', 'zero'):
                assert not xy.any() and np.array_equal(mv, maps.reshape(len(maps), -1).max(1))
            if name == 'corners_edges':                # every maximum on the border: quarter moves along the edge only, taylor nothing
                assert (mv == 512).all() and (mode < 2 or np.isnan(det).all())
            assert np.array_equal(_bits(xy), _bits(rxy)), (name, mname)


def _ulps(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


def check_taylor(tag, xy, rxy, det, det_min=T.DET_MIN):
    """The comparison of the module docstring; returns (cases checked to one ulp, cases left out for a small determinant)."""
    applied = np.isfinite(det) & (det != 0)
    exact = ~applied
    assert np.array_equal(_bits(xy[exact]), _bits(rxy[exact])), '%s: the arg-max coordinates where the taylor step does not apply' % tag
    ok = applied & (np.abs(det) >= det_min)
    u = _ulps(xy[ok], rxy[ok]) if ok.any() else np.zeros((0, 2))
    print('MEASURE flip_decode taylor %s: %d cases, %.2f %% of the coordinates not bit-identical, largest deviation %.2f ulp, %d left out for |det| < %g'
          % (tag, int(ok.sum()), 100.0 * float((u != 0).mean()) if u.size else 0.0, float(u.max()) if u.size else 0.0, int((applied & ~ok).sum()), det_min))
    assert (u <= 1.0).all(), '%s: %s ulp' % (tag, u.max())
    return int(ok.sum()), int((applied & ~ok).sum())


@functools.lru_cache(maxsize=None)
def taylor_reference(name, scale):
    return T.decode(T.taylor_cases()[name], 'taylor', 2.0, scale)


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('name', ['clean', 'noisy', 'normal', 'map64k', 'beyond_lds'])
def test_taylor_within_one_ulp(gpu, name, off):
    maps = T.taylor_cases()[name]
    checked = left_out = 0
    for scale in ((4., 4.), (1., 1.)):                 # powers of two: the scaling itself rounds nothing
        ridx, rxy, rmv, det = taylor_reference(name, scale)
        for flip in (None, 0):                         # hm_flip = the mirror image of hm, unshifted: the average is hm again, exactly
            hf = None if flip is None else np.ascontiguousarray(maps[..., ::-1])
            idx, xy, mv, avg = run_flip_decode(maps, hf, 0, 2, scale, gpu, off, flip is not None)
            assert np.array_equal(idx, ridx) and np.array_equal(_bits(mv), _bits(rmv))
            if avg is not None:
                assert np.array_equal(_bits(avg), _bits(maps))
            a, b = check_taylor('%s scale %g flip %s off %d' % (name, scale[0], flip, off), xy, rxy, det)
            checked, left_out = checked + a, left_out + b
    assert checked > 0 and left_out <= 0.01 * (checked + left_out)


def test_taylor_adds_nothing_at_borders_and_below_the_clamp(gpu):
    maps, spots = T.border_maps()
    ridx, rxy, rmv, det = T.decode(maps, 'taylor', 2.0, (4., 4.))
    idx, xy, mv, _ = run_flip_decode(maps, None, 0, 2, (4., 4.), gpu, 0, False)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(mv), _bits(rmv))
    outside = np.array([not (2 <= x <= maps.shape[2] - 3 and 2 <= y <= maps.shape[1] - 3) for x, y in spots])
    assert outside.sum() == 12 and np.array_equal(xy[outside], np.float32(spots)[outside] * 4) and np.isnan(det[outside]).all()
    check_taylor('borders', xy, rxy, det)
    faint = T.faint_maps()
    idx, xy, mv, _ = run_flip_decode(faint, None, 0, 2, (1., 1.), gpu, 0, False)
    assert xy.tolist() == [[20, 13], [2, 37]] and (mv > 0).all()
    # other sigmas: radius 3 and the largest one, 16.  Label and smoothing of sigma 6.4 add up to a variance of 82, det = 1 / 82^2 =
    # 1.5e-4 by construction; the one-ulp argument still holds there: the smoothed values lie in (0.1, 1], so each log is off by
    # at most an ulp of 3 (4.4e-16), the differences by a few of those, and the division by second derivatives of 1 / 82 leaves
    # under 1e-12 pixels against an fp32 spacing of 2e-6 at these coordinates
    for sigma, det_min in ((1.0, T.DET_MIN), (6.4, 1e-4)):
        g, _ = T.gaussians(6, sigma=sigma, seed=11, lo=20.0, hi=43.0)
        ridx, rxy, rmv, det = T.decode(g, 'taylor', sigma, (4., 4.))
        idx, xy, mv, _ = run_flip_decode(g, None, 0, 2, (4., 4.), gpu, 1, False, sigma=sigma)
        assert np.array_equal(idx, ridx) and (np.abs(det) >= det_min).all()
        assert check_taylor('sigma %g' % sigma, xy, rxy, det, det_min) == (6, 0)


def test_python_surface(gpu):
    """ops.flip_decode / decode_keypoints on (B,K,h,w) tensors."""
    from utils.keypoint_detection import decode_keypoints
    mi355, ops = _mi()
    hm, hf = exact_inputs((42, 16, 16))
    d_hm, d_hf = torch.from_numpy(hm).view(2, 21, 16, 16).to(gpu), torch.from_numpy(hf).view(2, 21, 16, 16).to(gpu)
    for mode in ('argmax', 'quarter', 'taylor'):
        ridx, rxy, rmv, det, rm = T.flip_decode(hm, hf, 1, mode, 2.0, (4., 4.))
        idx, xy, mv, avg = ops.flip_decode(d_hm, d_hf, 1, mode, 2.0, (4., 4.), want_avg=True)
        assert tuple(idx.shape) == (2, 21) and tuple(xy.shape) == (2, 21, 2) and tuple(mv.shape) == (2, 21, 1) and idx.dtype == torch.int32
        assert np.array_equal(idx.cpu().numpy().reshape(-1), ridx) and np.array_equal(avg.cpu().numpy().reshape(hm.shape), rm)
        if mode != 'taylor':
            assert np.array_equal(xy.cpu().numpy().reshape(-1, 2), rxy)
        kp, kmv, kavg = decode_keypoints(d_hm, 64, mode, with_maxval=True, y_flip=d_hf, return_avg=True)
        assert torch.equal(kp, xy) and torch.equal(kmv, mv) and torch.equal(kavg, avg)
        assert torch.equal(decode_keypoints(d_hm, 64, mode, y_flip=d_hf), xy)
        assert ops.flip_decode(d_hm, d_hf, 1, mode, 2.0, (4., 4.))[3] is None
    up = decode_keypoints(d_hm, 64, 'upsample', y_flip=d_hf, flip_shift=0)
    want = E.first_argmax(E.upsample_kernel_order(T.working_map(hm, hf, 0), (64, 64)))[1]
    assert np.array_equal(up.cpu().numpy().reshape(-1, 2), want)
    plain = decode_keypoints(d_hm, 64, 'argmax', with_maxval=True, return_avg=True)
    assert len(plain) == 3 and plain[2].data_ptr() == d_hm.data_ptr() and torch.equal(plain[0], ops.argmax2d(d_hm)[1] * 4)
    for bad in (dict(mode='soft'), dict(shift=2), dict(hm_flip=d_hf[:1]), dict(mode='taylor', sigma=7.0)):
        with pytest.raises(mi355.Mi355Error):
            ops.flip_decode(d_hm, **bad)
    with pytest.raises(mi355.Mi355Error):
        ops.mirror_batch(d_hm[0])


# ------------------------------------------------------------------------------------------------------------------ validation
def test_argument_validation_names_the_argument(gpu):
    """Every refusal returns before any launch (the outputs keep their sentinels)."""
    mi355, _ = _mi()
    lib = mi355.load()
    hm = torch.zeros(64, device=gpu)
    taps, r = taps_on(2.0, gpu)
    outs = [Slot(4, gpu, torch.int32), Slot(8, gpu), Slot(4, gpu), Slot(64, gpu)]
    good = dict(hm=hm.data_ptr(), hm_flip=hm.data_ptr(), shift=1, avg_out=outs[3].out.data_ptr(), mode=2, taps=taps.data_ptr(), radius=r,
                scale_x=1.0, scale_y=1.0, idx=outs[0].out.data_ptr(), xy=outs[1].out.data_ptr(), maxval=outs[2].out.data_ptr(), rows=4, h=4,
                w=4, stream=mi355.stream_ptr())
    bad = [(dict(hm=0), 'hm'), (dict(rows=0), 'rows=0'), (dict(h=0), 'h=0'), (dict(w=-1), 'w=-1'), (dict(rows=1, h=65536, w=65536), 'beyond 32-bit'),
           (dict(hm=hm.data_ptr() + 2), 'aligned'), (dict(xy=good['xy'] + 1), 'aligned'), (dict(hm_flip=good['hm_flip'] + 2), 'aligned'),
           (dict(mode=3), 'mode=3'), (dict(mode=-1), 'mode=-1'), (dict(taps=0), 'taps'), (dict(radius=0), 'radius=0'), (dict(radius=17), 'radius=17'),
           (dict(shift=2), 'shift=2'), (dict(shift=-1), 'shift=-1')]
    for change, word in bad:
        rc = lib.mi355_flip_decode(*dict(good, **change).values())
        assert rc == EINVAL and word in lib.mi355_last_error().decode() and 'flip_decode' in lib.mi355_last_error().decode(), (change, lib.mi355_last_error())
    x = torch.zeros(2 * 3 * 4 * 4, device=gpu)
    big = Slot(2 * 2 * 3 * 4 * 4, gpu)
    goodm = dict(x=x.data_ptr(), out=big.out.data_ptr(), B=2, C=3, H=4, W=4, stream=mi355.stream_ptr())
    for change, word in [(dict(x=0), 'null'), (dict(out=0), 'null'), (dict(B=0), 'B=0'), (dict(C=0), 'C=0'), (dict(H=0), 'H=0'), (dict(W=0), 'W=0'),
                         (dict(x=x.data_ptr() + 1), 'aligned'), (dict(out=goodm['out'] + 2), 'aligned')]:
        rc = lib.mi355_mirror_batch(*dict(goodm, **change).values())
        assert rc == EINVAL and word in lib.mi355_last_error().decode() and 'mirror_batch' in lib.mi355_last_error().decode(), (change, lib.mi355_last_error())
    torch.cuda.synchronize()
    assert all(s.untouched() for s in outs + [big])
    # taps and radius are not looked at in modes 0 and 1
    assert lib.mi355_flip_decode(*dict(good, mode=1, taps=0, radius=99).values()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ end to end
from test_gpu_eval import B, COMMON, HM, IMG, LINE, THR, _model, _recompute          # noqa: E402  (the set-up of its `runs` fixture)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """test.py on one seeded checkpoint: default flags, --metrics pck, and --flip-test with the taylor and the upsample decode."""
    from seeded import fill_module_
    tmp = tmp_path_factory.mktemp('tta')
    m = _model()
    fill_module_(m, 11)
    ck = str(tmp / 'ck.pth')
    torch.save({'model': m.state_dict(), 'epoch': 0}, ck)
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(tag, extra):
        r = subprocess.run([sys.executable, os.path.join(PKG, 'test.py')] + COMMON + ['--checkpoint', ck, '--log', str(tmp / ('log_' + tag))] + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    out = {'ck': ck, 'tmp': tmp}
    out['default'] = run('default', [])
    out['pck'] = run('pck', ['--metrics', 'pck'])
    out['taylor'] = run('taylor', ['--metrics', 'full', '--flip-test', '--decode', 'taylor', '--dump-preds', str(tmp / 'taylor')])
    out['up'] = run('up', ['--metrics', 'full', '--flip-test', '--decode', 'upsample', '--dump-preds', str(tmp / 'up')])
    return out


@functools.lru_cache(maxsize=None)
def _two_forwards(ck, seed):
    """(y, y_flip, images): the heat-maps of two plain forwards of the checkpoint over the synthetic test split `seed` -- the
    images, and the second half of mirror_batch -- in test.py's batches."""
    import mi355
    from mi355 import ops
    from mi355.infer import GraphedForward
    from utils.synthetic_dataset import SyntheticHand21
    dev = torch.device('cuda:0')
    saved = (mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs)
    mi355.set_compute_dtype('bf16')
    try:
        m = _model().to(dev)
        m.load_state_dict(torch.load(ck, map_location='cpu', weights_only=False)['model'])
        m.eval()
        f1, f2, ds, ys, yfs, xs = GraphedForward(m), GraphedForward(m), SyntheticHand21(4 * B, (IMG, IMG), (HM, HM), seed=seed), [], [], []
        with torch.no_grad():
            for i in range(0, len(ds), B):
                x = torch.stack([ds[j][0] for j in range(i, i + B)]).to(dev)
                xs.append(x.cpu())
                ys.append(f1(x).float().cpu())
                yfs.append(f2(ops.mirror_batch(x)[B:]).float().cpu())
        return torch.cat(ys).numpy(), torch.cat(yfs).numpy(), torch.cat(xs), float(ds.sigma)
    finally:
        mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs = saved


def _check_dump(d, out, split, decode):
    assert d['pred'].shape == (4 * B, 21, 2) and d['maxval'].shape == (4 * B, 21)
    assert int(d['image_size']) == IMG and str(d['decode']) == decode and np.array_equal(d['thresholds'], THR)
    assert bool(d['flip_test']) is True and int(d['flip_shift']) == 1
    epe, auc, curve = _recompute(d)
    assert abs(float(d['epe']) - epe) <= 1e-12 * epe and abs(float(d['auc']) - auc) <= 1e-12 and np.allclose(d['pck_curve'], curve, rtol=0, atol=1e-15)
    printed = LINE.findall(out)
    assert len(printed) == 2, out[-2000:]
    assert printed[0 if split == 'source' else 1] == ('%.3f' % epe, '%.4f' % auc)


@pytest.mark.parametrize('split,seed', [('source', 12), ('target', 14)])
def test_flip_test_taylor_dump_matches_print_and_reference(gpu, runs, split, seed):
    d = np.load(str(runs['tmp'] / ('taylor.%s.npz' % split)))
    _check_dump(d, runs['taylor'], split, 'taylor')
    y, yf, _, sigma = _two_forwards(runs['ck'], seed)
    ridx, rxy, rmv, det, bound, _ = T.flip_decode(y.reshape(-1, HM, HM), yf.reshape(-1, HM, HM), 1, 'taylor', sigma, (IMG / HM, IMG / HM), with_bound=True)
    bad = np.flatnonzero(_bits(d['maxval'].reshape(-1)) != _bits(rmv))
    assert not len(bad), '%d of %d maxima differ from the reference average of two plain forwards, first %s' % (len(bad), len(rmv), bad[:4])
    # Heat-maps of a seeded random network are nearly flat: most determinants are far below 0.01 (the MEASURE line counts them),
    # where the division amplifies the difference between two float64 logarithms.  Those cases are not left out: they are
    # held to the reference's own propagated bound (tta_ref.taylor_offsets) on top of the final fp32 rounding; the cases with
    # |det| >= 0.01 to one ulp as everywhere.
    pred = d['pred'].reshape(-1, 2)
    check_taylor('test.py %s' % split, pred, rxy, det)
    small = np.isfinite(det) & (det != 0) & (np.abs(det) < T.DET_MIN)
    tol = np.spacing(np.abs(rxy)).astype(np.float64) + (IMG / HM) * bound
    dev = np.abs(pred.astype(np.float64) - rxy.astype(np.float64))
    print('MEASURE test.py %s, %d cases with |det| < %g: largest propagated bound %.3g px, largest deviation %.3g px, %.2f %% of the coordinates not bit-identical'
          % (split, int(small.sum()), T.DET_MIN, float((IMG / HM) * bound[small].max()) if small.any() else 0.0,
             float(dev[small].max()) if small.any() else 0.0, 100.0 * float((dev[small] != 0).mean()) if small.any() else 0.0))
    assert (dev[small] <= tol[small]).all()


def test_pose_predictor_returns_what_test_py_dumps(gpu, runs):
    import mi355
    from mi355.infer import PosePredictor
    d = np.load(str(runs['tmp'] / 'taylor.source.npz'))
    x = _two_forwards(runs['ck'], 12)[2]
    saved = (mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs)
    mi355.set_compute_dtype('bf16')
    try:
        m = _model().to(gpu)
        m.load_state_dict(torch.load(runs['ck'], map_location='cpu', weights_only=False)['model'])
        predict = PosePredictor(m, IMG, decode='taylor', flip_test=True, flip_shift=1, sigma=2.0)
        got = [predict(x[i:i + B].to(gpu)) for i in range(0, len(x), B)]
        assert not m.training
    finally:
        mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs = saved
    xy, mv = torch.cat([g[0] for g in got]).cpu().numpy(), torch.cat([g[1] for g in got]).cpu().numpy()
    assert xy.shape == (4 * B, 21, 2) and mv.shape == (4 * B, 21, 1)
    assert np.array_equal(_bits(xy), _bits(d['pred'])) and np.array_equal(_bits(mv.reshape(4 * B, 21)), _bits(d['maxval']))


@pytest.mark.parametrize('split,seed', [('source', 12), ('target', 14)])
def test_flip_test_upsample_decodes_the_reference_average(gpu, runs, split, seed):
    d = np.load(str(runs['tmp'] / ('up.%s.npz' % split)))
    _check_dump(d, runs['up'], split, 'upsample')
    y, yf, _, _ = _two_forwards(runs['ck'], seed)
    avg = T.working_map(y.reshape(-1, HM, HM), yf.reshape(-1, HM, HM), 1)
    ridx, rxy, rmv = E.first_argmax(E.upsample_kernel_order(avg, (IMG, IMG)))
    assert np.array_equal(d['pred'].reshape(-1, 2), rxy) and np.array_equal(_bits(d['maxval'].reshape(-1)), _bits(rmv))


def test_default_flags_print_what_metrics_pck_prints(gpu, runs):
    keep = lambda out: [l for l in out.splitlines() if l.startswith(('Source:', 'MCP:', 'PIP:', 'DIP:', 'fingertip:', 'all:', 'loaded checkpoint'))]
    assert 'EPE' not in runs['default'] and 'EPE' not in runs['pck'] and len(keep(runs['default'])) == 7
    assert keep(runs['default']) == keep(runs['pck'])
    assert 'flip_test=False' in runs['default'] and keep(runs['taylor']) == keep(runs['up']) and len(keep(runs['taylor'])) == 7
