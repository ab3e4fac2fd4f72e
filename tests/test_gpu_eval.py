"""Image-resolution evaluation on the MI355X: mi355_upsample_argmax (csrc/eval.hip) bit for bit against tests/eval_ref.py where
the up-sampling is exact (integer maps, power-of-two ratios: test_eval_cpu.py asserts fp32 == float64 for every such case, so
the first-index arg-max is uniquely defined), against a float64 up-sampling within a worked-out bound where it is not;
mi355_pose_metrics bit for bit against the sequential float64 loop; and test.py end to end.

As in test_gpu_heatmap_rows.py: outputs sit inside sentinel-filled buffers whose guard words must survive, every call is made
twice and must give the same bits, and the input is read once from a 16-byte-aligned pointer and once from `buf[1:1 + n]`.

Inexact bound (M = max|in| of the map; every weight pair is in [0, 1] and sums to 1 to rounding).  In
v = hy * (hx * a + lx * b) + ly * (hx * c + lx * d) each of the 7 operations rounds by at most half an ulp of a value no larger
than M, i.e. 2^-24 * M, and the errors of the inner operations reach v scaled by the weights outside them: 3 * 2^-24 * M * (hy +
ly) from the two rows plus 2^-24 * M of the last sum, 4 * 2^-24 * M per output.  So maxval is within 4 * 2^-24 * M of the float64
value at the returned index, and -- the kernel's winner being at least the kernel's value of the true maximum -- the float64
value at the returned index within 8 * 2^-24 * M of the float64 maximum.  On the two ratios used, the arg-max outputs sit where
the fp32 weights are exact (64 -> 256: multiples of 1/8) or at a pixel centre (16 -> 48), so the weights' own rounding does not
enter."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_ref as E
from conftest import PKG
from test_gpu_heatmap_rows import Slot, _place, _twice

pytestmark = pytest.mark.gpu
EPS24 = 2.0 ** -24


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run_upsample(maps, H, W, dev, off):
    """mi355_upsample_argmax on (rows, h, w) fp32 maps placed `off` floats past a 16-byte boundary: (idx, xy, maxval) as numpy,
    after the twice-the-same-bits and guard-word checks."""
    mi355, _ = _mi()
    rows, h, w = maps.shape
    hm = _place(torch.from_numpy(np.ascontiguousarray(maps)), dev, off)
    s_idx, s_xy, s_mv = Slot(rows, dev, torch.int32), Slot(2 * rows, dev), Slot(rows, dev)
    fn = lambda: mi355.call('mi355_upsample_argmax', hm.data_ptr(), s_idx.out.data_ptr(), s_xy.out.data_ptr(), s_mv.out.data_ptr(),
                            rows, h, w, H, W, mi355.stream_ptr())
    b = _twice(fn, [s_idx, s_xy, s_mv])
    return b[0].copy(), b[1].view(np.float32).reshape(rows, 2).copy(), b[2].view(np.float32).copy()


@functools.lru_cache(maxsize=None)
def exact_reference(case):
    return E.upsample_argmax(E.exact_case_maps(case), case[3:])


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('case', E.EXACT_CASES, ids=lambda c: '%dx%dx%d_to_%dx%d' % c)
def test_upsample_argmax_bit_exact(gpu, case, off):
    rows, h, w, H, W = case
    maps = E.exact_case_maps(case)
    ridx, rxy, rmv = exact_reference(case)
    idx, xy, mv = run_upsample(maps, H, W, gpu, off)
    bad = np.nonzero(idx != ridx)[0]
    assert not len(bad), 'rows %s: idx %s, reference %s' % (bad[:4], idx[bad[:4]], ridx[bad[:4]])
    assert np.array_equal(_bits(xy), _bits(rxy)) and np.array_equal(_bits(mv), _bits(rmv))
    if (h, w) == (H, W):                               # the maps at their own size: mi355_argmax2d's bits
        _, ops = _mi()
        hm = _place(torch.from_numpy(maps), gpu, off).view(1, rows, h, w)
        aidx, axy, amv = ops.argmax2d(hm)
        assert np.array_equal(aidx.cpu().numpy().reshape(-1), idx)
        assert np.array_equal(_bits(axy.cpu().numpy().reshape(rows, 2)), _bits(xy)) and np.array_equal(_bits(amv.cpu().numpy().reshape(-1)), _bits(mv))


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
def test_upsample_argmax_special_maps(gpu, off):
    for name, maps in E.special_maps().items():
        for size in ((64, 64), (32, 128)):
            up = E.upsample(maps, size)
            ridx, rxy, rmv = E.first_argmax(up)
            idx, xy, mv = run_upsample(maps, size[0], size[1], gpu, off)
            assert np.array_equal(idx, ridx), (name, size)
            assert np.array_equal(_bits(xy), _bits(rxy)), (name, size)
            if name == 'nan':                          # the first NaN-contaminated output; its payload is not compared
                assert np.isnan(mv).all() and np.isnan(rmv).all() and not xy.any()
                first = np.array([int(np.flatnonzero(np.isnan(u.reshape(-1)))[0]) for u in up.numpy()])
                assert np.array_equal(idx, first)
            else:
                assert np.array_equal(_bits(mv), _bits(rmv)), (name, size)
            if name == 'negative':                     # xy zeroed, maxval the true maximum
                assert not xy.any() and np.array_equal(mv, up.reshape(len(maps), -1).max(1).values.numpy()) and (mv < 0).all()
            if name == 'zero':
                assert not xy.any() and not idx.any() and np.array_equal(_bits(mv), np.zeros(len(maps), np.int32))
            if name == 'corners_edges':
                # a corner pixel is replicated to the border outputs (first of them wins); between two pixel centres of an edge
                # no output of these grids sits on the centre, so the maximum there is an interpolated value
                assert (mv[:4] == 512.0).all() and (mv[4:] < 512.0).all() and idx[0] == 0


# ------------------------------------------------------------------------------------------------------------------ inexact cases
@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('case', [(8, 64, 64, 256, 256), (21, 16, 16, 48, 48)], ids=['64to256', '16to48'])
def test_upsample_argmax_random_maps_within_bound(gpu, case, off):
    rows, h, w, H, W = case
    maps = np.random.default_rng([9, h, H]).standard_normal((rows, h, w)).astype(np.float32)
    up64 = E.upsample(maps, (H, W), torch.float64).numpy().reshape(rows, -1)
    idx, xy, mv = run_upsample(maps, H, W, gpu, off)
    assert ((idx >= 0) & (idx < H * W)).all()
    amax = np.abs(maps).reshape(rows, -1).max(1).astype(np.float64)
    at = up64[np.arange(rows), idx]
    gap, dv = up64.max(1) - at, np.abs(mv.astype(np.float64) - at)
    print('MEASURE upsample_argmax %dx%d>%dx%d off=%d: max (f64 max - f64 at idx) / (2^-24 max|in|) = %.3f, max |maxval - f64 at idx| / (2^-24 max|in|) = %.3f'
          % (h, w, H, W, off, (gap / (EPS24 * amax)).max(), (dv / (EPS24 * amax)).max()))
    assert (gap <= 8 * EPS24 * amax).all()
    assert (dv <= 4 * EPS24 * amax).all()
    pos = mv > 0
    assert np.array_equal(xy[:, 0], np.where(pos, idx % W, 0)) and np.array_equal(xy[:, 1], np.where(pos, idx // W, 0))


# ------------------------------------------------------------------------------------------------------------------ memory
def test_upsample_argmax_allocates_no_intermediate(gpu):
    _, ops = _mi()
    hm = torch.randn(64, 21, 64, 64, device=gpu)
    ops.upsample_argmax(hm[:1], 256)                   # (first use of anything lazy is not the call measured)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    idx, xy, mv = ops.upsample_argmax(hm, 256)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < (1 << 20), grown                    # outputs: 21.5 KB; the up-sampled maps would be 352 MB
    assert tuple(idx.shape) == (64, 21) and tuple(xy.shape) == (64, 21, 2) and tuple(mv.shape) == (64, 21, 1)
    assert idx.dtype == torch.int32 and xy.dtype == torch.float32


def test_python_surface_decode(gpu):
    """ops.upsample_argmax / compute_uv_from_heatmaps2 / decode_keypoints on a (B,K,h,w) tensor."""
    from utils.keypoint_detection import compute_uv_from_heatmaps2, decode_keypoints, get_max_preds_device
    mi355, ops = _mi()
    case = (42, 16, 16, 64, 64)
    maps = E.exact_case_maps(case)
    ridx, rxy, rmv = exact_reference(case)
    hm = torch.from_numpy(maps).view(2, 21, 16, 16).to(gpu)
    idx, xy, mv = ops.upsample_argmax(hm, 64)
    assert np.array_equal(idx.cpu().numpy().reshape(-1), ridx) and np.array_equal(xy.cpu().numpy().reshape(-1, 2), rxy)
    uv = compute_uv_from_heatmaps2(hm, (64, 64))
    assert uv.is_cuda and uv.dtype == torch.float32 and tuple(uv.shape) == (2, 21, 2) and torch.equal(uv, xy)
    assert torch.equal(decode_keypoints(hm, 64, 'upsample'), xy)
    assert torch.equal(decode_keypoints(hm, 64, 'argmax'), get_max_preds_device(hm)[0] * 4)
    with pytest.raises(ValueError):
        decode_keypoints(hm, 64, 'soft')
    with pytest.raises(mi355.Mi355Error):              # an output buffer too small for the launch
        ops.upsample_argmax(hm, 64, out=(idx.reshape(-1)[:41], xy, mv))


# ------------------------------------------------------------------------------------------------------------------ pose_metrics
def run_metrics(batches, thr, dev, K):
    """Accumulate `batches` of (pred, gt, vis) numpy arrays through ops.pose_metrics into guarded accumulators; twice."""
    _, ops = _mi()
    T = len(thr)
    s_sum, s_cnt, s_hit = Slot(2 * K, dev, torch.int32), Slot(K, dev, torch.int32), Slot(K * T, dev, torch.int32)
    state = (s_sum.out.view(torch.float64), s_cnt.out, s_hit.out.view(K, T))
    thr_d = torch.from_numpy(thr).to(dev)
    dev_b = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in b) for b in batches]

    def fn():
        for t in state:
            t.zero_()
        for p, g, v in dev_b:
            ops.pose_metrics(p, g, v, thr_d, state)

    b = _twice(fn, [s_sum, s_cnt, s_hit])
    return b[0].view(np.float64).copy(), b[1].copy(), b[2].reshape(K, T).copy()


def _points(B, K, seed):
    rng = np.random.default_rng([31, B, K, seed])
    gt = rng.uniform(8, 248, (B, K, 2)).astype(np.float32)
    pred = (gt + rng.normal(0, 12, (B, K, 2))).astype(np.float32)
    vis = (rng.uniform(size=(B, K)) > 0.25).astype(np.float32)
    return pred, gt, vis


def _same(got, ref):
    assert got[0].tobytes() == ref[0].tobytes(), 'sum_err: %s vs %s' % (got[0], ref[0])
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


THR = np.linspace(0, 30, 31).astype(np.float32)


@pytest.mark.parametrize('B,K', [(1, 1), (5, 21), (64, 21), (3, 17)])
def test_pose_metrics_shapes(gpu, B, K):
    pred, gt, vis = _points(B, K, 0)
    ref = E.accumulate(pred, gt, vis, THR, E.metrics_state(K, len(THR)))
    _same(run_metrics([(pred, gt, vis)], THR, gpu, K), ref)
    _same(run_metrics([(pred, gt, vis.reshape(B, K, 1))], THR[:1], gpu, K), E.accumulate(pred, gt, vis, THR[:1], E.metrics_state(K, 1)))


def test_pose_metrics_threshold_is_strict(gpu):
    pred, gt, vis = np.array([[[3.0, 4.0]]], np.float32), np.zeros((1, 1, 2), np.float32), np.ones((1, 1), np.float32)
    thr = np.array([5.0, np.nextafter(np.float32(5.0), np.float32(6.0)), 4.0], np.float32)
    s, c, h = run_metrics([(pred, gt, vis)], thr, gpu, 1)
    assert s[0] == 5.0 and c[0] == 1 and h.tolist() == [[0, 1, 0]]


def test_pose_metrics_invisible_rows_do_not_contaminate(gpu):
    pred, gt, vis = _points(6, 21, 1)
    vis[2] = 0; vis[4, ::2] = 0
    pred[2] = np.nan; pred[4, ::2] = np.nan; gt[2, 3] = np.inf
    ref = E.accumulate(pred, gt, vis, THR, E.metrics_state(21, len(THR)))
    got = run_metrics([(pred, gt, vis)], THR, gpu, 21)
    assert np.isfinite(got[0]).all()
    _same(got, ref)
    none = run_metrics([(pred, gt, np.zeros_like(vis))], THR, gpu, 21)
    assert not none[0].any() and not none[1].any() and not none[2].any()


def test_pose_metrics_batching_gives_the_same_bits(gpu):
    parts = [_points(B, 21, 2) for B in (1, 5, 64)]
    whole = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    assert whole[0].shape == (70, 21, 2)
    one = run_metrics([whole], THR, gpu, 21)
    many = run_metrics(parts, THR, gpu, 21)
    _same(many, one)
    _same(one, E.accumulate(whole[0], whole[1], whole[2], THR, E.metrics_state(21, len(THR))))


def test_pose_metrics_class_on_device(gpu):
    from utils.keypoint_detection import PoseMetrics
    from utils.synthetic_dataset import HAND_GROUPS
    m = PoseMetrics(21, 30.0, device=gpu)
    parts = [_points(B, 21, 3) for B in (4, 2)]
    ref = E.metrics_state(21, 31)
    for p, g, v in parts:
        m.update(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu), torch.from_numpy(v).to(gpu).view(-1, 21, 1))
        E.accumulate(p, g, v, THR, ref)
    want, got = E.summary(ref, THR, 30.0, HAND_GROUPS), m.result(HAND_GROUPS)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    empty = PoseMetrics(21, device=gpu).result({'all': range(21)})
    assert np.isnan(empty['epe']) and np.isnan(empty['auc']) and np.isnan(empty['epe_all'])


# ------------------------------------------------------------------------------------------------------------------ end to end
B, IMG, HM = 2, 64, 16
COMMON = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', str(B), '-j', '0', '-p', '100',
          '--image-size', str(IMG), '--heatmap-size', str(HM)]
LINE = re.compile(r'^EPE: ([0-9.naN]+) px  AUC\(0-30px\): ([0-9.naN]+)$', re.M)


def _model():
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    bb = models.resnet18(pretrained=False)
    return PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """test.py on one seeded checkpoint: default flags, --metrics full with either decode (with dumps), and two ranks."""
    from seeded import fill_module_
    tmp = tmp_path_factory.mktemp('eval')
    m = _model()
    fill_module_(m, 11)
    ck = str(tmp / 'ck.pth')
    torch.save({'model': m.state_dict(), 'epoch': 0}, ck)
    env = dict(os.environ, PYTHONPATH=PKG, MI355_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')

    def run(tag, extra, ranks=1):
        cmd = [sys.executable, os.path.join(PKG, 'test.py')]
        if ranks > 1:
            import socket
            with socket.socket() as s:
                s.bind(('127.0.0.1', 0))
                port = s.getsockname()[1]
            cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr', '127.0.0.1',
                   '--master-port', str(port), os.path.join(PKG, 'test.py'), '--']
        r = subprocess.run(cmd + COMMON + ['--checkpoint', ck, '--log', str(tmp / ('log_' + tag))] + extra, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    out = {'ck': ck, 'tmp': tmp}
    out['pck'] = run('pck', [])
    out['up'] = run('up', ['--metrics', 'full', '--decode', 'upsample', '--dump-preds', str(tmp / 'up')])
    out['arg'] = run('arg', ['--decode', 'argmax', '--metrics', 'full', '--dump-preds', str(tmp / 'arg')])
    out['up2'] = run('up2', ['--decode', 'upsample', '--dump-preds', str(tmp / 'up2')], ranks=2)      # (--dump-preds implies --metrics full)
    return out


def _recompute(d):
    pred, gt, vis = d['pred'].astype(np.float64), d['gt'].astype(np.float64), d['visible'] > 0
    e = np.sqrt(((pred - gt) ** 2).sum(-1))[vis]
    thr = d['thresholds'].astype(np.float64)
    curve = np.array([(e < t).sum() / e.size for t in thr])
    return e.mean(), E.trapz(curve, thr) / 30.0, curve


def _forward_heatmaps(ck, seed, dev):
    """The heat-maps test.py's forward gives for the synthetic test split `seed`: same weights, same batches, same graphed path."""
    import mi355
    from mi355.infer import GraphedForward
    from utils.synthetic_dataset import SyntheticHand21
    saved = (mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs)
    mi355.set_compute_dtype('bf16')
    try:
        m = _model().to(dev)
        m.load_state_dict(torch.load(ck, map_location='cpu', weights_only=False)['model'])
        m.eval()
        fwd, ds, ys = GraphedForward(m), SyntheticHand21(4 * B, (IMG, IMG), (HM, HM), seed=seed), []
        with torch.no_grad():
            for i in range(0, len(ds), B):
                ys.append(fwd(torch.stack([ds[j][0] for j in range(i, i + B)]).to(dev)).float().cpu())
        gt = np.stack([ds[j][3]['keypoint2d'].numpy() for j in range(len(ds))])
        return torch.cat(ys), gt
    finally:
        mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs = saved


@pytest.mark.parametrize('split,seed', [('source', 12), ('target', 14)])
def test_dump_upsample_matches_print_and_reference(gpu, runs, split, seed):
    d = np.load(str(runs['tmp'] / ('up.%s.npz' % split)))
    assert d['pred'].shape == (4 * B, 21, 2) and d['gt'].shape == (4 * B, 21, 2) and d['visible'].shape == (4 * B, 21) and d['maxval'].shape == (4 * B, 21)
    assert int(d['image_size']) == IMG and str(d['decode']) == 'upsample' and np.array_equal(d['thresholds'], THR)
    epe, auc, curve = _recompute(d)
    assert abs(float(d['epe']) - epe) <= 1e-12 * epe and abs(float(d['auc']) - auc) <= 1e-12 and np.allclose(d['pck_curve'], curve, rtol=0, atol=1e-15)
    printed = LINE.findall(runs['up'])
    assert len(printed) == 2, runs['up'][-2000:]
    line = printed[0 if split == 'source' else 1]
    assert line == ('%.3f' % epe, '%.4f' % auc)
    for name in ('MCP', 'PIP', 'DIP', 'fingertip', 'all'):
        assert runs['up'].count('EPE %s: ' % name) == 2
    y, gt = _forward_heatmaps(runs['ck'], seed, gpu)
    assert np.array_equal(d['gt'], gt) and (d['visible'] == 1).all()
    # heat-maps of a network are arbitrary floats: the bit comparison is against the up-sampling in the specified expression
    # order (eval_ref.upsample_kernel_order; torch's own fp32 kernel rounds border replicas differently by an ulp) ...
    maps = y.reshape(-1, HM, HM).numpy()
    ridx, rxy, rmv = E.first_argmax(E.upsample_kernel_order(maps, (IMG, IMG)))
    bad = np.nonzero((d['pred'].reshape(-1, 2) != rxy).any(1))[0]
    assert not len(bad), '%d of %d maps differ, first %s: %s vs %s' % (len(bad), len(rxy), bad[:4], d['pred'].reshape(-1, 2)[bad[:4]], rxy[bad[:4]])
    assert np.array_equal(_bits(d['maxval'].reshape(-1)), _bits(rmv))
    # ... and against torch's float64 up-sampling by the bound of the inexact kernel cases
    up64 = E.upsample(maps, (IMG, IMG), torch.float64).numpy().reshape(len(maps), -1)
    amax = np.abs(maps).reshape(len(maps), -1).max(1).astype(np.float64)
    at = up64[np.arange(len(maps)), ridx]
    assert (up64.max(1) - at <= 8 * EPS24 * amax).all() and (np.abs(d['maxval'].reshape(-1) - at) <= 4 * EPS24 * amax).all()
    t32 = E.upsample_argmax(maps, (IMG, IMG))[1]
    print('MEASURE %s: %d of %d maps decode to another replica under torch fp32 CPU rounding' % (split, int((t32 != rxy).any(1).sum()), len(rxy)))


def test_dump_argmax_is_heatmap_argmax_times_stride(gpu, runs):
    from utils.keypoint_detection import get_max_preds_device
    d = np.load(str(runs['tmp'] / 'arg.source.npz'))
    assert str(d['decode']) == 'argmax'
    y, _ = _forward_heatmaps(runs['ck'], 12, gpu)
    want = (get_max_preds_device(y.to(gpu))[0] * (IMG // HM)).cpu().numpy()
    assert IMG // HM == 4 and np.array_equal(d['pred'], want)
    epe, auc, _ = _recompute(d)
    assert LINE.findall(runs['arg'])[0] == ('%.3f' % epe, '%.4f' % auc)


def test_two_ranks_report_what_one_rank_reports(gpu, runs):
    assert len(LINE.findall(runs['up2'])) == 2 and LINE.findall(runs['up2']) == LINE.findall(runs['up'])
    assert [l for l in runs['up2'].splitlines() if l.startswith('EPE ')] == [l for l in runs['up'].splitlines() if l.startswith('EPE ')]
    # rank 0 writes the gathered predictions in data-set order: the single-rank files, array for array
    for split in ('source', 'target'):
        one, two = np.load(str(runs['tmp'] / ('up.%s.npz' % split))), np.load(str(runs['tmp'] / ('up2.%s.npz' % split)))
        assert sorted(one.files) == sorted(two.files)
        for k in ('pred', 'gt', 'visible', 'maxval', 'thresholds', 'pck_curve'):
            assert np.array_equal(one[k], two[k]), (split, k)
        assert abs(float(one['epe']) - float(two['epe'])) <= 1e-12 * float(one['epe']) and abs(float(one['auc']) - float(two['auc'])) <= 1e-12


def test_default_flags_print_what_full_prints_minus_the_added_lines(gpu, runs):
    keep = lambda out: [l for l in out.splitlines() if l.startswith(('Source:', 'MCP:', 'PIP:', 'DIP:', 'fingertip:', 'all:', 'loaded checkpoint'))]
    assert 'EPE' not in runs['pck'] and len(keep(runs['pck'])) == 7
    assert keep(runs['pck']) == keep(runs['up']) == keep(runs['arg'])
    strip = lambda out: [l for l in out.splitlines() if not l.startswith(('EPE', 'Namespace(', 'Test: '))]
    assert strip(runs['pck']) == strip(runs['up'])


def test_validate_returns_the_same_with_and_without_full_metrics(gpu, capsys):
    """train1.validate in process: the returned dict is the same object by value, the printed lines differ by the added ones."""
    import argparse
    import train1
    from uda.model.loss import JointsKLLoss
    from seeded import fill_module_
    from torch.utils.data import DataLoader
    from utils.synthetic_dataset import SyntheticHand21
    import mi355
    saved = (mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs)
    mi355.set_compute_dtype('bf16')
    try:
        m = _model()
        fill_module_(m, 11)
        m = m.to(gpu)
        loader = DataLoader(SyntheticHand21(3 * B + 1, (IMG, IMG), (HM, HM), seed=12), batch_size=B)
        res, outs = [], []
        for kw in (dict(), dict(metrics='full', decode='upsample', auc_max_px=30.0), dict(metrics='full', decode='argmax', auc_max_px=30.0)):
            res.append(train1.validate(loader, m, JointsKLLoss(), argparse.Namespace(print_freq=100, **kw)))
            outs.append(capsys.readouterr().out)
    finally:
        mi355._compute_dtype, mi355._fp8_convs, mi355._mx_convs = saved
    assert res[0] == res[1] == res[2]
    body = lambda o: [l for l in o.splitlines() if not l.startswith('EPE') and not l.startswith('Test: ')]
    assert 'EPE' not in outs[0] and outs[1].count('EPE: ') == 1 and outs[1].count('EPE ') == 5
    assert body(outs[0]) == body(outs[1]) == body(outs[2])
