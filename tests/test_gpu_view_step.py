"""The geometric teacher view inside the training iteration (ResNet-18, B = 2, 64 x 64 images, 16 x 16 heat-maps): a view pinned to
the identity is the run without a view bit for bit; random views eager and replayed; one teacher forward per iteration; the
command line; a resumed run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import resume_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ITERS = 3


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _training(gpu, view=None, coord=False, mixup=False):
    """resnet18, 64 x 64 images, 16 x 16 heat-maps, fp32, a moving teacher and --mt-loss on.  view: None or the keyword arguments of
    GeometricView."""
    import mi355
    from mi355.da_step import CoordRegression, CrossDomainMixup, build_training
    from mi355.optim import EMATeacher
    from mi355.teacher import GeometricView, MeanTeacher
    from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('f32')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=16)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    teacher = _pose(gpu, PoseResNetx10, 5)
    teacher.load_state_dict(model.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    step.ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)
    step.mt = MeanTeacher(step.ema, weight=0.05, k='all')
    if coord:
        step.coord = CoordRegression(weight=0.5, target='teacher', target_weight=0.5, ema=step.ema)
    if mixup:
        step.mixup = CrossDomainMixup(beta=1.0, weight=0.5, labels='teacher', ema=step.ema, seed=1)
    if view is not None:
        step.view = GeometricView(seed=4, **view)
    return model, step, scheds


def _batch(gpu):
    from utils.synthetic import make_batch
    b = make_batch(2, 64, 16, seed=3, device=gpu, with_keypoints=True)
    b['x_t_ema'] = (b['x_t'] * 0.5 + 0.25).contiguous()
    return b


def _checksum(model):
    return {k: _bits(v) for k, v in model.state_dict().items()}


def _iterate(gpu, view, capture_at=None, **kw):
    model, step, scheds = _training(gpu, view, **kw)
    batch = _batch(gpu)
    rec = []
    for i in range(ITERS):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        one = {k: _bits(v) for k, v in out.items() if torch.is_tensor(v)}
        one['model'] = _checksum(model)
        if step.view is not None:
            one['valid'] = _bits(step._last_teacher.valid)
            one['recs'] = _bits(step.view.recs)
            assert _same(step.view.recs.view(-1, 18), step.view.recs_host)
        rec.append(one)
    return rec, step


IDENTITY = dict(rot_deg=0.0, scale=(1.0, 1.0), shift=0.0, margin=0)
RANDOM = dict(rot_deg=30.0, scale=(0.75, 1.25), shift=0.1, margin=2)


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        same, _ = _iterate(gpu, None)
        ident, step_i = _iterate(gpu, IDENTITY)
        eager, _ = _iterate(gpu, RANDOM)
        graph, step_g = _iterate(gpu, RANDOM, capture_at=1)
        assert step_g.graphs is not None and len(step_g.graphs) == 6
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(same=same, ident=ident, eager=eager, graph=graph)


def test_identity_view_is_the_run_without_a_view_bit_for_bit(runs):
    """The identity record copies the batch and the teacher's maps and margin 0 flags every map: every output, every loss and the
    parameters of three iterations."""
    for it in range(ITERS):
        a, b = runs['same'][it], runs['ident'][it]
        assert set(a) <= set(b) and 'loss_mt' in a and 'y_t_ema' in a
        for k in a:
            assert a[k] == b[k], (it, k)
        assert np.frombuffer(b['valid'][2], np.float32).tolist() == [1.0] * 42


def test_random_views_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    for it in range(ITERS):                                             # iterations 1 and 2 of `graph` are replays
        assert set(a[it]) == set(b[it])
        for k in a[it]:
            assert a[it][k] == b[it][k], (it, k)
    assert len({a[it]['recs'][2] for it in range(ITERS)}) == ITERS      # new views every iteration, replays included


def test_random_views_change_the_losses(runs):
    for it in range(ITERS):
        assert runs['eager'][it]['loss_mt'] != runs['same'][it]['loss_mt'], it
        assert runs['eager'][it]['y_t_ema'] != runs['same'][it]['y_t_ema'], it
    assert runs['eager'][ITERS - 1]['model'] != runs['same'][ITERS - 1]['model']


def test_one_teacher_forward_per_iteration_with_all_three_consumers(gpu):
    import mi355
    from mi355 import ops
    try:
        logs = {}
        for name, view in (('same', None), ('geom', RANDOM)):
            model, step, scheds = _training(gpu, view, coord=True, mixup=True)
            batch = _batch(gpu)
            for _ in range(2):
                step.run(batch)
            torch.cuda.synchronize()
            ops.prof_reset(); ops.prof_enable(2)
            try:
                out = step.run(batch)
                torch.cuda.synchronize()
                logs[name] = [e['label'] for e in ops.prof_launches()]
            finally:
                ops.prof_enable(0); ops.prof_reset()
            assert all(k in out for k in ('loss_mt', 'loss_coordt', 'loss_mix'))
        count = lambda log, word: sum(l.split()[0] == word for l in log)
        geom, same = logs['geom'], logs['same']
        assert count(geom, 'affine_warp') == 1 and count(geom, 'affine_unwarp') == 1 and count(geom, 'mse_heatmap_w') == 1
        assert count(geom, 'mse_heatmap') == 0 and count(same, 'mse_heatmap') == 1
        assert not any(l.split()[0] in ('affine_warp', 'affine_unwarp', 'mse_heatmap_w') for l in same)
        # the same launches otherwise: the teacher's convs are in the log once, with or without the view
        rest = lambda log: [re.sub(r'\s+', ' ', l) for l in log if l.split()[0] not in ('affine_warp', 'affine_unwarp', 'mse_heatmap_w', 'mse_heatmap')]
        assert rest(geom) == rest(same)
        assert ' +w' in [l for l in geom if l.startswith('affine_unwarp')][0]
    finally:
        mi355.set_compute_dtype('bf16')


def test_view_needs_a_draw_and_matching_shapes(gpu):
    import mi355
    from mi355.teacher import GeometricView
    v = GeometricView(**RANDOM)
    x = torch.zeros(2, 3, 64, 64, device=gpu)
    with pytest.raises(mi355.Mi355Error, match='draw'):
        v.apply(x)
    with pytest.raises(RuntimeError):
        v.draw()
    v.draw(2, gpu, image_size=64, heatmap_size=16)
    assert v.apply(x).data_ptr() == v.apply(x).data_ptr()               # fixed addresses
    y_hat, valid, w_out = v.undo(torch.zeros(2, 21, 16, 16, device=gpu), torch.ones(2, 21, 1, device=gpu))
    assert y_hat.shape == (2, 21, 16, 16) and valid.shape == (2, 21) and w_out.shape == (2, 21, 1)
    for bad in (torch.zeros(3, 3, 64, 64, device=gpu), torch.zeros(2, 3, 32, 32, device=gpu)):
        with pytest.raises(mi355.Mi355Error):
            v.apply(bad)
    with pytest.raises(mi355.Mi355Error):
        v.undo(torch.zeros(2, 21, 32, 32, device=gpu))
    with pytest.raises(mi355.Mi355Error):
        v.draw(2, gpu, image_size=(64, 32), heatmap_size=16)           # unequal strides


# ---------------------------------------------------------------- command line
def test_train_cli_runs_two_synthetic_iterations_with_the_view(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(log, extra):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '2', '-p', '1', '-j', '0',
                  '--pretrain_epochs', '1', '--epochs', '1', '--pretrain', str(tmp_path / 'none.pth'), '--log', log,
                  '--ema-update', 'const', '--mt-loss', 'on', '--mt-weight', '0.1']
        r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env,
                           capture_output=True, text=True, timeout=330)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [re.sub(r'(Time|Data) +\S+ +\( *\S+\)', '', l) for l in r.stdout.splitlines() if l.startswith('Epoch: [0]')]
        return lines[-2:]                                                # (the adaptation epoch; the pre-training one prints the same prefix)

    on = run(str(tmp_path / 'on'), ['--mt-view', 'geom'])
    same = run(str(tmp_path / 'same'), ['--mt-view', 'same'])
    none = run(str(tmp_path / 'none'), [])
    assert len(on) == len(same) == 2 and all('Loss (mt)' in l for l in on + same)
    losses = [float(v) for l in on for v in re.findall(r'Loss \([^)]*\) +(\S+) ', l)]
    assert len(losses) >= 6 and all(np.isfinite(v) for v in losses)
    assert on != same and same == none
    ck = torch.load(os.path.join(str(tmp_path / 'on'), 'checkpoints', '0.pth'), map_location='cpu', weights_only=False)
    assert ck['view_state']['draws'] == 2 and 'view_state' not in torch.load(os.path.join(str(tmp_path / 'same'), 'checkpoints', '0.pth'),
                                                                            map_location='cpu', weights_only=False)


# ---------------------------------------------------------------- resume
def test_resumed_run_equals_the_uninterrupted_one_with_the_view_on(gpu, tmp_path):
    child = os.path.join(HERE, 'view_resume_child.py')
    env = dict(os.environ, PYTHONPATH=PKG)

    def start(mode, out, ckpt=None):
        cmd = ['timeout', '-k', '10', '300', sys.executable, child, '--mode', mode, '--out', out] + (['--from', ckpt] if ckpt else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=330)
        assert r.returncode == 0, '%s child: status %d\n%s' % (mode, r.returncode, (r.stdout + r.stderr)[-4000:])
        return out

    full = start('full', str(tmp_path / 'full'))
    res = start('resume', str(tmp_path / 'resume'), os.path.join(full, 'checkpoints', '0.pth'))
    lf, lr = (resume_ref.read_lines(os.path.join(d, 'fp.jsonl')) for d in (full, res))
    assert [l['it'] for l in lf] == list(range(10)) and [l['it'] for l in lr] == list(range(5, 10))
    assert len({l['all'] for l in lf}) == 10 and all('view/params' in l['tensors'] and 'view/valid' in l['tensors'] for l in lf)

    def final(d):
        with np.load(os.path.join(d, 'final.npz'), allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    msg = resume_ref.describe_difference(lf, lr, range(5, 10), final(full), final(res))
    assert msg is None, 'resumed against uninterrupted: %s' % msg
