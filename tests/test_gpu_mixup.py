"""Cross-domain mixup on the GPU: mi355_mixup_pairs bit for bit against tests/mixup_ref.py inside the poisoned guard buffers of
tests/guarded.py, uda.model.loss.mixup against the reference's live function (tests/golden/g17_mixup.npz), DAStep's `mixup`
(step M) eager and replayed, the launch log, the clipper's fourth record, the command lines and two ranks on one GPU."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden
import guarded
import mixup_ref

pytestmark = pytest.mark.gpu

ONE_MINUS = float(np.float32(1) - np.float32(2.0 ** -24))             # the largest float32 below 1: om = 2^-24
EDGE_LAM = (1.0, 0.5, ONE_MINUS)
IMAGES = [(3, 2, 2), (3, 5, 7), (3, 16, 16)]                           # planes of 12, 105 and 768 floats
MAPS = [(21, 1, 1), (21, 5, 7), (21, 8, 8), (21, 64, 64)]             # planes of 21, 735, 1344 and 86016 floats


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


# ---------------------------------------------------------------- the kernel
def _operands(B, img, hm, seed):
    rng = np.random.default_rng(seed)
    K = hm[0]
    x_s = rng.standard_normal((B,) + img).astype(np.float32)
    x_t = (rng.standard_normal((B,) + img) * 0.7 + 0.1).astype(np.float32)
    hm_s = rng.random((B,) + hm).astype(np.float32)
    hm_t = (rng.random((B,) + hm) ** 4).astype(np.float32)
    w_s = (rng.random((B, K, 1)) < 0.8).astype(np.float32)
    w_t = (rng.random((B, K, 1)) < 0.6).astype(np.float32)
    return x_s, hm_s, w_s, x_t, hm_t, w_t


def _check_kernel(gpu, B, img, hm, lam, in_start=guarded.START, out_start=guarded.START, seed=0):
    """One guarded launch: outputs equal the restatement bit for bit, every output element is written, no flank byte changes
    and the inputs are what they were."""
    from mi355 import ops
    host = _operands(B, img, hm, seed)
    lam = np.asarray(lam, np.float32)
    assert lam.shape == (B,)
    names = ('x_s', 'hm_s', 'w_s', 'x_t', 'hm_t', 'w_t')
    dev = [guarded.place(torch.from_numpy(a).to(gpu), n, start=in_start) for a, n in zip(host, names)]
    lam_d = guarded.place(torch.from_numpy(lam).to(gpu), 'lam', start=in_start)
    out = tuple(guarded.empty((2 * B,) + a.shape[1:], torch.float32, gpu, n, start=out_start)
                for a, n in zip(host[:3], ('x_mix', 'hm_mix', 'w_mix')))
    assert all(t.data_ptr() % 16 == in_start % 16 for t in dev) and all(t.data_ptr() % 16 == out_start % 16 for t in out)
    got = ops.mixup_pairs(*dev, lam_d, out=out)
    torch.cuda.synchronize()
    guarded.check('mixup_pairs B%d %s %s' % (B, img, hm))
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    want = mixup_ref.mixup_pairs(*host, lam)
    for g, w, n in zip(got, want, ('x_mix', 'hm_mix', 'w_mix')):
        assert guarded.unwritten(g) == 0, n
        assert _same(g, w), (n, B, img, hm, lam.tolist())
    for t, a, n in zip(dev + [lam_d], host + (lam,), names + ('lam',)):
        assert _same(t, a), n                                          # the inputs are only read


@pytest.mark.parametrize('hm', MAPS, ids=lambda s: 'hm%dx%d' % s[1:])
@pytest.mark.parametrize('img', IMAGES, ids=lambda s: 'img%dx%d' % s[1:])
@pytest.mark.parametrize('B', [1, 3])
def test_kernel_bit_exact_inside_guard_buffers(gpu, B, img, hm):
    """Planes of 12, 105, 21 and 735 floats: 16-byte vectors straddle samples (up to four samples in one vector at 1 x 1 maps of
    ... 21 floats: two), and with B = 3 the second half of x_mix / hm_mix starts off a 16-byte boundary (n % 4 != 0)."""
    try:
        if B == 3:
            _check_kernel(gpu, B, img, hm, EDGE_LAM, seed=B * 100 + img[1] + hm[1])
            _check_kernel(gpu, B, img, hm, (0.7316, ONE_MINUS, 0.5000001), seed=7)
        else:
            for lam in EDGE_LAM + (0.8125,):
                _check_kernel(gpu, B, img, hm, (lam,), seed=B * 100 + img[1] + hm[1])
    finally:
        guarded.reset()


@pytest.mark.parametrize('which', ['all', 'inputs', 'outputs'])
def test_kernel_scalar_path_on_views_4_bytes_off_a_16_byte_boundary(gpu, which):
    """Every operand (or only the inputs, or only the outputs) starts 4 bytes past a 16-byte boundary: the scalar build of the
    range, same bits."""
    off = guarded.START + 4
    try:
        for img, hm in (((3, 16, 16), (21, 8, 8)), ((3, 5, 7), (21, 5, 7))):
            _check_kernel(gpu, 3, img, hm, EDGE_LAM, in_start=off if which != 'outputs' else guarded.START,
                          out_start=off if which != 'inputs' else guarded.START, seed=11)
    finally:
        guarded.reset()


def test_kernel_image_tensor_larger_than_one_pass_of_the_capped_grid(gpu):
    """3 x 3 x 512 x 512 = 2 359 296 floats: more 16-byte vectors than MI355_MIXUP_MAX_BLOCKS x 256 lanes take in one pass, so the
    grid-stride loop runs a second, partial pass.  A second call with an odd plane does the same on the straddling path."""
    blocks = int(re.search(r'#define MI355_MIXUP_MAX_BLOCKS (\d+)', open(os.path.join(os.path.dirname(PKG), 'include', 'mi355pose.h')).read()).group(1))
    try:
        for img in ((3, 512, 512), (3, 511, 513)):
            assert 3 * img[0] * img[1] * img[2] // 4 > blocks * 256
            _check_kernel(gpu, 3, img, (21, 5, 7), EDGE_LAM, seed=5)
    finally:
        guarded.reset()


def test_wrapper_refuses_what_the_kernel_cannot_index(gpu):
    import mi355
    from mi355 import ops
    z = lambda *s: torch.zeros(s, device=gpu)
    ok = dict(x_s=z(2, 3, 4, 4), hm_s=z(2, 21, 2, 2), w_s=z(2, 21, 1), x_t=z(2, 3, 4, 4), hm_t=z(2, 21, 2, 2), w_t=z(2, 21, 1), lam=z(2))
    order = ('x_s', 'hm_s', 'w_s', 'x_t', 'hm_t', 'w_t', 'lam')
    ops.mixup_pairs(*[ok[k] for k in order])
    bad = [dict(x_t=z(2, 3, 4, 5)), dict(hm_t=z(2, 20, 2, 2)), dict(w_t=z(2, 20, 1)), dict(lam=z(3)), dict(lam=z(2).double()),
           dict(x_s=z(2, 3, 4, 8)[..., ::2]), dict(hm_s=z(2, 21, 2, 2).cpu()), dict(x_s=z(2, 3, 4, 4).half(), x_t=z(2, 3, 4, 4).half()),
           dict(hm_s=z(3, 21, 2, 2), hm_t=z(3, 21, 2, 2)), dict(w_s=z(2, 21, 2), w_t=z(2, 21, 2))]
    for change in bad:
        with pytest.raises(mi355.Mi355Error):
            ops.mixup_pairs(*[dict(ok, **change)[k] for k in order])
    outs = lambda **c: tuple(dict(dict(x=z(4, 3, 4, 4), hm=z(4, 21, 2, 2), w=z(4, 21, 1)), **c)[k] for k in ('x', 'hm', 'w'))
    ops.mixup_pairs(*[ok[k] for k in order], out=outs())
    for change in (dict(x=z(3, 3, 4, 4)), dict(hm=z(4, 21, 2, 1)), dict(w=z(2, 21, 1)), dict(x=z(4, 3, 4, 4).double()),
                   dict(hm=z(4, 21, 2, 4)[..., ::2])):
        with pytest.raises(mi355.Mi355Error):                           # no room, or not dense
            ops.mixup_pairs(*[ok[k] for k in order], out=outs(**change))
    with pytest.raises(mi355.Mi355Error, match='overlap'):             # refused by the library: in place
        buf = z(4, 3, 4, 4)
        ops.mixup_pairs(buf[:2], ok['hm_s'], ok['w_s'], ok['x_t'], ok['hm_t'], ok['w_t'], ok['lam'], out=outs(x=buf))


def test_launch_is_logged_under_the_mixup_label(gpu):
    from mi355 import ops
    host = _operands(3, (3, 5, 7), (21, 5, 7), 1)
    dev = [torch.from_numpy(a).to(gpu) for a in host]
    lam = torch.tensor(EDGE_LAM, device=gpu)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        ops.mixup_pairs(*dev, lam)
        torch.cuda.synchronize()
        log = ops.prof_launches()
    finally:
        ops.prof_enable(0); ops.prof_reset()
    assert len(log) == 1 and log[0]['family'] == 2 and log[0]['label'].startswith('mixup B3 img105 hm735 K21')
    assert log[0]['bytes'] == 16.0 * (3 * 105 + 3 * 735 + 3 * 21) + 12


# ---------------------------------------------------------------- the reference's function
@pytest.mark.parametrize('tag,beta', [('b0.5', 0.5), ('b1', 1.0)])
def test_mixup_against_the_reference(gpu, tag, beta):
    from uda.model.loss import mixup
    g = golden('g17_mixup')
    args = [torch.from_numpy(g[k]).to(gpu) for k in ('x_s', 'hm_s', 'w_s', 'x_t', 'hm_t', 'w_t')]
    out = mixup(*args, beta, mix=torch.from_numpy(g[tag + '/lam']))
    assert isinstance(out, tuple) and len(out) == 6 and out[2] is out[5]
    for i, o in enumerate(out):
        assert o.is_cuda and not o.requires_grad and _same(o, g['%s/out%d' % (tag, i)]), (tag, i)
    # views into the kernel's three outputs: the two halves of one storage
    assert out[3].data_ptr() == out[0].data_ptr() + 4 * out[0].numel() and out[4].data_ptr() == out[1].data_ptr() + 4 * out[1].numel()
    # mix=None draws as the reference does: under the golden's seed the same blends, where this torch build draws the same
    state = torch.get_rng_state()
    try:
        torch.manual_seed(int(g['seed']))
        drawn = mixup(*args, beta)
    finally:
        torch.set_rng_state(state)
    if _same(drawn[0], g[tag + '/out0']):
        for i, o in enumerate(drawn):
            assert _same(o, g['%s/out%d' % (tag, i)]), (tag, i)
    else:
        print('this torch build draws Beta(%g, %g) differently from the one that wrote the golden' % (beta, beta))
        assert drawn[0].shape == out[0].shape and torch.isfinite(drawn[0]).all()


# ---------------------------------------------------------------- the step
def _training(gpu, mixup=None, mt=False, with_ema=True, clip=False):
    """tests/test_gpu_mt.py's _training (resnet18, 32 x 32 heat-maps, bf16) with the mixup stage; mixup: None or the keyword
    arguments of CrossDomainMixup."""
    import mi355
    from mi355.da_step import CrossDomainMixup, build_training
    from mi355.optim import EMATeacher, GradClipper
    from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if with_ema:
        teacher = _pose(gpu, PoseResNetx10, 5)
        teacher.load_state_dict(model.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        step.ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)
    if mt:
        from mi355.teacher import MeanTeacher
        step.mt = MeanTeacher(step.ema, weight=0.05, k='all')
    if mixup is not None:
        step.mixup = CrossDomainMixup(ema=step.ema, seed=1, **mixup)
    if clip:
        step.clip = GradClipper(float('inf'), gpu)
    return model, step, scheds


def _batch(gpu):
    from utils.synthetic import make_batch
    b = make_batch(2, 128, 32, seed=3, device=gpu)
    b['x_t_ema'] = (b['x_t'] * 0.5 + 0.25).contiguous()
    return b


def _kl64(y, hm, w, weight):
    import heatmap_ref
    rows, _ = heatmap_ref.kl(y.float().cpu(), hm.cpu(), w.cpu(), 0.0, 1.0)
    return weight * float(rows.mean())


def _run(gpu, mixup, iters, capture_at=None, recompute=False, **kw):
    from mi355 import ops
    from uda.model.loss import JointsKLLoss
    from uda.model.regda_4 import PseudoLabelGenerator
    model, step, scheds = _training(gpu, mixup, **kw)
    batch = _batch(gpu)
    B = batch['x_s'].shape[0]
    rec = dict(model=[], loss_mix=[], lam=[], want=[], after_b=[], after_m=[])
    seen = {}
    if recompute:                                                       # what step M hands the criterion, and the state between the updates
        kl = step.crit['kl']

        class Spy(torch.nn.Module):
            def forward(self, y, target, weight=None, scale=1.0):
                if y.shape[0] == 2 * B:
                    seen.update(y=y.detach().clone(), hm=target.detach().clone(), w=weight.detach().clone(), scale=scale)
                return kl(y, target, weight, scale=scale)
        step.crit['kl'] = Spy()
        # (parameters: the BatchNorm statistics of the adversarial heads also move in step C's forward, with or without mixup)
        adv = lambda: {k: np.ascontiguousarray(p.detach().permute(0, 2, 3, 1).cpu().numpy() if p.dim() == 4 else p.detach().cpu().numpy())
                       for k, p in model.named_parameters() if k.startswith('head_adv')}
        upd_b, upd_m = step._update_B, step._update_M
        step._update_B = lambda: (upd_b(), torch.cuda.synchronize(), rec['after_b'].append(adv()))[0]
        step._update_M = lambda: (upd_m(), torch.cuda.synchronize(), rec['after_m'].append(adv()))[0]
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        rec['model'].append(_host(model))
        if mixup is None:
            assert 'loss_mix' not in out
            continue
        rec['loss_mix'].append(float(out['loss_mix']))
        rec['lam'].append(step.mixup.lam.cpu().numpy().copy())
        assert _same(rec['lam'][-1], step.mixup.lam_host.numpy())
        if recompute:
            # the same kernels on cloned operands outside the step: the labels from y_t, the blend, the criterion
            hm_t = PseudoLabelGenerator(21, 32, 32).labels(out['y_t'].clone(), kind=0, want_gf=False)[0]
            x_mix, hm_mix, w_mix = ops.mixup_pairs(batch['x_s'].clone(), batch['label_s'].clone(), batch['w_s'].clone(), batch['x_t'].clone(),
                                                   hm_t, batch['w_t'].clone(), step.mixup.lam.clone())
            assert _same(hm_mix, seen['hm']) and _same(w_mix, seen['w']) and seen['scale'] == mixup['weight']
            again = float(JointsKLLoss()(seen['y'], hm_mix, w_mix, scale=mixup['weight']))
            rec['want'].append((float(out['loss_mix']), again, _kl64(seen['y'], hm_mix, w_mix, mixup['weight'])))
    return rec, step


MIX = dict(beta=1.0, weight=0.5, labels='student')


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        eager, _ = _run(gpu, MIX, 6, recompute=True)
        graph, step = _run(gpu, MIX, 6, capture_at=3)
        assert step.graphs is not None and len(step.graphs) == 8
        off, step_off = _run(gpu, None, 4, capture_at=3)
        assert len(step_off.graphs) == 6
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(eager=eager, graph=graph, off=off)


def test_step_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    assert a['loss_mix'] == b['loss_mix'] and len(set(a['loss_mix'])) == 6 and all(v > 0 for v in a['loss_mix'])
    for it in range(6):                                                 # iterations 3 .. 5 of `graph` are replays
        assert _same(a['lam'][it], b['lam'][it]) and (a['lam'][it] >= 0.5).all()
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)
    assert len({l.tobytes() for l in a['lam']}) == 6                    # new coefficients every iteration, replays included


def test_step_loss_mix_is_the_recomputed_term(runs):
    assert len(runs['eager']['want']) == 6
    for got, again, want64 in runs['eager']['want']:
        assert got == again and got > 0                                 # the same kernels on the same operands outside the step
        print('loss_mix %.8e, weight * KL in float64 %.8e, relative distance %.2e' % (got, want64, abs(got - want64) / want64))
        assert abs(got - want64) <= 1e-4 * want64


def test_step_m_trains_backbone_and_main_head_and_leaves_the_adversarial_heads(runs):
    on, off = runs['eager'], runs['off']
    for k in ('backbone.layer1.0.conv1.weight', 'head.0.weight'):
        assert k in on['model'][0] and not _same(on['model'][0][k], off['model'][0][k]), k
    assert len(on['after_b']) == len(on['after_m']) == 6
    for it in range(6):                                                 # after update M: what update B left, bit for bit
        assert len(on['after_b'][it]) > 10
        for k, v in on['after_b'][it].items():
            assert _same(v, on['after_m'][it][k]), (it, k)
            if it > 0 and k.endswith('0.weight'):
                assert not _same(v, on['after_b'][it - 1][k]), k       # (and update B does move them)


def _logged(step, batch):
    from mi355 import ops
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        step.run(batch)
        torch.cuda.synchronize()
        return [(e['family'], e['label']) for e in ops.prof_launches()]
    finally:
        ops.prof_enable(0); ops.prof_reset()


def test_teacher_labels_reuse_the_teacher_forward_of_step_c(gpu):
    """labels='teacher' with the consistency term on: one teacher forward per iteration (the launches of an iteration are those of
    labels='student', launch for launch), one fold behind update M, one mse_heatmap, exactly one mixup launch.  Without the
    consistency term the mixup stage runs the teacher itself: one forward more than with student labels, and its own fold."""
    import mi355
    try:
        logs, calls = {}, {}
        for name, labels, mt in (('student', 'student', True), ('teacher', 'teacher', True), ('alone', 'teacher', False),
                                 ('alone_student', 'student', False)):
            model, step, scheds = _training(gpu, dict(MIX, labels=labels), mt=mt)
            batch = _batch(gpu)
            teacher = step.mixup.teacher(step)
            n = [0]
            fwd = teacher.forward
            teacher.forward = lambda x, fwd=fwd, n=n: (n.__setitem__(0, n[0] + 1), fwd(x))[1]
            for _ in range(2):
                step.run(batch)
            n[0] = 0
            logs[name] = [l for _, l in _logged(step, batch)]
            calls[name] = n[0]
        assert calls['teacher'] == 1 and calls['student'] == 1 and calls['alone'] == 1 and calls['alone_student'] == 0
        strip = lambda log: [re.sub(r'\s+', ' ', l) for l in log]
        assert strip(logs['teacher']) == strip(logs['student'])          # no second teacher forward, nothing else either
        for name in ('teacher', 'student'):
            assert sum(l.startswith('mixup') for l in logs[name]) == 1
            assert sum(l.startswith('bn_fold') for l in logs[name]) == 1 and sum(l.startswith('mse_heatmap') for l in logs[name]) == 1
        assert sum(l.startswith('mixup') for l in logs['alone']) == 1 and sum(l.startswith('bn_fold') for l in logs['alone']) == 1
        assert not any(l.startswith('bn_fold') for l in logs['alone_student'])
        convs = lambda log: sum(l.startswith('fwd ') for l in log)
        assert convs(logs['alone']) > convs(logs['alone_student'])        # the teacher's forward is in the log when it runs
    finally:
        mi355.set_compute_dtype('bf16')


def test_step_off_launch_log_is_unchanged_by_the_new_code(gpu):
    """With mixup off an iteration launches what it launched before CrossDomainMixup existed in the process: the logged launches
    are the same with the class removed from mi355.da_step and with it back, and none of them is a mixup launch."""
    import mi355
    import mi355.da_step as ds
    try:
        model, step, scheds = _training(gpu, None, with_ema=False)
        batch = _batch(gpu)
        for _ in range(2):
            step.run(batch)
        cls = ds.CrossDomainMixup
        del ds.CrossDomainMixup
        try:
            before = _logged(step, batch)
        finally:
            ds.CrossDomainMixup = cls
        after = _logged(step, batch)
        assert len(before) > 100 and before == after
        assert not any(l.startswith('mixup') for _, l in after)
        step.mixup = cls(**MIX)
        step.run(batch)
        on = [l for _, l in _logged(step, batch)]
        assert sum(l.startswith('mixup') for l in on) == 1 and len(on) > len(after)
    finally:
        mi355.set_compute_dtype('bf16')


def test_clipper_reports_a_fourth_finite_norm(gpu):
    import mi355
    from mi355.optim import GradClipper
    try:
        model, step, scheds = _training(gpu, MIX, clip=True)
        batch = _batch(gpu)
        for i in range(4):
            if i == 3:
                step.capture(batch, warmup=0)
            step.run(batch)
        torch.cuda.synchronize()
        norms, skipped = step.clip.read()
        assert tuple(step.clip.SLOTS) == ('a', 'b', 'c', 'm') and sorted(norms) == ['a', 'b', 'c', 'm'] and skipped == 0
        for s in step.clip.SLOTS:
            assert np.isfinite(norms[s][0]) and norms[s][0] > 0 and norms[s][1] == 1.0 and norms[s][2] == 0, (s, norms[s])
        assert 'gn_m' in step.out and len(step.graphs) == 8
        # mixup off: the three records of today, byte for byte the layout a fresh clipper has
        assert GradClipper.SLOTS == ('a', 'b', 'c') and GradClipper(1.0, gpu).recs.numel() == 3 * 32
        model, step, scheds = _training(gpu, None, clip=True, with_ema=False)
        step.run(batch)
        assert tuple(step.clip.SLOTS) == ('a', 'b', 'c') and step.clip.recs.numel() == 3 * 32 and 'gn_m' not in step.out
    finally:
        mi355.set_compute_dtype('bf16')


# ---------------------------------------------------------------- command lines
def test_train_cli_with_the_mixup_switch(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(log, extra, ok=True):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0',
                  '--pretrain_epochs', '1', '--log', log]
        r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    def mix_values(out):
        return [float(v) for v in re.findall(r'Loss \(mix\) (\S+) \(', out)]

    state = lambda log, epoch: torch.load(os.path.join(log, 'checkpoints', '%d.pth' % epoch), map_location='cpu', weights_only=False)['mixup_state']
    pre = str(tmp_path / 'none.pth')
    # one epoch, then the second one resumed ...
    log = str(tmp_path / 'mix')
    out = run(log, ['--epochs', '1', '--pretrain', pre, '--mixup', 'on', '--mixup-beta', '0.5'])
    assert 'Loss (mix)' in out and 'HIP graphs captured' in out and 'replay 8 graphs' in out
    assert len(mix_values(out)) == 3 and all(v > 0 for v in mix_values(out))
    out = run(log, ['--epochs', '2', '--resume', os.path.join(log, 'checkpoints', '0.pth'), '--mixup', 'on', '--mixup-beta', '0.5'])
    assert 'Epoch: [1]' in out and 'Epoch: [0]' not in out and all(v > 0 for v in mix_values(out))
    # ... against two epochs without interruption: the resumed epoch drew what the uninterrupted one drew
    log2 = str(tmp_path / 'mix2')
    run(log2, ['--epochs', '2', '--pretrain', pre, '--mixup', 'on', '--mixup-beta', '0.5'])
    a0, a1, b0, b1 = state(log, 0), state(log, 1), state(log2, 0), state(log2, 1)
    assert a0['draws'] == b0['draws'] == 6 and a1['draws'] == b1['draws'] == 12
    assert torch.equal(a0['rng_state'], b0['rng_state']) and torch.equal(a0['lam'], b0['lam'])
    assert torch.equal(a1['rng_state'], b1['rng_state']) and torch.equal(a1['lam'], b1['lam']) and not torch.equal(a1['lam'], a0['lam'])
    # the first coefficients of the second epoch, drawn here from the state the first epoch's checkpoint holds, and again from
    # the state a run that never stopped held at that point: the same, and not those of a fresh start
    from mi355.da_step import CrossDomainMixup

    def first_of_epoch_1(st):
        m = CrossDomainMixup(beta=0.5, seed=1)
        fresh = m.state_dict()['rng_state']
        m.load_state_dict(st)
        m.lam = torch.zeros(4)
        return m.draw(), fresh

    la, fresh = first_of_epoch_1(a0)
    lb, _ = first_of_epoch_1(b0)
    assert torch.equal(la, lb) and not torch.equal(a0['rng_state'], fresh) and (la >= 0.5).all()
    # labelled by the teacher
    out = run(str(tmp_path / 'mixt'), ['--epochs', '1', '--pretrain', pre, '--mixup', 'on', '--mixup-labels', 'teacher', '--ema-update', 'const'])
    assert 'Loss (mix)' in out and 'HIP graphs captured' in out and len(mix_values(out)) == 3 and all(v > 0 for v in mix_values(out))
    assert len(re.findall(r'^ema: +\d+\.\d{3}$', out, re.M)) == 1


# ---------------------------------------------------------------- two ranks on one GPU
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    from conftest import PKG  # noqa: F401  (package source root on sys.path in the spawned process)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), MI355_OVERLAP_ALLREDUCE='1', MI355_BN_RESIDENT='0')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import mi355
    import mi355.da_step as ds
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic import make_batch
    mi355.load(); mi355.set_compute_dtype('f32')
    torch.manual_seed(1)
    bb = models.resnet18(pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    ds.broadcast_module(model, 0)
    step, opts, scheds = ds.build_training(model, heatmap_size=32)
    step.mixup = ds.CrossDomainMixup(beta=1.0, weight=0.5, seed=1, rank=rank)
    batch = make_batch(2, 128, 32, seed=1 + rank, device=dev)
    lams = []
    for _ in range(2):
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        lams.append(step.mixup.lam.cpu().tolist())
    torch.cuda.synchronize()
    cs = [float(p.detach().double().abs().sum()) for p in model.parameters()]
    q.put((rank, cs, lams, float(out['loss_mix'])))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_parameters_and_draw_different_coefficients(gpu):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1], 'ranks diverged with the mixup stage'
    assert all(np.isfinite(c) for c in res[0][1]) and res[0][3] > 0 and res[1][3] > 0
    assert res[0][2] != res[1][2] and res[0][2][0] != res[0][2][1]      # per rank, per iteration
