"""Adaptive occlusion and the teacher-confidence gate inside the training iteration (the step of tests/test_gpu_bone.py: ResNet-18,
B = 2, 128 x 128 images, 32 x 32 heat-maps, bf16, a moving teacher):

1. occlusion on with prob = 0 (no box is ever drawn) and --mt-loss on is the run without the switch bit for bit over three eager
   iterations -- hoisting the teacher's forward to the head of step B changes neither its weights nor its input;
2. with boxes on, replayed graphs give what eager iterations give; batch['x_t'] is untouched; the student's input is the
   restatement applied to the recorded boxes; the teacher runs once per iteration with all three consumers on;
3. --teacher-conf alone: loss_mt is the float64 reference over the gated maps, within the ceiling tests/test_gpu_coord.py holds its
   scalar to; a tau above every p gives loss_mt == 0 exactly and leaves the parameters and the head's gradients untouched;
4. under a geometric view, a sample whose maps are all invalid gets no box."""
import numpy as np
import pytest
import torch

import occlude_ref as R

pytestmark = pytest.mark.gpu

ITERS = 3


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _training(gpu, occlude=None, conf=0.0, mt=True, coord=False, mixup=False, view=None):
    """test_gpu_mixup._training (resnet18, 32 x 32 heat-maps, bf16, a moving teacher).  occlude: None or the keyword arguments of
    KeypointOcclusion; view: None or those of GeometricView."""
    from test_gpu_mixup import _training as base
    from mi355.da_step import CoordRegression
    from mi355.teacher import GeometricView, KeypointOcclusion
    model, step, scheds = base(gpu, dict(beta=1.0, weight=0.5, labels='teacher') if mixup else None, mt=mt)
    if coord:
        step.coord = CoordRegression(weight=0.5, target='teacher', target_weight=0.5, ema=step.ema)
    if view is not None:
        step.view = GeometricView(seed=4, **view)
    if occlude is not None:
        step.occlude = KeypointOcclusion(seed=5, **occlude)
    step.teacher_conf = float(conf)
    return model, step, scheds


def _batch(gpu):
    from test_gpu_coord import _batches
    return _batches(gpu, 1)[0]


def _iterate(gpu, capture_at=None, iters=ITERS, **kw):
    model, step, scheds = _training(gpu, **kw)
    batch = _batch(gpu)
    x_t = batch['x_t'].clone()
    rec = []
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        one = {k: _bits(v) for k, v in out.items() if torch.is_tensor(v)}
        one['model'] = {k: _bits(v) for k, v in model.state_dict().items()}
        src = step.static if step.graphs is not None else batch
        assert torch.equal(src['x_t'], x_t), 'x_t changed'
        o = step.occlude
        if o is not None and o.n > 0:
            one.update(u=_bits(o.u), boxes=_bits(o.boxes), count=_bits(o.count), x_student=_bits(step._x_student), p=_bits(o.p), xy=_bits(o.xy),
                       conf=_bits(o.conf))
            one['raw'] = dict(u=o.u.cpu().numpy(), boxes=o.boxes.cpu().numpy(), count=o.count.cpu().numpy(), p=o.p.cpu().numpy(),
                              xy=o.xy.cpu().numpy(), x_student=step._x_student.cpu().numpy(), w_out=o.w_out.cpu().numpy())
            assert torch.equal(o.u.cpu(), o.u_host)
        rec.append(one)
    return rec, step, model, batch


BOXES = dict(prob=1.0, n=3, size=(0.08, 0.16), beta=1.0)


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        off, _, _, _ = _iterate(gpu)
        never, step_n, _, _ = _iterate(gpu, occlude=dict(prob=0.0, n=1))
        eager, step_e, _, batch = _iterate(gpu, occlude=BOXES)
        graph, step_g, _, _ = _iterate(gpu, occlude=BOXES, capture_at=1)
        assert step_g.graphs is not None and len(step_g.graphs) == 6
        x_t, w_t = batch['x_t'].cpu().numpy(), batch['w_t'].cpu().numpy()
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(off=off, never=never, eager=eager, graph=graph, x_t=x_t, w_t=w_t)


def test_occlusion_that_never_draws_is_the_run_without_it_bit_for_bit(runs):
    for it in range(ITERS):
        a, b = runs['off'][it], runs['never'][it]
        assert set(a) <= set(b) and 'loss_mt' in a and 'y_t' in a and 'y_t_ema' in a and 'occ_boxes' in b and 'occ_boxes' not in a
        for k in a:
            assert a[k] == b[k], (it, k)
        assert np.frombuffer(b['occ_boxes'][2], np.float32).tolist() == [0.0]
        assert not np.frombuffer(b['count'][2], np.int32).any()
        assert b['raw']['x_student'].tobytes() == runs['x_t'].tobytes()          # a copy: every bit


def test_boxes_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    for it in range(ITERS):                                             # iterations 1 and 2 of `graph` are replays
        assert set(a[it]) == set(b[it])
        for k in a[it]:
            if k != 'raw':
                assert a[it][k] == b[it][k], (it, k)
    assert len({a[it]['u'][2] for it in range(ITERS)}) == ITERS         # new draws every iteration, replays included
    assert runs['eager'][ITERS - 1]['model'] != runs['off'][ITERS - 1]['model']
    assert runs['eager'][0]['y_t'] != runs['off'][0]['y_t'] and runs['eager'][0]['y_t_ema'] == runs['off'][0]['y_t_ema']


def test_student_input_is_the_restatement_on_the_recorded_boxes(runs):
    for name in ('eager', 'graph'):
        for it in range(ITERS):
            raw = runs[name][it]['raw']
            assert raw['count'].tolist() == [3, 3] and raw['boxes'].shape == (2, 3, 4)
            assert raw['x_student'].tobytes() == R.occlude_images(runs['x_t'], raw['boxes']).tobytes()
            assert (raw['x_student'] != runs['x_t']).any()
            # ... and the boxes are the restatement's on the recorded p, xy and draws (tau = 0: every finite map is a candidate)
            want = R.teacher_select(raw['p'], raw['xy'], None, runs['w_t'], raw['u'], 0.0, 1.0, 3, 10, 20, 128, 32, 32)
            assert raw['boxes'].tobytes() == want[2].tobytes() and raw['w_out'].tobytes() == want[1].tobytes()
            assert np.frombuffer(runs[name][it]['occ_boxes'][2], np.float32).tolist() == [3.0]


def test_one_teacher_forward_per_iteration_with_all_three_consumers(gpu):
    import mi355
    try:
        model, step, scheds = _training(gpu, occlude=BOXES, conf=1e-4, coord=True, mixup=True)
        batch = _batch(gpu)
        step.run(batch)                                                 # (the first forward also lays the folded operands out)
        teacher = step.mt.teacher
        n = [0]
        run = teacher._run
        teacher._run = lambda x: (n.__setitem__(0, n[0] + 1), run(x))[1]
        for _ in range(2):
            n[0] = 0
            out = step.run(batch)
            torch.cuda.synchronize()
            assert n[0] == 1
        assert all(k in out for k in ('loss_mt', 'loss_coordt', 'loss_mix', 'occ_boxes', 'conf_share'))
        assert step.coord._teacher is None and step.mixup._teacher is None and step._occ_teacher is None
        assert all(np.isfinite(float(out[k])) for k in ('loss_mt', 'loss_coordt', 'loss_mix'))
    finally:
        mi355.set_compute_dtype('bf16')


def test_confidence_gate_alone_loss_mt_is_the_reference_over_the_gated_maps(gpu):
    import mi355
    try:
        # a first iteration without the gate gives the teacher's maps: tau is put into the widest gap of their sorted float64 p
        first, _, _, _ = _iterate(gpu, iters=1)
        y_ema = np.frombuffer(first[0]['y_t_ema'][2], np.float32).reshape(first[0]['y_t_ema'][1])
        B, K, H, W = y_ema.shape
        p64 = R.peak_prob(y_ema.reshape(B * K, H, W), 1.0)[2]
        tau = R.tau_in_widest_gap(p64)
        assert R.tau_clear(p64, tau) and np.isfinite(p64).all()
        gate = (p64 >= tau).reshape(B, K)
        assert 0 < gate.sum() < gate.size
        model, step, scheds = _training(gpu, conf=tau)
        out = step.run(_batch(gpu))
        torch.cuda.synchronize()
        assert _bits(out['y_t_ema']) == first[0]['y_t_ema'] and _bits(out['y_t']) == first[0]['y_t']
        assert step.occlude is None and 'occ_boxes' not in out
        sel = step._selector()
        assert np.array_equal(sel.conf.cpu().numpy(), gate.astype(np.float32))
        assert float(out['conf_share']) == float(np.float32(gate.sum()) / np.float32(gate.size))
        # m / n * the sum over the gated maps of the squared differences: float64, and the float32 CPU expression for the ceiling
        y_t = out['y_t'].float().cpu()
        d64 = ((y_t.double() - torch.from_numpy(y_ema).double()) ** 2).sum((2, 3)) * torch.from_numpy(gate).double()
        d32 = ((y_t - torch.from_numpy(y_ema)) ** 2).sum((2, 3)) * torch.from_numpy(gate).float()
        n = B * K
        k = float(np.float32(0.05 / (B * K * H * W)))
        b_rows = 8.0 * float((d32.double() - d64).abs().max()) + 2.0 ** -23 * float(d64.abs().max())
        want, ceiling = float(d64.sum()) * k, k * (n * b_rows + (n + 1) * 2.0 ** -24 * float(d64.abs().sum()))
        got = float(out['loss_mt'])
        print('loss_mt %.8e, float64 reference over %d of %d maps %.8e, error %.3e, ceiling %.3e' % (got, int(gate.sum()), n, want, abs(got - want), ceiling))
        assert want > 0 and abs(got - want) <= ceiling
        assert got != float(np.frombuffer(first[0]['loss_mt'][2], np.float32)[0])          # not the ungated term
    finally:
        mi355.set_compute_dtype('bf16')


def test_a_threshold_above_every_peak_switches_the_term_off_exactly(gpu):
    import mi355
    try:
        res = {}
        for name, kw in (('none', dict(mt=False)), ('gated', dict(conf=2.0))):
            model, step, scheds = _training(gpu, **kw)
            if step.ema is None:
                raise AssertionError('the step has no teacher')
            out = step.run(_batch(gpu))
            torch.cuda.synchronize()
            res[name] = dict(out=out, model={k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                             head={k: p.grad.detach().cpu().clone() for k, p in model.head.named_parameters() if p.grad is not None})
        out = res['gated']['out']
        assert _bits(out['loss_mt'])[2] == np.zeros(1, np.float32).tobytes()      # +0.0, every bit
        assert float(out['conf_share']) == 0.0
        # zero times anything: the head's gradients and every parameter are what the run without the term has
        assert res['gated']['head'] and set(res['gated']['head']) == set(res['none']['head'])
        for k, g in res['gated']['head'].items():
            assert torch.equal(g, res['none']['head'][k]), k
        for k, v in res['gated']['model'].items():
            assert torch.equal(v, res['none']['model'][k]), k
        # the loss on its own: zero flags give a zero gradient, bit for bit
        from uda.model.loss import MeanTeacherLoss
        crit = MeanTeacherLoss(gpu).set(0.05, 400, (2, 21, 32, 32))
        pre = torch.randn(2, 21, 32, 32, device=gpu, requires_grad=True)
        loss = crit(pre, torch.randn(2, 21, 32, 32, device=gpu), wmap=torch.zeros(2, 21, device=gpu))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not pre.grad.view(torch.int32).any()
    finally:
        mi355.set_compute_dtype('bf16')


def test_under_a_view_a_sample_with_no_valid_map_gets_no_box(gpu):
    import mi355
    try:
        # margin 16 on 32 x 32 maps: no peak lies 16 pixels inside the frame, so every map of every sample is invalid
        seen = {}
        for name, margin in (('invalid', 16), ('valid', 0)):
            rec, step, _, batch = _iterate(gpu, iters=1, occlude=BOXES, view=dict(rot_deg=10.0, scale=(0.9, 1.1), shift=0.05, margin=margin))
            valid = step._last_teacher.valid.cpu().numpy()
            seen[name] = (valid, rec[0]['raw'], step.occlude.conf.cpu().numpy())
        valid, raw, conf = seen['invalid']
        assert not valid.any() and not conf.any() and not raw['count'].any() and not raw['boxes'].any()
        assert raw['x_student'].tobytes() == batch['x_t'].cpu().numpy().tobytes()
        valid, raw, conf = seen['valid']
        assert valid.any() and np.array_equal(conf, valid) and raw['count'].sum() > 0
        for b in range(2):                                              # per sample: boxes only where a map is valid
            assert raw['count'][b] == min(3, int((valid[b] * (batch['w_t'].cpu().numpy().reshape(2, -1)[b] > 0)).sum()))
    finally:
        mi355.set_compute_dtype('bf16')


def test_occlusion_needs_a_teacher_and_a_draw(gpu):
    import mi355
    from mi355.teacher import KeypointOcclusion
    try:
        from test_gpu_mixup import _training as base
        model, step, scheds = base(gpu, None, with_ema=False)
        step.occlude = KeypointOcclusion(**BOXES)
        with pytest.raises(ValueError, match='ema-update'):
            step.run(_batch(gpu))
        o = KeypointOcclusion(**BOXES)
        y = torch.zeros(2, 21, 32, 32, device=gpu)
        with pytest.raises(mi355.Mi355Error, match='draw'):
            o.select(y, 0.0, 128)
        with pytest.raises(mi355.Mi355Error, match='select'):
            o.apply(torch.zeros(2, 3, 128, 128, device=gpu))
        with pytest.raises(RuntimeError):
            o.draw()
        o.draw(2, gpu)
        conf, w_out = o.select(y, 0.0, 128, w_in=torch.ones(2, 21, 1, device=gpu))
        assert conf.shape == (2, 21) and w_out.shape == (2, 21, 1) and o.boxes.shape == (2, 3, 4)
        x = torch.ones(2, 3, 128, 128, device=gpu)
        assert o.apply(x).data_ptr() == o.apply(x).data_ptr()           # fixed addresses
        assert float(o.p[0, 0]) == 1.0 / 1024                           # flat maps
    finally:
        mi355.set_compute_dtype('bf16')
