"""Fourier-domain stylisation on the GPU: mi355_fda_transfer against the float64 partial-DFT oracle of tests/fda_ref.py inside the
poisoned guard buffers of tests/guarded.py, the exact cases (identity, zero plane, non-finite pixels), determinism eagerly and
under graph replay, the wrapper's refusals, DAStep's `fda` (step A on the stylised batch) eager and replayed, the launch log and
the command lines.

Tolerance, derived and not tuned: |got - fl32(want64)| <= spacing(fl32(|want64|)) + 1e-8 element-wise.  One fp32 ulp for the
single rounding at the store; 1e-8 absolute for the order-dependent error of the fp64 sums (about 1e-15 relative per coefficient
after the division by H W, amplified by at most 1 / (|Fs| / HW) in the phase, over at most (2b+1)^2 coefficients).  That needs
min |Fs[u,v]| / (H W) >= 1e-5 over the window of every source plane: asserted on the oracle, a condition on the inputs."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import fda_ref
import guarded

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (C, H, W, b): seed; B = 1 and 3 where not fixed.  Seeds: the first for which the oracle alone meets the amplitude condition.
CASES = [(3, 16, 16, 0), (3, 16, 16, 1), (3, 16, 16, 7), (3, 16, 32, 2), (3, 48, 16, 2), (3, 17, 19, 2), (1, 24, 40, 3), (3, 64, 64, 5),
         (3, 128, 128, 32)]
SEEDS = {(3, 3, 128, 128, 32): 1}


def _beta(H, W, b):
    beta = (b + 0.5) / min(H, W)
    assert fda_ref.band(H, W, beta) == b
    return beta


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, b):
    """Inputs and the oracle of one case, computed once and shared (read-only)."""
    x_s, x_t = fda_ref.inputs((B, C, H, W), SEEDS.get((B, C, H, W, b), 0), MEAN, STD)
    want, amin = fda_ref.partial_dft(x_s, x_t, b, MEAN, STD, want_min=True)
    assert amin >= 1e-5, 'inputs of %s break the amplitude condition: %.3e' % ((B, C, H, W, b), amin)
    for a in (x_s, x_t, want):
        a.setflags(write=False)
    return x_s, x_t, want


def _within(got, want64, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    want32 = want64.astype(np.float32)
    tol = np.spacing(np.abs(want32)).astype(np.float64) + 1e-8
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    print('%s: worst |got - fl32(want)| / tolerance = %.3f' % (what, float((err / tol).max())))
    assert np.isfinite(got).all() and (err <= tol).all(), (what, float((err / tol).max()))


def _launch(gpu, x_s, x_t, b, in_start=guarded.START, out_start=guarded.START, what=''):
    """One guarded call: every output and workspace element written, no flank byte changed, the inputs what they were."""
    import mi355
    from mi355 import ops
    B, C, H, W = x_s.shape
    need = mi355.load().mi355_fda_workspace_bytes(B, C, H, W, b)
    assert need > 0
    d_s = guarded.place(torch.from_numpy(np.array(x_s)).to(gpu), 'x_s', start=in_start)
    d_t = guarded.place(torch.from_numpy(np.array(x_t)).to(gpu), 'x_t', start=in_start)
    out = guarded.empty((B, C, H, W), torch.float32, gpu, 'out', start=out_start)
    ws = guarded.empty((need,), torch.uint8, gpu, 'ws', start=guarded.START)
    assert d_s.data_ptr() % 16 == in_start % 16 and out.data_ptr() % 16 == out_start % 16 and ws.data_ptr() % 16 == 0
    got = ops.fda_transfer(d_s, d_t, _beta(H, W, b), MEAN, STD, out=out, ws=ws)
    torch.cuda.synchronize()
    guarded.check('fda_transfer %s b%d %s' % ((B, C, H, W), b, what))
    assert got.data_ptr() == out.data_ptr()
    assert _same(d_s, x_s) and _same(d_t, x_t)                          # the inputs are only read
    assert guarded.unwritten(ws.view(torch.float64)) == 0               # every partial was written
    return got


def _check_kernel(gpu, B, C, H, W, b, **kw):
    x_s, x_t, want = _case(B, C, H, W, b)
    got = _launch(gpu, x_s, x_t, b, **kw)
    assert guarded.unwritten(got) == 0
    _within(got, want, 'B%d C%d %dx%d b%d' % (B, C, H, W, b))


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'c%d-%dx%d-b%d' % c)
@pytest.mark.parametrize('B', [1, 3])
def test_kernel_within_one_ulp_of_the_oracle_inside_guard_buffers(gpu, B, case):
    try:
        _check_kernel(gpu, B, *case)
    finally:
        guarded.reset()


def test_kernel_at_the_workloads_plane_and_default_band(gpu):
    try:
        _check_kernel(gpu, 2, 3, 256, 256, 2)
    finally:
        guarded.reset()


@pytest.mark.parametrize('which', ['all', 'inputs', 'outputs'])
@pytest.mark.parametrize('case', [(3, 16, 16, 1), (3, 17, 19, 2)], ids=lambda c: '%dx%d' % c[1:3])
def test_kernel_scalar_path_on_views_4_bytes_off_a_16_byte_boundary(gpu, case, which):
    """The second start offset: x_s, x_t and out (or only the inputs, or only the output) start 4 bytes past a 16-byte boundary, so
    the launches that read or write them take their rows float by float.  Same tolerance."""
    off = guarded.START + 4
    try:
        _check_kernel(gpu, 3, *case, in_start=off if which != 'outputs' else guarded.START,
                      out_start=off if which != 'inputs' else guarded.START, what=which)
    finally:
        guarded.reset()


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize('case', [(3, 16, 16, 7), (3, 17, 19, 2), (3, 64, 64, 5), (3, 128, 128, 32)], ids=lambda c: '%dx%d-b%d' % c[1:])
def test_a_target_equal_to_the_source_returns_the_source_bit_for_bit(gpu, case):
    x_s, _, _ = _case(3, *case)
    try:
        got = _launch(gpu, x_s, x_s, case[3])
        assert guarded.unwritten(got) == 0 and _same(got, x_s)
    finally:
        guarded.reset()


def test_an_all_zero_source_plane_takes_phase_zero(gpu):
    """Every non-DC coefficient of a zero plane is exactly 0 in any summation order: the phase factor is 1 there."""
    x_s, x_t, _ = _case(3, 3, 16, 16, 1)
    x_s = np.array(x_s)
    x_s[1, 2] = 0.0
    want = fda_ref.partial_dft(x_s, x_t, 1, MEAN, STD)
    win = np.abs(fda_ref.window(x_s, 1, MEAN, STD))
    assert (win[1, 2] == 0).sum() == 8 and np.isfinite(want).all()
    try:
        got = _launch(gpu, x_s, x_t, 1)
        _within(got, want, 'zero plane')
    finally:
        guarded.reset()


@pytest.mark.parametrize('bad', [float('inf'), float('nan')], ids=['inf', 'nan'])
@pytest.mark.parametrize('side', ['x_s', 'x_t'])
@pytest.mark.parametrize('case', [(3, 16, 16, 0), (3, 16, 16, 1), (3, 17, 19, 2)], ids=lambda c: '%dx%d-b%d' % c[1:])
def test_a_non_finite_pixel_poisons_its_plane_and_no_other(gpu, case, side, bad):
    x_s, x_t, _ = _case(3, *case)
    C, H, W, b = case
    try:
        clean = _launch(gpu, x_s, x_t, b).clone()
        dirty = {'x_s': np.array(x_s), 'x_t': np.array(x_t)}
        dirty[side][1, 2, H // 3, W - 2] = bad
        got = _launch(gpu, dirty['x_s'], dirty['x_t'], b)
        assert not torch.isfinite(got[1, 2]).any()
        keep = torch.ones(3, C, dtype=torch.bool)
        keep[1, 2] = False
        assert _same(got[keep.to(gpu)], clean[keep.to(gpu)])
    finally:
        guarded.reset()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize('case', [(3, 17, 19, 2), (3, 64, 64, 5), (3, 128, 128, 32)], ids=lambda c: '%dx%d-b%d' % c[1:])
def test_same_bits_on_every_call_and_under_graph_replay(gpu, case):
    import mi355
    from mi355 import ops
    C, H, W, b = case
    x_s, x_t, want = _case(3, *case)
    d_s, d_t = torch.from_numpy(np.array(x_s)).to(gpu), torch.from_numpy(np.array(x_t)).to(gpu)
    beta = _beta(H, W, b)
    first = ops.fda_transfer(d_s, d_t, beta).clone()
    second = ops.fda_transfer(d_s, d_t, beta).clone()
    assert _same(first, second)
    _within(first, want, 'eager')
    out = torch.full_like(d_s, 7.0)
    ws = torch.empty(mi355.load().mi355_fda_workspace_bytes(3, C, H, W, b), dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fda_transfer(d_s, d_t, beta, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with mi355.no_gc_in_capture():
        with torch.cuda.graph(g):
            ops.fda_transfer(d_s, d_t, beta, out=out, ws=ws)
    for _ in range(2):
        out.fill_(7.0)
        ws.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, first)


# ---------------------------------------------------------------- the wrapper
def test_wrapper_refuses_what_the_kernels_do_not_take(gpu, monkeypatch):
    import mi355
    from mi355 import ops
    z = lambda *s: torch.zeros(s, device=gpu)
    x = z(2, 3, 16, 20)
    assert ops.fda_transfer(x, z(2, 3, 16, 20), 0.1).shape == x.shape
    for bad, word in ((dict(x_t=z(2, 3, 16, 24)), 'x_t'), (dict(x_t=z(2, 3, 16, 20).double()), 'x_t'), (dict(x_s=z(2, 3, 16, 40)[..., ::2]), 'x_s'),
                      (dict(x_t=z(2, 3, 16, 20).cpu()), 'CUDA'), (dict(x_s=z(3, 16, 20), x_t=z(3, 16, 20)), 'x_s'),
                      (dict(beta=0.5), 'b=8'), (dict(beta=-0.1), 'beta'), (dict(beta=float('nan')), 'beta'),
                      (dict(x_s=z(2, 5, 16, 20), x_t=z(2, 5, 16, 20), mean=(0.5,) * 5, std=(0.5,) * 5), 'C=5'),
                      (dict(std=(0.2, 0.0, 0.2)), r'std\[1\]'), (dict(mean=(0.2, 0.1, float('inf'))), r'mean\[2\]'), (dict(mean=(0.2, 0.1)), 'mean'),
                      (dict(out=z(2, 3, 16, 24)), 'out'), (dict(out=z(2, 3, 16, 20).double()), 'out'), (dict(out=x), 'out and x_s overlap'),
                      (dict(ws=torch.zeros(64, dtype=torch.uint8, device=gpu)), 'ws_bytes'), (dict(ws=z(4096)), 'ws')):
        kw = dict(dict(x_s=x, x_t=z(2, 3, 16, 20), beta=0.1), **bad)
        with pytest.raises(mi355.Mi355Error, match=word):
            ops.fda_transfer(kw.pop('x_s'), kw.pop('x_t'), kw.pop('beta'), **kw)
    x256 = z(1, 3, 256, 256)
    with pytest.raises(mi355.Mi355Error, match='b=51'):
        ops.fda_transfer(x256, z(1, 3, 256, 256), 0.2)
    # nothing is allocated while a graph is being captured: out and ws must come from the caller then
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(mi355.Mi355Error, match='during graph capture'):
        ops.fda_transfer(x, z(2, 3, 16, 20), 0.1)
    with pytest.raises(mi355.Mi355Error, match='during graph capture'):
        ops.fda_transfer(x, z(2, 3, 16, 20), 0.1, out=z(2, 3, 16, 20))
    from mi355.da_step import FourierStyle
    with pytest.raises(mi355.Mi355Error, match='during graph capture'):
        FourierStyle(0.1).stylise(dict(x_s=x, x_t=z(2, 3, 16, 20)))
    monkeypatch.undo()
    f = FourierStyle(0.1)
    a = f.stylise(dict(x_s=x, x_t=z(2, 3, 16, 20)))
    assert f.stylise(dict(x_s=x, x_t=z(2, 3, 16, 20))).data_ptr() == a.data_ptr()       # fixed addresses while the signature holds
    with pytest.raises(mi355.Mi355Error, match='b=8'):
        FourierStyle(0.5).stylise(dict(x_s=x, x_t=z(2, 3, 16, 20)))


def test_launches_are_logged_under_the_fda_labels(gpu):
    from mi355 import ops
    x_s, x_t, _ = _case(3, 3, 17, 19, 2)
    d_s, d_t = torch.from_numpy(np.array(x_s)).to(gpu), torch.from_numpy(np.array(x_t)).to(gpu)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        ops.fda_transfer(d_s, d_t, _beta(17, 19, 2))
        torch.cuda.synchronize()
        log = ops.prof_launches()
    finally:
        ops.prof_enable(0); ops.prof_reset()
    assert [e['family'] for e in log] == [2, 2]
    assert log[0]['label'].startswith('fda spectrum B3 C3 17x19 b2') and log[1]['label'].startswith('fda apply B3 C3 17x19 b2')


# ---------------------------------------------------------------- the step
BETA_STEP = 0.05                                                        # b = 3 on 64 x 64 images


def _training(gpu, fda='absent', mixup=False):
    """resnet18, 64 x 64 images, 16 x 16 heat-maps, fp32.  fda: 'absent' (the argument is not given), None or a FourierStyle."""
    import mi355
    from mi355.da_step import CrossDomainMixup, build_training
    from uda.model.regda_7 import PoseResNetx9
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('f32')
    model = _pose(gpu, PoseResNetx9, 731)
    kw = {} if isinstance(fda, str) else dict(fda=fda)
    step, opts, scheds = build_training(model, heatmap_size=16, **kw)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if mixup:
        step.mixup = CrossDomainMixup(beta=1.0, weight=0.5, seed=1)
    return model, step, scheds


def _batch(gpu):
    from utils.synthetic import make_batch
    return make_batch(2, 64, 16, seed=3, device=gpu)


def _host(model):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in model.state_dict().items()}


def _iterate(gpu, fda, batch, iters=4, capture_at=2, after_a=None):
    model, step, scheds = _training(gpu, fda)
    rec = []
    if after_a is not None:
        upd = step._update_A
        step._update_A = lambda: (upd(), torch.cuda.synchronize(), after_a.append(_host(model)))[0]
    for i in range(iters):
        if i == capture_at:
            if after_a is not None:
                del step._update_A                                      # (the spy synchronises: not inside a capture)
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        rec.append(dict(loss_s=_bits(out['loss_s']), y_s=_bits(out['y_s']), loss_gt=_bits(out['loss_gt']), y_t=_bits(out['y_t']), model=_host(model)))
    return rec, step


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


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    from mi355 import ops
    from mi355.da_step import FourierStyle
    try:
        batch = _batch(gpu)
        before = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        after_on, after_pre = [], []
        on, step_on = _iterate(gpu, FourierStyle(BETA_STEP), batch, after_a=after_on)
        untouched = all(_same(batch[k], v) for k, v in before.items()) and _same(step_on.static['x_s'], before['x_s'])
        styled = ops.fda_transfer(batch['x_s'], batch['x_t'], BETA_STEP)
        pre, _ = _iterate(gpu, 'absent', dict(batch, x_s=styled), after_a=after_pre)
        plain, _ = _iterate(gpu, 'absent', batch)
        none, _ = _iterate(gpu, None, batch)
        assert len(step_on.graphs) == 6
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(on=on, pre=pre, plain=plain, none=none, after_on=after_on, after_pre=after_pre, untouched=untouched,
                styled_differs=not _same(styled, batch['x_s']))


def test_step_a_on_the_stylised_batch_equals_a_step_fed_the_pre_stylised_batch(runs):
    """Iterations 0 and 1 are eager, 2 and 3 replays of the captured graphs: loss_s, y_s and every parameter, bit for bit."""
    on, pre = runs['on'], runs['pre']
    assert runs['styled_differs'] and len(on) == len(pre) == 4
    assert len(runs['after_on']) >= 2 and len(runs['after_on']) == len(runs['after_pre'])
    for a, b in zip(runs['after_on'], runs['after_pre']):             # the parameters right behind update A (the eager iterations)
        for k in a:
            assert _same(a[k], b[k]), k
    for it in range(4):
        assert on[it]['loss_s'] == pre[it]['loss_s'] and on[it]['y_s'] == pre[it]['y_s'], it
        for k in on[it]['model']:
            assert _same(on[it]['model'][k], pre[it]['model'][k]), (it, k)
    assert on[0]['loss_s'] != runs['plain'][0]['loss_s']                 # (and the stylised batch is not the batch)


def test_step_leaves_the_batch_as_it_was(runs):
    assert runs['untouched']


def test_step_without_fda_is_the_step_built_without_the_argument(runs):
    plain, none = runs['plain'], runs['none']
    for it in range(4):
        for k in ('loss_s', 'y_s', 'loss_gt', 'y_t'):
            assert plain[it][k] == none[it][k], (it, k)
        for k in plain[it]['model']:
            assert _same(plain[it]['model'][k], none[it]['model'][k]), (it, k)


def test_launch_log_has_two_fda_launches_when_on_and_none_when_off(gpu):
    import mi355
    from mi355.da_step import FourierStyle
    try:
        batch = _batch(gpu)
        model, step, scheds = _training(gpu, None)
        for _ in range(2):
            step.run(batch)
        off = _logged(step, batch)
        assert len(off) > 100 and not any('fda' in l for _, l in off)
        step.fda = FourierStyle(BETA_STEP)                               # assignable after construction
        step.run(batch)
        on = _logged(step, batch)
        fda = [l for _, l in on if 'fda' in l]
        assert len(fda) == 2 and fda[0].startswith('fda spectrum B2 C3 64x64 b3') and fda[1].startswith('fda apply B2 C3 64x64 b3')
        assert [l for l in on if 'fda' not in l[1]] == off                  # nothing else moved
        at = [i for i, (_, l) in enumerate(on) if 'fda' in l]
        assert at[1] == at[0] + 1 and not any(l.startswith('fwd') for _, l in on[:at[0]])      # at the head of step A's forward
    finally:
        mi355.set_compute_dtype('bf16')


def test_mixup_blends_the_unstylised_source(gpu):
    import mi355
    from mi355 import ops
    from mi355.da_step import FourierStyle
    try:
        batch = _batch(gpu)
        model, step, scheds = _training(gpu, FourierStyle(BETA_STEP), mixup=True)
        for _ in range(2):
            out = step.run(batch)
        torch.cuda.synchronize()
        assert float(out['loss_mix']) > 0
        x_mix = step.mixup._bufs[1][0]
        lam = step.mixup.lam.clone()
        want = ops.mixup_pairs(batch['x_s'], batch['label_s'], batch['w_s'], batch['x_t'], batch['label_s'].clone(), batch['w_t'], lam)[0]
        styled = ops.fda_transfer(batch['x_s'], batch['x_t'], BETA_STEP)
        other = ops.mixup_pairs(styled, batch['label_s'], batch['w_s'], batch['x_t'], batch['label_s'].clone(), batch['w_t'], lam)[0]
        assert _same(x_mix, want) and not _same(x_mix, other)
    finally:
        mi355.set_compute_dtype('bf16')


# ---------------------------------------------------------------- command lines
def test_train_cli_with_the_fda_switch(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(log, extra):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '2', '-p', '1', '-j', '0',
                  '--pretrain_epochs', '1', '--epochs', '1', '--pretrain', str(tmp_path / 'none.pth'), '--log', log]
        r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env,
                           capture_output=True, text=True, timeout=330)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [re.sub(r'(Time|Data) +\S+ +\( *\S+\)', '', l) for l in r.stdout.splitlines() if l.startswith('Epoch: [0]')]
        return lines[-2:]                                                # (the adaptation epoch; the pre-training one prints the same prefix)

    on = run(str(tmp_path / 'on'), ['--fda', 'on', '--fda-beta', '0.05'])
    off = run(str(tmp_path / 'off'), ['--fda', 'off'])
    none = run(str(tmp_path / 'none'), [])
    assert len(on) == len(off) == 2 and all('Loss (s)' in l for l in on + off)
    losses = [float(v) for l in on for v in re.findall(r'Loss \([^)]*\) +(\S+) ', l)]
    assert len(losses) >= 6 and all(np.isfinite(v) for v in losses)
    assert on != off and off == none
