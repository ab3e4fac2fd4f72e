"""Adaptive occlusion and teacher confidence without a GPU: the properties of the restatement of tests/occlude_ref.py, the
yardstick and the ceiling of mi355_peak_prob's p, the threshold clearance of every case, the command line, and the state of
mi355.teacher.KeypointOcclusion.

Ceiling of p (`peak_yardstick`, in the manner of `coord_yardstick` of tests/test_coord_cpu.py): 8 x the error of the float32 CPU
expression on the same inputs + 2^-23 max |ref|, both against float64.

The flags of mi355_teacher_select are discontinuous in p, so every case is built such that no map's float64 p lies within a
relative 1e-4 of the tau it is compared with; `test_no_case_sits_on_its_threshold` asserts that of the reference alone, for every
case the GPU tests use."""
import functools

import numpy as np
import pytest
import torch

import occlude_ref as R

PEAK_SIDES = ((64, 64), (32, 32), (16, 16), (24, 40))          # the last takes the loop form
PEAK_ROWS = (1, 4, 5, 21)
PEAK_BETAS = (1.0, 3.0)
PEAK_CASES = [(H, W, rows, beta) for (H, W) in PEAK_SIDES for rows in PEAK_ROWS for beta in PEAK_BETAS]


@functools.lru_cache(maxsize=None)
def peak_yardstick(H, W, rows, beta):
    """-> dict(hm float32 [rows, H, W], beta (the float32 value), idx, xy, ref (float64 p), yard, bound, tau): tau lies between two
    neighbours of the sorted p, for the chain peak_prob -> teacher_select."""
    hm = R.maps(H, W, rows)
    b32 = R.f32(beta)
    idx, xy, ref = R.peak_prob(hm, b32)
    p32 = R.peak_prob(hm, b32, dtype=np.float32)[2]
    assert np.isfinite(ref).all() and np.isfinite(p32).all()
    yard = float(np.abs(p32.astype(np.float64) - ref).max())
    return dict(hm=hm, beta=b32, idx=idx, xy=xy, ref=ref, yard=yard, bound=8.0 * yard + 2.0 ** -23 * float(np.abs(ref).max()),
                tau=R.tau_between(ref))


# ------------------------------------------------------------------------------------------------------------- peak_prob
def test_peak_of_a_perfect_label_and_of_a_flat_map():
    # the softmax of log(label) is the label: a normalised sigma = 2 Gaussian far from the border peaks at 1 / (8 pi)
    g = R.gaussian_label(64, 64, 31, 30)
    with np.errstate(divide='ignore'):
        hm = np.maximum(np.log(g), -80.0).astype(np.float32)[None]
    idx, xy, p = R.peak_prob(hm, 1.0)
    assert idx[0] == 30 * 64 + 31 and abs(p[0] - 1.0 / (8.0 * np.pi)) < 1e-6 * p[0] + 1e-7
    # its raw maximum is a logit, no confidence; a non-positive maximum gives the coordinates (0, 0), as mi355_argmax2d does
    assert hm.max() < 0 and xy[0].tolist() == [0.0, 0.0]
    for H, W in PEAK_SIDES:
        flat = np.full((2, H, W), -3.25, np.float32)
        idx, xy, p = R.peak_prob(flat, 1.0)
        assert idx.tolist() == [0, 0] and np.array_equal(p, np.full(2, 1.0 / (H * W)))


def test_peak_ties_nan_and_infinities():
    hm = R.maps(16, 16, 6)
    hm[0, 3, 4] = hm[0, 9, 1] = 50.0                              # a tie: the first index
    hm[1, 5, 5] = np.nan
    hm[2, 0, 7] = np.inf
    hm[3, 15, 15] = -np.inf
    hm[4, 2, 2] = np.nan; hm[4, 1, 1] = np.nan                    # two NaNs: the first
    idx, xy, p = R.peak_prob(hm, 1.0)
    assert idx[0] == 3 * 16 + 4 and idx[1] == 5 * 16 + 5 and idx[2] == 7 and idx[4] == 17
    assert xy[1].tolist() == [0.0, 0.0] and xy[2].tolist() == [7.0, 0.0]       # NaN > 0 is False; inf > 0 is True
    assert np.isnan(p[[1, 2, 3, 4]]).all() and np.isfinite(p[[0, 5]]).all()
    assert abs(p[0] - 0.5) < 1e-6                                  # two equal winners far above the rest
    # a NaN passes no threshold
    conf = R.teacher_select(p.astype(np.float32).reshape(1, 6), None, None, None, None, 0.0, 0.0, 0, 1, 1, 16, 16, 16)[0]
    assert conf.tolist() == [[1, 0, 0, 0, 0, 1]]


@pytest.mark.parametrize('case', PEAK_CASES, ids=lambda c: '%dx%d-rows%d-beta%g' % c)
def test_peak_yardstick_spreads_and_clears_its_threshold(case):
    y = peak_yardstick(*case)
    assert y['bound'] > 0 and y['yard'] <= 64 * 2.0 ** -24 * float(y['ref'].max())      # the float32 expression is a few ulp off
    assert R.tau_clear(y['ref'], y['tau'])
    if case[2] >= 4:
        passing = int((y['ref'] >= y['tau']).sum())
        assert 0 < passing < case[2]                               # some maps pass, some do not
        assert y['ref'].max() > 5 * y['ref'].min()                 # the peaks spread: the threshold separates unlike maps


# ---------------------------------------------------------------------------------------------------------- teacher_select
def _select(c):
    return R.teacher_select(c['p'], c['xy'], c['gate_in'], c['w_in'], c['u'], c['tau'], c['prob'], c['N'], c['lo'], c['hi'], c['S'], c['H'], c['W'])


@pytest.mark.parametrize('case', R.SELECT_CASES, ids=lambda c: 'B%d-K%d-N%d-%s-%s-g%d-%s-%s' % (c[0], c[1], c[2], c[3], c[4][0], c[5], c[6], c[7]))
def test_select_properties(case):
    B, K, N, mode, sides, gate, w, u_mode = case
    c = R.select_case(*case)
    assert R.tau_clear(c['p'].astype(np.float64), c['tau'])
    conf, w_out, boxes, count, stats = _select(c)
    ok = c['p'] >= np.float32(c['tau'])
    if gate:
        ok &= c['gate_in'] > 0
    assert np.array_equal(conf, ok.astype(np.float32))
    if w is not None:
        assert w_out.shape == c['w_in'].shape and np.array_equal(w_out.reshape(B, K), c['w_in'].reshape(B, K) * conf)
    else:
        assert w_out is None
    assert stats[1] == np.float32(ok.sum()) / np.float32(B * K)
    if N == 0:
        assert boxes is None and count is None and stats[0] == 0
        return
    cand = ok if w is None else ok & (c['w_in'].reshape(B, K) > 0)
    S, Hs = sides
    for b in range(B):
        m = int(cand[b].sum())
        want = 0 if c['u'][b, 0] >= np.float32(c['prob']) else min(N, m)
        assert count[b] == want
        assert not boxes[b, want:].any()                           # unused slots are (0, 0, 0, 0)
        cell = S // Hs
        for (x0, y0, x1, y1) in boxes[b, :want]:
            assert 0 <= x0 < x1 <= S and 0 <= y0 < y1 <= S          # inside the image, never empty
            assert x1 - x0 <= c['hi'] and y1 - y0 <= c['hi']
            # the box belongs to a candidate joint: it holds the centre of that joint's cell
            assert any(cand[b, k] and x0 <= int(c['xy'][b, k, 0]) * cell + cell // 2 < x1 and y0 <= int(c['xy'][b, k, 1]) * cell + cell // 2 < y1
                       for k in range(K))
    assert stats[0] == np.float32(int(count.sum())) / np.float32(B)
    if mode == 'none':
        assert not count.any() and not conf.any()
    if mode == 'equal':
        drawn = boxes[count > 0][:, 0]
        assert all(min(x1 - x0, y1 - y0) <= c['lo'] for x0, y0, x1, y1 in drawn)


def test_select_takes_distinct_joints_and_clips_in_the_corners():
    # eight boxes from 21 passing joints at distinct places: eight distinct joints
    c = R.select_case(3, 21, 8, 'corners', R.SIDES[0], False, None, 'rand')
    c['xy'] = np.stack([np.arange(21) * 3, np.arange(21) * 2], 1).astype(np.float32)[None].repeat(3, 0)
    c['lo'] = c['hi'] = 9
    c['u'][:, 0] = 0.0
    conf, _, boxes, count, _ = _select(c)
    assert conf.all() and count.tolist() == [8, 8, 8]
    for b in range(3):
        assert len({tuple(r) for r in boxes[b]}) == 8
    # the largest draw takes the last candidate and the largest side, the smallest the first and the smallest
    for u_mode, joint, side in (('max', 20, 128), ('zero', 0, 64)):
        c = R.select_case(1, 21, 1, 'corners', R.SIDES[0], False, None, u_mode)
        c['xy'] = np.stack([np.arange(21) * 3, np.arange(21) * 2], 1).astype(np.float32)[None]
        _, _, boxes, count, _ = _select(c)
        cx, cy = joint * 3 * 4 + 2, joint * 2 * 4 + 2
        want = (max(cx - side // 2, 0), max(cy - side // 2, 0), min(cx - side // 2 + side, 256), min(cy - side // 2 + side, 256))
        assert count[0] == 1 and tuple(boxes[0, 0]) == want
    # the four corners at 16 / 16: clipped on two sides each
    c = R.select_case(1, 21, 8, 'corners', R.SIDES[2], False, None, 'zero')
    _, _, boxes, count, _ = _select(c)
    assert count[0] == 8 and all((x0 == 0 or x1 == 16) and (y0 == 0 or y1 == 16) for x0, y0, x1, y1 in boxes[0])


def test_select_draw_at_the_largest_float_below_one_stays_in_range():
    for m in range(1, 65):
        t = R.U_MAX * np.float32(m)
        assert t < np.float32(m) and int(t) == m - 1                # the float32 product stays below m: the last candidate
        assert int(min(np.float32(1.0) * np.float32(m), np.float32(m - 1))) == m - 1      # a draw of 1.0 (outside the contract) is held by the minimum


# ---------------------------------------------------------------------------------------------------------- occlude_images
@pytest.mark.parametrize('shape', [(1, 3, 16, 16), (3, 3, 48, 48), (2, 1, 16, 20)], ids=str)
def test_occlude_restatement(shape):
    B, C, H, W = shape
    x = R.random_words(shape, seed=H + W)
    assert (x == 0x80000000).any() and (x == 0x7FC00001).any()
    for kind in ('empty', 'pixel', 'full', 'overlap', 'eight', 'wild'):
        boxes = R.image_boxes(B, H, W, kind)
        out = R.occlude_images(x, boxes)
        changed = out != x
        assert not out[changed].any()                              # what changed is +0.0
        if kind == 'empty':
            assert np.array_equal(out, x)
        elif kind == 'full':
            assert not out.any()
        elif kind == 'pixel':
            assert not out[:, :, H - 1, W - 1].any() and np.array_equal(out.reshape(B, C, -1)[:, :, :-1], x.reshape(B, C, -1)[:, :, :-1])
        else:
            # every channel of a pixel goes together; pixels outside every box keep every bit
            hit = np.zeros((B, H, W), bool)
            for b in range(B):
                for (x0, y0, x1, y1) in boxes[b].astype(np.int64):
                    hit[b, max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = True
            assert hit.any() and not hit.all()
            for ch in range(C):
                assert not out[:, ch][hit].any() and np.array_equal(out[:, ch][~hit], x[:, ch][~hit])
    f = x.view(np.float32)
    assert R.occlude_images(f, R.image_boxes(B, H, W, 'overlap')).dtype == np.float32


def test_no_case_sits_on_its_threshold():
    """Every (p, tau) pair the GPU tests compare: the peak cases with their own tau, and every select case."""
    n = 0
    for case in PEAK_CASES:
        y = peak_yardstick(*case)
        assert R.tau_clear(y['ref'], y['tau']), case
        n += 1
    for case in R.SELECT_CASES:
        c = R.select_case(*case)
        assert R.tau_clear(c['p'].astype(np.float64), c['tau']), case
        n += 1
    assert n == len(PEAK_CASES) + len(R.SELECT_CASES) and not R.tau_clear(np.array([0.5, 0.25 * (1 + 5e-5)]), 0.25)


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
    assert (a.occlude, a.occlude_p, a.occlude_n, list(a.occlude_size), a.teacher_conf, a.conf_beta) == ('off', 0.5, 1, [0.08, 0.16], 0.0, 1.0)
    ok = train1.build_parser().parse_args(BASE + ['--occlude', 'keypoint', '--ema-update', 'const', '--occlude-p', '0.25', '--occlude-n', '8',
                                                  '--occlude-size', '0.1', '0.2', '--teacher-conf', '0.02', '--conf-beta', '2'])
    assert (ok.occlude, ok.occlude_p, ok.occlude_n, list(ok.occlude_size), ok.teacher_conf, ok.conf_beta) == ('keypoint', 0.25, 8, [0.1, 0.2], 0.02, 2.0)
    for consumer in (['--mt-loss', 'on'], ['--coord-loss', 'both'], ['--mixup', 'on', '--mixup-labels', 'teacher'], ['--occlude', 'keypoint']):
        train1.build_parser().parse_args(BASE + ['--teacher-conf', '0.01', '--ema-update', 'warmup'] + consumer)
    err = _error(capsys, ['--occlude', 'keypoint'])
    assert '--occlude keypoint' in err and '--ema-update' in err
    err = _error(capsys, ['--teacher-conf', '0.01', '--ema-update', 'const'])
    assert '--mt-loss on' in err and '--coord-loss both' in err and '--mixup-labels teacher' in err and '--occlude keypoint' in err
    err = _error(capsys, ['--teacher-conf', '0.01', '--ema-update', 'const', '--mixup', 'on'])     # student labels: no teacher forward
    assert '--teacher-conf' in err
    on = ['--occlude', 'keypoint', '--ema-update', 'const']
    for bad, word in ((['--occlude-p', '-0.1'], '--occlude-p'), (['--occlude-p', '1.5'], '--occlude-p'), (['--occlude-p', 'nan'], '--occlude-p'),
                      (['--occlude-n', '0'], '--occlude-n'), (['--occlude-n', '9'], '--occlude-n'), (['--occlude-size', '0', '0.1'], '--occlude-size'),
                      (['--occlude-size', '0.2', '0.1'], '--occlude-size'), (['--occlude-size', '0.1', '1.5'], '--occlude-size'),
                      (['--teacher-conf', '-1'], '--teacher-conf'), (['--teacher-conf', 'inf'], '--teacher-conf'), (['--teacher-conf', 'nan'], '--teacher-conf'),
                      (['--conf-beta', '0'], '--conf-beta'), (['--conf-beta', 'inf'], '--conf-beta'), (['--image-size', '100'], '--image-size')):
        assert word in _error(capsys, on + bad), bad
    for flag in ('--occlude', '--occlude-p', '--occlude-n', '--occlude-size', '--teacher-conf', '--conf-beta'):
        text = [kw['help'] for flags, kw in train1._OPTIONS if flag in flags][0]
        assert 'placeholder' in text or flag == '--occlude'


# ---------------------------------------------------------------- KeypointOcclusion's state
def _occ(**kw):
    from mi355.teacher import KeypointOcclusion
    return KeypointOcclusion(**dict(dict(prob=0.5, n=3, size=(0.08, 0.16), beta=1.0, seed=3, rank=0), **kw))


def test_occlusion_draws_leave_the_global_generator_alone():
    o = _occ()
    torch.manual_seed(11)
    before = torch.get_rng_state().clone()
    for _ in range(20):
        u = o.draw(4, 'cpu')
        assert u.shape == (4, 7) and u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1
        assert torch.equal(o.u, u) and torch.equal(o.u_host, u)
    assert torch.equal(torch.get_rng_state(), before) and o.draws == 20
    assert _occ(n=0).draw(4, 'cpu') is None                        # the gate alone draws nothing
    assert o.sides(256) == (20, 41) and o.sides(16) == (1, 3) and _occ(size=(0.001, 0.002)).sides(64) == (1, 1)


def test_occlusion_state_round_trip_and_ranks():
    a = _occ()
    for _ in range(3):
        a.draw(4, 'cpu')
    state = a.state_dict()
    assert state['draws'] == 3 and torch.equal(state['u'], a.u_host)
    want = [a.draw(4, 'cpu').clone() for _ in range(3)]
    b = _occ()
    b.load_state_dict(state)
    assert b.draws == 3
    assert all(torch.equal(b.draw(4, 'cpu'), w) for w in want)
    other = _occ(rank=1)
    assert not torch.equal(other.draw(4, 'cpu'), _occ().draw(4, 'cpu'))                # ranks draw different boxes from the start
    other = _occ(rank=1)
    other.load_state_dict(state)                                                       # rank 0's checkpoint: the count, a state of its own
    assert other.draws == 3
    got = [other.draw(4, 'cpu').clone() for _ in range(3)]
    assert all(not torch.equal(g, w) for g, w in zip(got, want))
    again = _occ(rank=1)
    again.load_state_dict(state)
    assert all(torch.equal(again.draw(4, 'cpu'), g) for g in got)


class _Stub:
    """Stands for a model, an optimizer or a scheduler in utils.checkpoint: keeps what it is given."""

    def __init__(self, **state):
        self.state, self.gl_layer = dict(state), None

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, state, *a):
        self.state = dict(state)


def _checkpoint_objects(occlude):
    model, model_ema = _Stub(w=torch.ones(2)), _Stub(w=torch.zeros(2))
    model.gl_layer = _Stub()
    model.gl_layer.iter_num = 7
    keys = ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3')
    opts, scheds = {k: _Stub(state={}, param_groups=[]) for k in keys}, {k: _Stub(last_epoch=3) for k in keys}
    step = _Stub()
    step.occlude = occlude
    return model, model_ema, opts, scheds, step


def test_occlude_state_travels_in_the_checkpoint_and_old_checkpoints_load(tmp_path):
    from utils import checkpoint as ck
    assert 'occlude_state' in ck.OPTIONAL_KEYS and 'occlude_state' not in ck.REFERENCE_KEYS + ck.ADDITIVE_KEYS
    a = _occ()
    for _ in range(3):
        a.draw(4, 'cpu')
    model, model_ema, opts, scheds, step = _checkpoint_objects(a)
    saved = ck.training_state(0, None, model, opts, scheds, step, None)
    assert saved['occlude_state']['draws'] == 3 and set(ck.REFERENCE_KEYS) <= set(saved)
    want = [a.draw(4, 'cpu').clone() for _ in range(2)]
    # a run without the switch writes no such key
    assert 'occlude_state' not in ck.training_state(0, None, *_checkpoint_objects(None)[:1], opts, scheds, _checkpoint_objects(None)[4], None)
    # restored into fresh objects: the draws go on where the saved run was
    b = _occ()
    model2, ema2, opts2, scheds2, step2 = _checkpoint_objects(b)
    path = str(tmp_path / '0.pth')
    assert ck.apply_training_state(saved, path, None, model2, ema2, opts2, scheds2, step2, None, 'cpu') == 1
    assert b.draws == 3 and all(torch.equal(b.draw(4, 'cpu'), w) for w in want) and model2.gl_layer.iter_num == 7
    # a checkpoint from before the feature (no key) loads into a run that has the switch on, which then starts its draws afresh
    old = {k: v for k, v in saved.items() if k != 'occlude_state'}
    c = _occ()
    model3, ema3, opts3, scheds3, step3 = _checkpoint_objects(c)
    assert ck.apply_training_state(old, path, None, model3, ema3, opts3, scheds3, step3, None, 'cpu') == 1
    assert c.draws == 0 and torch.equal(c.draw(4, 'cpu'), _occ().draw(4, 'cpu'))
    # ... and a checkpoint with the key loads into a run that has it off
    model4, ema4, opts4, scheds4, step4 = _checkpoint_objects(None)
    assert ck.apply_training_state(saved, path, None, model4, ema4, opts4, scheds4, step4, None, 'cpu') == 1


def test_occlusion_state_from_other_ranges_is_loaded_with_a_warning():
    import warnings
    a = _occ()
    a.draw(4, 'cpu')
    state = a.state_dict()
    assert state['ranges'] == (0.5, 3, (0.08, 0.16), 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _occ().load_state_dict(state)                              # the same ranges: silent
        _occ().load_state_dict({k: v for k, v in state.items() if k != 'ranges'})
    for other in (dict(n=2), dict(size=(0.08, 0.2)), dict(prob=0.25), dict(beta=2.0)):
        with pytest.warns(UserWarning, match='KeypointOcclusion'):
            o = _occ(**other)
            o.load_state_dict(state)
        assert o.draws == 1


def test_occlusion_refuses_bad_ranges():
    for bad in (dict(prob=-0.1), dict(prob=1.5), dict(prob=float('nan')), dict(n=-1), dict(n=9), dict(n=1.5), dict(size=(0.0, 0.1)),
                dict(size=(0.2, 0.1)), dict(size=(0.1, 1.5)), dict(size=(0.1, float('nan'))), dict(beta=0.0), dict(beta=float('inf'))):
        with pytest.raises(ValueError):
            _occ(**bad)
    from mi355.da_step import DAStep
    import inspect
    sig = inspect.signature(DAStep.__init__).parameters
    assert sig['occlude'].default is None and sig['teacher_conf'].default == 0.0


def test_ops_have_no_cpu_fallback_and_name_their_arguments():
    import mi355
    from mi355 import ops
    from uda.model.loss import peak_confidence
    with pytest.raises(mi355.Mi355Error):
        ops.peak_prob(torch.zeros(1, 2, 8, 8))
    with pytest.raises(mi355.Mi355Error):
        ops.occlude_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 4, dtype=torch.int32))
    with pytest.raises(mi355.Mi355Error):
        ops.teacher_select(torch.zeros(1, 2))
    with pytest.raises(mi355.Mi355Error):
        peak_confidence(torch.zeros(1, 2, 8, 8))
    # the C ABI refuses before any launch (safe without a GPU), naming the argument
    lib = mi355.load()
    one = 16                                                       # any non-null, 4-byte-aligned value: nothing is dereferenced
    for args, word in (((0, 1.0, one, one, one, 1, 4, 4, 0), 'hm'), ((one, 1.0, 0, one, one, 1, 4, 4, 0), 'idx'), ((one, 1.0, one, one, 0, 1, 4, 4, 0), 'null p'),
                       ((one, float('nan'), one, one, one, 1, 4, 4, 0), 'beta'), ((one, float('inf'), one, one, one, 1, 4, 4, 0), 'beta'),
                       ((one, 1.0, one, one, one, 0, 4, 4, 0), 'rows'), ((one + 2, 1.0, one, one, one, 1, 4, 4, 0), 'aligned')):
        assert lib.mi355_peak_prob(*args) == -1 and word in lib.mi355_last_error().decode(), (args, lib.mi355_last_error())
    good = dict(p=one, xy=one, gate=0, w_in=0, u=one, tau=0.1, prob=0.5, N=1, lo=2, hi=4, S=16, H=4, W=4, conf=one, w_out=0, boxes=one, count=one,
                stats=0, B=1, K=2, stream=0)
    for change, word in ((dict(p=0), 'null p'), (dict(conf=0), 'conf'), (dict(xy=0), 'xy'), (dict(u=0), 'null u'), (dict(boxes=0), 'boxes'),
                         (dict(count=0), 'count'), (dict(w_in=one), 'w_in'), (dict(N=9), 'N=9'), (dict(N=-1), 'N=-1'), (dict(lo=5), 'lo=5'),
                         (dict(lo=0), 'lo=0'), (dict(hi=17), 'hi=17'), (dict(prob=1.5), 'prob'), (dict(prob=-0.1), 'prob'), (dict(prob=float('nan')), 'prob'),
                         (dict(tau=float('nan')), 'tau'), (dict(tau=float('inf')), 'tau'), (dict(S=18), 'multiple'), (dict(H=5), 'multiple'),
                         (dict(K=65), 'K=65'), (dict(B=0), 'B=0')):
        rc = lib.mi355_teacher_select(*dict(good, **change).values())
        assert rc == -1 and word in lib.mi355_last_error().decode() and 'teacher_select' in lib.mi355_last_error().decode(), (change, lib.mi355_last_error())
    good = dict(x=4096, boxes=64, N=1, out=1 << 20, B=1, C=3, H=8, W=8, stream=0)
    for change, word in ((dict(x=0), 'null x'), (dict(out=0), 'null out'), (dict(boxes=0), 'boxes'), (dict(N=9), 'N=9'), (dict(B=0), 'B=0'),
                         (dict(W=0), 'W=0'), (dict(H=5000), 'H=5000'), (dict(out=4096 + 64), 'overlap'), (dict(x=4098), 'aligned'),
                         (dict(boxes=1 << 20), 'overlap')):
        rc = lib.mi355_occlude_images(*dict(good, **change).values())
        assert rc == -1 and word in lib.mi355_last_error().decode() and 'occlude_images' in lib.mi355_last_error().decode(), (change, lib.mi355_last_error())
