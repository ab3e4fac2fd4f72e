"""The float64 reference of the bone-ratio prior, its statistics and the soft-arg-max backward (tests/bone_ref.py) is pinned here,
on the CPU, so that a wrong reference cannot pass a wrong kernel: closed-form gradients against torch.autograd, invariance under a
similarity transform, the selection rules, the first-batch and blend rules of the statistics, and the exact cases.

This module also owns the yardsticks of tests/test_gpu_bone.py.  `backward_yardstick`: the inputs, the float64 reference and the
ceiling of tests/test_coord_cpu.py (8 x the float32 CPU expression's error on the same inputs + 2^-23 max |ref|).
`bone_yardstick`: per element 2^-23 |ref| + 2^-40 x the largest |ref| of the sample -- one float32 rounding at the store, and
fewer than 2^8 float64 operations (2^-53 each) behind every value, with a margin of 16.

Also here: the --bone-* command line, batch['kp_s'] with --bone-loss alone and the bone_state round trip."""
import functools

import numpy as np
import pytest
import torch

import bone_ref as R
import coord_ref as C
from test_coord_cpu import ROWS, SIDES

torch.set_num_threads(8)

BWD_CASES = [(H, W, rows, beta) for (H, W) in SIDES for rows in ROWS for beta in (1.0, 100.0)]
# (B, table, weights case, margin, unseen bones)
BONE_CASES = [(B, table, wcase, margin, unseen) for B in (1, 3, 5) for table in ('hand', 'chain') for wcase in ('all', 'invisible', 'onebone')
              for margin in (0.0, 1.0) for unseen in ((), (1,))]
TABLES = {'hand': (R.HAND, 21), 'chain': (R.CHAIN, 4)}


def upstream(rows, seed=0):
    """[rows, 2] float32 upstream gradients of either sign; row 2 (where there is one) is exactly zero: a skipped row."""
    g = torch.Generator().manual_seed(4400 + rows + seed)
    out = (torch.randn(rows, 2, generator=g, dtype=torch.float64) * 0.1).float()
    if rows > 2:
        out[2] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def backward_yardstick(H, W, rows, beta):
    pred = C.maps(H, W, rows, beta)
    g_uv = upstream(rows, seed=H)
    b32 = C.f32(beta)
    ref = R.softargmax_backward(pred, g_uv, b32)
    o32 = R.softargmax_backward(pred, g_uv, b32, dtype=torch.float32)
    assert torch.isfinite(ref).all() and torch.isfinite(o32).all()
    yard = float((o32.double() - ref).abs().max())
    return dict(pred=pred, g_uv=g_uv, ref=ref, yard=yard, bound=8.0 * yard + 2.0 ** -23 * float(ref.abs().max()))


def bone_bound(ref):
    """Elementwise ceiling for a float64 reference [B, ...]: 2^-23 |ref| + 2^-40 x the largest |ref| of the sample."""
    ref = np.asarray(ref, np.float64)
    top = np.abs(ref.reshape(ref.shape[0], -1)).max(1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * top


@functools.lru_cache(maxsize=None)
def bone_yardstick(B, table, wcase, margin, unseen, collapsed=False):
    bones, K = TABLES[table]
    uv = R.hands(B, K, seed=len(unseen))
    if collapsed:                                    # every joint of the last sample on one point: S == 0, skipped
        uv[B - 1] = uv[B - 1, 0]
    w = R.weights_case(B, K, bones, wcase)
    mean, var, seen = R.stats_for(bones, unseen=unseen)
    coef = R.f32(R.f32(0.7) / B)
    rows, g = R.bone_prior(uv, w, bones, mean, var, seen, margin, 1e-4, coef)
    assert np.isfinite(rows).all() and np.isfinite(g).all()
    return dict(bones=bones, K=K, uv=uv, w=w, mean=mean, var=var, seen=seen, margin=margin, eps=1e-4, coef=coef, ref_rows=rows, ref_grad=g,
                bound_rows=bone_bound(rows), bound_grad=bone_bound(g))


# ------------------------------------------------------------------------------------------------------------------- pins
def test_softargmax_backward_closed_form_equals_autograd():
    for (H, W, rows, beta) in [(16, 16, 5, 1.0), (24, 20, 4, 1.0), (6, 10, 5, 100.0), (64, 64, 2, 1.0)]:
        pred, g_uv = C.maps(H, W, rows, beta), upstream(rows)
        z = pred.double().clone().requires_grad_(True)
        uv = R.softargmax(z, beta)
        (uv * g_uv.double()).sum().backward()
        closed = R.softargmax_backward(pred, g_uv, beta)
        assert float(z.grad.abs().max()) > 1e-6
        assert float((z.grad - closed).abs().max()) <= 1e-10 * float(z.grad.abs().max())
        # the forward is the coordinate reference's soft-arg-max
        assert torch.equal(uv.detach(), C.coord(pred, torch.zeros(rows, 2), None, beta, 1.0, 1.0)[2])


def test_softargmax_backward_zero_row_is_selected_out_and_a_nan_stays_in_its_row():
    pred, g_uv = C.maps(6, 10, 4, 1.0), upstream(4)
    pred[2, 1, 1] = float('nan')                                          # row 2 has a zero upstream gradient
    out = R.softargmax_backward(pred, g_uv, 1.0)
    assert bool((out[2] == 0).all()) and torch.isfinite(out).all()
    pred[1, 0, 0] = float('nan')
    out = R.softargmax_backward(pred, g_uv, 1.0)
    assert bool(torch.isnan(out[1]).all()) and torch.isfinite(out[[0, 2, 3]]).all()


@pytest.mark.parametrize('margin', [0.0, 1.0])
def test_bone_closed_form_gradient_equals_autograd(margin):
    for table, B, wcase, unseen in (('hand', 5, 'invisible', (3,)), ('hand', 3, 'onebone', ()), ('chain', 4, 'all', ())):
        bones, K = TABLES[table]
        uv = R.hands(B, K, seed=11)
        w = R.weights_case(B, K, bones, wcase)
        mean, var, seen = R.stats_for(bones, unseen=unseen)
        rows, g = R.bone_prior(uv, w, bones, mean, var, seen, margin, 1e-4, 0.37)
        t = torch.from_numpy(uv).double().requires_grad_(True)
        rows_t = R.bone_prior_torch(t, torch.from_numpy(w), bones, mean, var, seen, R.f32(margin), R.f32(1e-4))
        (R.f32(0.37) * rows_t.sum()).backward()
        assert float(t.grad.abs().max()) > 1e-4                          # (not a comparison of zeros)
        assert np.abs(rows - rows_t.detach().numpy()).max() <= 1e-12 * max(np.abs(rows).max(), 1.0)
        assert np.abs(g - t.grad.numpy()).max() <= 1e-10 * float(t.grad.abs().max()), (table, margin)
        if wcase == 'onebone':
            assert rows[0] == 0 and not g[0].any()


def test_bone_loss_is_invariant_under_a_similarity_transform():
    bones, K = TABLES['hand']
    uv = R.hands(4, K, seed=5).astype(np.float64)
    w = R.weights_case(4, K, bones, 'invisible')
    mean, var, seen = R.stats_for(bones, unseen=(7,))
    a = 0.7
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    moved = 1.7 * uv @ rot.T + 3.0
    t0 = R.bone_prior_torch(torch.from_numpy(uv), torch.from_numpy(w), bones, mean, var, seen, 0.5, 1e-4)
    t1 = R.bone_prior_torch(torch.from_numpy(moved), torch.from_numpy(w), bones, mean, var, seen, 0.5, 1e-4)
    assert float(t0.min()) > 0 and float((t0 - t1).abs().max()) <= 1e-12 * float(t0.max())


def test_bone_selection_rules():
    bones, K = TABLES['chain']
    mean, var, seen = np.full(3, 0.5, np.float32), np.full(3, 0.01, np.float32), np.ones(3, np.int32)
    uv = np.array([[[0, 0], [3, 4], [3, 4], [9, 12]],            # bone 1 has length 0: it counts (r = 0) but gets no gradient
                   [[5, 5], [5, 5], [5, 5], [5, 5]],             # collapsed: S == 0, skipped
                   [[0, 0], [3, 4], [6, 8], [9, 12]]], np.float32)
    rows, g = R.bone_prior(uv, None, bones, mean, var, seen, 0.0, 1e-4, 1.0)
    assert rows[0] > 0 and rows[1] == 0 and not g[1].any() and np.isfinite(g).all()
    assert np.array_equal(g[0, 1] + g[0, 2], -(g[0, 0] + g[0, 3]))       # bone (1, 2) moved nothing: its two joints carry the others' sum
    # an unseen bone is absent: the sample with one present bone left is skipped
    rows2, g2 = R.bone_prior(uv[2:], None, bones, mean, var, np.array([1, 0, 0], np.int32), 0.0, 1e-4, 1.0)
    assert rows2[0] == 0 and not g2.any()
    # ... and with two left it is the two-bone result, whatever the unseen bone's statistics hold
    m2, v2 = mean.copy(), var.copy()
    m2[1], v2[1] = np.nan, np.nan
    rows3, g3 = R.bone_prior(uv[2:], None, bones, m2, v2, np.array([1, 0, 1], np.int32), 0.0, 1e-4, 1.0)
    assert np.isfinite(rows3).all() and np.isfinite(g3).all() and rows3[0] > 0
    # a NaN coordinate of a present bone stays in its sample
    bad = uv.copy()
    bad[0, 3, 0] = np.nan
    rows4, g4 = R.bone_prior(bad, None, bones, mean, var, seen, 0.0, 1e-4, 1.0)
    assert np.isnan(rows4[0]) and np.isnan(g4[0]).any() and np.array_equal(rows4[1:], rows[1:]) and np.array_equal(g4[1:], g[1:])
    # an invisible joint takes its bones with it, NaN coordinates included
    rows5, g5 = R.bone_prior(bad, np.array([[1, 1, 1, 0]] * 3, np.float32), bones, mean, var, seen, 0.0, 1e-4, 1.0)
    assert np.isfinite(rows5).all() and np.isfinite(g5).all() and not g5[:, 3].any()


@pytest.mark.parametrize('name', R.EXACT)
def test_exact_cases_hold_bit_for_bit(name):
    e = R.exact_case(name)
    rows, g = R.bone_prior(e['uv'], None, e['bones'], e['mean'], e['var'], e['seen'], e['margin'], e['eps'], 1.0)
    assert np.float32(rows[0]).tobytes() == e['loss'].tobytes() and rows[0] == float(e['loss'])
    assert (name == 'inside') == (not g.any())
    np.testing.assert_array_equal(g.sum(1), 0.0) if name == 'inside' else None


def test_statistics_first_batch_blend_and_untouched_bone():
    bones, K = TABLES['chain']
    kp = np.array([[[0, 0], [3, 4], [6, 8], [12, 16]],             # lengths 5, 5, 10: lbar 20/3, r = .75, .75, 1.5
                   [[0, 0], [6, 8], [9, 12], [12, 16]]], np.float32)  # lengths 10, 5, 5: r = 1.5, .75, .75
    w = np.array([[1, 1, 1, 1], [1, 1, 1, 1]], np.float32)
    mean, var, seen = R.bone_stats_update(kp, w, bones, np.zeros(3), np.zeros(3), np.zeros(3), 0.25)
    assert seen.tolist() == [1, 1, 1]
    np.testing.assert_allclose(mean, [1.125, 0.75, 1.125], rtol=1e-7)
    np.testing.assert_allclose(var, [0.375 ** 2, 0.0, 0.375 ** 2], rtol=1e-6, atol=1e-15)
    # second batch: joint 3 invisible everywhere -> bone 2 is not touched, the others blend with rho
    w2 = np.array([[1, 1, 1, 0], [1, 1, 1, 0]], np.float32)
    mean2, var2, seen2 = R.bone_stats_update(kp, w2, bones, mean, var, seen, 0.25)
    assert mean2[2] == mean[2] and var2[2] == var[2] and seen2.tolist() == [1, 1, 1]
    # with two bones left: r = (1, 1) and (4/3, 2/3): batch mean (7/6, 5/6), variance 1/36 each
    np.testing.assert_allclose(mean2[:2], [0.75 * 1.125 + 0.25 * 7 / 6, 0.75 * 0.75 + 0.25 * 5 / 6], rtol=1e-6)
    np.testing.assert_allclose(var2[:2], [0.75 * 0.375 ** 2 + 0.25 / 36, 0.25 / 36], rtol=1e-6)
    # a skipped sample (one bone) is left out; a bone nobody shows stays unseen; presence ignores `seen`
    w3 = np.array([[1, 1, 0, 0], [1, 1, 1, 0]], np.float32)
    mean3, var3, seen3 = R.bone_stats_update(kp, w3, bones, np.zeros(3), np.zeros(3), np.zeros(3), 0.25)
    assert seen3.tolist() == [1, 1, 0] and mean3[2] == 0 and var3.tolist() == [0, 0, 0]
    np.testing.assert_allclose(mean3[:2], [4 / 3, 2 / 3], rtol=1e-6)


@pytest.mark.parametrize('case', BWD_CASES, ids=lambda c: '%dx%d-r%d-b%g' % c)
def test_yardstick_of_every_backward_case(case):
    y = backward_yardstick(*case)
    top = float(y['ref'].abs().max())
    assert y['bound'] > 0 and top > 1e-6 and y['bound'] < 1e-3 * top
    if case[2] > 2:
        assert not y['ref'][2].any()


@pytest.mark.parametrize('case', BONE_CASES, ids=lambda c: 'B%d-%s-%s-m%g-u%d' % (c[0], c[1], c[2], c[3], len(c[4])))
def test_yardstick_of_every_bone_case(case):
    for collapsed in (False, True):
        y = bone_yardstick(*case, collapsed=collapsed)
        B = case[0]
        live = [b for b in range(B) if y['ref_rows'][b] != 0]
        if case[2] == 'onebone':
            assert 0 not in live and not y['ref_grad'][0].any()
        if collapsed:
            assert B - 1 not in live and not y['ref_grad'][B - 1].any()
        if B > 2 and not (case[1] == 'chain' and case[2] == 'invisible' and case[4]):      # (that one leaves a single bone: all skipped)
            assert live and np.abs(y['ref_grad']).max() > 1e-6               # (not a comparison of zeros)
        assert (y['bound_grad'] <= 2.0 ** -22 * np.abs(y['ref_grad']).max() + 1e-300).all()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_hand_bones_is_the_table_of_the_specification():
    from uda.model.loss import HAND_BONES
    assert HAND_BONES == R.HAND and len(HAND_BONES) == 20
    assert HAND_BONES[:5] == ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5)) and HAND_BONES[-1] == (19, 20)


def test_bone_flags_parse_and_default_to_off():
    import inspect
    import train1
    from mi355.da_step import DAStep, KinematicPrior
    a = train1.build_parser().parse_args(['d'])
    assert (a.bone_loss, a.bone_weight, a.bone_margin, a.bone_momentum, a.bone_beta, a.bone_eps) == ('off', 1.0, 1.0, 0.01, 1.0, 1e-4)
    assert train1.bone_term(a) is None and not train1.wants_keypoints(a)
    p = inspect.signature(DAStep.__init__).parameters
    assert 'bone' in p and p['bone'].default is None
    b = train1.build_parser().parse_args(['d', '--bone-loss', 'on', '--bone-weight', '0.5', '--bone-margin', '0', '--bone-momentum', '0.1',
                                          '--bone-beta', '2', '--bone-eps', '0.001'])
    t = train1.bone_term(b)
    assert isinstance(t, KinematicPrior) and (t.key, t.needs_head_graph) == ('bone', True)
    assert (t.weight, t.crit.margin, t.stats.momentum, t.crit.beta, t.crit.eps) == (0.5, 0.0, 0.1, 2.0, 0.001)
    assert t.stats.bones == R.HAND and t.stats.table is None                # nothing is allocated before the first batch
    for flag in ('--bone-weight', '--bone-margin', '--bone-momentum', '--bone-beta', '--bone-eps'):      # placeholders, and said so
        assert 'placeholder' in [kw for flags, kw in train1._OPTIONS if flag in flags][0]['help']
    for bad in (['--bone-weight', '0'], ['--bone-margin', '-1'], ['--bone-momentum', '1.5'], ['--bone-beta', '0'], ['--bone-eps', '0']):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--bone-loss', 'on'] + bad)


def test_key_points_reach_the_batch_when_only_the_bone_switch_is_on():
    """train(): batch['kp_s'] is built for --bone-loss on without --coord-loss, and not with both switches off."""
    import types
    import train1
    from utils.synthetic_dataset import SyntheticHand21

    class Stop(Exception):
        pass

    def first_batch(bone):
        seen = {}

        def run(batch):
            seen.update(batch)
            raise Stop

        step = types.SimpleNamespace(mt=None, mixup=None, coord=None, bone=bone, clip=None, graphs=None, terms=lambda: [], run=run)
        ds = SyntheticHand21(4, (64, 64), (16, 16))
        items = [ds[i] for i in range(2)]
        pack = (torch.stack([i[0] for i in items]), torch.stack([i[1] for i in items]), torch.stack([i[2] for i in items]),
                {'keypoint2d': torch.stack([i[3]['keypoint2d'] for i in items])})
        args = types.SimpleNamespace(iters_per_epoch=1, image_size=64, heatmap_size=16, synthetic=True, no_graph=True, print_freq=1, batch_size=2)
        with pytest.raises(Stop):
            train1.train(iter([pack]), iter([pack]), step, {}, 0, args)
        return seen

    on = first_batch(object())
    assert torch.equal(on['kp_s'].cpu(), on['kp_s'].cpu()) and tuple(on['kp_s'].shape) == (2, 21, 2) and on['kp_s'].dtype == torch.float32
    assert 'kp_s' not in first_batch(None)
    a = train1.build_parser().parse_args(['d', '--bone-loss', 'on'])
    assert a.coord_loss == 'off' and train1.wants_keypoints(a)


def test_bone_state_round_trip(tmp_path):
    from mi355.da_step import KinematicPrior
    from uda.model.loss import BoneStatistics
    from utils import checkpoint as C2
    assert 'bone_state' in C2.OPTIONAL_KEYS
    s = BoneStatistics(R.CHAIN, 0.25, device='cpu')
    assert s.state_dict()['seen'].tolist() == [0, 0, 0]
    s.mean.copy_(torch.tensor([1.0, 2.0, 3.0])); s.var.copy_(torch.tensor([0.1, 0.2, 0.3])); s.seen.copy_(torch.tensor([1, 0, 1]))
    state = s.state_dict()
    torch.save(state, str(tmp_path / 's.pth'))
    state = torch.load(str(tmp_path / 's.pth'))
    addr = None
    for early in (True, False):                       # loaded before and after the buffers exist
        t = BoneStatistics(R.CHAIN, 0.25)
        if not early:
            t.to('cpu')
            addr = t.mean.data_ptr()
        t.load_state_dict(state)
        assert (t.table is None) == early
        assert t.state_dict()['mean'].tolist() == [1.0, 2.0, 3.0]
        t.to('cpu')
        assert torch.equal(t.mean, s.mean) and torch.equal(t.var, s.var) and torch.equal(t.seen, s.seen) and t.seen.dtype == torch.int32
        if not early:
            assert t.mean.data_ptr() == addr               # in place: a captured graph keeps the address
    with pytest.raises(ValueError, match='bones'):
        BoneStatistics(R.HAND).load_state_dict(state)
    # the term hands its statistics to the checkpoint and takes them back
    k = KinematicPrior(bones=R.CHAIN)
    step = type('S', (), {'bone': k, 'proto': None, 'mixup': None, 'view': None})()
    k.load_state_dict(state)
    assert k.state_dict()['var'].tolist() == pytest.approx([0.1, 0.2, 0.3])
    fresh = KinematicPrior(bones=R.CHAIN)
    assert fresh.state_dict()['mean'] is None
    fresh.load_state_dict({'mean': None, 'var': None, 'seen': None})
    assert fresh.state_dict()['mean'] is None and step.bone is k
