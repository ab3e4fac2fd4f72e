"""Prototype alignment, CPU side: the fixture tests/golden/g16_proto.npz (the reference's own lossx / lossx3 over three
consecutive calls and torch autograd, written by make_golden_proto.py) is what its generator describes; the restatement of
tests/proto_ref.py equals it in float64 over all three calls -- the (1 - m) * memory term is 1e-3 of a prototype, far above that
tolerance, so the memory path is pinned by the reference itself; the tolerance rule of the GPU tests on the fixture; the closed-form
gradients agree with central differences; the zero-sum-source rule, empty windows and the exact-order models; the
surface of lossx / lossx3 (reset / updata round trip) without a GPU; the command line has the five new switches; the four entry
points are in the ctypes table and refuse bad arguments before any launch."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG, golden
import proto_ref

CASES = ['a', 'b']
CLASSES = {'x': 'kl', 'x3': 'softkl'}


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_fixture_is_what_the_generator_describes():
    g = golden('g16_proto')
    for c, B in (('a', 2), ('b', 1)):
        calls = proto_ref.fixture_calls(g, c)
        assert len(calls) == 3
        for i, (f1, f2, pre1, pre2) in enumerate(calls):
            assert f1.shape == f2.shape == (B, 8, 64, 64) and pre1.shape == pre2.shape == (B, 21, 2) and pre1.dtype == np.float32
            for f in (f1, f2):
                assert f.dtype == np.float32 and f.min() >= 0 and f.max() < 2 and np.array_equal(f * 4, np.round(f * 4))      # dyadic
            assert min(pre1.min(), pre2.min()) >= 0 and max(pre1.max(), pre2.max()) <= 63
            assert not np.array_equal(pre1, pre2)                                           # different joint orders on the two sides
            win = proto_ref.windows(pre2, 64, 64)
            for b in range(B):                                                              # source: positive somewhere in every window
                for r0, r1, q0, q1 in win[b]:
                    assert r1 > r0 and q1 > q0 and f2[b, :, r0:r1, q0:q1].max() > 0
            for k in CLASSES:
                r32, r64 = proto_ref.fixture_results(g, c, k, i), proto_ref.fixture_results(g, c, k, i, '_64')
                assert r32['loss'].dtype == np.float32 and r64['loss'].dtype == np.float64 and float(r64['loss']) > 0
                assert r32['grad_f1'].shape == f1.shape and r64['grad_f2'].shape == f2.shape and r64['val1'].shape == (21, 8)
                assert all(np.isfinite(v).all() for v in list(r32.values()) + list(r64.values()))
                assert np.abs(r64['grad_f1']).max() > 0 and np.abs(r64['grad_f2']).max() > 0 and r64['val2'].sum(-1).min() > 0
        if c == 'a':
            pts = [tuple(p) for p in calls[0][2][0].tolist()]
            assert {(0., 0.), (63., 63.), (0., 63.), (63., 0.), (5., 30.), (58., 30.), (30., 5.), (30., 58.)} <= set(pts)
            assert pts.count((20., 33.)) == 3 and pts.count((0., 0.)) == 3 and any(p[0] != int(p[0]) for p in pts)
            assert not np.array_equal(calls[0][2], calls[1][2])                             # fresh operands per call
        else:
            assert np.any(calls[0][2] != np.round(calls[0][2]))                             # random non-integer key points
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_proto.npz')) < 1 << 20


def run_ref(g, case, cls, dtype, **kw):
    crit = proto_ref.Loss(CLASSES[cls], dtype=dtype, **kw)
    return [crit(*call) for call in proto_ref.fixture_calls(g, case)]


@pytest.mark.parametrize('cls', sorted(CLASSES))
@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_the_reference_in_float64_over_three_calls(case, cls):
    g = golden('g16_proto')
    for i, got in enumerate(run_ref(g, case, cls, np.float64)):
        want = proto_ref.fixture_results(g, case, cls, i, '_64')
        for k in proto_ref.KEYS:
            assert np.abs(np.asarray(got[k]) - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), (i, k)
    # the memory term is what the tolerance sees: without it (a fresh instance per call) calls two and three are 1e-3 off
    fresh = proto_ref.Loss(CLASSES[cls])(*proto_ref.fixture_calls(g, case)[1])
    want = proto_ref.fixture_results(g, case, cls, 1, '_64')
    assert np.abs(fresh['val1'] - want['val1']).max() > 1e-4 * np.abs(want['val1']).max()
    # and a swapped axis shows
    other = proto_ref.Loss(CLASSES[cls], axes='xy')(*proto_ref.fixture_calls(g, case)[0])
    assert np.abs(other['val1'] - proto_ref.fixture_results(g, case, cls, 0, '_64')['val1']).max() > 1e-3


@pytest.mark.parametrize('cls', sorted(CLASSES))
@pytest.mark.parametrize('case', CASES)
def test_tolerance_rule_on_the_fixture(case, cls):
    """The bound of the GPU tests over all three calls: 4 times the reference's own float32 distance from its float64 run, or the
    floor of jfa_ref where that is larger; the figures are printed.  On the loss the reference's own distance is below the floor."""
    g = golden('g16_proto')
    floors = dict(loss=proto_ref.LOSS_FLOOR, grad_f1=proto_ref.GRAD_FLOOR, grad_f2=proto_ref.GRAD_FLOOR, val1=proto_ref.PROTO_FLOOR,
                  val2=proto_ref.PROTO_FLOOR)
    for i in range(3):
        r32, r64 = proto_ref.fixture_results(g, case, cls, i), proto_ref.fixture_results(g, case, cls, i, '_64')
        own, bound = proto_ref.bounds(r32, r64)
        for k in proto_ref.KEYS:
            scale = float(np.abs(r64[k]).max())
            print('%s %s call %d %-8s reference fp32 - fp64 %.3e = %.3e of max, floor %.1e, bound %.3e' % (case, cls, i, k, own[k], own[k] / scale, floors[k], bound[k]))
            assert bound[k] == max(4 * own[k], floors[k] * scale) and bound[k] < 1e-4 * scale, (i, k)
        assert own['loss'] <= proto_ref.LOSS_FLOOR * abs(float(r64['loss']))


@pytest.mark.parametrize('mode', ['kl', 'softkl'])
def test_closed_form_gradients_agree_with_central_differences(mode):
    """At m = 0.5 with a non-zero memory, radius 3, a non-square map, both axes."""
    rng = np.random.default_rng(5)
    B, C, H, W, K = 2, 8, 12, 10, 3
    f1, f2 = rng.random((B, C, H, W)), rng.random((B, C, H, W)) + 0.1
    pre1, pre2 = rng.random((B, K, 2)) * 9, rng.random((B, K, 2)) * 9
    mem = rng.random((K, C)), rng.random((K, C))
    for axes in ('ref', 'xy'):
        def loss(a, b):
            crit = proto_ref.Loss(mode, radius=3, axes=axes, m=0.5, scale=1.7)
            crit.updata(mem[0].copy(), mem[1].copy())
            return crit(a, b, pre1, pre2)
        base = loss(f1, f2)
        assert np.abs(base['val1'] - (0.5 * proto_ref.pool(f1, pre1, 3, axes).mean(0) + 0.5 * mem[0])).max() < 1e-15
        for which, grad in ((0, base['grad_f1']), (1, base['grad_f2'])):
            idx = np.argwhere(np.abs(grad) > 0)
            assert len(idx) > 20
            for ix in idx[rng.choice(len(idx), 12, replace=False)]:
                h = 1e-5
                ops_p, ops_m = [f1.copy(), f2.copy()], [f1.copy(), f2.copy()]
                ops_p[which][tuple(ix)] += h
                ops_m[which][tuple(ix)] -= h
                num = (loss(*ops_p)['loss'] - loss(*ops_m)['loss']) / (2 * h)
                assert abs(num - grad[tuple(ix)]) <= 1e-6 * np.abs(grad).max() + 1e-10, (axes, which, ix, num, grad[tuple(ix)])


def test_zero_sum_source_empty_windows_and_divisors():
    K, C = 3, 8
    rng = np.random.default_rng(7)
    pt, ps = rng.random((K, C)), rng.random((K, C))
    ps[1] = 0                                     # an all-zero source prototype: the reference returns NaN, here the joint drops out
    ps[2, 3] = 0                                  # one zero element: contributes 0 (xlogy)
    loss, rows, gt, gs = proto_ref.criterion(pt, ps, 'kl', 2.0)
    assert np.isfinite(loss) and np.isfinite(gt).all() and np.isfinite(gs).all()
    assert rows[1] == 0 and not gt[1].any() and not gs[1].any() and gs[2, 3] == 0 and gt[2, 3] > 0
    assert loss == pytest.approx(2.0 * (rows[0] + rows[2]) / 3)
    q = ps[0] / ps[0].sum()
    assert rows[0] == pytest.approx(float((q * (np.log(q) - np.log(np.exp(pt[0]) / np.exp(pt[0]).sum()))).sum()))
    loss3, rows3, _, gs3 = proto_ref.criterion(pt, ps, 'softkl', 2.0)          # softkl has no zero sum
    assert np.isfinite(gs3).all() and rows3[1] > 0 and loss3 == pytest.approx(2.0 * rows3.sum())
    # windows: s = hi - lo + 1 is one more than the pixels summed; outside and NaN coordinates give empty windows, zero descriptors
    pre = np.array([[[0, 0], [63, 63], [30.5, 5], [70, 5], [-20, 5], [np.nan, 5], [5, np.inf]]], np.float32)
    win = proto_ref.windows(pre, 64, 64)
    div = proto_ref.divisors(win)
    assert div[0, :3].tolist() == [7 * 7, 7 * 7, 13 * 12] and div[0, 3:].tolist() == [1, 1, 1, 1]
    f = np.ones((1, 8, 64, 64))
    d = proto_ref.pool(f, pre)
    assert np.allclose(d[0, :3, 0], [36 / 49, 36 / 49, 12 * 11 / (13 * 12)]) and not d[0, 3:].any()
    g = proto_ref.scatter(np.ones((7, 8)), pre, f.shape, m=1.0)
    assert g[0, 0, 0, 0] == pytest.approx(1 / 49) and g[0, 0, 6, 6] == 0 and g.sum() == pytest.approx(8 * (36 / 49 * 2 + 132 / 156))


def test_exact_order_models_agree_with_the_plain_restatement():
    rng = np.random.default_rng(11)
    B, C, H, W, K = 3, 8, 16, 12, 5
    f = rng.integers(-8, 9, (B, H, W, C)).astype(np.float32)
    pre = rng.integers(0, 12, (B, K, 2)).astype(np.float32)
    pre[1, 2] = (40, 3)
    mem = rng.integers(-4, 5, (K, C)).astype(np.float32)
    for axes in ('ref', 'xy'):
        d = proto_ref.pool_model(f, pre, 2, axes)
        assert np.abs(d - proto_ref.pool(f.transpose(0, 3, 1, 2), pre, 2, axes)).max() < 1e-6 and not d[1, 2].any()
        p = proto_ref.update_model(d, mem, 0.5)
        assert np.abs(p - proto_ref.blend(d.astype(np.float64), mem, 0.5)).max() < 1e-6
        gp = rng.integers(-8, 9, (K, C)).astype(np.float32)
        s, cov = proto_ref.scatter_model(gp, pre, (B, H, W, C), 0.5, 2, axes)
        want = proto_ref.scatter(gp, pre, (B, C, H, W), 0.5, 2, axes).transpose(0, 2, 3, 1)
        assert np.abs(s - want).max() < 1e-5 and not s[~cov].any()
        onto = rng.integers(-8, 9, (B, H, W, C)).astype(np.float32)
        acc, _ = proto_ref.scatter_model(gp, pre, (B, H, W, C), 0.5, 2, axes, onto=onto)
        assert np.array_equal(acc[~cov], onto[~cov]) and np.abs(acc - (onto + want)).max() < 1e-5
    assert proto_ref.blend_record(0.999) == (np.float32(0.999), np.float32(1.0 - 0.999)) and proto_ref.blend_record(1.0)[1] == 0


def test_loss_classes_have_the_reference_surface():
    """Names, constructor signature, reset / updata (sic) and val1 / val2, without a GPU: nothing is launched."""
    import inspect
    import torch
    from uda.model import loss as L
    for cls, crit in ((L.lossx, 'kl'), (L.lossx3, 'softkl')):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters)[:3] == ['self', 'reduction', 'epsilon']
        assert sig.parameters['reduction'].default == 'mean' and sig.parameters['epsilon'].default == 0.
        assert {k: sig.parameters[k].default for k in ('radius', 'axes', 'm', 'scale')} == dict(radius=6, axes='ref', m=0.999, scale=1.0)
        c = cls()
        assert c.criterion == crit and c.val1 == 0. and c.val2 == 0.             # the reference's scalars until first used
        a, b = torch.arange(16.).view(2, 8), torch.ones(2, 8)
        c.updata(a, b)
        assert torch.equal(c.val1, a) and torch.equal(c.val2, b) and c.val1 is not a
        ptr = c.val1.data_ptr()
        c.updata(b, a)                                                          # copies into the fixed tensors
        assert c.val1.data_ptr() == ptr and torch.equal(c.val1, b) and torch.equal(c.val2, a)
        c.reset()
        assert c.val1.data_ptr() == ptr and not c.val1.any() and not c.val2.any()
        for bad in (dict(m=0.), dict(m=1.5), dict(radius=0), dict(axes='yx')):
            with pytest.raises(ValueError):
                cls(**bad)
        with pytest.raises(ValueError):
            c(torch.zeros(2, 8, 4), torch.zeros(2, 8, 4, 4), torch.zeros(2, 3, 2), torch.zeros(2, 3, 2))
    from mi355.da_step import PrototypeAlign
    p = PrototypeAlign(weight=0.5, radius=4, axes='ref', m=0.9, criterion='softkl')
    assert p.state_dict() == {'memory_s': None, 'memory_t': None, 'm': 0.9}
    p.load_state_dict({'memory_s': torch.ones(3, 8), 'memory_t': torch.zeros(3, 8), 'm': 0.5})
    st = p.state_dict()
    assert st['m'] == 0.5 and torch.equal(st['memory_s'], torch.ones(3, 8)) and torch.equal(st['memory_t'], torch.zeros(3, 8))
    for bad in (dict(weight=0), dict(radius=17), dict(m=0), dict(m=1.01), dict(criterion='on'), dict(axes='yx')):
        with pytest.raises(ValueError):
            PrototypeAlign(**bad)


def test_parser_has_the_proto_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert (a.proto_loss, a.proto_weight, a.proto_radius, a.proto_axes, a.proto_m) == ('off', 1.0, 6, 'xy', 0.999)
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    b = train1.build_parser().parse_args(['d', '--proto-loss', 'softkl', '--proto-weight', '0.25', '--proto-radius', '4', '--proto-axes', 'ref',
                                          '--proto-m', '0.5'])
    assert (b.proto_loss, b.proto_weight, b.proto_radius, b.proto_axes, b.proto_m) == ('softkl', 0.25, 4, 'ref', 0.5)
    assert train1.build_parser().parse_args(['d', '--proto-loss', 'kl', '--proto-m', '1']).proto_m == 1.0
    for bad in (['--proto-weight', '0'], ['--proto-weight', '-0.1'], ['--proto-weight', 'nan'], ['--proto-radius', '0'], ['--proto-radius', '17'],
                ['--proto-m', '0'], ['--proto-m', '1.001'], ['--proto-m', '-0.5'], ['--proto-m', 'nan'], ['--proto-axes', 'yx']):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--proto-loss', 'kl'] + bad)
        assert '--proto-' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--proto-loss', 'on'])
    assert '--proto-loss' in capsys.readouterr().err
    assert train1.build_parser().parse_args(['d', '--proto-m', '0']).proto_loss == 'off'            # (only checked when the term is on)
    allof = train1.build_parser().parse_args(['d', '--proto-loss', 'kl', '--jfa-loss', 'on', '--mmd-loss', 'on'])
    assert (allof.proto_loss, allof.jfa_loss, allof.mmd_loss) == ('kl', 'on', 'on')
    assert 'placeholder' in [kw['help'] for flags, kw in train1._OPTIONS if flags == ('--proto-weight',)][0]


def test_proto_entry_points_exist_and_refuse_bad_arguments(lib_path):
    import ctypes
    import mi355
    lib = mi355.load()
    for name in ('mi355_proto_pool', 'mi355_proto_update', 'mi355_proto_kl', 'mi355_proto_scatter'):
        assert name in mi355.SIGNATURES and hasattr(lib, name)
    P = lambda i, off=0: ctypes.c_void_p(0x100000000 + (i << 28) + off)
    err = lambda: lib.mi355_last_error().decode()
    pool = lambda B=2, K=21, C=256, H=64, W=64, r=6, f=P(1), d=P(3): lib.mi355_proto_pool(f, P(2), d, B, K, C, H, W, r, 1, mi355.BF16, None)
    scat = lambda B=2, K=21, C=256, H=64, W=64, r=6, g=P(1), o=P(4): lib.mi355_proto_scatter(g, P(2), P(3), o, 1, B, K, C, H, W, r, 0, mi355.BF16, None)
    for call in (pool, scat):
        assert call(C=12) == -1 and 'C=12' in err()
        assert call(K=33) == -1 and 'K=33' in err()
        assert call(r=0) == -1 and 'radius=0' in err()
        assert call(B=0) == -1 and 'B=0' in err()
        assert call(H=0) == -1 and 'H=0' in err()
    assert pool(f=P(1, 2)) == -1 and 'aligned' in err() and pool(d=P(3, 4)) == -1 and 'aligned' in err()
    assert scat(g=P(1, 4)) == -1 and 'aligned' in err() and scat(o=P(4, 2)) == -1 and 'aligned' in err()
    upd = lambda B=2, K=21, C=256, m=P(2), p=P(4), d=P(1): lib.mi355_proto_update(d, m, P(3), p, B, K, C, None)
    assert upd(C=12) == -1 and 'C=12' in err() and upd(K=33) == -1 and 'K=33' in err() and upd(B=0) == -1 and 'B=0' in err()
    assert upd(p=P(2)) == -1 and 'memory itself' in err() and upd(m=P(2, 4)) == -1 and 'aligned' in err()
    assert lib.mi355_proto_update(None, P(2), P(3), P(4), 2, 21, 256, None) == -1 and 'null' in err()
    kl = lambda K=21, C=256, mode=0, coef=1.0, a=P(1), gs=P(5): lib.mi355_proto_kl(a, P(2), P(3), P(4), gs, K, C, mode, coef, None)
    assert kl(C=12) == -1 and 'C=12' in err() and kl(K=0) == -1 and 'K=0' in err() and kl(mode=2) == -1 and 'mode=2' in err()
    assert kl(coef=float('nan')) == -1 and 'coef' in err() and kl(a=P(1, 4)) == -1 and 'aligned' in err() and kl(gs=P(5, 8)) == -1
    # the ops layer refuses before the library is reached (Mi355Error, nothing launched); CPU tensors are refused as everywhere
    import torch
    from mi355 import ops
    for m in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(mi355.Mi355Error):
            ops.proto_blend(m)
    assert ops.proto_blend(0.999).tolist() == [float(np.float32(0.999)), float(np.float32(1.0 - 0.999))]
    with pytest.raises(mi355.Mi355Error):
        ops.proto_pool(torch.zeros(1, 8, 4, 4).contiguous(memory_format=torch.channels_last), torch.zeros(1, 3, 2))
    with pytest.raises(mi355.Mi355Error):
        ops.proto_kl(torch.zeros(3, 8), torch.zeros(3, 8), True, False, mode='on')
