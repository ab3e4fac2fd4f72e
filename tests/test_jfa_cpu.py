"""Joint feature alignment, CPU side: the fixture tests/golden/g15_jfa.npz (the reference's own loss1 / loss3 and torch autograd,
written by make_golden_jfa.py) is what its generator describes; the restatement of tests/jfa_ref.py equals it in float64 and
stays inside the tolerance of the GPU tests in float32; the floors of that tolerance are above the reference's own float32
distance from float64; the exact-order model of the scatter kernel agrees with the plain backward; the command line has the four
new switches with the reference's defaults untouched; the three entry points are in the ctypes table and refuse bad arguments
before any launch."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG, golden
import jfa_ref

CASES = ['a', 'b']
KEYS = ('loss', 'grad_f1', 'grad_f2', 'desc1', 'desc2')


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def gold(g, case, suffix=''):
    """The reference's results of one case as the dict jfa_ref.bounds takes; suffix '64': its float64 run."""
    sep = '_' if suffix else ''
    return dict(loss=float(g[case + '/loss' + suffix]), grad_f1=g[case + '/grad_f1' + sep + suffix], grad_f2=g[case + '/grad_f2' + sep + suffix],
                desc1=g[case + '/desc1' + sep + suffix], desc2=g[case + '/desc2' + sep + suffix])


def restated(g, case, dtype):
    r = jfa_ref.loss3(g[case + '/f1'], g[case + '/f2'], g[case + '/pre1'], g[case + '/pre2'], dtype=dtype)
    return dict(zip(KEYS, r))


def test_fixture_is_what_the_generator_describes():
    g = golden('g15_jfa')
    assert g['a/f1'].shape == (2, 8, 64, 64) and g['b/f1'].shape == (1, 8, 64, 64)
    for c in CASES:
        B = g[c + '/f1'].shape[0]
        for side in '12':
            f, pre = g[c + '/f' + side], g[c + '/pre' + side]
            assert f.dtype == np.float32 and pre.dtype == np.float32 and pre.shape == (B, 21, 2)
            assert f.min() >= 0 and np.array_equal(f * 8, np.round(f * 8)) and f.max() <= 15 / 8          # non-negative, dyadic
            assert pre.min() >= 0 and pre.max() <= 63
            assert g[c + '/desc' + side].shape == (B, 21, 8) and g[c + '/desc' + side].dtype == np.float32
            assert g[c + '/grad_f' + side].shape == f.shape and g[c + '/grad_f' + side + '_64'].dtype == np.float64
            assert np.abs(g[c + '/grad_f' + side + '_64']).max() > 0
        assert g[c + '/loss'].dtype == np.float32 and g[c + '/loss64'].dtype == np.float64 and float(g[c + '/loss64']) > 0
    pts = {tuple(p) for p in g['a/pre1'][0].tolist()}
    assert {(0., 0.), (63., 63.), (0., 63.), (63., 0.), (5., 30.), (58., 30.), (30., 5.), (30., 58.)} <= pts
    assert sum(tuple(p) == (20., 33.) for p in g['a/pre1'][0].tolist()) == 3                       # several joints on one pixel
    assert sum(tuple(p) == (0., 0.) for p in g['a/pre1'][0].tolist()) == 3                         # zeroed predictions
    assert any(p[0] != int(p[0]) for p in g['a/pre1'][0].tolist())                                # non-integer coordinates
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_jfa.npz')) < 1 << 20


@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_the_reference_in_float64(case):
    g = golden('g15_jfa')
    got, want = restated(g, case, np.float64), gold(g, case, '64')
    for k in KEYS:
        assert np.abs(np.asarray(got[k]) - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    # a swapped axis shows: the geometric indexing gives other descriptors for (0, 63) and (63, 0)
    other = jfa_ref.pool(g[case + '/f1'], g[case + '/pre1'], axes='xy')
    assert np.abs(other - want['desc1']).max() > 1e-3


@pytest.mark.parametrize('case', CASES)
def test_float32_restatement_is_within_the_tolerance_of_the_gpu_tests(case):
    g = golden('g15_jfa')
    got = restated(g, case, np.float32)
    assert got['loss'].dtype == np.float32 and got['grad_f1'].dtype == np.float32
    ref64 = gold(g, case, '64')
    own, bound = jfa_ref.bounds(gold(g, case), ref64)
    err = jfa_ref.errors(got, ref64)
    for k in KEYS:
        print('%s %s: float32 restatement |err| %.3e; reference float32 %.3e; bound %.3e' % (case, k, err[k], own[k], bound[k]))
        assert err[k] <= bound[k], k


@pytest.mark.parametrize('case', CASES)
def test_the_floors_are_above_the_reference_float32_distance(case):
    """The reference's own float32 run against its float64 run stays below the floors, so a kernel that is as good as torch's
    float32 passes the GPU tests on the floors alone."""
    g = golden('g15_jfa')
    ref64 = gold(g, case, '64')
    own, _ = jfa_ref.bounds(gold(g, case), ref64)
    floors = dict(loss=jfa_ref.LOSS_FLOOR, grad_f1=jfa_ref.GRAD_FLOOR, grad_f2=jfa_ref.GRAD_FLOOR, desc1=jfa_ref.DESC_FLOOR, desc2=jfa_ref.DESC_FLOOR)
    for k in KEYS:
        rel = own[k] / np.abs(ref64[k]).max()
        print('%s %s: reference float32 vs float64: %.2e of the largest magnitude (floor %.0e)' % (case, k, rel, floors[k]))
        assert rel < floors[k], k


def test_options_and_the_scatter_model():
    """radius, axes, scale and a non-square side against finite differences; the exact-order fp32 model of the scatter kernel
    against the plain backward; empty windows."""
    rng = np.random.default_rng(15)
    f1, f2 = rng.random((2, 8, 12, 20)), rng.random((2, 8, 12, 20))
    p1 = np.stack([rng.random((5, 2)) * [19, 11], rng.random((5, 2)) * [19, 11]]).astype(np.float32)
    p2 = p1[::-1].copy()
    for radius, axes, scale in ((3, 'xy', 1.0), (2, 'xy', 0.5), (6, 'xy', 2.0), (3, 'ref', 1.0)):
        if axes == 'ref':
            p1c, p2c = p1[..., ::-1].copy(), p2[..., ::-1].copy()          # (x, y) exchanged: the same windows as 'xy'
            same = jfa_ref.loss3(f1, f2, p1, p2, radius, 'xy', scale)[0]
        else:
            p1c, p2c = p1, p2
        loss, g1, g2, d1, d2 = jfa_ref.loss3(f1, f2, p1c, p2c, radius, axes, scale)
        if axes == 'ref':
            assert loss == same
        for g, which in ((g1, 0), (g2, 1)):
            idx = np.unravel_index(np.abs(g).argmax(), g.shape)
            for sign_h in (1e-5,):
                fp, fm = [f1.copy(), f2.copy()], [f1.copy(), f2.copy()]
                fp[which][idx] += sign_h
                fm[which][idx] -= sign_h
                fd = (jfa_ref.loss3(fp[0], fp[1], p1c, p2c, radius, axes, scale)[0] - jfa_ref.loss3(fm[0], fm[1], p1c, p2c, radius, axes, scale)[0]) / (2 * sign_h)
                assert abs(fd - g[idx]) <= 1e-5 * abs(g[idx]) + 1e-12
        ga = jfa_ref.kl(d1, d2, scale)[2]
        model, cov = jfa_ref.scatter_model(ga, p1c, (2, 12, 20, 8), radius, axes)
        assert np.abs(model.transpose(0, 3, 1, 2) - g1).max() <= 1e-6 * np.abs(g1).max()
        assert np.array_equal(cov, jfa_ref.covered(p1c, 12, 20, radius, axes)) and (model[~cov] == 0).all()
        onto = rng.random((2, 12, 20, 8)).astype(np.float32)
        acc, _ = jfa_ref.scatter_model(ga, p1c, (2, 12, 20, 8), radius, axes, onto=onto)
        assert np.array_equal(acc[~cov], onto[~cov]) and np.array_equal(acc[cov], (onto + model)[cov])
    outside = np.array([[[-7., 3.], [3., -7.], [30., 3.], [3., 30.], [np.float32(1e9), 0.]]], np.float32)
    assert (jfa_ref.pool(f1[:1], outside, 3, 'xy') == 0).all() and not jfa_ref.covered(outside, 12, 20, 3, 'xy').any()
    empty = jfa_ref.loss3(f1[:1], f2[:1], outside, outside, 3, 'xy')
    assert np.isfinite(empty[0]) and abs(empty[0]) < 1e-12 and (empty[1] == 0).all()


def test_parser_has_the_jfa_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert (a.jfa_loss, a.jfa_weight, a.jfa_radius, a.jfa_axes) == ('off', 1.0, 6, 'xy')
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    assert (a.mmd_loss, a.mt_loss, a.ema_update, a.no_graph, a.debug) == ('off', 'off', 'off', False, False)
    b = train1.build_parser().parse_args(['d', '--jfa-loss', 'on', '--jfa-weight', '0.25', '--jfa-radius', '4', '--jfa-axes', 'ref', '--debug'])
    assert (b.jfa_loss, b.jfa_weight, b.jfa_radius, b.jfa_axes, b.debug) == ('on', 0.25, 4, 'ref', True)
    c = train1.build_parser().parse_args(['d', '--jfa-loss', 'on'])
    assert (c.jfa_weight, c.jfa_radius, c.jfa_axes) == (1.0, 6, 'xy')
    for bad in (['--jfa-weight', '0'], ['--jfa-weight', '-0.1'], ['--jfa-weight', 'nan'], ['--jfa-radius', '0'], ['--jfa-radius', '17'],
                ['--jfa-radius', '-3'], ['--jfa-axes', 'yx'], ['--jfa-radius', '2.5']):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--jfa-loss', 'on'] + bad)
        assert '--jfa-' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--jfa-loss', 'maybe'])
    assert '--jfa-loss' in capsys.readouterr().err
    assert train1.build_parser().parse_args(['d', '--jfa-loss', 'on', '--jfa-radius', '16', '--jfa-radius', '1']).jfa_radius == 1
    assert train1.build_parser().parse_args(['d', '--jfa-weight', '0']).jfa_loss == 'off'         # (only checked when the term is on)
    both = train1.build_parser().parse_args(['d', '--jfa-loss', 'on', '--mmd-loss', 'on'])                # composes with the MMD term
    assert (both.jfa_loss, both.mmd_loss) == ('on', 'on')


def test_jfa_entry_points_exist_and_refuse_bad_arguments(lib_path):
    import ctypes
    import mi355
    for name in ('mi355_jfa_pool', 'mi355_jfa_kl', 'mi355_jfa_scatter'):
        assert name in mi355.SIGNATURES
    lib = mi355.load()
    f = ctypes.c_float

    def refused(fn, ok, i, v, word):
        a = list(ok)
        a[i] = v
        assert fn(*a) == -1 and word in lib.mi355_last_error(), (i, v, lib.mi355_last_error())

    #         feature xy  desc  B  K   C   H   W  r  divisor  axes dtype stream
    pool_ok = [256, 512, 1024, 2, 21, 256, 64, 64, 6, f(169.), 1, 1, 0]
    for i in (0, 1, 2):
        refused(lib.mi355_jfa_pool, pool_ok, i, 0, b'null')
    refused(lib.mi355_jfa_pool, pool_ok, 0, 264, b'aligned'); refused(lib.mi355_jfa_pool, pool_ok, 2, 1028, b'aligned')
    refused(lib.mi355_jfa_pool, pool_ok, 1, 514, b'aligned')
    for i, v, word in ((3, 0, b'B=0'), (4, 0, b'K=0'), (4, 33, b'K=33'), (5, 0, b'C=0'), (5, 4, b'C=4'), (5, 20, b'C=20'), (5, 257, b'C=257'),
                       (6, 0, b'H=0'), (7, 0, b'W=0'), (7, -4, b'W=-4'), (8, 0, b'radius=0'), (8, -6, b'radius=-6'), (9, f(0.), b'divisor'),
                       (9, f(-169.), b'divisor'), (9, f(float('nan')), b'divisor'), (11, 2, b'dtype=2'), (11, -1, b'dtype=-1')):
        refused(lib.mi355_jfa_pool, pool_ok, i, v, word)
    #       a    b    rows  ga    gb   nrows C   coef    stream
    kl_ok = [256, 512, 1024, 2048, 4096, 42, 256, f(1 / 42), 0]
    for i in (0, 1, 2):
        refused(lib.mi355_jfa_kl, kl_ok, i, 0, b'null')
    for i in (0, 1, 3, 4):
        refused(lib.mi355_jfa_kl, kl_ok, i, kl_ok[i] + 4, b'aligned')
    refused(lib.mi355_jfa_kl, kl_ok, 2, 1026, b'aligned')
    for i, v, word in ((5, 0, b'nrows=0'), (5, -1, b'nrows=-1'), (6, 0, b'C=0'), (6, 12, b'C=12'), (7, f(float('inf')), b'coef')):
        refused(lib.mi355_jfa_kl, kl_ok, i, v, word)
    #          gdesc xy  out  acc B  K   C   H   W  r  divisor  axes dtype stream
    scat_ok = [256, 512, 1024, 0, 2, 21, 256, 64, 64, 6, f(169.), 0, 1, 0]
    for i in (0, 1, 2):
        refused(lib.mi355_jfa_scatter, scat_ok, i, 0, b'null')
    refused(lib.mi355_jfa_scatter, scat_ok, 0, 260, b'aligned'); refused(lib.mi355_jfa_scatter, scat_ok, 2, 1032, b'aligned')
    for i, v, word in ((4, 0, b'B=0'), (5, 0, b'K=0'), (5, 33, b'K=33'), (6, 4, b'C=4'), (6, 44, b'C=44'), (7, 0, b'H=0'), (8, 0, b'W=0'),
                       (9, 0, b'radius=0'), (10, f(0.), b'divisor'), (12, 3, b'dtype=3')):
        refused(lib.mi355_jfa_scatter, scat_ok, i, v, word)
