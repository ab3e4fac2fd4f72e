"""MMD alignment, CPU side: the closed form of tests/mmd_ref.py equals what the reference's own MMD_loss3 / MMD_loss and
torch autograd produced (tests/golden/g14_mmd.npz, written by make_golden_mmd.py) -- in float64 to 1e-12, in float32 within the
tolerance the GPU tests use; the zero-bandwidth rule; the floors of that tolerance are above the reference's own float32
distance from float64; the command line has the new switches with the reference's defaults untouched; the entry point is in
the ctypes table and refuses bad arguments before any launch."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG, golden
import mmd_ref

CASES = ['a', 'b', 'c', 'd']


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def _operands(g, case):
    s, t = g[case + '/source'], g[case + '/target']
    if case == 'd':                                   # MMD_loss on (n, D) features: the same expression with K = 1
        s, t = s[:, None, :], t[:, None, :]
    return s, t


def _gold(g, case, suffix=''):
    shape = _operands(g, case)[0].shape
    return (float(g[case + '/loss' + suffix]), g[case + '/grad_source' + suffix].reshape(shape),
            g[case + '/grad_target' + suffix].reshape(shape))


def test_fixture_is_what_the_generator_describes():
    g = golden('g14_mmd')
    assert g['a/source'].shape == (2, 21, 8, 8) and g['b/source'].shape == (3, 21, 5, 7) and g['c/source'].shape == (4, 21, 8, 8)
    assert g['d/source'].shape == (5, 70)
    for c in CASES:
        assert g[c + '/source'].dtype == np.float32 and g[c + '/loss'].dtype == np.float32 and g[c + '/grad_target'].dtype == np.float32
        assert g[c + '/loss64'].dtype == np.float64 and g[c + '/grad_source64'].dtype == np.float64
        assert g[c + '/grad_source'].shape == g[c + '/source'].shape and np.isfinite(g[c + '/loss64'])
        assert float(g[c + '/loss64']) > 0 and np.abs(g[c + '/grad_target64']).max() > 0


@pytest.mark.parametrize('case', CASES)
def test_closed_form_equals_the_reference_in_float64(case):
    g = golden('g14_mmd')
    s, t = _operands(g, case)
    loss, rows, gs, gt = mmd_ref.mmd(s, t, dtype=np.float64)
    want, ws, wt = _gold(g, case, '64')
    assert abs(float(loss) - want) <= 1e-12 * abs(want)
    assert np.abs(gs - ws).max() <= 1e-12 * np.abs(ws).max() and np.abs(gt - wt).max() <= 1e-12 * np.abs(wt).max()
    assert rows.shape == (s.shape[1],) and abs(rows.mean() - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize('case', CASES)
def test_float32_restatement_is_within_the_tolerance_of_the_gpu_tests(case):
    g = golden('g14_mmd')
    s, t = _operands(g, case)
    loss, _, gs, gt = mmd_ref.mmd(s, t, dtype=np.float32)
    assert loss.dtype == np.float32 and gs.dtype == np.float32
    l64, s64, t64 = _gold(g, case, '64')
    own, bound = mmd_ref.bounds(*_gold(g, case), l64, s64, t64)
    got = (abs(float(loss) - l64), float(np.abs(gs.astype(np.float64) - s64).max()), float(np.abs(gt.astype(np.float64) - t64).max()))
    print('%s: float32 restatement |err| loss %.3e grads %.3e %.3e; reference float32 %.3e %.3e %.3e; bound %.3e %.3e %.3e'
          % ((case,) + got + own + bound))
    assert all(a <= b for a, b in zip(got, bound))


@pytest.mark.parametrize('case', CASES)
def test_the_floors_are_above_the_reference_float32_distance(case):
    """The reference's own float32 run against its float64 run: below 5e-7 relative on the loss and below 1e-6 of max |grad| on
    the gradients, so a kernel that is as good as torch's float32 passes the GPU tests on the floors alone."""
    g = golden('g14_mmd')
    l64, s64, t64 = _gold(g, case, '64')
    own, _ = mmd_ref.bounds(*_gold(g, case), l64, s64, t64)
    rel = (own[0] / abs(l64), own[1] / np.abs(s64).max(), own[2] / np.abs(t64).max())
    print('%s: reference float32 vs float64: loss %.2e relative, grad_source %.2e, grad_target %.2e of max |grad|' % ((case,) + rel))
    assert rel[0] < mmd_ref.LOSS_FLOOR and rel[1] < mmd_ref.GRAD_FLOOR and rel[2] < mmd_ref.GRAD_FLOOR


def test_options_of_the_closed_form():
    """kernel_num, kernel_mul, fix_sigma and scale against a direct evaluation of the definition with finite differences."""
    rng = np.random.default_rng(5)
    s, t = rng.standard_normal((3, 2, 6)), rng.standard_normal((3, 2, 6)) * 0.5 + 0.2

    def direct(s, t, mul, num, fix):
        B, K = s.shape[:2]
        total = 0.0
        for k in range(K):
            X = np.concatenate([s[:, k], t[:, k]], 0)
            D = ((X[:, None] - X[None]) ** 2).sum(-1)
            bw = fix if fix else D.sum() / (4 * B * B - 2 * B)
            bw /= mul ** (num // 2)
            Km = sum(np.exp(-D / (bw * mul ** m)) for m in range(num))
            total += (Km[:B, :B] + Km[B:, B:] - Km[:B, B:] - Km[B:, :B]).mean()
        return total / K

    for mul, num, fix, scale in ((2.0, 5, None, 1.0), (2.0, 1, None, 0.3), (1.5, 8, None, 2.0), (2.0, 5, 3.0, 1.0), (3.0, 4, 0.7, 0.1)):
        loss, _, gs, gt = mmd_ref.mmd(s, t, mul, num, fix, scale)
        assert abs(loss - scale * direct(s, t, mul, num, fix)) <= 1e-13
        if fix:                                       # (with a data-dependent bandwidth the gradient takes it as a constant)
            h = 1e-6
            for arr, grad in ((s, gs), (t, gt)):
                for idx in ((0, 0, 0), (2, 1, 5), (1, 0, 3)):
                    save = arr[idx]
                    arr[idx] = save + h
                    up = direct(s, t, mul, num, fix)
                    arr[idx] = save - h
                    dn = direct(s, t, mul, num, fix)
                    arr[idx] = save
                    assert abs(scale * (up - dn) / (2 * h) - grad[idx]) <= 1e-8


def test_zero_bandwidth_joint_gives_zeros_and_leaves_the_others_alone():
    rng = np.random.default_rng(8)
    s, t = rng.standard_normal((3, 4, 10)).astype(np.float32), rng.standard_normal((3, 4, 10)).astype(np.float32)
    live = mmd_ref.mmd(s, t, dtype=np.float64)
    s2, t2 = s.copy(), t.copy()
    s2[:, 2] = t2[:, 2] = s[0, 2]                     # every row of joint 2 identical: all distances 0
    for dtype in (np.float64, np.float32):
        loss, rows, gs, gt = mmd_ref.mmd(s2, t2, dtype=dtype)
        assert np.isfinite(loss) and rows[2] == 0 and not gs[:, 2].any() and not gt[:, 2].any()
    loss, rows, gs, gt = mmd_ref.mmd(s2, t2, dtype=np.float64)
    keep = [0, 1, 3]
    assert np.array_equal(rows[keep], live[1][keep]) and np.array_equal(gs[:, keep], live[2][:, keep]) and np.array_equal(gt[:, keep], live[3][:, keep])
    assert loss == rows.mean()
    # target = source: the loss is 0, in either precision
    for dtype in (np.float64, np.float32):
        assert mmd_ref.mmd(s, s, dtype=dtype)[0] == 0


def test_parser_has_the_mmd_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert (a.mmd_loss, a.mmd_weight, a.mmd_kernels, a.mmd_mul) == ('off', 0.1, 5, 2.0)
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    assert (a.mt_loss, a.ema_update, a.no_graph, a.debug) == ('off', 'off', False, False)
    b = train1.build_parser().parse_args(['d', '--mmd-loss', 'on', '--mmd-weight', '0.25', '--mmd-kernels', '3', '--mmd-mul', '1.5', '--debug'])
    assert (b.mmd_loss, b.mmd_weight, b.mmd_kernels, b.mmd_mul, b.debug) == ('on', 0.25, 3, 1.5, True)
    assert train1.build_parser().parse_args(['d', '--mmd-loss', 'on']).mmd_weight == 0.1
    for bad in (['--mmd-weight', '0'], ['--mmd-weight', '-0.1'], ['--mmd-weight', 'nan'], ['--mmd-kernels', '0'], ['--mmd-kernels', '9'],
                ['--mmd-mul', '0'], ['-b', '129']):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--mmd-loss', 'on'] + bad)
        assert '--mmd-' in capsys.readouterr().err
    assert train1.build_parser().parse_args(['d', '--mmd-loss', 'on', '-b', '128']).batch_size == 128
    assert train1.build_parser().parse_args(['d', '--mmd-weight', '0']).mmd_loss == 'off'        # (only checked when the term is on)


def test_mmd_entry_point_exists_and_refuses_bad_arguments(lib_path):
    import ctypes
    import mi355
    assert 'mi355_mmd_heatmap' in mi355.SIGNATURES and 'mi355_mmd_workspace' in mi355.SIGNATURES
    lib = mi355.load()
    assert lib.mi355_mmd_workspace(2, 21) == 21 * 16 * 4 and lib.mi355_mmd_workspace(128, 1) == 256 * 256 * 4
    assert lib.mi355_mmd_workspace(129, 1) == 0 and lib.mi355_mmd_workspace(0, 1) == 0 and lib.mi355_mmd_workspace(1, 0) == 0
    f = ctypes.c_float
    call = lambda *a: lib.mi355_mmd_heatmap(*a)
    ok = [64, 128, 192, 1 << 20, 256, 320, 384, 2, 21, 64, f(2.0), 5, f(0.0), f(1.0), 0]

    def refused(i, v, word):
        a = list(ok)
        a[i] = v
        assert call(*a) == -1 and word in lib.mi355_last_error(), (i, v, lib.mi355_last_error())

    for i in (0, 1, 2, 4):
        refused(i, 0, b'null')
    refused(0, 66, b'aligned'); refused(5, 321, b'aligned'); refused(6, 386, b'aligned')
    refused(7, 0, b'B=0'); refused(8, 0, b'K=0'); refused(9, 0, b'HW=0'); refused(7, 129, b'258 rows')
    refused(11, 0, b'kernel_num=0'); refused(11, 9, b'kernel_num=9'); refused(10, f(0.0), b'kernel_mul'); refused(10, f(-2.0), b'kernel_mul')
    refused(3, 21 * 16 * 4 - 1, b'workspace')
