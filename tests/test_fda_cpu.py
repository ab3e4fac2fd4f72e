"""Fourier-domain stylisation, CPU side: the two numpy float64 restatements of tests/fda_ref.py -- the published full-FFT form
and the partial-DFT form the kernels follow -- agree; the identity and the b = 0 case hold in the partial form; the command line
has the two switches with the reference's defaults untouched and refuses a band the kernels do not take; the two entry points
are in the ctypes table and in the header and refuse bad arguments before any launch; a DAStep built without `fda` has none."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG, ROOT
import fda_ref

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# B, H, W, beta -> b: the shapes at which the algebra was checked when the feature was proposed; seed = position
SHAPES = [(1, 16, 16, 0.07, 1), (3, 16, 32, 0.13, 2), (2, 24, 40, 0.01, 0), (2, 64, 64, 0.09, 5), (1, 16, 16, 0.49, 7), (2, 48, 16, 0.20, 3)]


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_constants_are_those_of_the_package():
    from mi355.augment import MEAN as M, STD as S
    assert tuple(M) == MEAN and tuple(S) == STD


@pytest.mark.parametrize('seed,case', list(enumerate(SHAPES)), ids=lambda v: None if isinstance(v, int) else '%dx%dx%d-b%d' % (v[0], v[1], v[2], v[4]))
def test_full_fft_and_partial_dft_agree(seed, case):
    B, H, W, beta, b = case
    assert fda_ref.band(H, W, beta) == b
    x_s, x_t = fda_ref.inputs((B, 3, H, W), seed, MEAN, STD)
    a = fda_ref.full_fft(x_s, x_t, b, MEAN, STD)
    p, amin = fda_ref.partial_dft(x_s, x_t, b, MEAN, STD, want_min=True)
    print('B%d %dx%d b%d: max |full - partial| = %.3e, min |Fs| / HW = %.3e' % (B, H, W, b, np.abs(a - p).max(), amin))
    assert np.abs(a - p).max() <= 1e-12
    assert np.abs(p - x_s).max() > 1e-2                                 # (and the band does change the image)
    assert amin >= 1e-5                                                 # the condition the GPU tolerance rests on


@pytest.mark.parametrize('seed,case', list(enumerate(SHAPES)), ids=lambda v: None if isinstance(v, int) else '%dx%dx%d-b%d' % (v[0], v[1], v[2], v[4]))
def test_identity_is_exact_in_the_partial_form(seed, case):
    B, H, W, beta, b = case
    x_s, _ = fda_ref.inputs((B, 3, H, W), seed, MEAN, STD)
    out = fda_ref.partial_dft(x_s, x_s.copy(), b, MEAN, STD)
    assert np.array_equal(out, x_s.astype(np.float64))


def test_b0_moves_every_plane_by_the_difference_of_the_means():
    x_s, x_t = fda_ref.inputs((2, 3, 24, 40), 2, MEAN, STD)
    out = fda_ref.partial_dft(x_s, x_t, 0, MEAN, STD)
    m = np.asarray(MEAN, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(STD, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    mean01 = lambda x: (x.astype(np.float64) * s + m).mean(axis=(2, 3), keepdims=True)
    want = (mean01(x_t) - mean01(x_s)) / s
    delta = out - x_s
    assert np.abs(delta - want).max() <= 1e-13
    assert np.abs(delta - delta[:, :, :1, :1]).max() <= 1e-13 and np.abs(want).min() > 1e-3


def test_zero_amplitude_takes_phase_zero():
    """An all-zero normalised plane has |Fs| exactly 0 off DC: the phase factor is 1 there, nothing divides by zero."""
    x_s, x_t = fda_ref.inputs((1, 3, 16, 16), 0, MEAN, STD)
    x_s[0, 1] = 0.0
    out = fda_ref.partial_dft(x_s, x_t, 2, MEAN, STD)
    assert np.isfinite(out).all()
    assert np.abs(out - fda_ref.full_fft(x_s, x_t, 2, MEAN, STD)).max() <= 1e-12


def test_parser_has_the_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert (a.fda, a.fda_beta) == ('off', 0.01)
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    b = train1.build_parser().parse_args(['d', '--fda', 'on', '--fda-beta', '0.09'])
    assert (b.fda, b.fda_beta) == ('on', 0.09)
    assert train1.build_parser().parse_args(['d', '--fda', 'on', '--fda-beta', '0.125']).fda == 'on'      # b = 32 at 256: the cap itself
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--fda', 'on', '--fda-beta', '0.2', '--image-size', '256'])
    err = capsys.readouterr().err
    assert '--fda-beta' in err and 'beta = 0.2' in err and 'b = 51' in err and '32' in err
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--fda', 'on', '--fda-beta', '0.5', '--image-size', '32'])   # b = 16: 33 > 32
    err = capsys.readouterr().err
    assert 'b = 16' in err and '2b+1 = 33' in err and '32' in err
    for bad in ('0', '-0.01', 'nan'):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--fda', 'on', '--fda-beta', bad])
        assert '--fda-beta' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--fda-beta', '0'])
    assert '--fda-beta' in capsys.readouterr().err
    act = [x for x in train1.build_parser()._actions if '--fda-beta' in x.option_strings][0]
    assert 'placeholder' in act.help and 'not been measured' in act.help
    act = [x for x in train1.build_parser()._actions if '--fda' in x.option_strings][0]
    assert 'not been measured' in act.help


def test_entry_points_are_in_the_table_and_in_the_header():
    import mi355
    header = open(os.path.join(ROOT, 'include', 'mi355pose.h')).read()
    for name, nargs, res in (('mi355_fda_workspace_bytes', 5, 'long'), ('mi355_fda_transfer', 13, 'int')):
        assert name in mi355.SIGNATURES and len(mi355.SIGNATURES[name][1]) == nargs
        proto = header[header.index('%s %s(' % (res, name)):]
        assert proto[:proto.index(';')].count(',') == nargs - 1
    assert '#define MI355_FDA_MAX_B 32' in header and 'Yang and Soatto' in header and 'no file:line' in header
    from mi355 import ops
    assert ops.FDA_MAX_B == 32 and ops.fda_band(256, 256, 0.01) == 2 and ops.fda_band(256, 256, 0.09) == 23 and ops.fda_band(24, 40, 0.01) == 0


def test_entry_points_refuse_bad_arguments(lib_path):
    import ctypes
    import mi355
    lib = mi355.load()
    B, C, H, W, b = 2, 3, 16, 20, 2
    need = lib.mi355_fda_workspace_bytes(B, C, H, W, b)
    assert need == B * C * 1 * 2 * 5 * 3 * 16
    assert lib.mi355_fda_workspace_bytes(1, 1, 1, 1, 0) == 32 and lib.mi355_fda_workspace_bytes(1, 3, 128, 128, 32) == 3 * 4 * 2 * 65 * 33 * 16

    def no_bytes(args, word):
        assert lib.mi355_fda_workspace_bytes(*args) == -1 and word in lib.mi355_last_error(), (args, lib.mi355_last_error())

    fl = ctypes.c_float * 4
    mean, std = fl(*MEAN, 0.5), fl(*STD, 0.25)
    # x_s, x_t, out, mean, std, B, C, H, W, b, ws, ws_bytes, stream (fake device addresses, far apart)
    base = [(i + 1) << 32 for i in range(4)]
    ok = [base[0], base[1], base[2], mean, std, B, C, H, W, b, base[3], need, 0]
    nx = 4 * B * C * H * W

    def refused(changes, word):
        a = list(ok)
        for i, v in changes.items():
            a[i] = v
        assert lib.mi355_fda_transfer(*a) == -1 and word in lib.mi355_last_error(), (changes, lib.mi355_last_error())

    for shape, word in (({4: -1}, b'b=-1'), ({4: 33}, b'b=33'), ({4: 8}, b'b=8'), ({1: 0}, b'C=0'), ({1: 5}, b'C=5'), ({0: 0}, b'B=0'),
                        ({0: -3}, b'B=-3'), ({2: 0}, b'H=0'), ({2: 1025}, b'H=1025'), ({3: 0}, b'W=0'), ({3: 1025}, b'W=1025')):
        a = [B, C, H, W, b]
        for i, v in shape.items():
            a[i] = v
        no_bytes(a, word)
        refused({5 + i: v for i, v in shape.items()}, word)
    no_bytes([1, 3, 1024, 1024, 33], b'MI355_FDA_MAX_B')
    assert lib.mi355_fda_workspace_bytes(1, 3, 64, 15, 7) > 0           # 2b+1 = 15 fits a side of 15, ...
    no_bytes([1, 3, 14, 64, 7], b'b=7')                                 # ... and not one of 14
    no_bytes([1, 3, 64, 14, 7], b'min(H, W)')
    for i, name in ((0, b'x_s'), (1, b'x_t'), (2, b'out'), (3, b'mean'), (4, b'std'), (10, b'ws')):
        refused({i: 0}, name + b' is null')
    for i, name in ((0, b'x_s'), (1, b'x_t'), (2, b'out')):
        refused({i: base[i] + 2}, name + b' must be 4-byte aligned')
    refused({10: base[3] + 8}, b'ws must be 16-byte aligned')
    refused({11: need - 1}, b'ws_bytes'); refused({11: 0}, b'too small'); refused({11: -5}, b'ws_bytes=-5')
    for bad, word in ((0.0, b'std[1]'), (-0.2, b'std[1]'), (float('inf'), b'std[1]'), (float('nan'), b'std[1]')):
        s = fl(*STD, 0.25); s[1] = bad
        refused({4: s}, word)
    for bad in (float('inf'), float('nan')):
        m = fl(*MEAN, 0.5); m[2] = bad
        refused({3: m}, b'mean[2]')
    refused({2: base[0]}, b'out and x_s overlap'); refused({2: base[0] + nx - 4}, b'out and x_s overlap')
    refused({2: base[1] - nx + 4}, b'out and x_t overlap')
    refused({10: base[0] + 16}, b'ws and x_s overlap'); refused({10: base[1] + nx - 16}, b'ws and x_t overlap')
    refused({10: base[2] - need + 16}, b'ws and out overlap'); refused({0: base[3] + need - 4}, b'ws and x_s overlap')
    # (every call above is refused before a launch: the addresses are fake.  Ranges that only touch, which are accepted, are walked
    #  by the stand-alone driver of tests/test_host_fda.py, which hides the GPU from itself.)


def test_a_step_built_without_fda_has_none():
    import inspect
    from mi355.da_step import DAStep, FourierStyle, build_training
    assert inspect.signature(DAStep.__init__).parameters['fda'].default is None
    assert inspect.signature(build_training).parameters['fda'].default is None
    assert inspect.signature(FourierStyle.__init__).parameters['beta'].default == 0.01

    class _M:                                                           # (what DAStep.__init__ touches of a model)
        class _H:
            def parameters(self):
                return []
        head_adv = head_adv2 = head_adv3 = _H()
    step = DAStep(_M(), {}, {})
    assert step.fda is None
    f = FourierStyle()
    assert f.beta == 0.01 and f.mean == MEAN and f.std == STD and f.band(256, 256) == 2
    step.fda = f
    assert step.fda is f
    for bad in (0, -0.01, float('nan')):
        with pytest.raises(ValueError):
            FourierStyle(beta=bad)
