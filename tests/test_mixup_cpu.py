"""Cross-domain mixup, CPU side: the numpy restatement (tests/mixup_ref.py) equals what the reference's live mixup produced
(tests/golden/g17_mixup.npz, written by make_golden_mixup.py) bit for bit; a draw under the golden's seed gives the stored
coefficients; the entry point is in the ctypes table and in the header and refuses bad arguments before any launch; the command
line has the four switches with the reference's defaults untouched, and `--mixup-labels teacher` without a moving teacher ends
before anything is written."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, golden
import mixup_ref

TAGS = (('b0.5', 0.5), ('b1', 1.0))
INPUTS = ('x_s', 'hm_s', 'w_s', 'x_t', 'hm_t', 'w_t')


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_fixture_is_what_the_generator_describes():
    g = golden('g17_mixup')
    assert g['x_s'].shape == g['x_t'].shape == (5, 3, 16, 16) and g['hm_s'].shape == g['hm_t'].shape == (5, 21, 8, 8)
    assert g['w_s'].shape == g['w_t'].shape == (5, 21, 1)
    for k in INPUTS:
        assert g[k].dtype == np.float32 and np.isfinite(g[k]).all()
    for k in ('w_s', 'w_t'):
        assert set(np.unique(g[k])) == {0.0, 1.0}
    assert (g['w_s'] != g['w_t']).any()                               # the maximum is not a copy of either side
    for tag, _ in TAGS:
        lam = g[tag + '/lam']
        assert lam.shape == (5,) and lam.dtype == np.float32 and (lam >= 0.5).all() and (lam <= 1.0).all() and len(set(lam.tolist())) == 5
        for i, k in enumerate(('x_s', 'hm_s', 'w_s', 'x_t', 'hm_t', 'w_s')):
            assert g['%s/out%d' % (tag, i)].shape == g[k].shape and g['%s/out%d' % (tag, i)].dtype == np.float32
    assert not mixup_ref.same(g['b0.5/lam'], g['b1/lam'])


@pytest.mark.parametrize('tag', [t for t, _ in TAGS])
def test_mixup_ref_equals_the_reference_bit_for_bit(tag):
    g = golden('g17_mixup')
    out = mixup_ref.mixup(*[g[k] for k in INPUTS], g[tag + '/lam'])
    for i, o in enumerate(out):
        assert mixup_ref.same(o, g['%s/out%d' % (tag, i)]), (tag, i)
    assert mixup_ref.same(out[2], out[5]) and mixup_ref.same(out[2], np.maximum(g['w_s'], g['w_t']))
    # the packed form the kernel writes is the same arrays, source-dominant half first
    x, hm, w = mixup_ref.mixup_pairs(*[g[k] for k in INPUTS], g[tag + '/lam'])
    assert mixup_ref.same(x, np.concatenate([out[0], out[3]])) and mixup_ref.same(hm, np.concatenate([out[1], out[4]]))
    assert mixup_ref.same(w, np.concatenate([out[2], out[2]]))


def test_an_fma_would_not_pass():
    """Why the kernel keeps three roundings: contracting a product into the sum changes bits of the golden case."""
    g = golden('g17_mixup')
    lam = g['b1/lam'].astype(np.float64).reshape(-1, 1, 1, 1)
    om = (np.float32(1.0) - g['b1/lam']).astype(np.float64).reshape(-1, 1, 1, 1)
    a, b = g['x_s'].astype(np.float64), g['x_t'].astype(np.float64)
    fma = (a * lam + (b * om).astype(np.float32).astype(np.float64)).astype(np.float32)     # fma(a, lam, fl(b * om))
    assert not mixup_ref.same(fma, g['b1/out0'])
    assert np.abs(fma - g['b1/out0']).max() <= np.spacing(np.abs(g['b1/out0'])).max()


@pytest.mark.parametrize('tag,beta', TAGS)
def test_a_draw_under_the_goldens_seed_gives_the_stored_coefficients(tag, beta):
    import torch
    from uda.model.loss import draw_mixup_coefficients
    g = golden('g17_mixup')
    state = torch.get_rng_state()
    try:
        torch.manual_seed(int(g['seed']))
        lam = draw_mixup_coefficients(5, beta)
    finally:
        torch.set_rng_state(state)
    assert lam.shape == (5,) and lam.dtype == torch.float32
    if not mixup_ref.same(lam.numpy(), g[tag + '/lam']):
        pytest.skip('this torch build draws Beta(%g, %g) differently from the one that wrote the golden: %s vs %s'
                    % (beta, beta, lam.tolist(), g[tag + '/lam'].tolist()))


def test_the_coefficients_of_a_step_do_not_advance_the_global_rng():
    import torch
    from mi355.da_step import CrossDomainMixup
    from uda.model.loss import draw_mixup_coefficients
    a, b, other = CrossDomainMixup(beta=0.5, seed=3, rank=0), CrossDomainMixup(beta=0.5, seed=3, rank=0), CrossDomainMixup(beta=0.5, seed=3, rank=1)
    for m in (a, b, other):
        m.lam = torch.zeros(4)                                        # (a host stand-in for the device buffer)
    before = torch.get_rng_state()
    first, second = a.draw().clone(), a.draw().clone()
    assert torch.equal(torch.get_rng_state(), before)
    assert not torch.equal(first, second) and torch.equal(a.lam, second) and (first >= 0.5).all() and (first <= 1).all()
    assert torch.equal(b.draw(), first) and not torch.equal(other.draw(), first)        # the seed decides, and the rank
    # the state travels: a fresh object that loads it goes on where `a` is
    c = CrossDomainMixup(beta=0.5, seed=99, rank=0)
    c.lam = torch.zeros(4)
    c.load_state_dict(a.state_dict())
    assert c.draws == 2 and torch.equal(c.draw(), a.draw())
    # and the expression is the reference's: the same state in the global generator gives the same coefficients
    d = CrossDomainMixup(beta=0.5, seed=3, rank=0)
    try:
        torch.set_rng_state(d._rng)
        want = draw_mixup_coefficients(4, 0.5)
    finally:
        torch.set_rng_state(before)
    assert torch.equal(want, first)
    with pytest.raises(ValueError, match='--ema-update'):
        CrossDomainMixup(labels='teacher')
    for bad in (dict(beta=0), dict(beta=-1.0), dict(weight=0), dict(weight=float('nan')), dict(labels='both')):
        with pytest.raises(ValueError):
            CrossDomainMixup(**bad)


def test_parser_has_the_mixup_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert (a.mixup, a.mixup_beta, a.mixup_weight, a.mixup_labels) == ('off', 1.0, 1.0, 'student')
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    b = train1.build_parser().parse_args(['d', '--mixup', 'on', '--mixup-beta', '0.5', '--mixup-weight', '0.25', '--mixup-labels', 'teacher',
                                          '--ema-update', 'const'])
    assert (b.mixup, b.mixup_beta, b.mixup_weight, b.mixup_labels) == ('on', 0.5, 0.25, 'teacher')
    for bad in (['--mixup-beta', '0'], ['--mixup-beta', '-1'], ['--mixup-beta', 'nan'], ['--mixup-weight', '0'], ['--mixup-weight', '-0.5']):
        with pytest.raises(SystemExit):
            train1.build_parser().parse_args(['d', '--mixup', 'on'] + bad)
        assert '--mixup-' in capsys.readouterr().err
    assert train1.build_parser().parse_args(['d', '--mixup-weight', '0']).mixup == 'off'         # (only checked when the switch is on)
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['d', '--mixup', 'on', '--mixup-labels', 'teacher'])
    assert '--ema-update' in capsys.readouterr().err
    assert train1.build_parser().parse_args(['d', '--mixup-labels', 'teacher']).mixup == 'off'  # (the labels matter with the switch on)
    for flag in ('--mixup-beta', '--mixup-weight'):                    # the defaults are placeholders, and the help says so
        act = [x for x in train1.build_parser()._actions if flag in x.option_strings][0]
        assert 'placeholder' in act.help and 'not been measured' in act.help


def test_teacher_labels_without_a_moving_teacher_end_before_the_log_directory(tmp_path):
    log = str(tmp_path / 'bad')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train1.py'), 'data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18',
                        '--mixup', 'on', '--mixup-labels', 'teacher', '--log', log], env=dict(os.environ, PYTHONPATH=PKG),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--ema-update' in r.stderr and not os.path.exists(log), r.stdout[-2000:] + r.stderr[-2000:]


def test_entry_point_is_in_the_table_and_in_the_header():
    import mi355
    assert 'mi355_mixup_pairs' in mi355.SIGNATURES
    res, args = mi355.SIGNATURES['mi355_mixup_pairs']
    assert len(args) == 15
    header = open(os.path.join(ROOT, 'include', 'mi355pose.h')).read()
    assert 'int mi355_mixup_pairs(' in header and 'uda/model/loss.py:13-24' in header and 'MI355_MIXUP_MAX_BLOCKS' in header
    proto = header[header.index('int mi355_mixup_pairs('):]
    proto = proto[:proto.index(';')]
    assert proto.count(',') == 14                                     # fifteen parameters, as the table says


def test_mixup_entry_point_refuses_bad_arguments(lib_path):
    import mi355
    lib = mi355.load()
    # x_s, x_t, hm_s, hm_t, w_s, w_t, lam, x_mix, hm_mix, w_mix (fake device addresses, far apart), B, img_plane, hm_plane, K, stream
    base = [(i + 1) << 32 for i in range(10)]
    ok = base + [3, 105, 735, 21, 0]

    def refused(changes, word):
        a = list(ok)
        for i, v in changes.items():
            a[i] = v
        assert lib.mi355_mixup_pairs(*a) == -1 and word in lib.mi355_last_error(), (changes, lib.mi355_last_error())

    for i in range(10):
        refused({i: 0}, b'null')
    refused({10: 0}, b'B=0'); refused({10: -2}, b'B=-2')
    refused({11: 0}, b'img_plane=0'); refused({12: 0}, b'hm_plane=0'); refused({13: 0}, b'K=0'); refused({11: -4}, b'img_plane=-4')
    refused({11: (1 << 40)}, b'too large'); refused({12: (1 << 39)}, b'too large')
    for i in range(10):
        refused({i: base[i] + 2}, b'aligned')
    # overlapping in / out ranges: an output that starts inside an input, an input that starts inside the (twice as long) output,
    # in place, two outputs on each other, the coefficients inside an output
    refused({7: base[0]}, b'x_mix and x_s overlap')
    refused({7: base[0] + 4 * (3 * 105 - 1)}, b'x_mix and x_s overlap')
    refused({1: base[7] + 4 * (2 * 3 * 105 - 1)}, b'x_mix and x_t overlap')
    refused({8: base[3]}, b'hm_mix and hm_t overlap')
    refused({9: base[4] + 4}, b'w_mix and w_s overlap')
    refused({8: base[7] + 4 * 3 * 105}, b'x_mix and hm_mix overlap')
    refused({6: base[9] + 4 * (2 * 3 * 21 - 1)}, b'w_mix and lam overlap')
    refused({9: base[0] + 4 * 100}, b'w_mix and x_s overlap')
    # (every call above is refused before a launch: the addresses are fake.  Ranges that only touch, which are accepted, are
    #  walked by the stand-alone driver of tests/test_host_mixup.py, which hides the GPU from itself.)
