"""EMA teacher, CPU side: the restated update (tests/ema_ref.py) equals what the reference's live update_ema_variables5 /
update_ema_variables2 produced (tests/golden/g11_ema.npz, written by make_golden_ema.py) bit for bit; the command line has
the new switch with the reference's defaults untouched; the two new entry points are in the ctypes table and reject null
arguments before any launch."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG, golden
import ema_ref

KEYS = ['0.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var', '1.num_batches_tracked']


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def _state(g, tag):
    return {k: g['%s/%s' % (tag, k)] for k in KEYS}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_ema_ref_equals_the_reference_bit_for_bit():
    g = golden('g11_ema')
    assert sorted({k.split('/', 1)[1] for k in g.files}) == sorted(KEYS)
    for tag, mom in (('m999', lambda t: 0.999), ('m9', lambda t: 0.9), ('warm', lambda t: ema_ref.warmup_momentum(t, 0.999))):
        ema = _state(g, 'init')
        for t in range(3):
            ema = ema_ref.ema_state(ema, _state(g, 'main%d' % t), mom(t))
            want = _state(g, '%s_%d' % (tag, t))
            for k in KEYS:
                assert _same(ema[k], want[k]), (tag, t, k)
    # the golden is not degenerate: the teacher moves, the counter is copied, the warm-up's first step is a plain copy
    assert not _same(g['m9_0/0.weight'], g['init/0.weight']) and not _same(g['m9_2/0.weight'], g['m9_1/0.weight'])
    assert int(g['m999_1/1.num_batches_tracked']) == int(g['main1/1.num_batches_tracked']) == 10
    assert _same(g['warm_0/1.running_var'], g['main0/1.running_var'])
    assert [ema_ref.warmup_momentum(t, 0.999) for t in range(3)] == [0.0, 0.5, 1 - 1 / 3]


def test_an_fma_or_the_in_place_form_would_not_pass():
    """Why the kernels keep three roundings: contracting either multiply into the add changes bits of the golden case."""
    g = golden('g11_ema')
    e, p, m = g['init/0.weight'].astype(np.float64), g['main0/0.weight'].astype(np.float64), 0.9
    k, c = np.float64(np.float32(m)), np.float64(np.float32(1.0 - m))
    fma = (e * k + np.float64((p * c).astype(np.float32))).astype(np.float32)        # fma(e, k, fl(p * c)): exact product, one rounding
    assert not _same(fma, g['m9_0/0.weight'])


def test_parser_has_the_ema_switch_and_keeps_the_reference_defaults():
    import train1
    from test_cli import REF_DEFAULTS
    a = train1.build_parser().parse_args(['data/H3D'])
    assert a.ema_update == 'off'
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    b = train1.build_parser().parse_args(['d', '--ema-update', 'warmup', '--ema-decay', '0.9', '--ema_model', 'x.pth'])
    assert (b.ema_update, b.ema_decay, b.ema_model) == ('warmup', 0.9, 'x.pth')
    assert train1.build_parser().parse_args(['d', '--ema-update', 'const']).ema_update == 'const'
    for flag in ('--ema_model', '--ema-decay'):
        act = [x for x in train1.build_parser()._actions if flag in x.option_strings][0]
        assert 'unused' not in act.help


def test_ema_entry_points_exist_and_reject_null_arguments(lib_path):
    import mi355
    assert 'mi355_ema_update' in mi355.SIGNATURES and 'mi355_ema_update_batched' in mi355.SIGNATURES
    lib = mi355.load()
    assert lib.mi355_ema_update(0, 0, 16, 0, 0) == -1
    assert b'ema_update' in lib.mi355_last_error()
    assert lib.mi355_ema_update(64, 64, 0, 64, 0) == -1                 # n < 1
    assert lib.mi355_ema_update(68, 64, 16, 64, 0) == -1                # e not 16-byte aligned
    assert b'aligned' in lib.mi355_last_error()
    assert lib.mi355_ema_update_batched(0, 1, 1, 0, 0) == -1
    assert b'ema_update_batched' in lib.mi355_last_error()
    assert lib.mi355_ema_update_batched(64, 0, 1, 64, 0) == -1          # count < 1
    assert lib.mi355_ema_update_batched(64, 1, 0, 64, 0) == -1          # no blocks
