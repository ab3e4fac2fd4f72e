"""Gradient-norm clipping, CPU side: the numpy reference tests/gradclip_ref.py against torch (clip_grad_norm_ + SGD with Nesterov
momentum in float64; the float32 coefficient bit for bit), the --clip-grad-norm switch of the parser, the refused arguments of
the three entry points (mi355_grad_sumsq_batched, mi355_grad_clip_coef, mi355_sgd_nesterov_clipped) and of their wrappers, and
GradClipper's refusal of optimizers that are not FusedSGD.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gradclip_ref as ref
from conftest import PKG


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


@pytest.mark.parametrize('nesterov', [True, False])
def test_reference_equals_torch_in_float64_over_five_steps(nesterov):
    rng = np.random.default_rng(5)
    shapes, lr, mu, wd, max_norm = [(7, 5), (33,), (4, 3, 3)], 0.1, 0.9, 1e-4, 4.0
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    opt = torch.optim.SGD(ps, lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov)
    p_ref = [p.detach().numpy().copy() for p in ps]
    b_ref = [np.zeros(s) for s in shapes]
    clipped = []
    for it in range(5):
        gs = [rng.standard_normal(s) * (0.2 if it % 2 else 2.0) for s in shapes]      # norms on both sides of max_norm
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        ss, norm, coef, skip = ref.clip_record(gs, max_norm, np.float64)
        assert skip == 0 and abs(norm - float(total)) <= 1e-12 * float(total)
        clipped.append(coef < 1.0)
        for i in range(len(ps)):
            p_ref[i], b_ref[i] = ref.sgd_step(p_ref[i], gs[i], b_ref[i], lr, coef, skip, mu, wd, nesterov, np.float64)
            assert np.abs(p_ref[i] - ps[i].detach().numpy()).max() <= 1e-12
            assert np.abs(b_ref[i] - opt.state[ps[i]]['momentum_buffer'].numpy()).max() <= 1e-12
    assert any(clipped) and not all(clipped)


def test_reference_coefficient_is_torchs_float32_expression_bit_for_bit():
    rng = np.random.default_rng(6)
    norms = np.concatenate([rng.uniform(0, 8, 2000), 10.0 ** rng.uniform(-8, 8, 2000), [0.0, 1.0, 4.0]]).astype(np.float32)
    for max_norm in (0.5, 1.0, 4.0, float('inf')):
        t = torch.from_numpy(norms)
        want = torch.clamp(max_norm / (t + 1e-6), max=1.0).numpy()
        got = np.array([ref.norm_coef_skip(np.float64(n) ** 2, max_norm)[1] for n in norms], dtype=np.float32)
        # (norm -> norm ** 2 -> sqrt is the identity on float32 values in float64)
        assert np.array_equal(np.array([ref.norm_coef_skip(np.float64(n) ** 2, max_norm)[0] for n in norms]), norms)
        assert got.tobytes() == want.tobytes()
    for bad in (float('inf'), float('nan')):
        norm, coef, skip = ref.norm_coef_skip(bad, 1.0)
        assert skip == 1 and coef == 0.0
    p, b = ref.sgd_step([1.0, 2.0], [np.nan, 1.0], [0.5, 0.5], 0.1, 0.0, 1, 0.9, 1e-4, True)
    assert p.tolist() == [1.0, 2.0] and b.tolist() == [0.5, 0.5]


def test_parser_has_the_switch_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    parse = train1.build_parser().parse_args
    a = parse(['data/H3D'])
    assert a.clip_grad_norm == 0
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    assert parse(['d', '--clip-grad-norm', 'inf']).clip_grad_norm == float('inf')
    assert parse(['d', '--clip-grad-norm', '2.5']).clip_grad_norm == 2.5
    for bad in ('-1', 'nan', '-inf'):
        with pytest.raises(SystemExit):
            parse(['d', '--clip-grad-norm', bad])
        assert '--clip-grad-norm' in capsys.readouterr().err


def test_entry_points_refuse_bad_arguments_without_a_gpu(lib_path):
    import mi355
    lib = mi355.load()
    for name in ('mi355_grad_sumsq_batched', 'mi355_grad_clip_coef', 'mi355_sgd_nesterov_clipped'):
        assert name in mi355.SIGNATURES and hasattr(lib, name)
    P = lambda i, off=0: 0x100000000 + (i << 28) + off
    err = lambda: lib.mi355_last_error().decode()
    ss = lambda items=P(1), count=3, blocks=5, partials=P(2): lib.mi355_grad_sumsq_batched(items, count, blocks, partials, None)
    assert ss(items=None) == -1 and 'null' in err()
    assert ss(partials=None) == -1 and 'null' in err()
    assert ss(count=0) == -1 and 'count=0' in err()
    assert ss(count=-3) == -1 and 'count=-3' in err()
    assert ss(blocks=0) == -1 and 'total_blocks=0' in err()
    assert ss(blocks=-1) == -1 and 'total_blocks=-1' in err()
    assert ss(count=6, blocks=5) == -1 and 'total_blocks=5' in err()
    cc = lambda partials=P(2), blocks=5, rec=P(3): lib.mi355_grad_clip_coef(partials, blocks, rec, None)
    assert cc(partials=None) == -1 and 'null' in err()
    assert cc(rec=None) == -1 and 'null' in err()
    assert cc(blocks=0) == -1 and 'total_blocks=0' in err()
    assert cc(rec=P(3, 4)) == -1 and 'aligned' in err()
    sgd = lambda p=P(1), g=P(2), buf=P(3), n=100, lr=P(4), rec=P(5): lib.mi355_sgd_nesterov_clipped(p, g, buf, n, lr, rec, 0.9, 1e-4, 1, None, None)
    for k in ('p', 'g', 'buf', 'lr', 'rec'):
        assert sgd(**{k: None}) == -1 and 'null' in err(), k
    assert sgd(n=0) == -1 and 'n=0' in err()
    assert sgd(n=-4) == -1 and 'n=-4' in err()
    for off in (4, 8, 12):
        for k, i in (('p', 1), ('g', 2), ('buf', 3)):
            assert sgd(**{k: P(i, off)}) == -1 and '16-byte aligned' in err(), (k, off)
    # the existing entry point answers as before
    assert lib.mi355_sgd_nesterov(0, 0, 0, 0, 0, 0.9, 0.0, 1, 0, 0) == -1


def test_wrappers_refuse_cpu_tensors_and_short_buffers(lib_path):
    import mi355
    from mi355 import ops
    assert ops.GN_CHUNK == 16384 and ops.clip_rec_dtype().itemsize == ops.CLIP_REC_BYTES == 32
    g = torch.zeros(16)
    with pytest.raises(mi355.Mi355Error):
        ops.gn_table([g], 'cpu')
    with pytest.raises(mi355.Mi355Error):
        ops.gn_table([], 'cpu')
    with pytest.raises(mi355.Mi355Error):
        ops.grad_sumsq_batched(torch.zeros(24, dtype=torch.uint8), 1, 1, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(mi355.Mi355Error):
        ops.grad_clip_coef(torch.zeros(1, dtype=torch.float64), 1, torch.zeros(32, dtype=torch.uint8))
    with pytest.raises(mi355.Mi355Error):
        ops.sgd_nesterov_clipped(g, g, g, torch.zeros(()), torch.zeros(32, dtype=torch.uint8), 0.9, 0.0, True)
    rec = ops.clip_records(3, 2.5, 'cpu').numpy().view(ops.clip_rec_dtype())
    assert rec['max_norm'].tolist() == [2.5] * 3 and not rec['n_skipped'].any() and not rec['skip'].any()


def test_grad_clipper_takes_fused_sgd_only_and_a_positive_norm():
    from mi355.optim import FusedSGD, GradClipper
    clip = GradClipper(1.0, 'cpu')
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(TypeError):
        clip.measure([torch.optim.SGD([p], lr=0.1)], 'a')
    with pytest.raises(TypeError):
        clip.measure([FusedSGD([p], lr=0.1), torch.optim.SGD([p], lr=0.1)], 'b')
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            GradClipper(bad, 'cpu')
    norms, skipped = GradClipper(float('inf'), 'cpu').read()
    assert set(norms) == {'a', 'b', 'c'} and skipped == 0
    # the optimizer keeps torch's state_dict layout: no key of the clipper in defaults or param_groups
    opt = FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    assert set(opt.defaults) == {'lr', 'momentum', 'dampening', 'weight_decay', 'nesterov'}
    assert set(opt.state_dict()['param_groups'][0]) == set(torch.optim.SGD([p], lr=0.1).state_dict()['param_groups'][0]) & \
        set(opt.state_dict()['param_groups'][0])
