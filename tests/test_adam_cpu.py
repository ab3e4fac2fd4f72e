"""Adam / AdamW, CPU side: the --optimizer / --adam-betas / --adam-eps switches of the parser, FusedAdam's constructor against
torch.optim.Adam's (defaults, param_groups keys, refusals, wording of the errors), the state-dict round trip with torch on CPU
tensors, the float32 restatement tests/adam_ref.py against torch.optim.Adam / AdamW within the bound of tests/test_gpu_adam.py,
the refused arguments of mi355_adam_step_batched / mi355_adam_tick_batched and of their wrappers, GradClipper's acceptance of
FusedAdam, and FusedSGD's unchanged defaults.  No GPU."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import adam_ref as ref
from conftest import PKG


@pytest.fixture(scope='module')
def lib_path():
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_parser_has_the_switches_and_keeps_the_reference_defaults(capsys):
    import train1
    from test_cli import REF_DEFAULTS
    parse = train1.build_parser().parse_args
    a = parse(['data/H3D'])
    assert a.optimizer == 'sgd' and tuple(a.adam_betas) == (0.9, 0.999) and a.adam_eps == 1e-8
    for k, v in REF_DEFAULTS.items():
        assert getattr(a, k) == v, k
    a = parse(['d', '--optimizer', 'adamw', '--adam-betas', '0.8', '0.95', '--adam-eps', '1e-6'])
    assert a.optimizer == 'adamw' and tuple(a.adam_betas) == (0.8, 0.95) and a.adam_eps == 1e-6
    assert parse(['d', '--optimizer', 'adam']).optimizer == 'adam'
    for bad, flag in ((['--optimizer', 'rmsprop'], '--optimizer'), (['--optimizer', 'adam', '--adam-betas', '0.9', '1.0'], '--adam-betas'),
                      (['--optimizer', 'adam', '--adam-betas', '0.9'], '--adam-betas'), (['--optimizer', 'adamw', '--adam-eps', '-1'], '--adam-eps')):
        with pytest.raises(SystemExit):
            parse(['d'] + bad)
        assert flag in capsys.readouterr().err
    text = train1.build_parser().format_help()
    flat = ' '.join(text.split())
    assert '--momentum is ignored' in flat and 'placeholder' in flat and 'has not been measured' in flat


def test_constructor_follows_torch_and_refuses_what_is_not_built():
    from mi355.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(3))
    mine, theirs = FusedAdam([p]), torch.optim.Adam([p])
    assert mine.defaults == theirs.defaults
    assert list(mine.state_dict()['param_groups'][0]) == list(theirs.state_dict()['param_groups'][0])
    assert mine.state_dict()['param_groups'] == theirs.state_dict()['param_groups']
    w_mine, w_theirs = FusedAdam([p], decoupled=True), torch.optim.AdamW([p])
    assert w_mine.defaults == w_theirs.defaults and w_mine.defaults['weight_decay'] == 1e-2
    assert FusedAdam([p], weight_decay=0.0, decoupled=True).defaults['weight_decay'] == 0.0
    assert FusedAdam([p], lr=3e-4, betas=(0.5, 0.75), eps=0.0, weight_decay=0.1).defaults == \
        torch.optim.Adam([p], lr=3e-4, betas=(0.5, 0.75), eps=0.0, weight_decay=0.1).defaults
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(capturable=True), dict(differentiable=True), dict(fused=True)):
        with pytest.raises(NotImplementedError):
            FusedAdam([p], **kw)
    FusedAdam([p], amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
    with pytest.raises(TypeError):
        FusedAdam([p], nesterov=True)
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError) as mine_err:
            FusedAdam([p], **kw)
        with pytest.raises(ValueError) as torch_err:
            torch.optim.Adam([p], **kw)
        assert str(mine_err.value) == str(torch_err.value)


def _params(rng, shapes, dtype=torch.float32):
    return [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s)).to(dtype)) for s in shapes]


def test_state_dict_round_trip_with_torch_on_cpu_tensors():
    from mi355.optim import FusedAdam
    rng = np.random.default_rng(11)
    shapes = [(7, 5), (33,), (4, 3, 3)]
    for decoupled, cls in ((False, torch.optim.Adam), (True, torch.optim.AdamW)):
        ps = _params(rng, shapes)
        theirs = cls(ps, lr=1e-2, betas=(0.8, 0.9), weight_decay=0.05)
        for _ in range(3):
            for p in ps[:2]:                                   # (the third never gets a gradient: no state, as in torch)
                p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape))).float()
            theirs.step()
        sd = theirs.state_dict()
        mine = FusedAdam(ps, decoupled=decoupled)
        mine.load_state_dict(copy.deepcopy(sd))
        back = mine.state_dict()
        assert back['param_groups'] == sd['param_groups'] and sorted(back['state']) == sorted(sd['state']) == [0, 1]
        for k, st in sd['state'].items():
            assert sorted(back['state'][k]) == sorted(st) == ['exp_avg', 'exp_avg_sq', 'step']
            assert back['state'][k]['step'].dtype == torch.float32 and back['state'][k]['step'].dim() == 0
            assert float(back['state'][k]['step']) == 3.0
            for name in st:
                assert torch.equal(back['state'][k][name], st[name]), (k, name)
        # and into a fresh torch optimizer, which then steps
        again = cls(ps)
        again.load_state_dict(copy.deepcopy(back))
        for p in ps[:2]:
            p.grad = torch.ones_like(p)
        again.step()
        assert float(again.state_dict()['state'][0]['step']) == 4.0
        assert again.param_groups[0]['decoupled_weight_decay'] == decoupled


@pytest.mark.parametrize('decoupled', [False, True])
def test_float32_restatement_follows_torch_within_the_bound_over_six_steps(decoupled):
    rng = np.random.default_rng(12 + decoupled)
    shapes, hyper = [(17, 5), (33,), (4, 3, 3)], dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    p0 = [rng.standard_normal(s) for s in shapes]
    ps32 = [torch.nn.Parameter(torch.from_numpy(x).float()) for x in p0]
    opt32 = cls(ps32, **hyper)
    # the restatement takes what a FusedAdam group holds, as the table rows of FusedAdam.step() do
    from mi355.optim import FusedAdam
    gr = FusedAdam(ps32, decoupled=decoupled, **hyper).param_groups[0]
    assert {k: v for k, v in gr.items() if k != 'params'} == {k: v for k, v in opt32.param_groups[0].items() if k != 'params'}
    args = (gr['lr'],) + tuple(gr['betas']) + (gr['eps'], gr['weight_decay'], gr['decoupled_weight_decay'])
    assert args == (hyper['lr'],) + hyper['betas'] + (hyper['eps'], hyper['weight_decay'], decoupled)
    s64 = [(x.astype(np.float32).astype(np.float64), np.zeros(x.shape), np.zeros(x.shape), 0) for x in p0]
    s32 = [(x.astype(np.float32), np.zeros(x.shape, np.float32), np.zeros(x.shape, np.float32), 0) for x in p0]
    ps64 = [torch.nn.Parameter(torch.from_numpy(x).float().double()) for x in p0]
    opt64 = cls(ps64, **hyper)
    for it in range(6):
        gs = [(rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for s in shapes]
        for i, g in enumerate(gs):
            ps32[i].grad = torch.from_numpy(g.copy())
            ps64[i].grad = torch.from_numpy(g.astype(np.float64))
            s64[i] = ref.adam_step64(s64[i][0], g, s64[i][1], s64[i][2], s64[i][3], *args)
            s32[i] = ref.adam_step32(s32[i][0], g, s32[i][1], s32[i][2], s32[i][3], *args)
        opt32.step(); opt64.step()
        for i in range(len(shapes)):
            st32, st64 = opt32.state[ps32[i]], opt64.state[ps64[i]]
            assert s32[i][3] == s64[i][3] == it + 1 == float(st32['step'])
            # the oracle is torch in float64 to within float64 rounding
            for mine, theirs in zip(s64[i][:3], (ps64[i], st64['exp_avg'], st64['exp_avg_sq'])):
                assert ref.distance(theirs.detach().numpy(), mine) <= 1e-12 * max(1.0, float(np.abs(mine).max()))
            for name, mine, oracle, theirs in zip('pmv', s32[i][:3], s64[i][:3], (ps32[i], st32['exp_avg'], st32['exp_avg_sq'])):
                allowed, d_torch = ref.bound(theirs.detach().numpy(), oracle)
                d = ref.distance(mine, oracle)
                print('step %d tensor %d %s: restatement %.3g  torch %.3g  allowed %.3g' % (it + 1, i, name, d, d_torch, allowed))
                assert d <= allowed, (it, i, name, d, allowed)


def test_entry_points_refuse_bad_arguments_without_a_gpu(lib_path):
    import mi355
    lib = mi355.load()
    for name in ('mi355_adam_step_batched', 'mi355_adam_tick_batched'):
        assert name in mi355.SIGNATURES and hasattr(lib, name)
    P = lambda i, off=0: 0x100000000 + (i << 28) + off
    err = lambda: lib.mi355_last_error().decode()
    step = lambda items=P(1), count=3, blocks=5, rec=P(2): lib.mi355_adam_step_batched(items, count, blocks, rec, None)
    assert step(items=None) == -1 and 'null' in err()
    assert step(count=0) == -1 and 'count=0' in err()
    assert step(count=-3) == -1 and 'count=-3' in err()
    assert step(blocks=0) == -1 and 'total_blocks=0' in err()
    assert step(blocks=-1) == -1 and 'total_blocks=-1' in err()
    assert step(count=6, blocks=5) == -1 and 'total_blocks=5' in err()
    assert step(items=P(1, 4)) == -1 and 'aligned' in err()
    assert step(rec=P(2, 4)) == -1 and 'aligned' in err()
    tick = lambda items=P(1), count=3, rec=P(2): lib.mi355_adam_tick_batched(items, count, rec, None)
    assert tick(items=None) == -1 and 'null' in err()
    assert tick(count=0) == -1 and 'count=0' in err()
    assert tick(count=-1) == -1 and 'count=-1' in err()
    assert tick(items=P(1, 4)) == -1 and 'aligned' in err()
    assert tick(rec=P(2, 4)) == -1 and 'aligned' in err()


def test_wrappers_refuse_cpu_tensors_and_malformed_items(lib_path):
    import mi355
    from mi355 import ops
    assert ops.ADAM_CHUNK == 16384 and ops.adam_item_dtype().itemsize == ops.ADAM_ITEM_BYTES == 88
    assert list(ops.adam_item_dtype().names) == ['p', 'g', 'm', 'v', 'step', 'lr', 'n', 'beta1', 'beta2', 'eps', 'wd', 'decoupled', 'blk0']
    x, s = torch.zeros(16), torch.zeros(())
    with pytest.raises(mi355.Mi355Error):
        ops.adam_table([(x, x, x, x, s, s, 0.9, 0.999, 1e-8, 0.0, False)], 'cpu')
    with pytest.raises(mi355.Mi355Error):
        ops.adam_table([], 'cpu')
    table = torch.zeros(88, dtype=torch.uint8)
    with pytest.raises(mi355.Mi355Error):
        ops.adam_step_batched(table, 1, 1)
    with pytest.raises(mi355.Mi355Error):
        ops.adam_tick_batched(table, 1)
    with pytest.raises(mi355.Mi355Error):
        ops.adam_step_batched(table, 1, 1, torch.zeros(32, dtype=torch.uint8))


def test_grad_clipper_takes_fused_adam_and_still_refuses_torch_optimizers():
    from mi355.optim import FusedAdam, FusedSGD, GradClipper, check_state_dict_kind, make_optimizer, state_dict_kind
    clip = GradClipper(1.0, 'cpu')
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(TypeError):
        clip.measure([torch.optim.Adam([p])], 'a')
    with pytest.raises(TypeError):
        clip.measure([FusedAdam([p]), torch.optim.SGD([p], lr=0.1)], 'b')
    with pytest.raises(TypeError):
        clip.measure([FusedSGD([p], lr=0.1), torch.optim.AdamW([p])], 'c')
    # (a FusedAdam passes the type check: what follows needs the GPU and is tests/test_gpu_adam.py's)
    adam, adamw, sgd = (make_optimizer(k, [p], lr=0.1, momentum=0.9, weight_decay=1e-4) for k in ('adam', 'adamw', 'sgd'))
    assert type(adam) is type(adamw) is FusedAdam and type(sgd) is FusedSGD
    assert not adam.defaults['decoupled_weight_decay'] and adamw.defaults['decoupled_weight_decay']
    assert adam.defaults['weight_decay'] == adamw.defaults['weight_decay'] == 1e-4 and sgd.defaults['nesterov']
    with pytest.raises(ValueError):
        make_optimizer('lion', [p], lr=0.1)
    assert state_dict_kind(adamw.state_dict()) == 'adam' and state_dict_kind(sgd.state_dict()) == 'sgd'
    assert state_dict_kind(torch.optim.AdamW([p]).state_dict()) == 'adam'
    check_state_dict_kind(adam, adamw.state_dict()); check_state_dict_kind(sgd, sgd.state_dict())
    for opt, sd in ((adam, sgd.state_dict()), (sgd, adamw.state_dict())):
        with pytest.raises(ValueError) as e:
            check_state_dict_kind(opt, sd)
        assert 'SGD' in str(e.value) and 'Adam' in str(e.value)


def test_fused_sgd_keeps_its_constructor_defaults_and_state_layout():
    import inspect
    from mi355.optim import FusedSGD
    sig = inspect.signature(FusedSGD.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == \
        [('lr', 1e-3), ('momentum', 0.0), ('dampening', 0), ('weight_decay', 0.0), ('nesterov', False)]
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    assert opt.defaults == dict(lr=0.1, momentum=0.9, dampening=0, weight_decay=0.0, nesterov=True)
    assert FusedSGD._BUFFERS == (('momentum_buffer', 'M'),) and FusedSGD._COUNTER is None
    assert not opt.is_flat and opt.flat_range([p]) is None
    with pytest.raises(NotImplementedError):
        FusedSGD([p], dampening=0.1)
