"""tests/resume_ref.py on hand-made inputs, and utils.checkpoint (the functions train1.py saves and resumes with) on torch-native
stand-ins for the model and the optimizers.  No GPU."""
import argparse
import copy
import os
import struct
import types

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (puts the package on sys.path)
import resume_ref


def _f32(bits):
    return np.frombuffer(struct.pack('<I', bits), dtype='<f4').copy()


def _line(it, **named):
    return dict(it=it, **resume_ref.fingerprint(named))


# ---------------------------------------------------------------- fingerprints
def test_digest_sees_bytes_not_values():
    qnan, payload = _f32(0x7fc00000), _f32(0x7fc00001)
    assert np.isnan(qnan).all() and np.isnan(payload).all()
    assert resume_ref.digest(qnan) != resume_ref.digest(payload)                 # two NaNs, different payloads
    assert resume_ref.digest(qnan) == resume_ref.digest(_f32(0x7fc00000))
    assert resume_ref.digest(np.float32([0.0])) != resume_ref.digest(np.float32([-0.0]))
    assert resume_ref.digest(0.0) != resume_ref.digest(-0.0)
    assert resume_ref.digest(torch.tensor([0.0])) != resume_ref.digest(torch.tensor([-0.0]))
    # dtype and shape are part of it
    assert resume_ref.digest(np.zeros(4, np.float32)) != resume_ref.digest(np.zeros((2, 2), np.float32))
    assert resume_ref.digest(np.zeros(4, np.float32)) != resume_ref.digest(np.zeros(4, np.int32))
    assert resume_ref.digest(torch.zeros(2, dtype=torch.bfloat16)) == resume_ref.digest(np.zeros(2, np.int16))
    assert resume_ref.digest([0.1, 0.2]) != resume_ref.digest([0.1, 0.2000000000000001])
    assert resume_ref.digest(torch.arange(6).reshape(2, 3).t()) == resume_ref.digest(np.arange(6).reshape(2, 3).T.copy())


def test_first_difference_names_iteration_and_tensor():
    a = [_line(5, w=np.float32([1, 2]), m=np.float32([0])), _line(6, w=np.float32([1, 3]), m=np.float32([0])),
         _line(7, w=np.float32([1, 4]), m=np.float32([1]))]
    same = copy.deepcopy(a)
    assert resume_ref.first_difference(a, same) is None and resume_ref.describe_difference(a, same) is None
    b = copy.deepcopy(a)
    b[1] = _line(6, w=np.float32([1, 3]), m=np.float32([-0.0]))                   # -0.0 against 0.0, at iteration 6, in m
    b[2] = _line(7, w=np.float32([9, 9]), m=np.float32([5]))
    assert resume_ref.first_difference(a, b) == (6, 'm')
    assert resume_ref.first_difference(a, b, [5]) is None and resume_ref.first_difference(a, b, [7]) == (7, 'm')
    assert 'iteration 6 in m' in resume_ref.describe_difference(a, b)
    nan_a, nan_b = [_line(0, x=_f32(0x7fc00000))], [_line(0, x=_f32(0x7fc00123))]
    assert resume_ref.first_difference(nan_a, nan_b) == (0, 'x')
    # a missing line and a missing tensor are differences
    assert resume_ref.first_difference(a, a[:2]) == (7, '<missing in b>')
    assert resume_ref.first_difference(a[1:], a) == (5, '<missing in a>')
    c = copy.deepcopy(a)
    c[0] = _line(5, w=np.float32([1, 2]))
    assert resume_ref.first_difference(a, c) == (5, 'm <missing in b>')
    # the resumed run has lines 5.. only: asked about those, the uninterrupted run's earlier lines do not matter
    assert resume_ref.first_difference([_line(0, w=np.float32([0]))] + a, a, range(5, 8)) is None


def test_count_differences_counts_elements_by_bytes():
    fa = {'w': np.float32([0.0, 1.0, np.nan, 3.0]), 'n': np.int64(7), 'only_a': np.zeros(3, np.float32)}
    fb = {'w': np.float32([-0.0, 1.0, np.nan, 4.0]), 'n': np.int64(7)}
    fb['w'][2:3] = _f32(0x7fc00055)
    assert resume_ref.count_differences(fa, fa) == {}
    assert resume_ref.count_differences(fa, fb) == {'w': 3, 'only_a': 3}
    assert resume_ref.count_differences({'w': np.zeros(4, np.float32)}, {'w': np.zeros(4, np.int32)}) == {'w': 4}
    msg = resume_ref.describe_difference([_line(9, w=fa['w'])], [_line(9, w=fb['w'])], None, fa, fb)
    assert 'iteration 9 in w' in msg and '2 tensors differ' in msg and 'w in 3 elements' in msg


# ---------------------------------------------------------------- checkpoints
def _fake_checkpoint():
    sd = lambda: {'state': {0: {'momentum_buffer': torch.ones(3)}, 1: {'momentum_buffer': torch.full((2,), 2.0)}},
                  'param_groups': [{'lr': 0.01, 'momentum': 0.9, 'params': [0, 1]}]}
    sched = lambda: {'last_epoch': 5, '_step_count': 6, '_last_lr': [0.0099], 'base_lrs': [0.1]}
    ck = {'model': {'bn.weight': torch.ones(2), 'bn.running_mean': torch.zeros(2), 'bn.running_var': torch.full((2,), 0.5),
                    'bn2.running_var': torch.full((2,), 0.25)},
          'epoch': 0, 'args': argparse.Namespace(lr=0.1, arch='resnet18'), 'gl_iter_num': 5,
          'ema_state': {'step': 5, 'decay': 0.999, 'warmup': True},
          'proto_state': {'memory_s': torch.ones(2, 2), 'memory_t': torch.zeros(2, 2), 'm': 0.9},
          'mixup_state': {'rng_state': torch.arange(8, dtype=torch.uint8), 'draws': 5, 'lam': torch.ones(2)},
          'fp8_state': {'pools': {0: {'fmt': 0, 'used': 1, 'owners': ['a/_q_in'], 'buf': torch.ones(4)}}}}
    for k in ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'):
        ck['optimizer_' + k], ck['lr_scheduler_' + k] = sd(), sched()
    return ck


def test_compare_checkpoints_names_the_keys():
    a, b = _fake_checkpoint(), _fake_checkpoint()
    assert resume_ref.compare_checkpoints(a, b) == []
    b['model']['bn.running_mean'] = torch.tensor([0.0, -0.0])
    b['optimizer_h']['state'][1]['momentum_buffer'][0] = 3.0
    b['lr_scheduler_f']['_last_lr'] = [0.0098]
    b['args'].lr = 0.2
    del b['gl_iter_num']
    assert resume_ref.compare_checkpoints(a, b) == ['/args/lr', '/gl_iter_num', '/lr_scheduler_f/_last_lr', '/model/bn.running_mean',
                                                    '/optimizer_h/state/1/momentum_buffer']
    assert resume_ref.compare_checkpoints(a, b, ignore=('/args', '/gl_iter_num', '/lr_', '/model/')) == ['/optimizer_h/state/1/momentum_buffer']


@pytest.mark.parametrize('piece', sorted(resume_ref.DOCTORS))
def test_every_doctoring_touches_one_piece_only(piece):
    ck = _fake_checkpoint()
    before = copy.deepcopy(ck)
    out = resume_ref.doctor(piece, ck)
    assert resume_ref.compare_checkpoints(ck, before) == []                      # the input is not written
    bad = resume_ref.compare_checkpoints(before, out)
    want = {'none': [], 'model_ema.pth': [], 'running_var': ['/model/bn.running_var'],
            'optimizer_f': ['/optimizer_f/state/0/momentum_buffer', '/optimizer_f/state/1/momentum_buffer'],
            'lr_scheduler_f': ['/lr_scheduler_f/_step_count', '/lr_scheduler_f/last_epoch']}.get(piece)
    if want is None:                             # a dropped key: every leaf below it, nothing else
        assert piece not in out and bad and all(k.startswith('/%s/' % piece) or k == '/' + piece for k in bad)
    else:
        assert bad == want
    if piece == 'optimizer_f':
        assert all(not v['momentum_buffer'].any() for v in out['optimizer_f']['state'].values())
    if piece == 'running_var':
        assert out['model']['bn.running_var'].tolist() == [1.0, 1.0] and out['model']['bn2.running_var'].tolist() == [0.25, 0.25]
    assert resume_ref.keeps_ema_file(piece) == (piece != 'model_ema.pth')
    assert all(p in resume_ref.DOCTORS for ps in resume_ref.PIECES.values() for p in ps)


# ---------------------------------------------------------------- utils.checkpoint on stand-ins
class _Net(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.backbone = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
        self.heads = torch.nn.ModuleDict({k: torch.nn.Linear(4, 2) for k in ('h', 'h_adv', 'h_adv2', 'h_adv3')})
        self.gl_layer = types.SimpleNamespace(iter_num=0)


class _State:
    """Stands for the EMATeacher, the prototype term and the mixup: something with a state_dict."""

    def __init__(self, **kw):
        self.kw, self.loaded = kw, None

    def state_dict(self):
        return dict(self.kw)

    def load_state_dict(self, state, *a):
        self.loaded = state


def _standins(kind=torch.optim.SGD, seed=0, **terms):
    from torch.optim.lr_scheduler import LambdaLR
    model, model_ema = _Net(seed), _Net(seed + 100)
    mk = (lambda ps: kind(ps, lr=0.1, momentum=0.9)) if kind is torch.optim.SGD else (lambda ps: kind(ps, lr=0.1))
    opts = {'f': mk(model.backbone.parameters())}
    opts.update({k: mk(model.heads[k].parameters()) for k in ('h', 'h_adv', 'h_adv2', 'h_adv3')})
    scheds = {k: LambdaLR(o, lambda x: 0.01 * (1. + 1e-4 * float(x)) ** -0.75) for k, o in opts.items()}
    step = types.SimpleNamespace(proto=terms.get('proto'), mixup=terms.get('mixup'))
    return model, model_ema, opts, scheds, step


def _train_a_little(model, opts, scheds, n=3):
    for i in range(n):
        loss = model.backbone(torch.ones(1, 3, 5, 5) * (i + 1)).sum() + sum(h(torch.ones(4)).sum() for h in model.heads.values())
        loss.backward()
        for o in opts.values():
            o.step(); o.zero_grad()
        for s in scheds.values():
            s.step()
        model.gl_layer.iter_num += 1


def test_save_writes_the_reference_keys_and_the_additive_ones(tmp_path):
    from utils import checkpoint as C
    args = argparse.Namespace(ema_model=None, lr=0.1)
    model, model_ema, opts, scheds, step = _standins()
    path = str(tmp_path / '3.pth')
    C.save_training_state(path, 3, args, model, model_ema, opts, scheds, step, None)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ck) == set(C.REFERENCE_KEYS) | set(C.ADDITIVE_KEYS)
    assert set(C.REFERENCE_KEYS) == {'model', 'optimizer_f', 'optimizer_h', 'optimizer_h_adv', 'lr_scheduler_f', 'lr_scheduler_h',
                                     'lr_scheduler_h_adv', 'epoch', 'args'}
    assert ck['epoch'] == 3 and ck['args'].lr == 0.1 and ck['gl_iter_num'] == 0
    beside = torch.load(str(tmp_path / 'model_ema.pth'), map_location='cpu', weights_only=False)
    assert set(beside) == {'model_ema'} and resume_ref.compare_checkpoints(beside['model_ema'], model_ema.state_dict()) == []
    # each optional piece adds its own key and no other (fp8_state: only in 'fp8' mode, which needs the GPU)
    model, model_ema, opts, scheds, step = _standins(proto=_State(m=0.9), mixup=_State(draws=2))
    C.save_training_state(path, 4, args, model, model_ema, opts, scheds, step, _State(step=7))
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ck) == set(C.REFERENCE_KEYS) | set(C.ADDITIVE_KEYS) | {'ema_state', 'proto_state', 'mixup_state'}
    assert set(ck) - set(C.REFERENCE_KEYS) - set(C.ADDITIVE_KEYS) <= set(C.OPTIONAL_KEYS)
    assert ck['ema_state'] == {'step': 7} and ck['proto_state'] == {'m': 0.9} and ck['mixup_state'] == {'draws': 2}


def test_load_restores_what_save_wrote(tmp_path):
    from utils import checkpoint as C
    args = argparse.Namespace(ema_model=None)
    model, model_ema, opts, scheds, step = _standins(proto=_State(m=0.9), mixup=_State(draws=2))
    _train_a_little(model, opts, scheds)
    with torch.no_grad():
        for p in model_ema.parameters():
            p.add_(1.0)                                                          # a teacher that is not the model
    path = str(tmp_path / '0.pth')
    C.save_training_state(path, 0, args, model, model_ema, opts, scheds, step, _State(step=3))
    m2, e2, o2, s2, st2 = _standins(seed=9, proto=_State(), mixup=_State())
    ema2 = _State()
    assert C.load_training_state(path, args, m2, e2, o2, s2, st2, ema2, 'cpu') == 1
    same = lambda a, b: resume_ref.compare_checkpoints(a, b) == []
    assert same(m2.state_dict(), model.state_dict()) and same(e2.state_dict(), model_ema.state_dict())
    assert not same(e2.state_dict(), model.state_dict())
    assert all(same(o2[k].state_dict(), opts[k].state_dict()) and same(s2[k].state_dict(), scheds[k].state_dict()) for k in opts)
    assert m2.gl_layer.iter_num == 3 and s2['f'].last_epoch == 3
    assert ema2.loaded == {'step': 3} and st2.proto.loaded == {'m': 0.9} and st2.mixup.loaded == {'draws': 2}
    # without a teacher to keep up to date (--ema-update off) model_ema still takes the file beside the checkpoint: the frozen
    # teacher of the saved run; --ema_model is not consulted
    m3, e3, o3, s3, st3 = _standins(seed=11)
    assert C.load_training_state(path, argparse.Namespace(ema_model=str(tmp_path / 'nowhere.pth')), m3, e3, o3, s3, st3, None, 'cpu') == 1
    assert same(e3.state_dict(), model_ema.state_dict()) and same(m3.state_dict(), model.state_dict())
    # --ema_model goes before the file beside the checkpoint; with neither the teacher starts as the model
    other = str(tmp_path / 'other.pth')
    torch.save({'model_ema': _Net(77).state_dict()}, other)
    m4, e4, o4, s4, st4 = _standins(seed=12)
    C.load_training_state(path, argparse.Namespace(ema_model=other), m4, e4, o4, s4, st4, _State(), 'cpu')
    assert same(e4.state_dict(), _Net(77).state_dict())
    os.remove(str(tmp_path / 'model_ema.pth'))
    m5, e5, o5, s5, st5 = _standins(seed=13)
    C.load_training_state(path, args, m5, e5, o5, s5, st5, _State(), 'cpu')
    assert same(e5.state_dict(), model.state_dict())
    m7, e7, o7, s7, st7 = _standins(seed=15)
    C.load_training_state(path, args, m7, e7, o7, s7, st7, None, 'cpu')          # (and without a teacher, as the reference's resume)
    assert same(e7.state_dict(), model.state_dict())
    # a checkpoint of the reference's own layout (none of the additive keys) loads as before
    ck = torch.load(path, map_location='cpu', weights_only=False)
    for k in C.ADDITIVE_KEYS + C.OPTIONAL_KEYS:
        ck.pop(k, None)
    torch.save(ck, path)
    m6, e6, o6, s6, st6 = _standins(seed=14, proto=_State(), mixup=_State())
    fresh = copy.deepcopy(o6['h_adv3'].state_dict())
    assert C.load_training_state(path, args, m6, e6, o6, s6, st6, _State(), 'cpu') == 1
    assert m6.gl_layer.iter_num == 0 and st6.proto.loaded is None and same(o6['h_adv3'].state_dict(), fresh)
    assert same(o6['f'].state_dict(), opts['f'].state_dict())


def test_load_refuses_the_other_kind_of_optimizer(tmp_path):
    from utils import checkpoint as C
    args = argparse.Namespace(ema_model=None)
    model, model_ema, opts, scheds, step = _standins(kind=torch.optim.Adam)
    _train_a_little(model, opts, scheds, 1)
    path = str(tmp_path / '0.pth')
    C.save_training_state(path, 0, args, model, model_ema, opts, scheds, step, None)
    m2, e2, o2, s2, st2 = _standins()
    with pytest.raises(SystemExit) as e:
        C.load_training_state(path, args, m2, e2, o2, s2, st2, None, 'cpu')
    assert str(e.value) == ('--resume %s: optimizer_f was written by Adam / AdamW (--optimizer adam | adamw) but this run builds SGD '
                            '(--optimizer sgd); resume with the optimizer the checkpoint was trained with' % path)


# ---------------------------------------------------------------- fp8_state: the records and their owners (host logic only)
def test_fp8_records_go_back_to_their_owners_in_slot_order(monkeypatch):
    import mi355
    from mi355 import nn as mnn
    pools = {}

    def alloc(device, fmt):                      # mi355.fp8_alloc_state on host memory
        pool = pools.setdefault((0, int(fmt)), dict(buf=torch.zeros(64), used=0, fmt=int(fmt)))
        pool['used'] += 1
        return pool['buf'][4 * pool['used'] - 4: 4 * pool['used']]

    monkeypatch.setattr(mi355, '_fp8_pools', pools)
    monkeypatch.setattr(mi355, 'fp8_alloc_state', alloc)

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._packed8, self._q_in, self._q_dy = mnn._PackedFp8(), mnn._Fp8Stream(0), mnn._Fp8Stream(1)

    net = lambda n=2: torch.nn.Sequential(*[Layer() for _ in range(n)])
    assert mnn.fp8_state_dict(net()) is None                                     # no pool: nothing to keep
    a = net()
    order = [(a[1]._q_in, 0), (a[0]._packed8, 0), (a[1]._q_dy, 1), (a[0]._q_in, 0)]          # first use, not module order
    for i, (obj, fmt) in enumerate(order):
        obj.state = alloc('cpu', fmt)
        obj.state.copy_(torch.tensor([2.0 ** i, 2.0 ** -i, 0.0, 2.0 ** -(i + 1)]))
    alloc('cpu', 0).fill_(7.0)                                                   # a record no layer of this model owns
    sd = mnn.fp8_state_dict(a)
    assert sd['pools'][0]['owners'] == ['1/_q_in', '0/_packed8', '0/_q_in', None] and sd['pools'][1]['owners'] == ['1/_q_dy']
    assert sd['pools'][0]['used'] == 4 and sd['pools'][0]['buf'].tolist() == pools[(0, 0)]['buf'][:16].tolist()
    saved = {k: obj.state.clone() for k, (obj, _) in zip('abcd', order)}
    pools.clear()
    b = net()
    mnn.load_fp8_state_dict(b, sd, 'cpu')
    got = [b[1]._q_in, b[0]._packed8, b[1]._q_dy, b[0]._q_in]
    assert all(torch.equal(o.state, saved[k]) for o, k in zip(got, 'abcd'))
    base = pools[(0, 0)]['buf'].data_ptr()
    assert [(o.state.data_ptr() - base) // 16 for o in (got[0], got[1], got[3])] == [0, 1, 2]       # the saved slot order
    assert pools[(0, 0)]['used'] == 3 and pools[(0, 1)]['used'] == 1             # the ownerless record is left out
    assert all(o.ready(torch.device('cpu')) for o in (got[0], got[2], got[3]))   # no stream will take the just-in-time path
    assert torch.equal(b[0]._packed8.restored, saved['b']) and b[1]._packed8.restored is None and b[1]._packed8.state is None
    with pytest.raises(ValueError, match='owns a scaling record already'):
        mnn.load_fp8_state_dict(b, sd, 'cpu')
    used = {k: p['used'] for k, p in pools.items()}
    with pytest.raises(ValueError, match='this model does not have'):
        mnn.load_fp8_state_dict(net(1), sd, 'cpu')
    assert {k: p['used'] for k, p in pools.items()} == used                      # a refused checkpoint takes no slot
