"""EMA teacher on the GPU (mi355_ema_update, mi355_ema_update_batched, mi355.optim.EMATeacher, DAStep's `ema`, the command
lines).  Everything is compared bit for bit: the update is three fp32 roundings (tests/ema_ref.py, equal to the reference's
live functions through tests/golden/g11_ema.npz), so there is no tolerance to choose.

Guards (tests/guarded.py).  The two kernel-level tests and test_batched_table_of_every_tail_length keep the teacher's and the main
model's ranges, the coefficient pair, the counters and the item table in G.place() copies, launch inside a window and check
every flank afterwards.  The kernels update in place (no unwritten check); the comparisons are the ones from before.  The flat
kernel also runs on a range that ends exactly where its flank begins.  EMATeacher, DAStep and the command lines are not guarded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden
import ema_ref
import guarded as G

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guard(label, fn, *args):
    from mi355 import ops
    with G.window(ops, label):
        out = fn(*args)
    torch.cuda.synchronize()
    G.check(label)
    return out

GRID_CAP = 4096                       # blocks of one flat launch (as sgd_kernel): 256 lanes x float4 each per pass
KEYS = ['0.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var', '1.num_batches_tracked']


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


def _coef(m, dev):
    return torch.tensor([m, 1.0 - m], dtype=torch.float64).to(torch.float32).to(dev)


# ---------------------------------------------------------------- the flat kernel
@pytest.mark.parametrize('m', [0.999, 0.5])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025, GRID_CAP * 256 * 4 + 1029])
def test_flat_kernel_bit_exact(gpu, n, m):
    from mi355 import ops
    rng = np.random.default_rng(n % 1000 + int(m * 1000))
    e0 = rng.standard_normal(n + 64).astype(np.float32)
    p0 = rng.standard_normal(n).astype(np.float32)
    e, p = G.place(torch.from_numpy(e0).to(gpu), 'e'), G.place(torch.from_numpy(p0).to(gpu), 'p')
    coef = G.place(_coef(m, gpu), 'coef')
    _guard('ema_update n=%d' % n, ops.ema_update, e[:n], p, coef)
    assert _same(e[:n], ema_ref.ema_array(e0[:n], p0, m))
    assert _same(e[n:], e0[n:])                    # the guard band behind the range
    assert _same(p, p0)                            # the main model's side is only read
    tight = G.place(torch.from_numpy(e0[:n].copy()).to(gpu), 'e, tight')          # ... and a range that ends where its flank begins
    _guard('ema_update tight n=%d' % n, ops.ema_update, tight, p, coef)
    assert _same(tight, ema_ref.ema_array(e0[:n], p0, m)) and _same(p, p0)


def test_flat_wrapper_checks_room(gpu):
    import mi355
    from mi355 import ops
    z = lambda n: torch.zeros(n, device=gpu)
    with pytest.raises(mi355.Mi355Error):
        ops.ema_update(z(100), z(99), z(2))
    with pytest.raises(mi355.Mi355Error):
        ops.ema_update(z(100), z(100), z(1))
    with pytest.raises(mi355.Mi355Error):
        ops.ema_update(z(104)[1:], z(104)[1:], z(2))        # 4 bytes off: the flat entry point wants 16-byte alignment
    with pytest.raises(mi355.Mi355Error):
        ops.ema_update_batched(torch.zeros(32, dtype=torch.uint8, device=gpu), 2, 2, z(2))


# ---------------------------------------------------------------- the batched kernel
def test_batched_kernel_bit_exact(gpu):
    """Six float records (1 .. 70001 elements: less than a chunk, exactly one, one more, many) and two counter copies in ONE
    launch; the float destinations lie in one buffer with gaps between them, the second starts 4 bytes off a 16-byte boundary."""
    from mi355 import ops
    m = 0.9
    sizes = [1, 2, 64, 2048, 2049, 70001]
    rng = np.random.default_rng(5)
    offs, pos = [], 16
    for n in sizes:
        offs.append(pos)
        pos = (pos + n + 16 + 3) // 4 * 4          # next 16-byte boundary behind a gap of at least 16 floats
    offs[1] += 1                                   # 4 bytes off
    total = pos + 16
    d0 = rng.standard_normal(total).astype(np.float32)
    s0 = rng.standard_normal(total).astype(np.float32)
    dst, src = G.place(torch.from_numpy(d0).to(gpu), 'dst'), G.place(torch.from_numpy(s0).to(gpu), 'src')
    assert dst.data_ptr() % 16 == 0 and dst[offs[1]:].data_ptr() % 16 == 4
    cnt_src = G.place(torch.tensor([7, -1, 1 << 40, -1], dtype=torch.int64, device=gpu), 'counters, main')
    cnt_dst = G.place(torch.full((4,), -5, dtype=torch.int64, device=gpu), 'counters, teacher')
    recs = [(src[o:o + n], dst[o:o + n], ops.EMA_F32) for o, n in zip(offs, sizes)]
    recs.insert(2, (cnt_src[0], cnt_dst[0], ops.EMA_COPY64))
    recs.append((cnt_src[2], cnt_dst[2], ops.EMA_COPY64))
    table, count, blocks = ops.ema_table(recs, gpu)
    assert count == 8 and blocks == 1 + 1 + 1 + 1 + 1 + 2 + 35 + 1
    table = G.place(table, 'ema table')
    assert table.numel() == count * ops.EMA_ITEM_BYTES
    _guard('ema_update_batched', ops.ema_update_batched, table, count, blocks, G.place(_coef(m, gpu), 'coef'))
    want = d0.copy()
    for o, n in zip(offs, sizes):
        want[o:o + n] = ema_ref.ema_array(d0[o:o + n], s0[o:o + n], m)
    assert not _same(want, d0)
    assert _same(dst, want)                        # every record right, every gap untouched
    assert _same(src, s0)
    assert cnt_dst.tolist() == [7, -5, 1 << 40, -5] and cnt_src.tolist() == [7, -1, 1 << 40, -1]


def test_batched_table_of_every_tail_length(gpu):
    """Items of 1, 3, 4, 5, 1023, 1024, 1025 and 1 elements in one launch, each pair of ranges in buffers of its own that end where
    their flanks begin, and a counter copy between them."""
    from mi355 import ops
    m = 0.999
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, 1]
    rng = np.random.default_rng(15)
    d0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    s0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    dst = [G.place(torch.from_numpy(a).to(gpu), 'dst[%d]' % len(a)) for a in d0]
    src = [G.place(torch.from_numpy(a).to(gpu), 'src[%d]' % len(a)) for a in s0]
    cnt_src = G.place(torch.tensor([12345678901], dtype=torch.int64, device=gpu), 'counter, main')
    cnt_dst = G.place(torch.tensor([-5], dtype=torch.int64, device=gpu), 'counter, teacher')
    recs = [(a, b, ops.EMA_F32) for a, b in zip(src, dst)]
    recs.insert(4, (cnt_src[0], cnt_dst[0], ops.EMA_COPY64))
    table, count, blocks = ops.ema_table(recs, gpu)
    assert count == blocks == 9                          # every item less than a chunk: exactly one block each
    _guard('ema_update_batched tails', ops.ema_update_batched, G.place(table, 'ema table'), count, blocks, G.place(_coef(m, gpu), 'coef'))
    for d, a, b0, a0 in zip(dst, src, d0, s0):
        assert _same(d, ema_ref.ema_array(b0, a0, m)) and _same(a, a0), len(a0)
    assert cnt_dst.tolist() == [12345678901] and cnt_src.tolist() == [12345678901]


# ---------------------------------------------------------------- the golden case through EMATeacher
def _nets(gpu):
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, bias=False), torch.nn.BatchNorm2d(4)).to(gpu)
    return mk(), mk()


def _load(module, g, tag):
    module.load_state_dict({k: torch.from_numpy(g['%s/%s' % (tag, k)]) for k in KEYS})


@pytest.mark.parametrize('flat', [False, True])
@pytest.mark.parametrize('tag,decay,warmup', [('m999', 0.999, False), ('m9', 0.9, False), ('warm', 0.999, True)])
def test_golden_case_through_the_teacher(gpu, tag, decay, warmup, flat):
    """flat=False: no optimizer, everything goes through the batched launch; flat=True: the parameters sit in a flat FusedSGD
    group and its mirror (one flat launch), running statistics and the counter in the batched one."""
    from mi355.optim import EMATeacher, FusedSGD
    g = golden('g11_ema')
    main, teacher = _nets(gpu)
    _load(main, g, 'main0')
    _load(teacher, g, 'init')
    opts = []
    if flat:
        for p in main.parameters():
            p.grad = torch.zeros_like(p)
        opts = [FusedSGD(main.parameters(), lr=0.1, momentum=0.9)]
        opts[0].ensure_flat()
    ema = EMATeacher(main, teacher, opts, decay, warmup=warmup)
    objs = [id(p) for p in teacher.parameters()]
    for t in range(3):
        _load(main, g, 'main%d' % t)
        ema.sync()
        ema.update()
        torch.cuda.synchronize()
        for k, v in teacher.state_dict().items():
            assert _same(v, g['%s_%d/%s' % (tag, t, k)]), (t, k)
    assert ema.step == 3 and [id(p) for p in teacher.parameters()] == objs
    assert len(ema._flat) == (1 if flat else 0)
    if flat:        # the teacher's parameters live in the mirror, at the offsets of the group's parameter buffer
        E, P = ema._flat[0]
        for pm, pe in zip(main.parameters(), teacher.parameters()):
            assert pe.data_ptr() - E.data_ptr() == pm.data_ptr() - P.data_ptr() and pe.stride() == pm.stride()


# ---------------------------------------------------------------- state, aliasing, re-layout
class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)
        self.register_buffer('stat', torch.zeros(7))


def test_state_round_trip_aliasing_and_late_first_gradient(gpu):
    from mi355.optim import EMATeacher, FusedSGD
    torch.manual_seed(4)
    main, teacher = _Two().to(gpu), _Two().to(gpu)
    with torch.no_grad():
        main.stat.normal_(); teacher.stat.normal_()
    opt = FusedSGD(main.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    ema = EMATeacher(main, teacher, [opt], 0.9, warmup=True)
    objs = {k: id(p) for k, p in teacher.named_parameters()}
    state = _host(teacher)

    def iterate(with_b):
        nonlocal state
        opt.zero_grad()
        for p in main.a.parameters():
            p.grad = torch.randn_like(p) if p.grad is None else p.grad.copy_(torch.randn_like(p))
        if with_b:
            for p in main.b.parameters():
                p.grad = torch.randn_like(p) if p.grad is None else p.grad.copy_(torch.randn_like(p))
        opt.step()
        m = ema.momentum()
        ema.sync()
        ema.update()
        torch.cuda.synchronize()
        state = ema_ref.ema_state(state, _host(main), m)
        got = _host(teacher)
        for k in state:
            assert _same(got[k], state[k]), k

    iterate(False); iterate(False)                  # layer b has never had a gradient: FusedSGD laid out layer a only
    E = ema._flat[0][0]
    inside = lambda p, E: 0 <= p.data_ptr() - E.data_ptr() < E.numel() * 4
    assert E.numel() == 16 + 4 and inside(teacher.a.weight, E) and not inside(teacher.b.weight, E)
    iterate(True)                                   # first gradient of layer b: FusedSGD lays out again, the teacher follows
    E2 = ema._flat[0][0]
    assert E2.data_ptr() != E.data_ptr() and E2.numel() == 16 + 4 + 8 + 4
    assert all(inside(p, E2) for p in teacher.parameters())
    assert {k: id(p) for k, p in teacher.named_parameters()} == objs
    iterate(True)
    assert ema.step == 4 and ema.momentum() == 0.8

    # nn.Module.load_state_dict on the teacher copies into the flat views (no re-pointing): the next update reads the new values
    ptrs = [p.data_ptr() for p in teacher.parameters()]
    new = {k: torch.full_like(v, 0.25) for k, v in teacher.state_dict().items()}
    teacher.load_state_dict(new)
    assert [p.data_ptr() for p in teacher.parameters()] == ptrs
    o = teacher.a.weight.data_ptr() - E2.data_ptr()
    assert o % 4 == 0 and float(E2[o // 4]) == 0.25
    state = _host(teacher)
    iterate(True)

    # the step count travels through state_dict(): a fresh teacher continues the warm-up schedule where this one is
    sd = ema.state_dict()
    assert sd['step'] == 5
    other = EMATeacher(main, teacher, [opt], 0.9, warmup=True)
    assert other.momentum() == 0.0
    other.load_state_dict(sd)
    assert other.step == 5 and other.momentum() == ema.momentum() == 1 - 1 / 6


# ---------------------------------------------------------------- the tiny model: eager, then replayed
def _pose(gpu, cls, seed):
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from seeded import fill_module_
    bb = models.resnet18(pretrained=False)
    model = cls(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True)
    fill_module_(model, seed)
    return model.to(gpu)


def _training(gpu, with_ema):
    import mi355
    from mi355.da_step import build_training
    from mi355.optim import EMATeacher
    from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    teacher = None
    if with_ema:
        teacher = _pose(gpu, PoseResNetx10, 5)
        teacher.load_state_dict(model.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        step.ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)        # m = 0, 1/2, 2/3, 3/4, then 0.8 twice
    return model, teacher, step, scheds


@pytest.fixture(scope='module')
def tiny(gpu):
    """Twin ResNet-18 runs, 3 eager iterations + capture(warmup=0) + 3 replays, one with the teacher attached and one without;
    host copies of every state dict after every iteration."""
    from utils.synthetic import make_batch
    batch = make_batch(2, 128, 32, seed=3, device=gpu)
    runs = {}
    for with_ema in (True, False):
        model, teacher, step, scheds = _training(gpu, with_ema)
        rec = dict(model=[], teacher=[_host(teacher)] if with_ema else [], loss=[], m=[])
        for it in range(6):
            if it == 3:
                step.capture(batch, warmup=0)
            if with_ema:
                rec['m'].append(step.ema.momentum())
            out = step.run(batch)
            for s in scheds.values():
                s.step()
            torch.cuda.synchronize()
            rec['loss'].append(float(out['loss_s']))
            rec['model'].append(_host(model))
            if with_ema:
                rec['teacher'].append(_host(teacher))
        assert step.graphs is not None and len(step.graphs) == 6
        runs[with_ema] = rec
        if with_ema:
            live = (model, teacher, step, batch)
    return runs, live


def test_tiny_model_teacher_follows_the_reference_update(tiny):
    rec = tiny[0][True]
    assert rec['m'] == [0.0, 0.5, 1 - 1 / 3, 0.75, 0.8, 0.8]
    assert len(rec['teacher'][0]) == 222
    for it in range(6):
        want = ema_ref.ema_state(rec['teacher'][it], rec['model'][it], rec['m'][it])
        got = rec['teacher'][it + 1]
        for k in want:
            assert _same(got[k], want[k]), (it, k)
    k = 'backbone.layer1.0.conv1.weight'
    assert all(not _same(rec['teacher'][it][k], rec['teacher'][it + 1][k]) for it in range(6))      # it moves, eager and replayed
    assert all(not _same(rec['teacher'][it + 1][k], rec['model'][it][k]) for it in range(1, 6))     # and is not a plain copy
    kr = 'backbone.bn1.running_mean'
    assert not _same(rec['teacher'][5][kr], rec['teacher'][6][kr])
    kn = 'backbone.bn1.num_batches_tracked'
    assert [t[kn].item() for t in rec['teacher'][1:]] == [t[kn].item() for t in rec['model']] and rec['model'][5][kn].item() > 0


def test_tiny_model_trajectory_is_unchanged_by_the_teacher(tiny):
    a, b = tiny[0][True], tiny[0][False]
    assert a['loss'] == b['loss'] and len(set(a['loss'])) > 1
    for it in range(6):
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_teacher_eval_graph_goes_stale_with_every_update(tiny):
    from mi355.infer import GraphedForward
    from uda.model.regda_7 import MainOutput, PoseResNetx9
    model, teacher, step, batch = tiny[1]
    gpu = batch['x_t'].device
    x = batch['x_t'].clone()
    scored = MainOutput(teacher).eval()             # what train1.py validates: the first of the teacher's five outputs
    gf = GraphedForward(scored, warmup=1)

    def fresh_output():
        fresh = _pose(gpu, PoseResNetx9, 9)         # (eval mode: returns the main head's heat-maps)
        fresh.load_state_dict(teacher.state_dict())
        fresh.eval()
        with torch.no_grad():
            return fresh(x).float().clone()

    with torch.no_grad():
        ys = [gf(x).float().clone() for _ in range(3)]            # eager warm-up, capture + replay, replay
    assert len(gf._graphs) == 1
    y0 = fresh_output()
    assert all(torch.equal(y, y0) for y in ys)
    step.run(batch)                                               # one replayed training iteration: the teacher moved
    torch.cuda.synchronize()
    with torch.no_grad():
        y = gf(x).float().clone()
        assert len(gf._graphs) == 0                               # dropped: this call ran the updated weights eagerly
        y1 = fresh_output()
        assert torch.equal(y, y1) and not torch.equal(y1, y0)
        assert torch.equal(gf(x).float(), y1) and len(gf._graphs) == 1          # captured again, same answer


# ---------------------------------------------------------------- command lines
def test_train_and_test_cli_with_the_ema_switch(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(script, log, extra):
        common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '6', '-p', '2', '-j', '0',
                  '--pretrain_epochs', '1', '--log', log]
        r = subprocess.run([sys.executable, os.path.join(PKG, script)] + common + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    ema_line = re.compile(r'^ema: +\d+\.\d{3}$', re.M)
    load = lambda *p: torch.load(os.path.join(*p), map_location='cpu', weights_only=False)
    log = str(tmp_path / 'on')
    out = run('train1.py', log, ['--epochs', '1', '--pretrain', str(tmp_path / 'none.pth'), '--ema-update', 'const', '--ema-decay', '0.9'])
    assert 'Target(best)' in out and len(ema_line.findall(out)) == 1
    ck, teacher = load(log, 'checkpoints', '0.pth'), load(log, 'checkpoints', 'model_ema.pth')['model_ema']
    pre = load(log, 'checkpoints', 'pretrain.pth')['model']
    assert ck['ema_state']['step'] == 6 and list(teacher) == list(ck['model'])
    k = 'backbone.layer1.0.conv1.weight'
    assert not torch.equal(teacher[k], ck['model'][k]) and not torch.equal(teacher[k], pre[k])
    assert int(teacher['backbone.bn1.num_batches_tracked']) == int(ck['model']['backbone.bn1.num_batches_tracked'])
    out = run('test.py', log, ['--checkpoint', os.path.join(log, 'checkpoints', '0.pth'),
                               '--ema_model', os.path.join(log, 'checkpoints', 'model_ema.pth')])
    assert 'Source:' in out and 'fingertip:' in out and len(ema_line.findall(out)) == 1

    # off (the default): no ema line, no ema_state, model_ema.pth holds the pre-training weights as before
    log_off = str(tmp_path / 'off')
    out = run('train1.py', log_off, ['--epochs', '1', '--pretrain', os.path.join(log, 'checkpoints', 'pretrain.pth')])
    assert 'Target(best)' in out and not ema_line.findall(out)
    ck_off, frozen = load(log_off, 'checkpoints', '0.pth'), load(log_off, 'checkpoints', 'model_ema.pth')['model_ema']
    assert 'ema_state' not in ck_off
    shared = [k for k in frozen if k in pre]
    assert len(shared) > 100 and all(torch.equal(frozen[k], pre[k]) for k in shared)
    assert not torch.equal(frozen[k], ck_off['model'][k])
