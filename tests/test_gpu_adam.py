"""Adam / AdamW on the GPU (include/mi355pose.h: mi355_adam_step_batched, mi355_adam_tick_batched; mi355.optim.FusedAdam;
build_training(optimizer=...); train1.py --optimizer):

  1. exact operands: betas (0.5, 0.75), eps 0, no weight decay, lr 2^-6, p multiples of 2^-6, g = +-2^k -- after one step
     p' = p - lr * sign(g), m = g / 2, v = g * g / 4 and step = 1 bit for bit, at every length around the float4 tail and the
     chunk edge, each buffer inside guard bands; and one table of three items whose counts start at 0, 1 and 9;
  2. random operands, 5 steps, both weight-decay forms, two groups of different lr, betas and eps in one table, against the
     float64 oracle tests/adam_ref.py within the bound (below);
  3. the clip record: coef 0.5 = the unclipped step on g / 2, coef 1 = no record, skip = nothing written, bit for bit; and the
     kernel against the float32 restatement tests/adam_ref.py::adam_step32, bit for bit on random operands;
  4. FusedAdam beside torch.optim.Adam / AdamW on a three-layer module under LambdaLR, with a parameter that never gets a gradient
     and one that gets one every other step; the state dicts cross-loaded;
  5. step() captured and replayed with new gradients and learning rates = eager steps, bit for bit;
  6. the whole DAStep iteration under adamw with GradClipper(inf) and an EMATeacher: replayed = eager, bit for bit;
  7. the command line: --optimizer adamw, --resume, and the refusal of a checkpoint of the other kind.

The bound, per tensor: twice the distance of torch.optim.Adam(W) on CPU float32 from the float64 oracle, or 4 float32 ulps of the
tensor's largest magnitude, whichever is larger (the kernel rounds lr to float32 before the division: one rounding more per
operation than torch).

Guards (tests/guarded.py).  The kernel-level tests of sections 1 - 3 keep every buffer of an item (p, g, m, v with their sentinel
bands, the step count, lr), the item table and the clip record in G.place() copies and launch through _launch, which opens a
window, synchronises and checks every flank.  The kernels work in place (nothing is allocated, so there is no unwritten check);
the exact comparisons stay.  test_one_table_of_every_tail_length_against_the_flanks has no sentinel bands at all: every buffer
ends where its flank begins.  FusedAdam, the capture, DAStep and the command line (sections 4 - 7) are not guarded.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_ref as ref
import guarded as G
from conftest import PKG

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4, 7.0


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


@pytest.fixture
def rt(gpu):
    import mi355
    mi355.load()
    mi355.set_compute_dtype('bf16')
    yield mi355
    mi355.set_compute_dtype('bf16')


def _ops():
    from mi355 import ops
    return ops


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Item:
    """p, g, m, v of one parameter, each the view [GUARD : GUARD + n] of a buffer that holds SENTINEL around it, its step count and
    the hyper-parameters of its group."""

    def __init__(self, gpu, p, g, lr_dev, beta1, beta2, eps, wd, decoupled, step=0.0, m=None, v=None, band=GUARD):
        n = len(p)
        self.n, self.hyper, self.band = n, (beta1, beta2, eps, wd, decoupled), band
        zeros = np.zeros(n, dtype=np.float32)
        self.full = []
        for x, name in zip((p, g, zeros if m is None else m, zeros if v is None else v), 'pgmv'):
            buf = np.full(n + 2 * band, SENTINEL, dtype=np.float32)
            buf[band:band + n] = x
            self.full.append(G.place(torch.from_numpy(buf).to(gpu), '%s[%d]' % (name, n)))      # band = 0: the flank follows the last element
        self.p, self.g, self.m, self.v = (t[band:band + n] for t in self.full)
        self.step = G.place(torch.full((3,), SENTINEL, device=gpu), 'step')
        self.step[1] = step
        self.lr = lr_dev

    def row(self):
        return (self.p, self.g, self.m, self.v, self.step[1], self.lr) + self.hyper

    def guards_intact(self):
        s = torch.tensor(SENTINEL)
        b = self.band
        ok = all(_same(t[:b].cpu(), s.expand(b)) and _same(t[b + self.n:].cpu(), s.expand(b)) for t in self.full)
        return ok and float(self.step[0]) == SENTINEL and float(self.step[2]) == SENTINEL

    def host(self):
        return [t.cpu().numpy().copy() for t in (self.p, self.m, self.v)] + [float(self.step[1])]


def _launch(items, gpu, rec=None, table=None):
    ops = _ops()
    if table is None:
        table = ops.adam_table([it.row() for it in items], gpu)
        table = (G.place(table[0], 'adam table'),) + tuple(table[1:])
    assert table[2] == sum((it.n + ops.ADAM_CHUNK - 1) // ops.ADAM_CHUNK for it in items)      # exactly the blocks the table needs
    assert table[0].numel() == len(items) * ops.ADAM_ITEM_BYTES
    label = 'adam_step_batched + adam_tick_batched, items %s' % ([it.n for it in items],)
    with G.window(ops, label):
        ops.adam_step_batched(*table, rec)
        ops.adam_tick_batched(table[0], table[1], rec)
    torch.cuda.synchronize()
    G.check(label)
    return table


def _make_rec(coef, skip, gpu):
    ops = _ops()
    r = np.zeros(1, dtype=ops.clip_rec_dtype())
    r['coef'], r['skip'], r['max_norm'] = np.float32(coef), skip, 1.0
    return G.place(torch.from_numpy(r.view(np.uint8).copy()).to(gpu), 'clip record')


# ---------------------------------------------------------------- 1. exact operands
EXACT = dict(lr=2.0 ** -6, beta1=0.5, beta2=0.75, eps=0.0, wd=0.0, decoupled=False)
EXACT_LENS = [1, 3, 4, 5, 255, 1024, 16384, 16385, 32775]


def _exact_operands(seed, n):
    rng = np.random.default_rng(seed)
    p = (rng.integers(-128, 129, n) / 64.0).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-8, 9, n)).astype(np.float32)
    return p, g


def _exact_item(seed, n, gpu, lr_dev, step=0.0, band=GUARD):
    p, g = _exact_operands(seed, n)
    h = EXACT
    return _Item(gpu, p, g, lr_dev, h['beta1'], h['beta2'], h['eps'], h['wd'], h['decoupled'], step=step, band=band), p, g


@pytest.mark.parametrize('n', EXACT_LENS)
def test_one_exact_step_bit_for_bit(rt, gpu, n):
    assert _ops().ADAM_CHUNK == 16384
    lr_dev = G.place(torch.tensor(EXACT['lr'], device=gpu), 'lr')
    it, p, g = _exact_item(100 + n, n, gpu, lr_dev)
    _launch([it], gpu)
    got_p, got_m, got_v, step = it.host()
    assert got_p.tobytes() == (p - np.float32(EXACT['lr']) * np.sign(g)).astype(np.float32).tobytes()
    assert got_m.tobytes() == (g / 2).astype(np.float32).tobytes()
    assert got_v.tobytes() == (g * g / 4).astype(np.float32).tobytes()
    assert step == 1.0 and it.guards_intact()
    assert it.g.cpu().numpy().tobytes() == g.tobytes() and float(lr_dev) == EXACT['lr']


def test_one_table_of_three_items_at_step_counts_0_1_and_9(rt, gpu):
    lr_dev = G.place(torch.tensor(EXACT['lr'], device=gpu), 'lr')
    starts, lens = (0.0, 1.0, 9.0), (16385, 5, 1024)
    made = [_exact_item(200 + i, n, gpu, lr_dev, step=s) for i, (n, s) in enumerate(zip(lens, starts))]
    _launch([m[0] for m in made], gpu)
    h = EXACT
    for (it, p, g), start in zip(made, starts):
        got_p, got_m, got_v, step = it.host()
        o_p, o_m, o_v, o_t = ref.adam_step64(p, g, np.zeros_like(p), np.zeros_like(p), int(start), h['lr'], h['beta1'], h['beta2'], h['eps'],
                                             h['wd'], h['decoupled'])
        assert step == o_t == start + 1 and it.guards_intact()
        assert got_m.tobytes() == o_m.astype(np.float32).tobytes() and got_v.tobytes() == o_v.astype(np.float32).tobytes()
        # p: lr / (1 - beta1^t) is not a float32 number for t > 1 -- within the second arm of the bound, 4 ulps of the largest magnitude
        d, allowed = ref.distance(got_p, o_p), 4.0 * float(np.spacing(np.float32(np.abs(o_p).max())))
        print('start %d: p distance %.3g allowed %.3g' % (start, d, allowed))
        assert d <= allowed
        if start == 0:
            assert got_p.tobytes() == o_p.astype(np.float32).tobytes()


TAIL_LENS = [1, 3, 4, 5, 1023, 1024, 1025, 1]            # one launch; the first and the last item have one element


def test_one_table_of_every_tail_length_against_the_flanks(rt, gpu):
    """No sentinel bands: p, g, m and v of every item end where their back flank begins, so a float4 that reaches past a tail of
    1, 3 or 5 elements reads 0xFF bytes or writes into a flank.  Exact operands, one step from zero moments."""
    lr_dev = G.place(torch.tensor(EXACT['lr'], device=gpu), 'lr')
    made = [_exact_item(500 + i, n, gpu, lr_dev, band=0) for i, n in enumerate(TAIL_LENS)]
    assert all(t.data_ptr() % 16 == 0 and t.numel() == it.n for it, _, _ in made for t in it.full)
    table = _launch([m[0] for m in made], gpu)
    assert table[2] == len(TAIL_LENS)                     # one block each
    for it, p, g in made:
        got_p, got_m, got_v, step = it.host()
        assert got_p.tobytes() == (p - np.float32(EXACT['lr']) * np.sign(g)).astype(np.float32).tobytes(), it.n
        assert got_m.tobytes() == (g / 2).astype(np.float32).tobytes() and got_v.tobytes() == (g * g / 4).astype(np.float32).tobytes(), it.n
        assert step == 1.0 and it.g.cpu().numpy().tobytes() == g.tobytes()
        assert float(it.step[0]) == SENTINEL and float(it.step[2]) == SENTINEL


# ---------------------------------------------------------------- 2. random operands
GROUPS = (dict(lens=(1000, 16384 + 5, 37), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=0.05),
          dict(lens=(4100, 3), lr=3e-3, betas=(0.8, 0.95), eps=1e-6, wd=0.01))


@pytest.mark.parametrize('decoupled', [False, True])
def test_five_random_steps_of_two_groups_within_the_bound(rt, gpu, decoupled):
    """Measured on an MI355X: the largest distance from the float64 oracle over the five steps and all tensors of a kind (torch's
    on CPU float32 in brackets) and the largest share of the bound any tensor used (the test prints all three):
      L2 weight decay:        p 4.35e-07 (4.35e-07) 0.46   exp_avg 5.55e-07 (5.28e-07) 0.48   exp_avg_sq 4.22e-07 (4.22e-07) 0.60
      decoupled weight decay: p 9.14e-07 (9.14e-07) 0.50   exp_avg 3.86e-07 (3.55e-07) 0.45   exp_avg_sq 5.72e-06 (5.72e-06) 0.50"""
    rng = np.random.default_rng(300 + decoupled)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    items, t_params, t_groups, state64, hypers = [], [], [], [], []
    for gr in GROUPS:
        lr_dev = G.place(torch.tensor(gr['lr'], device=gpu), 'lr')
        ps = []
        for n in gr['lens']:
            p = rng.standard_normal(n).astype(np.float32)
            g = np.zeros(n, dtype=np.float32)
            items.append(_Item(gpu, p, g, lr_dev, gr['betas'][0], gr['betas'][1], gr['eps'], gr['wd'], decoupled))
            ps.append(torch.nn.Parameter(torch.from_numpy(p.copy())))
            state64.append((p.astype(np.float64), np.zeros(n), np.zeros(n), 0))
            hypers.append((gr['lr'],) + gr['betas'] + (gr['eps'], gr['wd'], decoupled))
        t_params += ps
        t_groups.append(dict(params=ps, lr=gr['lr'], betas=gr['betas'], eps=gr['eps'], weight_decay=gr['wd']))
    opt = cls(t_groups)
    table, worst = None, {}
    for step in range(5):
        for i, it in enumerate(items):
            g = (rng.standard_normal(it.n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)
            it.g.copy_(torch.from_numpy(g))
            t_params[i].grad = torch.from_numpy(g.copy())
            state64[i] = ref.adam_step64(state64[i][0], g, state64[i][1], state64[i][2], state64[i][3], *hypers[i])
        table = _launch(items, gpu, table=table)
        opt.step()
        for i, it in enumerate(items):
            got = it.host()
            st = opt.state[t_params[i]]
            assert got[3] == state64[i][3] == step + 1 == float(st['step']) and it.guards_intact()
            for name, mine, oracle, theirs in zip('pmv', got[:3], state64[i][:3], (t_params[i], st['exp_avg'], st['exp_avg_sq'])):
                allowed, d_torch = ref.bound(theirs.detach().numpy(), oracle)
                d = ref.distance(mine, oracle)
                w = worst.setdefault(name, [0.0, 0.0, 0.0])
                worst[name] = [max(w[0], d), max(w[1], d_torch), max(w[2], d / allowed)]
                assert d <= allowed, (step, i, name, d, d_torch, allowed)
    for name, (d, d_torch, ratio) in sorted(worst.items()):
        print('decoupled=%s %s: largest distance kernel %.3g  torch %.3g  largest share of the bound %.3f' % (decoupled, name, d, d_torch, ratio))


# ---------------------------------------------------------------- 3. the clip record
def _random_items(seed, gpu, lr_dev, g_scale=1.0, wd=0.05, decoupled=False):
    rng = np.random.default_rng(seed)
    out = []
    for n, start in ((16384 + 6, 0.0), (37, 3.0), (1023, 1.0)):
        p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        m, v = (0.1 * rng.standard_normal(n)).astype(np.float32), (0.01 * rng.standard_normal(n) ** 2).astype(np.float32)
        out.append(_Item(gpu, p, (g * np.float32(g_scale)).astype(np.float32), lr_dev, 0.9, 0.999, 1e-8, wd, decoupled, step=start, m=m, v=v))
    return out


@pytest.mark.parametrize('decoupled', [False, True])
def test_clip_coefficient_and_skip(rt, gpu, decoupled):
    lr_dev = G.place(torch.tensor(1e-2, device=gpu), 'lr')
    state = lambda items: [t.clone() for it in items for t in it.full + [it.step]]
    same = lambda a, b: all(_same(x, y) for x, y in zip(a, b))
    # coef = 0.5 is the unclipped step on g / 2 (halving is exact)
    a, b = _random_items(400, gpu, lr_dev, decoupled=decoupled), _random_items(400, gpu, lr_dev, g_scale=0.5, decoupled=decoupled)
    _launch(a, gpu, rec=_make_rec(0.5, 0, gpu))
    _launch(b, gpu)
    for x, y in zip(a, b):
        assert _same(x.p, y.p) and _same(x.m, y.m) and _same(x.v, y.v) and _same(x.step, y.step) and x.guards_intact()
        assert _same(x.g * 0.5, y.g)                     # (the clipped launch left its gradients alone)
    # coef = 1 is the launch without a record
    a, b = _random_items(401, gpu, lr_dev, decoupled=decoupled), _random_items(401, gpu, lr_dev, decoupled=decoupled)
    before = state(a)
    _launch(a, gpu, rec=_make_rec(1.0, 0, gpu))
    _launch(b, gpu)
    assert same(state(a), state(b)) and not same(state(a), before)
    assert [float(it.step[1]) for it in a] == [1.0, 4.0, 2.0]
    # skip: nothing is written, whatever the coefficient says
    a = _random_items(402, gpu, lr_dev, decoupled=decoupled)
    before = state(a)
    _launch(a, gpu, rec=_make_rec(0.25, 1, gpu))
    assert same(state(a), before) and all(it.guards_intact() for it in a)
    assert [float(it.step[1]) for it in a] == [0.0, 3.0, 1.0]


@pytest.mark.parametrize('decoupled', [False, True])
@pytest.mark.parametrize('coef', [None, 0.3712345])
def test_kernel_equals_the_float32_restatement_bit_for_bit(rt, gpu, decoupled, coef):
    """tests/adam_ref.py::adam_step32 is the kernel operation for operation (correctly rounded square root and division, nothing
    contracted, the bias corrections in float64 by squaring): three steps on random operands from non-zero moments and step counts
    0, 3 and 1, with and without a clip coefficient whose product with g rounds, give the same bits."""
    lr_dev = G.place(torch.tensor(1e-2, device=gpu), 'lr')
    items = _random_items(450, gpu, lr_dev, decoupled=decoupled)
    rec = None if coef is None else _make_rec(coef, 0, gpu)
    rng = np.random.default_rng(451)
    want = [tuple(it.host()) for it in items]
    table = None
    for step in range(3):
        for i, it in enumerate(items):
            g = (rng.standard_normal(it.n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)
            it.g.copy_(torch.from_numpy(g))
            want[i] = ref.adam_step32(want[i][0], g, want[i][1], want[i][2], want[i][3], float(np.float32(1e-2)), *it.hyper,
                                      coef=None if coef is None else np.float32(coef))
        table = _launch(items, gpu, rec=rec, table=table)
        for i, it in enumerate(items):
            got = it.host()
            assert got[3] == want[i][3] and it.guards_intact()
            for name, a, b in zip('pmv', got[:3], want[i][:3]):
                diff = int((a.view(np.int32) != b.view(np.int32)).sum())
                assert diff == 0, (step, i, name, diff, float(np.abs(a.astype(np.float64) - b).max()))


# ---------------------------------------------------------------- 4. FusedAdam beside torch
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l1, self.l2, self.l3 = torch.nn.Linear(8, 16), torch.nn.Linear(16, 16), torch.nn.Linear(16, 4)
        self.side = torch.nn.Linear(16, 4, bias=False)           # in the graph every other step only
        self.never = torch.nn.Parameter(torch.ones(5))             # never in the graph: no gradient, no state

    def forward(self, x, with_side):
        h = torch.tanh(self.l2(torch.tanh(self.l1(x))))
        return self.l3(h) + (self.side(h) if with_side else 0.0)


@pytest.mark.parametrize('decoupled', [False, True])
def test_fused_adam_follows_torch_on_a_small_module(rt, gpu, decoupled):
    from torch.optim.lr_scheduler import LambdaLR
    from mi355.optim import FusedAdam
    torch.manual_seed(5)
    net = _Net()
    net32, net64 = copy.deepcopy(net), copy.deepcopy(net).double()
    net = net.to(gpu)
    names = [k for k, _ in net.named_parameters()]
    hyper = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    # (`side` in a group of its own: views of one flat gradient buffer share a version counter, so a parameter of a torch-native
    # module shows as untouched since zero_grad() only when nothing else of its group was written)
    split = lambda m: [dict(params=[p for k, p in m.named_parameters() if k.startswith('l1')], lr=3e-3),
                       dict(params=[p for k, p in m.named_parameters() if not k.startswith(('l1', 'side'))]),
                       dict(params=[p for k, p in m.named_parameters() if k.startswith('side')])]
    mine, opt32, opt64 = FusedAdam(split(net), decoupled=decoupled, **hyper), cls(split(net32), **hyper), cls(split(net64), **hyper)
    fn = lambda it: 1.0 / (1.0 + 0.5 * it)
    scheds = [LambdaLR(o, fn) for o in (mine, opt32, opt64)]
    x = torch.randn(6, 8, generator=torch.Generator().manual_seed(6)).to(gpu)
    objs = {k: id(p) for k, p in net.named_parameters()}

    def iterate(i, others):
        """One step of `mine` and of `others` (pairs of module and optimizer) on the gradients the GPU module computed."""
        with_side = i % 2 == 0
        mine.zero_grad()
        net(x, with_side).square().sum().backward()
        for m, o in others:
            for k, p in m.named_parameters():
                g = dict(net.named_parameters())[k].grad
                p.grad = None if (g is None or (k.startswith('side') and not with_side)) else g.detach().cpu().to(p.dtype)
            o.step()
        mine.step()
        torch.cuda.synchronize()

    def check(what, modules=None):
        got, st_mine = dict(net.named_parameters()), mine.state_dict()['state']
        st32, st64 = opt32.state_dict()['state'], opt64.state_dict()['state']
        assert sorted(st_mine) == sorted(st32) == sorted(st64)
        for idx in st_mine:
            assert st_mine[idx]['step'].dtype == torch.float32 and st_mine[idx]['step'].device.type == 'cpu'
            assert float(st_mine[idx]['step']) == float(st32[idx]['step']), (what, idx)
        p32, p64 = dict(net32.named_parameters()), dict(net64.named_parameters())
        index = {k: i for i, k in enumerate(k for g in split(net) for k, p in net.named_parameters() if any(p is q for q in g['params']))}
        for k in names:
            tensors = [('p', got[k], p32[k], p64[k])]
            if index[k] in st_mine:
                tensors += [(s, st_mine[index[k]][s], st32[index[k]][s], st64[index[k]][s]) for s in ('exp_avg', 'exp_avg_sq')]
            for s, a, b, c in tensors:
                allowed, d_torch = ref.bound(b.detach().numpy(), c.detach().numpy())
                d = ref.distance(a.detach().cpu().numpy(), c.detach().numpy())
                assert d <= allowed, (what, k, s, d, d_torch, allowed)

    for i in range(6):
        iterate(i, [(net32, opt32), (net64, opt64)])
        for s in scheds:
            s.step()
        check('step %d' % i)
    st = mine.state_dict()['state']
    steps = sorted(float(v['step']) for v in st.values())
    assert steps == [3.0] + [6.0] * 6 and len(st) == 7                  # side: 3 fresh steps; `never`: no state at all
    assert {k: id(p) for k, p in net.named_parameters()} == objs and mine.is_flat
    assert float(net.never.detach().sum()) == 5.0 and net.never.grad is None
    assert abs(mine.param_groups[1]['lr'] - 1e-2 * fn(6)) < 1e-12 and abs(mine.param_groups[0]['lr'] - 3e-3 * fn(6)) < 1e-12

    # each side's state dict into the other: torch's into FusedAdam, FusedAdam's into a fresh torch optimizer on a copy of its module
    net_b = copy.deepcopy(net).cpu()
    opt_b = cls(split(net_b), **hyper)
    opt_b.load_state_dict(copy.deepcopy(mine.state_dict()))
    mine.load_state_dict(copy.deepcopy(opt32.state_dict()))
    assert {k: id(p) for k, p in net.named_parameters()} == objs
    for p in net.parameters():
        if p in mine.state and 'exp_avg' in mine.state[p]:
            assert mine.state[p]['exp_avg'].device.type == gpu.type and mine.state[p]['step'].data_ptr() != 0
            assert any(mine.state[p]['step'].data_ptr() == f['S'][i].data_ptr() for f in mine._flat if f is not None for i in range(len(f['params'])))
    iterate(6, [(net32, opt32), (net64, opt64), (net_b, opt_b)])
    check('after the exchange')
    got_b, p32, p64 = dict(net_b.named_parameters()), dict(net32.named_parameters()), dict(net64.named_parameters())
    for k in names:
        allowed, _ = ref.bound(p32[k].detach().numpy(), p64[k].detach().numpy())
        assert ref.distance(got_b[k].detach().numpy(), p64[k].detach().numpy()) <= allowed, k
    assert sorted(float(v['step']) for v in opt_b.state_dict()['state'].values()) == [4.0] + [7.0] * 6


# ---------------------------------------------------------------- 5. capture
def test_captured_step_replays_as_eager_steps(rt, gpu):
    from mi355.optim import FusedAdam
    rng = np.random.default_rng(500)
    shapes = [(16385,), (7, 5), (3,)]
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[(rng.standard_normal(s) * 10.0 ** -k).astype(np.float32) for s in shapes] for k in range(4)]
    lrs = [1e-2, 5e-3, 2e-3, 1e-3]

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(gpu)) for x in p0]
        return ps, FusedAdam([dict(params=ps[:2]), dict(params=ps[2:], betas=(0.8, 0.9))], lr=lrs[0], weight_decay=0.01, decoupled=True)

    def feed(ps, opt, k):
        for p, g in zip(ps, grads[k]):
            g = torch.from_numpy(g).to(gpu)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)
        for gr in opt.param_groups:
            gr['lr'] = lrs[k]
        opt.sync_lr()

    ps_e, opt_e = make()
    for k in range(4):
        feed(ps_e, opt_e, k)
        opt_e.step()
    ps_g, opt_g = make()
    feed(ps_g, opt_g, 0)
    opt_g.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with rt.no_gc_in_capture():
        with torch.cuda.graph(graph, capture_error_mode=rt.graph_capture_mode()):
            opt_g.step()
    torch.cuda.synchronize()
    assert [float(opt_g.state[p]['step']) for p in ps_g] == [1.0] * 3          # (capture executed nothing)
    for k in range(1, 4):
        feed(ps_g, opt_g, k)
        graph.replay()
    torch.cuda.synchronize()
    for a, b, start in zip(ps_e, ps_g, p0):
        assert _same(a, b) and not torch.equal(a.cpu(), torch.from_numpy(start))
        for s in ('exp_avg', 'exp_avg_sq', 'step'):
            assert _same(opt_e.state[a][s], opt_g.state[b][s]), s
        assert float(opt_g.state[b]['step']) == 4.0


# ---------------------------------------------------------------- 6. the whole iteration
def _da_run(gpu, capture_at, iters=4):
    """resnet18, B = 2, 64 x 64 images, 16 x 16 heat-maps, synthetic, adamw + GradClipper(inf) + EMATeacher."""
    import mi355
    from mi355.da_step import build_training
    from mi355.optim import EMATeacher, FusedAdam, GradClipper
    from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
    from utils.synthetic import make_batch
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=16, lr=1e-3, wd=1e-2, optimizer='adamw', adam_betas=(0.9, 0.99))
    assert all(type(o) is FusedAdam and o.defaults['decoupled_weight_decay'] and o.defaults['betas'] == (0.9, 0.99) for o in opts.values())
    teacher = _pose(gpu, PoseResNetx10, 5)
    teacher.load_state_dict(model.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    step.clip = GradClipper(float('inf'), gpu)
    step.ema = EMATeacher(model, teacher, opts, 0.8, warmup=True)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    batch = make_batch(2, 64, 16, seed=3, device=gpu)
    losses = []
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        losses += [float(out[k]) for k in ('loss_s', 'loss_gf', 'loss_gt')]
    host = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}
    counts = sorted({float(st['step']) for o in opts.values() for st in o.state_dict()['state'].values()})
    return dict(model=host(model), teacher=host(teacher), losses=losses, skipped=step.clip.read()[1], graphs=step.graphs, counts=counts)


def test_da_step_under_adamw_replays_as_it_runs_eagerly(gpu):
    import mi355
    try:
        eager, graph = _da_run(gpu, None), _da_run(gpu, 2)
    finally:
        mi355.set_compute_dtype('bf16')
    assert eager['graphs'] is None and graph['graphs'] is not None
    raw = lambda t: t.contiguous().view(-1).view(torch.uint8)
    for which in ('model', 'teacher'):
        a, b = eager[which], graph[which]
        assert list(a) == list(b)
        assert [k for k in a if not torch.equal(raw(a[k]), raw(b[k]))] == [], which
    assert eager['losses'] == graph['losses'] and all(np.isfinite(x) for x in eager['losses'])
    assert eager['skipped'] == graph['skipped'] == 0
    assert eager['counts'] == graph['counts'] and max(eager['counts']) == 8.0        # optimizer_f steps in updates A and C
    moved = [k for k in eager['model'] if 'weight' in k and not torch.equal(eager['model'][k], eager['teacher'][k])]
    assert len(moved) > 50


# ---------------------------------------------------------------- 7. the command line
def test_train_cli_runs_resumes_and_refuses_the_other_kind(gpu, tmp_path):
    log = str(tmp_path / 'run')
    pre = str(tmp_path / 'pre.pth')
    common = ['data/none', '-t', 'Hand3DStudio', '--synthetic', '-a', 'resnet18', '-b', '4', '-i', '4', '-p', '2', '-j', '0',
              '--pretrain_epochs', '1', '--pretrain', pre, '--lr', '0.001']
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(extra):
        return subprocess.run([sys.executable, os.path.join(PKG, 'train1.py')] + common + extra, env=env, capture_output=True, text=True, timeout=600)

    r = run(['--optimizer', 'adamw', '--epochs', '1', '--log', log])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Target(best)' in r.stdout
    ck_path = os.path.join(log, 'checkpoints', '0.pth')
    ck = torch.load(ck_path, map_location='cpu', weights_only=False)
    group = ck['optimizer_f']['param_groups'][0]
    assert group['decoupled_weight_decay'] and group['betas'] == (0.9, 0.999) and 'momentum' not in group
    steps = {float(st['step']) for st in ck['optimizer_f']['state'].values()}
    assert max(steps) == 8.0 and min(steps) >= 1.0         # update A and update C, four iterations
    assert all(sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in ck['optimizer_f']['state'].values())
    log2 = str(tmp_path / 'run2')
    r = run(['--optimizer', 'adamw', '--epochs', '2', '--resume', ck_path, '--log', log2])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ck2 = torch.load(os.path.join(log2, 'checkpoints', '1.pth'), map_location='cpu', weights_only=False)
    assert max(float(st['step']) for st in ck2['optimizer_f']['state'].values()) == 16.0 and ck2['epoch'] == 1
    r = run(['--optimizer', 'sgd', '--epochs', '2', '--resume', ck_path, '--log', str(tmp_path / 'run3')])
    assert r.returncode != 0
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert 'KeyError' not in tail and 'SGD' in tail and 'Adam' in tail and '--optimizer' in tail, tail
