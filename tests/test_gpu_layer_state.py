"""Host-side state of the mi355.nn layers across calls: packed weight copies, scratch buffers, gradient-slot flags, the
data_ptr-keyed hand-off maps and GraphedForward's state stamp.  Every other GPU test builds a fresh module for one shape and
one dtype; here ONE layer instance runs a sequence of steps that change the shape, the compute dtype, the weights, the
gradient mode and the train / eval mode, and after every step its output, input gradient and parameter gradients are compared
with a float64 CPU reference that reads its parameters from the layer under test (bf16: operands rounded to bf16 first).

  a  shape A in the base dtype                          baseline
  b  shape B (other batch, odd or smaller extents)       scratch buffers sized for A (Conv2d._stem_tmp, _g_tmp)
  c  the other compute dtype at B and A, then back       caches keyed without the dtype or the channel padding
  d  w.mul_(0.5) under no_grad, then load_state_dict     packed copies keyed on a stale version
  e  a forward with no backward, then one with           _BN_DX / _LAZY_MASK / _BWD_PARTIALS, leftover statistics partials
  f  two backwards without zero_grad, then zero + one    grad_slot / _mi_fresh (accumulate, then overwrite)
  g  eval under no_grad, then train again (BatchNorm)    _FoldedBn after the weights and running statistics moved

Before a step that overwrites the gradients they are filled with NaN, so a skipped write shows."""
import pytest
import torch
import torch.nn.functional as F

from seeded import fill_module_, randn

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
REL = {'f32': 1e-4, 'bf16': 1.2e-2}       # x max|ref| (test_stem_layer_folded_and_padded_forms_match_torch; test_gpu_kernels._tol)


@pytest.fixture
def rt(gpu):
    import mi355
    mi355.load()
    mi355.set_compute_dtype('bf16')
    yield mi355
    mi355.set_compute_dtype('bf16')


def _round(t, dt):
    """t rounded to the compute dtype (test_gpu_kernels._round), kept in float64."""
    return t.to(DT[dt]).double()


def _near(what, got, ref, rel, floor=0.0):
    ref = ref.detach().double()
    scale = max(float(ref.abs().max()), floor)
    err = float((got.detach().double().cpu() - ref).abs().max())
    assert err <= rel * scale, '%s: max |error| %.4g, allowed %.4g' % (what, err, rel * scale)


class _Dict:
    """A state dict posing as a module for seeded.fill_module_."""

    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd


def _fresh_state(mod, seed):
    return fill_module_(_Dict({k: v.detach().clone() for k, v in mod.state_dict().items()}), seed).sd


def _layers(mod):
    """(state-dict prefix, layer) of a layer or of a FusedSequential stack."""
    from mi355 import nn as mnn
    if isinstance(mod, mnn.FusedSequential):
        return [('%d.' % i, m) for i, m in enumerate(mod)]
    return [('', mod)]


class _Ref:
    """float64 CPU reference of `mod`: parameters read from `mod` at every call, running statistics kept on its own."""

    def __init__(self, mod):
        self.mod = mod
        self.load_buffers(mod.state_dict())

    def load_buffers(self, sd):
        self.buf = {k: v.detach().double().cpu().clone() for k, v in sd.items() if 'running' in k}

    def params(self, dt):
        P = {}
        for k, p in self.mod.named_parameters():
            t = p.detach().double().cpu()
            if t.dim() == 4 and dt == 'bf16':
                t = _round(t, dt)
            P[k] = t.requires_grad_(True)
        return P

    def forward(self, P, x, dt, training):
        from mi355 import nn as mnn
        lay = _layers(self.mod)
        for i, (pre, m) in enumerate(lay):
            if isinstance(m, mnn.Conv2d):
                x = F.conv2d(x, P[pre + 'weight'], P.get(pre + 'bias'), m.stride, m.padding, groups=m.groups)
            elif isinstance(m, mnn.ConvTranspose2d):
                x = F.conv_transpose2d(x, P[pre + 'weight'], None, m.stride, m.padding)
            elif isinstance(m, mnn.BatchNorm2d):
                x = F.batch_norm(x, self.buf[pre + 'running_mean'], self.buf[pre + 'running_var'], P[pre + 'weight'],
                                 P[pre + 'bias'], training, m.momentum, m.eps)
            elif isinstance(m, mnn.ReLU):
                x = F.relu(x)
            if dt == 'bf16' and i + 1 < len(lay) and not isinstance(lay[i + 1][1], mnn.ReLU):
                x = x + (_round(x.detach(), dt) - x.detach())    # the layer stores it in bf16 (value only: the gradient passes)
        return x


class _Seq:
    """Runs steps on one layer instance and checks each against the reference.  x_kind: 'feat' (channels_last compute-dtype
    feature map, the usual layer input), 'hm' (NCHW fp32 heat-map: the k2c conv) or 'img' (NCHW fp32 image: the stem, whose
    input gradient is never formed)."""

    def __init__(self, mod, x_kind, shapes, seed):
        self.mod, self.x_kind, self.shapes, self.seed = mod, x_kind, shapes, seed
        self.ref = _Ref(mod)
        self.exp = None
        self.dev = next(mod.parameters()).device

    def set_dtype(self, rt, dt):
        rt.set_compute_dtype(dt)
        self.dt = dt

    def _inputs(self, shape):
        self.seed += 2
        x64 = randn(self.seed, *shape).double()
        if self.x_kind == 'feat':
            x64 = _round(x64, self.dt)
            x = x64.float().to(self.dev).to(DT[self.dt]).contiguous(memory_format=torch.channels_last)
        else:
            x = x64.float().to(self.dev)
            if self.x_kind == 'img':
                x64 = _round(x64, self.dt)
        if self.x_kind != 'img':
            x.requires_grad_(True)
            x64.requires_grad_(True)
        return x, x64

    def zero_grad(self):
        from mi355.nn import mark_grads_fresh
        ps = [p for p in self.mod.parameters() if p.grad is not None]
        for p in ps:
            p.grad.fill_(float('nan'))
        mark_grads_fresh(ps)
        self.exp = None

    def forward(self, step, shape, backward=True, zero=True, training=True):
        what = '%s %s %s' % (step, self.dt, tuple(shape))
        self.mod.train(training)
        if backward and zero:
            self.zero_grad()
        x, x64 = self._inputs(shape)
        P = self.ref.params(self.dt)
        if backward:
            y = self.mod(x)
            y_ref = self.ref.forward(P, x64, self.dt, training)
        else:           # training: a forward whose autograd graph is dropped; eval: the no_grad inference path
            with torch.set_grad_enabled(training):
                y = self.mod(x)
            with torch.no_grad():
                y_ref = self.ref.forward(P, x64.detach(), self.dt, training)
        assert tuple(y.shape) == tuple(y_ref.shape), what
        _near(what + ': output', y.float(), y_ref, REL[self.dt])
        if not backward:
            return
        dy64 = randn(self.seed + 1, *y_ref.shape).double()
        if y.dtype == torch.bfloat16:
            dy64 = _round(dy64, 'bf16')
        dy = dy64.float().to(self.dev).to(y.dtype)
        if not y.is_contiguous():                       # a channels_last feature map (heat-maps are contiguous NCHW)
            dy = dy.contiguous(memory_format=torch.channels_last)
        y.backward(dy)
        y_ref.backward(dy64)
        if self.x_kind != 'img':
            _near(what + ': input gradient', x.grad.float(), x64.grad, REL[self.dt])
        got = dict(self.mod.named_parameters())
        if self.exp is None:
            self.exp = {k: P[k].grad.clone() for k in P}
        else:
            for k in P:
                self.exp[k] += P[k].grad
        # a bias in front of a training-mode BatchNorm has the gradient zero (rounding noise in the reference): the floor keeps
        # the bound meaningful there and still catches a stale value
        floor = 1e-3 * max(float(g.abs().max()) for g in self.exp.values())
        for k, g in self.exp.items():
            _near('%s: gradient of %s' % (what, k), got[k].grad, g, REL[self.dt], floor)

    def load_fresh(self, seed):
        sd = _fresh_state(self.mod, seed)
        self.mod.load_state_dict(sd)
        self.ref.load_buffers(sd)


def _run_sequence(rt, mod, x_kind, A, B, base='bf16', other='f32', seed=100):
    s = _Seq(mod, x_kind, (A, B), seed)
    s.set_dtype(rt, base)
    s.forward('a', A)
    s.forward('b', B)
    s.set_dtype(rt, other)
    s.forward('c', B)
    s.forward('c', A)
    s.set_dtype(rt, base)
    s.forward('c', B)
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() == 4:
                p.mul_(0.5)
    s.forward('d (in-place weight edit)', A)
    s.load_fresh(seed + 50)
    s.forward('d (load_state_dict)', A)
    s.forward('e (forward only)', A, backward=False)
    s.forward('e', A)
    s.forward('f (accumulate 1)', A, zero=False)
    s.forward('f (accumulate 2)', A, zero=False)
    s.forward('f (overwrite)', A)
    from mi355 import nn as mnn
    if any(isinstance(m, mnn.BatchNorm2d) for _, m in _layers(mod)):
        s.forward('g (eval, folded BatchNorm)', A, backward=False, training=False)
        s.forward('g (train again)', A)
        s.forward('g (train again, shape B)', B)


def _conv_bn(gpu, cin, cout, stride, seed):
    from mi355 import nn as mnn
    m = mnn.FusedSequential(mnn.Conv2d(cin, cout, 3, stride, 1, bias=True), mnn.BatchNorm2d(cout), mnn.ReLU()).to(gpu)
    assert m[0].bn_follows
    return fill_module_(m, seed)


@pytest.mark.parametrize('base,other', [('f32', 'bf16'), ('bf16', 'f32')])
def test_stem_conv_state_sequence(rt, gpu, base, other):
    """Conv2d(3, 64, 7, 2, 3): even extents take the folded 4x4 form, odd ones the 7x7 form over the channel-padded image (4
    channels in f32, 8 in bf16); both leave their weight-gradient scratch in _stem_tmp."""
    from mi355 import nn as mnn
    conv = fill_module_(mnn.Conv2d(3, 64, 7, 2, 3, bias=False).to(gpu), 1)
    _run_sequence(rt, conv, 'img', (2, 3, 32, 32), (3, 3, 29, 27), base, other)


@pytest.mark.parametrize('stride,cout', [(1, 64), (2, 128)])
def test_conv3x3_batchnorm_state_sequence(rt, gpu, stride, cout):
    """3x3 conv (with a bias) -> BatchNorm2d -> ReLU linked as in the model: fused statistics, the bias-gradient zero hand-off
    (_BN_DX) and the eval-mode fold are live."""
    m = _conv_bn(gpu, 64, cout, stride, 2)
    _run_sequence(rt, m, 'feat', (2, 64, 16, 16), (3, 64, 11, 9))


def test_conv1x1_streaming_gemm_state_sequence(rt, gpu):
    """1x1 conv at >= 32 K rows and K = 64: the weights-stationary streaming GEMM in bf16 (MI355_PGEMM default)."""
    from mi355 import nn as mnn
    conv = fill_module_(mnn.Conv2d(64, 64, 1, 1, 0, bias=True).to(gpu), 3)
    _run_sequence(rt, conv, 'feat', (8, 64, 64, 64), (9, 64, 61, 67))


def test_grouped_conv_state_sequence(rt, gpu):
    from mi355 import nn as mnn
    conv = fill_module_(mnn.Conv2d(128, 128, 3, 1, 1, bias=False, groups=32).to(gpu), 4)
    _run_sequence(rt, conv, 'feat', (2, 128, 16, 16), (3, 128, 7, 9))


def test_deconv_batchnorm_state_sequence(rt, gpu):
    """ConvTranspose2d(256, 256, 4, 2, 1) -> BatchNorm2d -> ReLU, as in the neck."""
    from mi355 import nn as mnn
    m = fill_module_(mnn.FusedSequential(mnn.ConvTranspose2d(256, 256, 4, 2, 1), mnn.BatchNorm2d(256), mnn.ReLU()).to(gpu), 5)
    _run_sequence(rt, m, 'feat', (2, 256, 8, 8), (3, 256, 5, 7))


@pytest.mark.parametrize('mode', ['c2k', 'k2c'])
def test_heatmap_1x1_state_sequence(rt, gpu, mode):
    """The heat-map head's 1x1 convs: features -> 21 heat-maps (c2k, _CastCopy of the weight) and 21 heat-maps -> features
    (k2c, the transposed _CastCopy in its input gradient)."""
    from mi355 import nn as mnn
    cin, cout = (256, 21) if mode == 'c2k' else (21, 256)
    conv = fill_module_(mnn.Conv2d(cin, cout, 1, 1, 0, bias=True).to(gpu), 6)
    assert conv.mode == mode
    _run_sequence(rt, conv, 'feat' if mode == 'c2k' else 'hm', (2, cin, 16, 16), (3, cin, 9, 13))


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_fp8_conv_state_sequence(rt, gpu):
    """'fp8' mode, 3x3 128 -> 128, steps a, b, d, f against the same layer in bf16 (a second instance that loads this one's
    state before every step) within test_fp8_layers_track_the_bf16_layers' bound: relative L2 <= 8e-2."""
    from mi355 import nn as mnn
    from mi355.nn import mark_grads_fresh
    mod = fill_module_(mnn.Conv2d(128, 128, 3, 1, 1, bias=True).to(gpu), 7)
    twin = mnn.Conv2d(128, 128, 3, 1, 1, bias=True).to(gpu)
    seed = [300]

    def step(what, shape, zero=True):
        seed[0] += 2
        x0 = randn(seed[0], *shape).to(gpu).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        twin.load_state_dict(mod.state_dict())
        res = []
        for m, dt in ((twin, 'bf16'), (mod, 'fp8')):
            rt.set_compute_dtype(dt)
            if zero:
                ps = [p for p in m.parameters() if p.grad is not None]
                for p in ps:
                    p.grad.fill_(float('nan'))
                mark_grads_fresh(ps)
            x = x0.clone().requires_grad_(True)
            y = m(x)
            dy = (randn(seed[0] + 1, *y.shape) * 1e-2).to(gpu).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            y.backward(dy)
            res.append((y.float(), x.grad.float(), m.weight.grad.clone(), m.bias.grad.clone()))
        for name, a, b in zip(('output', 'input gradient', 'weight gradient', 'bias gradient'), res[1], res[0]):
            e = _rel_l2(a, b)
            assert e <= 8e-2, '%s: %s relative L2 %.4g' % (what, name, e)

    step('a', (2, 128, 16, 16))
    step('b', (3, 128, 9, 13))
    with torch.no_grad():
        mod.weight.mul_(0.5)
    step('d (in-place weight edit)', (2, 128, 16, 16))
    mod.load_state_dict(_fresh_state(mod, 8))
    step('d (load_state_dict)', (2, 128, 16, 16))
    step('f (accumulate 1)', (2, 128, 16, 16), zero=False)
    step('f (accumulate 2)', (2, 128, 16, 16), zero=False)
    step('f (overwrite)', (2, 128, 16, 16))


# ---------------------------------------------------------------- flat gradient buffer (FusedSGD) written by others
def _small_net(gpu, seed):
    from mi355 import nn as mnn
    m = mnn.FusedSequential(mnn.Conv2d(32, 64, 3, 1, 1, bias=True), mnn.BatchNorm2d(64), mnn.ReLU(),
                            mnn.Conv2d(64, 32, 3, 1, 1, bias=True)).to(gpu)
    fill_module_(m, seed)
    ref = torch.nn.Sequential(torch.nn.Conv2d(32, 64, 3, 1, 1, bias=True), torch.nn.BatchNorm2d(64), torch.nn.ReLU(),
                              torch.nn.Conv2d(64, 32, 3, 1, 1, bias=True)).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in m.state_dict().items()})
    return m, ref


def _edit(i, mine, ref, opt):
    """Three writers into the gradients that are not the bias-gradient code, applied to both."""
    k = i % 3
    if k == 0:                                   # a manual write into one bias gradient
        mine[0].bias.grad.add_(1.0)
        ref[0].bias.grad.add_(1.0)
    elif k == 1:                                 # scaling the flat buffer itself
        opt.flat_grads()[0].mul_(3.0)
        for p in ref.parameters():
            p.grad.mul_(3.0)
    else:                                        # clipping (in place: the norm is far above the limit)
        n = torch.nn.utils.clip_grad_norm_(list(mine.parameters()), 0.05)
        torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 0.05)
        assert float(n) > 0.05


def _check_params(what, mine, ref):
    got = dict(mine.named_parameters())
    for k, p in ref.named_parameters():
        _near('%s: %s' % (what, k), got[k], p, REL['f32'])


@pytest.mark.parametrize('replayed', [False, True])
def test_fused_sgd_flat_gradients_written_by_others(rt, gpu, replayed):
    """conv (bias) -> BatchNorm -> ReLU -> conv under FusedSGD next to a float64 copy under torch.optim.SGD(nesterov=True).  The
    first conv's bias gradient is zero (it feeds a training-mode BatchNorm) and the backward skips its fill once it has written
    those zeros (_zero_grad_once): a write into the flat gradient buffer by anyone else must not survive into the next step.
    Replayed: forward + backward and opt.step() captured as two graphs after two eager iterations; the edits go between them."""
    from mi355.optim import FusedSGD
    rt.set_compute_dtype('f32')
    mine, ref = _small_net(gpu, 9)
    mine.train(); ref.train()
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt = FusedSGD(mine.parameters(), **kw)
    opt_ref = torch.optim.SGD(ref.parameters(), **kw)
    x64 = randn(400, 4, 32, 12, 12).double()
    dy64 = randn(401, 4, 32, 12, 12).double()
    x = x64.float().to(gpu).contiguous(memory_format=torch.channels_last)
    dy = dy64.float().to(gpu).contiguous(memory_format=torch.channels_last)

    def fwdbwd():
        opt.zero_grad()
        mine(x).backward(dy)
        rt.join_side()

    n_iter = 7
    g_fb = g_st = None
    for i in range(n_iter):
        if replayed and i == 2:
            torch.cuda.synchronize()
            mode = rt.graph_capture_mode()
            g_fb, g_st = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_fb, capture_error_mode=mode):
                fwdbwd()
            with torch.cuda.graph(g_st, capture_error_mode=mode):
                opt.step()
        if g_fb is not None:
            g_fb.replay()
        else:
            fwdbwd()
        opt_ref.zero_grad()
        ref(x64).backward(dy64)
        _edit(i, mine, ref, opt)
        if g_st is not None:
            g_st.replay()
        else:
            opt.step()
        opt_ref.step()
        torch.cuda.synchronize()
        _check_params('iteration %d%s' % (i, ' (replayed)' if g_fb is not None else ''), mine, ref)


# ---------------------------------------------------------------- a gradient tensor the caller created
@pytest.mark.parametrize('case', ['plain', 'plain-grouped-launch', 'groups', 'stem-folded', 'stem-padded', 'deconv'])
def test_foreign_order_gradient_tensor(rt, gpu, case):
    """p.grad set by the caller as a contiguous NCHW-order tensor (not the [Co][kh][kw][Ci] strides grad_slot creates), then a
    backward: every weight-gradient branch must either give the right values (accumulated onto the caller's) or raise
    Mi355Error -- never write its own layout into the foreign one."""
    import mi355
    from mi355 import Mi355Error, nn as mnn
    rt.set_compute_dtype('f32')
    x_kind, shape = 'feat', (2, 64, 12, 12)
    if case.startswith('plain'):
        mod = mnn.Conv2d(64, 64, 3, 1, 1, bias=False)
    elif case == 'groups':
        mod = mnn.Conv2d(64, 64, 3, 1, 1, bias=False, groups=16)
    elif case == 'deconv':
        mod, shape = mnn.ConvTranspose2d(64, 64, 4, 2, 1), (2, 64, 6, 6)
    else:
        mod, x_kind = mnn.Conv2d(3, 64, 7, 2, 3, bias=False), 'img'
        shape = (2, 3, 16, 16) if case == 'stem-folded' else (2, 3, 15, 17)
    mod = fill_module_(mod.to(gpu), 10)
    w = mod.weight
    w.grad = torch.full(w.shape, 0.5, device=gpu)
    assert not w.grad.permute(0, 2, 3, 1).is_contiguous()
    s = _Seq(mod, x_kind, (shape, shape), 500)
    s.dt = 'f32'
    x, x64 = s._inputs(shape)
    P = s.ref.params('f32')
    y_ref = s.ref.forward(P, x64, 'f32', True)
    dy64 = randn(501, *y_ref.shape).double()
    y_ref.backward(dy64)
    try:
        if case == 'plain-grouped-launch':
            with mi355.grouped_wgrads():
                mod(x).backward(dy64.float().to(gpu).contiguous(memory_format=torch.channels_last))
            mi355.join_side()
        else:
            mod(x).backward(dy64.float().to(gpu).contiguous(memory_format=torch.channels_last))
    except Mi355Error:
        return
    _near(case + ': weight gradient onto a foreign-order tensor', w.grad, P['weight'].grad + 0.5, REL['f32'])


# ---------------------------------------------------------------- GraphedForward
def test_graphed_forward_follows_the_compute_dtype(rt, gpu):
    """A forward captured in f32 must not be replayed after set_compute_dtype('bf16'): the output equals an eager bf16 forward."""
    from mi355 import nn as mnn
    from mi355.infer import GraphedForward
    m = fill_module_(mnn.FusedSequential(mnn.Conv2d(64, 64, 3, 1, 1, bias=False), mnn.BatchNorm2d(64), mnn.ReLU()).to(gpu), 11)
    m.eval()
    gf = GraphedForward(m, warmup=1)
    x = randn(600, 2, 64, 16, 16).to(gpu)
    rt.set_compute_dtype('f32')
    with torch.no_grad():
        for _ in range(3):                   # eager warm-up, capture, replay
            y32 = gf(x)
        assert len(gf._graphs) == 1 and y32.dtype == torch.float32
        rt.set_compute_dtype('bf16')
        y = gf(x)
        y_eager = m(x)
        assert y.dtype == y_eager.dtype == torch.bfloat16
        assert torch.equal(y, y_eager)
        for _ in range(2):                   # and the bf16 graph, once captured, too
            y = gf(x)
        assert torch.equal(y, y_eager)


# ---------------------------------------------------------------- caller buffers: size checks before any launch
def test_ops_reject_undersized_caller_buffers(rt, gpu):
    """Every ops.* wrapper that writes into a caller-provided buffer raises Mi355Error, without launching, when the buffer is one
    element short.  Only allocations happen here (torch.empty launches nothing)."""
    from mi355 import Mi355Error, ops
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=gpu)
    nhwc = lambda N, C, H, W, dt=torch.bfloat16: ops.nhwc_empty(N, C, H, W, dt, gpu)
    bf = torch.bfloat16
    d3 = ops.make_desc(1, 8, 8, 64, 64, 3, 3, 1, 1, bf)
    x, dy = nhwc(1, 64, 8, 8), nhwc(1, 64, 8, 8)
    wt = e(64 * 9 * 64, dt=bf)
    stem = ops.make_desc(1, 15, 15, 8, 64, 7, 7, 2, 3, bf)          # the 7x7 form: Ci padded to 8 in bf16
    cases = {
        'conv_wgrad dw': lambda: ops.conv_wgrad(d3, x, dy, e(64 * 9 * 64 - 1), False),
        'conv_wgrad dw (stem, 16384-float folded buffer)': lambda: ops.conv_wgrad(stem, nhwc(1, 8, 15, 15), nhwc(1, 64, 8, 8),
                                                                                  e(64 * 256), False),
        'conv_wgrad_grouped dw': lambda: ops.conv_wgrad_grouped([(d3, x, dy, e(64 * 9 * 64 - 1), False)]),
        'conv_dgrad out': lambda: ops.conv_dgrad(d3, dy, wt, out=nhwc(1, 64, 8, 7)),
        'conv_dgrad_masked_acc out': lambda: ops.conv_dgrad_masked_acc(d3, dy, wt, nhwc(1, 64, 8, 7), e(512, dt=torch.uint8)),
        'conv_dgrad_masked_acc mask': lambda: ops.conv_dgrad_masked_acc(d3, dy, wt, nhwc(1, 64, 8, 8), e(511, dt=torch.uint8)),
        'colsum out': lambda: ops.colsum(nhwc(2, 64, 4, 4), e(63), False),
        'pw_wgrad dw': lambda: ops.pw_wgrad(nhwc(1, 256, 4, 4), e(1, 21, 4, 4), e(21 * 256 - 1), True, False),
        'hm_rowsum out': lambda: ops.hm_rowsum(e(1, 21, 4, 4), e(20), False),
        'bilinear_up out': lambda: ops.bilinear_up(e(1, 21, 8, 8), 16, out=e(1, 21, 15, 16)),
        'cast_f32 dst': lambda: ops.cast_f32(e(100), e(99, dt=bf)),
        'sgd_nesterov g': lambda: ops.sgd_nesterov(e(100), e(99), e(100), e(()), 0.9, 1e-4, True),
        'sgd_nesterov buf': lambda: ops.sgd_nesterov(e(100), e(100), e(99), e(()), 0.9, 1e-4, True),
        'stem_s2d_pack out': lambda: ops.stem_s2d_pack(e(64 * 147), bf, out=e(64 * 256 - 1, dt=bf)),
        'stem_s2d_unpack_grad gs': lambda: ops.stem_s2d_unpack_grad(e(64 * 256 - 1), e(64 * 147), False),
        'apply_relu_mask mask': lambda: ops.apply_relu_mask(nhwc(1, 64, 8, 8), e(511, dt=torch.uint8)),
    }
    for name, call in cases.items():
        with pytest.raises(Mi355Error, match='buffer of'):
            call()
