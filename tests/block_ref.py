"""Two references for the composites of mi355.nn layers (stem, residual blocks, stages, neck, heads).  Nothing here imports
from mi355.nn: the glue under test -- its autograd Functions, its address-keyed hand-off tables, its per-forward module
attributes -- is not used, layers are told apart by class name and read only for their parameters and their geometry.

  Plain    the composite as explicit mi355.ops calls on named tensors: every forward intermediate kept in a dict, the backward
           written out by hand in reverse order, the fork sum and the ReLU mask as stand-alone tensors.  It rounds where the
           glue rounds, so the glue is held to it bit for bit.  What changes where a sum or a rounding happens is an explicit
           argument (Choices); the running statistics live in a dict of the caller's, never in the module.
  T64      the same composite on the CPU with torch autograd in float64 (or float32: the reference's own noise).

wgrad64 / wgrad_bound: the float64 weight gradient of one conv and the forward error bound of its fp32 sum.
anchor_err / anchor_bound: the element-wise comparison against T64.
"""
import torch
import torch.nn.functional as F

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
NAN = float('nan')


def kind(m):
    """class name of a layer: 'Conv2d', 'ConvTranspose2d', 'BatchNorm2d', 'ReLU', 'MaxPool2d', 'FusedSequential', ..."""
    return type(m).__name__


class Choices:
    """Where a sum or a rounding happens.
    stats  'epilogue': BatchNorm statistics from the producing conv's epilogue; 'pass': a stand-alone pass over its stored output
    fork   'epilogue': the residual fork's sum inside conv1's input-gradient epilogue (accumulate onto the branch gradient);
           'add': a separate element-wise add of the two stored gradients
    stem   'folded': the 7x7 stem as a 4x4 conv over the 2x2 space-to-depth image; 'padded': over the channel-padded image
    bnbwd  BatchNorm-backward sums from the input-gradient epilogue of the conv behind it
    mask   source of a BatchNorm backward's ReLU mask.  It selects the kernel form, and with it the order of the backward's sums:
           mi355_bn_bwd reduces in one launch unless it has to read y.  'x': recomputed from the BatchNorm input (no residual);
           'bits': the bit mask the forward wrote (with a residual); 'y': the stored output.  One choice for the BatchNorms
           without a residual (mask), one for the block's last (mask_res)."""

    def __init__(self, stats='epilogue', fork='epilogue', stem='folded', bnbwd=False, mask='x', mask_res='bits'):
        assert stats in ('epilogue', 'pass') and fork in ('epilogue', 'add') and stem in ('folded', 'padded')
        assert mask in ('x', 'y') and mask_res in ('bits', 'y')
        self.stats, self.fork, self.stem, self.bnbwd, self.mask, self.mask_res = stats, fork, stem, bool(bnbwd), mask, mask_res


def snapshot(mod):
    """clones of every BatchNorm buffer of mod, by state_dict name: Plain's own running statistics"""
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if 'running_' in k or k.endswith('num_batches_tracked')}


class Plain:
    """t: forward intermediates by layer name; g: gradients by parameter name (conv weights as [Co][kh][kw][Ci], the memory
    order of the parameter) -- NaN-filled before the kernel that must overwrite them."""

    def __init__(self, bufs, dtype, choices=None):
        from mi355 import ops
        self.ops, self.buf, self.dtype, self.c = ops, bufs, dtype, choices or Choices()
        self.t, self.g = {}, {}

    # ---- single layers
    def conv_f(self, name, conv, x):
        ops = self.ops
        N, C, H, W = x.shape
        Co, k = conv.out_channels, conv.kernel_size[0]
        desc = ops.make_desc(N, H, W, C, Co, k, k, conv.stride[0], conv.padding[0], x.dtype)
        wf, wt = ops.pack_weights(conv.weight.detach(), Co, k * k, conv.in_channels, C, x.dtype)
        if self.c.stats == 'epilogue':
            y, part = ops.conv_fwd_stats(desc, x, wf, None)
        else:
            y, part = ops.conv_fwd(desc, x, wf), None
        self.t[name] = dict(x=x, y=y, desc=desc, wf=wf, wt=wt, part=part, shape=(Co, k, k, C))
        return y, part

    def deconv_f(self, name, dc, x):
        """ConvTranspose2d = the adjoint of its conv-form (Co = in_channels, Ci = out_channels): forward = input gradient"""
        ops = self.ops
        N, C, H, W = x.shape
        k, s, p = dc.kernel_size[0], dc.stride[0], dc.padding[0]
        desc = ops.make_desc(N, (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k, dc.out_channels, dc.in_channels, k, k, s, p, x.dtype)
        wf, wt = ops.pack_weights(dc.weight.detach(), dc.in_channels, k * k, dc.out_channels, dc.out_channels, x.dtype)
        if self.c.stats == 'epilogue':
            y, part = ops.conv_dgrad_stats(desc, x, wt)
        else:
            y, part = ops.conv_dgrad(desc, x, wt), None
        self.t[name] = dict(x=x, y=y, desc=desc, wf=wf, wt=wt, part=part, shape=(dc.in_channels, k, k, dc.out_channels))
        return y, part

    def bn_f(self, name, bn, x, part, residual=None, relu=False):
        b = self.buf
        src = None if not relu else (self.c.mask if residual is None else self.c.mask_res)
        bits = self.ops.bn_relu_mask(x) if src == 'bits' else None
        y, mean, invstd = self.ops.bn_train_fwd(x, residual, bn.weight.detach(), bn.bias.detach(), b[name + '.running_mean'],
                                                b[name + '.running_var'], b[name + '.num_batches_tracked'], bn.eps, bn.momentum,
                                                relu, 1, partial=part, relu_mask=bits)
        self.t[name] = dict(x=x, y=y, mean=mean, invstd=invstd, relu=bool(relu), bn=bn, bits=bits, y_mask=y if src == 'y' else None)
        return y

    def bn_b(self, name, dy, want_dres=False, partial=None):
        """-> (dx, dres): dres is the masked gradient of the residual input, a tensor of its own"""
        s = self.t[name]
        bn = s['bn']
        dg, db = (torch.full((bn.num_features,), NAN, dtype=torch.float32, device=dy.device) for _ in range(2))
        dx, dres = self.ops.bn_bwd(dy, s['x'], s['y_mask'], bn.weight.detach(), s['mean'], s['invstd'], dg, db, False,
                                   s['relu'], want_dres, beta=bn.bias.detach(), partial=partial, relu_mask=s['bits'])
        self.g[name + '.weight'], self.g[name + '.bias'] = dg, db
        return dx, dres

    def _src(self, name):
        """the BatchNorm `name` as the input-gradient epilogue wants it: (x, y, gamma, beta, mean, invstd, relu)"""
        s = self.t[name]
        bn = s['bn']
        return (s['x'], s['y_mask'], bn.weight.detach(), bn.bias.detach(), s['mean'], s['invstd'], s['relu'])

    def _wgrad(self, name, x, dy):
        s = self.t[name]
        Co, kh, kw, Ci = s['shape']
        dw = torch.full((Co * kh * kw * Ci,), NAN, dtype=torch.float32, device=dy.device)
        self.ops.conv_wgrad(s['desc'], x, dy, dw, False)
        s['wx'], s['wdy'] = x, dy                     # the operands of this layer's weight gradient, for wgrad64
        self.g[name + '.weight'] = dw.view(Co, kh, kw, Ci)

    def conv_b(self, name, dy, want_dx=True, onto=None, src=None):
        """weight gradient, then the input gradient (added onto `onto` in the epilogue when given).  src: name of the BatchNorm
        that produced this conv's input -> with Choices.bnbwd its backward sums come from this epilogue.  -> (dx, partial)"""
        s = self.t[name]
        self._wgrad(name, s['x'], dy)
        if not want_dx:
            return None, None
        if self.c.bnbwd and src is not None:
            return self.ops.conv_dgrad_bnbwd(s['desc'], dy, s['wt'], self._src(src), out=onto, accumulate=onto is not None)
        return self.ops.conv_dgrad(s['desc'], dy, s['wt'], out=onto, accumulate=onto is not None), None

    def deconv_b(self, name, dy, want_dx=True, src=None):
        s = self.t[name]
        self._wgrad(name, dy, s['x'])                 # conv-form input = dy, conv-form output gradient = x
        if not want_dx:
            return None, None
        if self.c.bnbwd and src is not None:
            return self.ops.conv_fwd_bnbwd(s['desc'], dy, s['wf'], self._src(src))
        return self.ops.conv_fwd(s['desc'], dy, s['wf']), None

    # ---- composites: forward, then backward in reverse order
    def stem_f(self, pre, m, img):
        """img: NCHW fp32 image -> pool(relu(bn1(conv1(img))))"""
        ops, conv = self.ops, m.conv1
        dtype = self.dtype
        N, _, H, W = img.shape
        Co = conv.out_channels
        if self.c.stem == 'folded':
            x = ops.to_nhwc_s2d(img, dtype)
            desc = ops.make_desc(N, H // 2, W // 2, 16, Co, 4, 4, 1, 2, dtype, out_hw=(H // 2, W // 2))
            wf = ops.stem_s2d_pack(conv.weight.detach(), dtype)
        else:
            cp = 8 if dtype == torch.bfloat16 else 4
            x = ops.to_nhwc(img, dtype, cp)
            desc = ops.make_desc(N, H, W, cp, Co, 7, 7, 2, 3, dtype)
            wf, _ = ops.pack_weights(conv.weight.detach(), Co, 49, 3, cp, dtype)
        if self.c.stats == 'epilogue':
            y, part = ops.conv_fwd_stats(desc, x, wf, None)
        else:
            y, part = ops.conv_fwd(desc, x, wf), None
        self.t[pre + 'conv1'] = dict(x=x, y=y, desc=desc)
        a = self.bn_f(pre + 'bn1', m.bn1, y, part, relu=True)
        p, arg = ops.maxpool_fwd(a)
        self.t[pre + 'maxpool'] = dict(x=a, y=p, arg=arg)
        return p

    def stem_b(self, pre, m, dp):
        ops = self.ops
        s, c = self.t[pre + 'maxpool'], self.t[pre + 'conv1']
        da = ops.maxpool_bwd(dp, s['arg'], tuple(s['x'].shape))
        dy, _ = self.bn_b(pre + 'bn1', da)
        Co = m.conv1.out_channels
        g = torch.full((Co, 7, 7, 3), NAN, dtype=torch.float32, device=dp.device)
        if self.c.stem == 'folded':
            tmp = torch.full((Co * 256,), NAN, dtype=torch.float32, device=dp.device)
            ops.conv_wgrad(c['desc'], c['x'], dy, tmp, False)
            ops.stem_s2d_unpack_grad(tmp, g, False)
        else:
            cp = c['x'].shape[1]
            tmp = torch.full((Co, 7, 7, cp), NAN, dtype=torch.float32, device=dp.device)
            ops.conv_wgrad(c['desc'], c['x'], dy, tmp, False)
            g.copy_(tmp[..., :3])
        self.g[pre + 'conv1.weight'] = g

    def block_f(self, pre, blk, x):
        """BasicBlock / Bottleneck: conv-BN(-ReLU) chain, the last BatchNorm adds the identity branch and applies the ReLU"""
        n = 3 if hasattr(blk, 'conv3') else 2
        y, part = self.conv_f(pre + 'conv1', blk.conv1, x)
        idn = x
        if blk.downsample is not None:
            yd, pd = self.conv_f(pre + 'downsample.0', blk.downsample[0], x)
            idn = self.bn_f(pre + 'downsample.1', blk.downsample[1], yd, pd)
        for i in range(1, n):
            a = self.bn_f(pre + 'bn%d' % i, getattr(blk, 'bn%d' % i), y, part, relu=True)
            y, part = self.conv_f(pre + 'conv%d' % (i + 1), getattr(blk, 'conv%d' % (i + 1)), a)
        return self.bn_f(pre + 'bn%d' % n, getattr(blk, 'bn%d' % n), y, part, residual=idn, relu=True)

    def block_b(self, pre, blk, dy, partial=None, in_src=None):
        """dy: gradient of the block output (partial: its BatchNorm-backward sums, when the consumer's epilogue formed them);
        in_src: the BatchNorm that produced the block input.  -> (dx, partial of dx for in_src)"""
        n = 3 if hasattr(blk, 'conv3') else 2
        d, dres = self.bn_b(pre + 'bn%d' % n, dy, want_dres=True, partial=partial)
        for i in range(n, 1, -1):
            d, part = self.conv_b(pre + 'conv%d' % i, d, src=pre + 'bn%d' % (i - 1))
            d, _ = self.bn_b(pre + 'bn%d' % (i - 1), d, partial=part)
        if blk.downsample is not None:
            dd, _ = self.bn_b(pre + 'downsample.1', dres)
            dres, _ = self.conv_b(pre + 'downsample.0', dd, src=in_src)
        if self.c.fork == 'epilogue':
            return self.conv_b(pre + 'conv1', d, onto=dres, src=in_src)
        dx1, _ = self.conv_b(pre + 'conv1', d)
        return dx1 + dres, None            # one addition in fp32, one rounding to the storage dtype

    def stage_f(self, pre, seq, x):
        for i, blk in enumerate(seq):
            x = self.block_f('%s%d.' % (pre, i), blk, x)
        return x

    def stage_b(self, pre, seq, dy):
        part = None
        for i in range(len(seq) - 1, -1, -1):
            blk = seq[i]
            prev = None
            if i > 0:
                prev = '%s%d.bn%d' % (pre, i - 1, 3 if hasattr(seq[i - 1], 'conv3') else 2)
            dy, part = self.block_b('%s%d.' % (pre, i), blk, dy, partial=part, in_src=prev)
        return dy

    def neck_f(self, pre, seq, x):
        """[ConvTranspose2d, BatchNorm2d, ReLU] x n"""
        mods = list(seq)
        for i in range(0, len(mods), 3):
            y, part = self.deconv_f('%s%d' % (pre, i), mods[i], x)
            x = self.bn_f('%s%d' % (pre, i + 1), mods[i + 1], y, part, relu=True)
        return x

    def neck_b(self, pre, seq, dy):
        part = None
        for i in range(len(list(seq)) - 3, -1, -3):
            d, _ = self.bn_b('%s%d' % (pre, i + 1), dy, partial=part)
            dy, part = self.deconv_b('%s%d' % (pre, i), d, src=('%s%d' % (pre, i - 2)) if i > 0 else None)
        return dy


def plain(bufs, dtype, choices=None):
    return Plain(bufs, dtype, choices)


# ---------------------------------------------------------------- float64 weight gradient and the bound of its fp32 sum
def wgrad64(desc, x, dy):
    """float64 weight gradient [Co][kh][kw][Ci] of the conv `desc` from its stored operands, on their device"""
    N, Ci, Co, k = desc.N, desc.Ci, desc.Co, desc.kh
    cols = F.unfold(x.double().contiguous(), k, padding=desc.pad, stride=desc.stride)       # [N, Ci*k*k, Ho*Wo], rows (ci, kh, kw)
    d = dy.double().contiguous().reshape(N, Co, -1)
    return torch.einsum('nol,nkl->ok', d, cols).view(Co, Ci, k, k).permute(0, 2, 3, 1)


def wgrad_bound_terms(desc, x, dy):
    """sum |x| |dy| per weight-gradient element: the same weight gradient of |x|, |dy| in float64"""
    return wgrad64(desc, x.double().abs(), dy.double().abs())


U32 = 2.0 ** -24      # unit round-off of fp32


def wgrad_bound(M, sum_abs, ref):
    """|fp32 sum of M products - exact| per element, whatever the order of the sum.
    Each product is rounded once (factor 1 + d, |d| <= u: f32 operands; a product of two bf16 values has 16 significant bits
    and is exact, d = 0) and then takes part in at most M - 1 additions, each 1 + d: the computed sum is
    sum_i p_i * prod(1 + d_ij) with at most M factors per term, so |error| <= gamma_M * sum|x||dy|, gamma_M = M u / (1 - M u)
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2).  Partial sums that meet in a second kernel
    (split reduction) are additions like any other and are counted in M - 1.  One more fp32 ulp of the result covers the final
    store.  bf16 operands need gamma_(M-1) only; gamma_M is used for both."""
    gamma = M * U32 / (1.0 - M * U32)
    ulp = torch.abs(ref).clamp_min(2.0 ** -126) * 2.0 ** -23         # >= one fp32 ulp of the result
    return gamma * sum_abs + ulp


# ---------------------------------------------------------------- the float64 anchor
class T64:
    """The composite on the CPU with torch autograd.  Parameters are copied from the module at every step (P, leaves); running
    statistics are copied once and kept here (B)."""

    def __init__(self, mod, dtype=torch.float64):
        self.mod, self.dtype = mod, dtype
        self.B = {k: v.detach().cpu().to(dtype if v.is_floating_point() else v.dtype).clone() for k, v in mod.state_dict().items()
                  if 'running_' in k or k.endswith('num_batches_tracked')}
        self.P = {}

    def params(self):
        self.P = {k: p.detach().cpu().to(self.dtype).contiguous().requires_grad_(True) for k, p in self.mod.named_parameters()}
        return self.P

    def conv(self, name, m, x):
        return F.conv2d(x, self.P[name + '.weight'], self.P.get(name + '.bias'), m.stride, m.padding)

    def deconv(self, name, m, x):
        return F.conv_transpose2d(x, self.P[name + '.weight'], None, m.stride, m.padding)

    def bn(self, name, m, x, residual=None, relu=False):
        y = F.batch_norm(x, self.B[name + '.running_mean'], self.B[name + '.running_var'], self.P[name + '.weight'],
                         self.P[name + '.bias'], True, m.momentum, m.eps)
        self.B[name + '.num_batches_tracked'] += 1
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y

    def seq(self, pre, mods, x):
        """a FusedSequential of conv / transposed conv / BatchNorm / ReLU children, by child index"""
        for i, m in enumerate(mods):
            name, k = '%s%d' % (pre, i), kind(m)
            if k == 'Conv2d':
                x = self.conv(name, m, x)
            elif k == 'ConvTranspose2d':
                x = self.deconv(name, m, x)
            elif k == 'BatchNorm2d':
                x = self.bn(name, m, x)
            elif k == 'ReLU':
                x = F.relu(x)
            else:
                raise TypeError(k)
        return x

    def stem(self, pre, m, x):
        return F.max_pool2d(self.bn(pre + 'bn1', m.bn1, self.conv(pre + 'conv1', m.conv1, x), relu=True), 3, 2, 1)

    def block(self, pre, blk, x):
        n = 3 if hasattr(blk, 'conv3') else 2
        idn = x if blk.downsample is None else self.seq(pre + 'downsample.', blk.downsample, x)
        y = x
        for i in range(1, n):
            y = self.bn(pre + 'bn%d' % i, getattr(blk, 'bn%d' % i), self.conv(pre + 'conv%d' % i, getattr(blk, 'conv%d' % i), y), relu=True)
        y = self.conv(pre + 'conv%d' % n, getattr(blk, 'conv%d' % n), y)
        return self.bn(pre + 'bn%d' % n, getattr(blk, 'bn%d' % n), y, residual=idn, relu=True)

    def stage(self, pre, seq, x):
        for i, blk in enumerate(seq):
            x = self.block('%s%d.' % (pre, i), blk, x)
        return x

    def fusion_head(self, pre, h, f, hm):
        x = self.conv(pre + 'heatmap_conv', h.heatmap_conv, hm) + self.conv(pre + 'feature_conv', h.feature_conv, f)
        return self.seq(pre + 'model.', h.model, self.seq(pre + 'last_lay.', h.last_lay, x))

    def heads(self, m, f, lam):
        """f -> (y, y_adv, y_adv2, y_adv3); the three adversarial heads see f through the gradient layer (identity forward,
        gradient times lam)"""
        y = self.seq('head.', m.head, f)
        f_adv = f.detach() + lam * (f - f.detach())
        y_adv = self.seq('head_adv.', m.head_adv, f_adv)
        y_adv2 = self.fusion_head('head_adv2.', m.head_adv2, f_adv, y_adv)
        y_adv3 = self.fusion_head('head_adv3.', m.head_adv3, f_adv, y_adv2)
        return y, y_adv, y_adv2, y_adv3


torch64 = T64

ANCHOR_REL = 1e-4      # the project's fp32 layer bound (test_gpu_layer_state.REL['f32'])


def anchor_err(got, ref):
    return float((got.detach().double().cpu() - ref.detach().double()).abs().max())


def anchor_bound(e_cpu, ref):
    """[anchor] max|err| <= 3 * e_cpu + 1e-4 * max|ref|; e_cpu: max error of torch's own CPU float32 run of the same code"""
    return 3.0 * e_cpu + ANCHOR_REL * float(ref.detach().double().abs().max())


def run_t64(dtype, mod, fwd, xs, dys):
    """One step of composite `fwd(T, *xs) -> outputs` under T64(mod, dtype) with output gradients dys.
    -> (T, dict of every compared tensor: outputs y<i>, input gradients dx<i>, parameter gradients, running statistics)"""
    T = mod if isinstance(mod, T64) else T64(mod, dtype)
    T.params()
    xs = [x.detach().to(T.dtype).requires_grad_(x.requires_grad) for x in xs]
    ys = fwd(T, *xs)
    ys = ys if isinstance(ys, (tuple, list)) else (ys,)
    torch.autograd.backward(list(ys), [d.to(T.dtype) for d in dys])
    out = {}
    for i, y in enumerate(ys):
        out['y%d' % i] = y.detach()
    for i, x in enumerate(xs):
        if x.requires_grad:
            out['dx%d' % i] = x.grad.detach()
    for k, p in T.P.items():
        if p.grad is not None:
            out['grad ' + k] = p.grad.detach()
    for k, b in T.B.items():
        out[k] = b.detach().clone()
    return T, out
