"""The mean teacher inside a training iteration (reference train1.py:351-364, uda/model/loss.py:265-297).

``EMATeacher`` moves the teacher's weights after every iteration, so the BatchNorm-folded operands of its one-launch eval
convs go stale every iteration.  The host fold of ``mi355.nn._FoldedBn`` is several ATen launches per layer and allocates: it
cannot sit in a replayed graph.  ``InIterationTeacher`` owns fixed-address storage for every (conv, BatchNorm) pair the
teacher's eval forward folds -- fp32 scratch, packed operand, bias -- pins it into the layers' ``_FoldedBn`` and refreshes all
of it with ``refresh()``: one ``mi355_bn_fold_batched`` launch, one ``mi355_pack_weights_batched`` launch, the stem's pack, and
the ``repack_params`` / cast route for the convs with no BatchNorm behind them.  The packed operands are made from the folded
fp32 weights by the packers the host path uses, so they are that path's bits.  A grouped conv is folded in the dense
block-diagonal form the host path packs: its master is copied onto the diagonal of a zeroed fixed-address buffer first.

``MeanTeacher`` is what ``DAStep(mt=...)`` takes: the teacher, the device-resident loss and the per-epoch schedule of its weight
``m`` and of the joint curriculum ``k``.
"""
import torch

import mi355 as _rt
from . import Mi355Error, ops
from . import nn as _nn


class InIterationTeacher:
    def __init__(self, ema):
        self.ema, self.model = ema, ema.model_ema
        self._pairs = None              # [(folded, conv, bn, dtype, deconv, s2d)] in forward order
        self._sig = None
        self._pack_cache = {}
        self._plain = []

    # ------------------------------------------------------------ discovery and storage
    def _run(self, x):
        m = self.model
        if m.training:
            m.eval()
        prev = _rt.set_mx_eval(False)           # the teacher takes the folded bf16 path, as validate() does by default
        try:
            with torch.no_grad():
                return m.head(m.features(x))
        finally:
            _rt.set_mx_eval(prev)

    def _unpin(self):
        for mod in self.model.modules():
            f = getattr(mod, '_folded', None)
            if isinstance(f, _nn._FoldedBn):
                f.pin = None

    def _build(self, x):
        """One eval forward through the host fold records the (conv, BatchNorm) pairs; their storage is laid out once."""
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('InIterationTeacher: the first forward lays out the folded operands; run one eager iteration before capturing')
        self._unpin()
        convs = [mod for mod in self.model.modules() if isinstance(mod, (_nn.Conv2d, _nn.ConvTranspose2d))]
        _nn._FOLD_TRACE = trace = []
        try:
            self._run(x)
        finally:
            _nn._FOLD_TRACE = None
        seen, pairs = set(), []
        for ent in trace:
            if id(ent[0]) not in seen:
                seen.add(id(ent[0]))
                pairs.append(ent)
        self._pairs = pairs
        dev = x.device
        al = lambda n: (n + 3) // 4 * 4
        # (a grouped conv is folded and packed in its dense block-diagonal form, as the host path does: groups times the elements)
        self._n = [c.weight.numel() * getattr(c, 'groups', 1) for _, c, _, _, _, _ in pairs]
        self._dense = [torch.zeros(n, dtype=torch.float32, device=dev) if getattr(c, 'groups', 1) > 1 else None
                       for (_, c, _, _, _, _), n in zip(pairs, self._n)]
        self._C = [bn.num_features for _, _, bn, _, _, _ in pairs]
        self._w32 = torch.empty(sum(al(n) for n in self._n), dtype=torch.float32, device=dev)
        self._bias = torch.empty(sum(al(c) for c in self._C), dtype=torch.float32, device=dev)
        self._packed = []
        for (_, conv, _, dtype, deconv, s2d), n in zip(pairs, self._n):
            k2 = conv.kernel_size[0] * conv.kernel_size[1]
            if s2d:
                size = conv.out_channels * 256
            elif deconv:
                size = n
            else:
                size = conv.out_channels * k2 * conv._cin_pad(dtype)
            self._packed.append(torch.empty(size, dtype=dtype, device=dev))
        # the convs that run with no BatchNorm folded in (they own a packed or cast copy of their weight after this forward): those
        # copies follow through the existing routes
        folded = {id(conv) for _, conv, _, _, _, _ in pairs}
        owns = lambda m: (getattr(m.weight, '_mi_pack', None) is not None and m.weight._mi_pack[0].wf is not None) or \
            getattr(getattr(m, '_cast', None), 'buf', None) is not None
        self._plain = [mod for mod in convs if id(mod) not in folded and owns(mod)]
        self._sig = None

    def _sources(self):
        out = []
        for _, conv, bn, _, _, _ in self._pairs:
            out += [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.bias]
        return out

    def _ensure_tables(self):
        """The rule of EMATeacher._ensure_layout: when a source tensor moved (FusedSGD laid its buffers out again and the teacher's
        mirror followed), rebuild the record tables outside capture, raise inside."""
        sig = tuple(0 if t is None else t.data_ptr() for t in self._sources())
        if sig == self._sig:
            return
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('InIterationTeacher: a teacher tensor moved during graph capture; run one eager iteration before capturing')
        import numpy as np
        recs, packs, self._stem, self._diag = [], {}, [], []
        wo = bo = 0
        for (fold, conv, bn, dtype, deconv, s2d), n, C, packed, dense in zip(self._pairs, self._n, self._C, self._packed, self._dense):
            _nn._chk_convform(conv.weight)
            k2 = conv.kernel_size[0] * conv.kernel_size[1]
            O, I = (conv.in_channels, conv.out_channels) if deconv else (conv.out_channels, conv.in_channels)
            out_w, out_b = self._w32[wo:wo + n], self._bias[bo:bo + C]
            wo, bo = wo + (n + 3) // 4 * 4, bo + (C + 3) // 4 * 4
            wm = conv.weight.detach().permute(0, 2, 3, 1)                 # memory order [O][kh][kw][I]
            if dense is not None:
                # grouped: the master goes onto the diagonal of a dense [O][kh][kw][in_channels] buffer whose other elements stay
                # zero (nn._dense_from_grouped without its allocation: one strided copy per refresh), and the fold runs on that
                G, kh, kw = conv.groups, conv.kernel_size[0], conv.kernel_size[1]
                cog, cig = O // G, I // G
                diag = dense.as_strided((G, cog, kh, kw, cig), (cog * k2 * I + cig, k2 * I, kw * I, I, 1))
                self._diag.append((diag, wm.reshape(G, cog, kh, kw, cig)))
                wm = dense
            recs.append((wm, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                         None if conv.bias is None else conv.bias.detach(), out_w, out_b, float(bn.eps), O, k2, I, 1 if deconv else 0))
            if s2d:
                self._stem.append((out_w, dtype, packed))
            else:
                Ipad = I if deconv else conv._cin_pad(dtype)
                packs.setdefault(dtype, []).append((out_w, None if deconv else packed, packed if deconv else None, O, k2, I, Ipad))
            fold.pin = ((id(bn), dtype, deconv, s2d), packed, out_b)
        self._fold = ops.fold_table(recs, self._w32.device)
        self._packs = []
        for dtype, items in packs.items():
            rec = np.zeros(len(items), dtype=_nn.pack_item_dtype())
            blk = 0
            for i, (w, wf, wt, O, T, I, Ipad) in enumerate(items):
                need = O * T * Ipad
                for t in (wf, wt):
                    if t is not None and t.numel() < need:
                        raise Mi355Error('InIterationTeacher: packed operand of %d elements, the pack writes %d' % (t.numel(), need))
                rec[i] = (w.data_ptr(), _rt.ptr(wf), _rt.ptr(wt), O, T, I, Ipad, blk, 0)
                blk += ((Ipad + 31) // 32) * ((O + 31) // 32) * T
            self._packs.append((torch.from_numpy(rec.view(np.uint8).copy()).to(self._w32.device), len(items), blk, dtype))
        self._sig = sig

    # ------------------------------------------------------------ per iteration
    @torch.no_grad()
    def refresh(self):
        """Enqueue fold + pack of every pinned pair on the current stream, and the packed / cast copies of the other convs
        (capturable once one eager forward has run).  Whoever writes the teacher's tensors calls this afterwards."""
        if self._pairs is None:
            return                              # nothing pinned yet: the first forward() folds on the host and lays out
        self._ensure_tables()
        if self._pairs:
            for diag, src in self._diag:
                diag.copy_(src)
            ops.bn_fold_batched(*self._fold)
            for tab, count, blocks, dtype in self._packs:
                ops.pack_weights_batched(tab, count, blocks, dtype)
            for w32, dtype, out in self._stem:
                ops.stem_s2d_pack(w32, dtype, out=out)
        _nn.repack_params([m.weight for m in self._plain], self._pack_cache)
        for m in self._plain:
            # repack_params leaves the copies to the next forward when it cannot take them (a moved tensor, mixed dtypes): fine for
            # eager launches, but a captured update would replay with stale operands -- the layout rule: raise inside capture
            pk = getattr(m.weight, '_mi_pack', None)
            if pk is not None and pk[0].wf is not None and pk[0].key != (_nn._param_version(m.weight), pk[0].wf.dtype, pk[4]) and \
                    torch.cuda.is_current_stream_capturing():
                raise Mi355Error('InIterationTeacher: the packed copy of a teacher conv could not be refreshed during graph capture; '
                                 'run one eager iteration before capturing')
        for m in self._plain:                   # the bf16 copy of a point-wise C -> K weight (_CastCopy)
            cast = getattr(m, '_cast', None)
            if cast is not None and cast.buf is not None and not cast.transposed and cast.buf.dtype != torch.float32:
                ops.cast_f32(m.weight.detach(), cast.buf)
                cast.key = (_nn._param_version(m.weight), cast.buf.dtype)

    def forward(self, x):
        """y_t_ema = model_ema(x)[0]: eval mode, running statistics, no_grad (train1.py:364)."""
        if self._pairs is None:
            self._build(x)
            self.refresh()
        return self._run(x)

    __call__ = forward


class MeanTeacher:
    """The consistency term of step C: ``m * mt_loss(y_t, teacher(x_t_ema), weight_t, k)``.

    ``weight='ref'`` is the reference schedule (train1.py:351-353: m = 0.01 * epoch, 0.3 once epoch > 30), a float a constant;
    ``k='all'`` compares every joint (k = 400), ``'epoch'`` follows the reference's curriculum with k = epoch."""

    def __init__(self, ema, weight='ref', k='all'):
        if ema is None:
            raise ValueError('the mean-teacher loss needs an EMATeacher (--ema-update const|warmup)')
        if k not in ('all', 'epoch'):
            raise ValueError("k must be 'all' or 'epoch', got %r" % (k,))
        from uda.model.loss import MeanTeacherLoss
        self.ema, self.teacher = ema, InIterationTeacher(ema)
        self.weight = weight if weight == 'ref' else float(weight)
        self.k_mode, self.epoch, self.shape = k, 0, None
        self.loss = MeanTeacherLoss(ema.coef.device)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def m(self):
        if self.weight != 'ref':
            return self.weight
        return 0.3 if self.epoch > 30 else 0.01 * self.epoch

    def k(self):
        return 400 if self.k_mode == 'all' else self.epoch

    def sync(self, shape=None):
        """Write this epoch's mask and factors to the device (outside graph capture; nothing happens while they are unchanged)."""
        if shape is not None:
            self.shape = tuple(shape)
        if self.shape is not None:
            self.loss.set(self.m(), self.k(), self.shape)

    # one of DAStep's optional terms (mi355.da_step._Term)
    key, needs_head_graph = 'mt', True

    def step_a(self, f_s, y_s):
        return {}

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        """m * mt_loss(y_t, teacher(x_t_ema)) with y_t's autograd graph; x_t_ema is x_t itself when the batch has none."""
        x_t_ema = batch['x_t_ema'] if batch.get('x_t_ema') is not None else batch['x_t']
        y_ema = self.teacher.forward(x_t_ema)
        if not torch.cuda.is_current_stream_capturing():
            self.sync(y_t_grad.shape)
        return self.loss(y_t_grad, y_ema), {'y_t_ema': y_ema}     # (kept: step M's teacher labels reuse this forward)
