"""FusedSGD: torch.optim.SGD(momentum, weight_decay, nesterov) semantics (reference train1.py:141-148) with one
HIP kernel per parameter group over flat fp32 buffers.

Drop-in for ``torch.optim.SGD`` in the reference's training script: same constructor arguments, same
``param_groups`` / ``state_dict()`` layout (``momentum_buffer`` per parameter), so LambdaLR / MultiStepLR and
the reference checkpoint keys keep working.  Parameters that have never received a gradient (e.g. the unused
``backbone.fc``) are skipped exactly as torch does.

FusedAdam: torch.optim.Adam / AdamW semantics on the same flat storage, in two launches per ``step()`` whatever the number of
parameters and groups.  Both share ``_FlatOptimizer``: the flat layout, the device-side learning rates, the fresh / stale
bookkeeping of ``zero_grad()`` and the refresh of the packed weight copies behind every step.
"""
import torch
from torch.optim import Optimizer

import mi355 as _rt
from . import ops
from .nn import mark_grads_fresh, repack_params, repack_params_fp8, repack_params_mx


class _FlatOptimizer(Optimizer):
    """What FusedSGD and FusedAdam know about flat storage.  A subclass names its per-parameter state tensors:

    ``_BUFFERS``: ((state key, key of the flat record), ...) -- one flat fp32 buffer per group beside P and G for each, the
                  state tensor of a parameter being a view of it at the parameter's offset;
    ``_COUNTER``: the state key of a per-parameter fp32 scalar -- a 0-dim view into one device array per group (record key
                  'S', one float per parameter in layout order) -- or None;

    and launches its kernels from ``_step_begin`` (once per step) or ``_step_group`` (once per flat group)."""
    _BUFFERS = ()
    _COUNTER = None

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._flat = None          # list of per-group dicts once flattened
        self._lr_cache = {}

    # ------------------------------------------------------------ flat storage
    @property
    def is_flat(self):
        return self._flat is not None

    def ensure_flat(self):
        """Move every parameter that owns a gradient into flat (param, grad, state) buffers.  Parameter
        objects keep their identity; only their storage moves.  Called on the first step()."""
        if self._flat is not None:
            return
        flat = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group['params'] if p.requires_grad and p.grad is not None]
            if not ps:
                flat.append(None)
                continue
            dev = ps[0].device
            offs, total = [], 0
            for p in ps:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4          # 16-byte aligned slots
            P = torch.zeros(total, dtype=torch.float32, device=dev)
            G = torch.zeros(total, dtype=torch.float32, device=dev)
            bufs = {fk: torch.zeros(total, dtype=torch.float32, device=dev) for _, fk in self._BUFFERS}
            S = torch.zeros(len(ps), dtype=torch.float32, device=dev) if self._COUNTER else None
            zeroed = {}              # offset -> length of the bias gradients nn._zero_grad_once holds at zero (see zero_grad)
            for i, (p, o) in enumerate(zip(ps, offs)):
                n = p.numel()
                if p.dtype != torch.float32:
                    raise TypeError('%s handles fp32 master parameters only' % type(self).__name__)
                pv = P[o:o + n].as_strided(p.shape, p.stride())
                gv = G[o:o + n].as_strided(p.shape, p.stride())
                pv.copy_(p.data)
                gv.copy_(p.grad)
                st = self.state[p]
                for sk, fk in self._BUFFERS:
                    bv = bufs[fk][o:o + n].as_strided(p.shape, p.stride())
                    if st.get(sk) is not None:
                        bv.copy_(st[sk])
                    st[sk] = bv
                if self._COUNTER:
                    self._alias_counter(st, S[i])
                p.data = pv
                p.grad = gv
                gv._mi_flat = (zeroed, o, n)
                p._mi_epoch = getattr(p, '_mi_epoch', 0) + 1     # packed copies must be rebuilt (storage moved)
            lr_dev = torch.zeros((), dtype=torch.float32, device=dev)
            f = dict(P=P, G=G, params=ps, lr_dev=lr_dev, gi=gi, zeroed=zeroed, zero_idx=(None, None),
                     offs={id(p): (o, (p.numel() + 3) // 4 * 4) for p, o in zip(ps, offs)}, **bufs)
            if S is not None:
                f['S'] = S
            flat.append(f)
        self._flat = flat
        self.sync_lr(force=True)

    def _alias_counter(self, st, sv):
        """Make the 0-dim device view `sv` the counter of the state `st`, keeping a value the state already holds."""
        old = st.get(self._COUNTER)
        if torch.is_tensor(old):
            if old.data_ptr() != sv.data_ptr():
                sv.copy_(old.detach().reshape(()))
        elif old is not None:
            sv.fill_(float(old))
        st[self._COUNTER] = sv

    def flat_range(self, params):
        """(G buffer, lo, hi) covering `params` -- which must be neighbours inside one flat group -- or None when the
        optimizer is not flat yet / the parameters own no gradient.  Used to all-reduce a finished part of the backward
        while the rest is still running."""
        if self._flat is None:
            return None
        ids = [id(p) for p in params]
        for f in self._flat:
            if f is None:
                continue
            hit = [f['offs'][i] for i in ids if i in f['offs']]
            if hit:
                lo = min(o for o, _ in hit)
                hi = max(o + n for o, n in hit)
                if sum(n for _, n in hit) != hi - lo:
                    return None                  # not contiguous: leave it to the final pass
                return f['G'], lo, hi
        return None

    def flat_grads(self):
        """The contiguous gradient buffers (one per group) — what the data-parallel all-reduce operates on."""
        _rt.join_side()
        self.ensure_flat()
        return [f['G'] for f in self._flat if f is not None]

    def sync_lr(self, force=False):
        """Push the groups' current learning rates to their device scalars (call outside graph capture)."""
        if self._flat is None:
            return
        for f in self._flat:
            if f is None:
                continue
            lr = float(self.param_groups[f['gi']]['lr'])
            if force or self._lr_cache.get(f['gi']) != lr:
                f['lr_dev'].fill_(lr)
                self._lr_cache[f['gi']] = lr

    # ------------------------------------------------------------ torch.optim API
    def zero_grad(self, set_to_none=False):
        """torch.optim.SGD.zero_grad(set_to_none=True) semantics without freeing anything: a parameter that receives no
        gradient before the next step() is skipped by it (no weight decay, no momentum update), exactly like a parameter
        whose ``grad is None``.  Gradients written by the mi355 kernels are simply overwritten by the next backward (no
        memset, the flat buffers stay in place); gradients accumulated by autograd itself (torch-native modules in the
        same optimizer) are zeroed here and recognised as untouched by their version counter.

        The bias gradients whose backward writes zeros (a conv in front of a training-mode BatchNorm: nn._zero_grad_once) are
        zeroed here, with one launch per flat group, instead of one fill per bias in the backward: clipping, a manual weight
        decay or scaled flat gradients may have written into them since, which no version counter of the flat views shows."""
        if self._flat is not None:
            for f in self._flat:
                if f is not None and f['zeroed']:
                    self._refill_zeros(f)
        for group in self.param_groups:
            ps = group['params']
            mark_grads_fresh([p for p in ps if getattr(p, '_mi_slot', False)])
            for p in ps:
                if p.grad is not None and not getattr(p, '_mi_slot', False):
                    p.grad.zero_()
                    p._mi_zero_ver = p.grad._version

    @staticmethod
    def _refill_zeros(f):
        key = tuple(sorted(f['zeroed'].items()))
        if f['zero_idx'][0] != key:
            if torch.cuda.is_current_stream_capturing():      # (no index yet: one fill per range, captured as they are)
                for o, n in key:
                    f['G'][o:o + n].zero_()
                return
            idx = torch.cat([torch.arange(o, o + n, dtype=torch.long) for o, n in key])
            f['zero_idx'] = (key, idx.to(f['G'].device))
        f['G'].index_fill_(0, f['zero_idx'][1], 0.0)

    @staticmethod
    def _stale(p):
        """True when `p` received no gradient since the last zero_grad()."""
        if getattr(p, '_mi_slot', False):
            return bool(getattr(p, '_mi_fresh', False))
        return p.grad is not None and getattr(p, '_mi_zero_ver', None) == p.grad._version

    def _late_params(self):
        """Parameters that own a gradient now but did not when the flat buffers were laid out."""
        known = {i for f in self._flat if f is not None for i in f['offs']}
        return [p for g in self.param_groups for p in g['params']
                if p.requires_grad and p.grad is not None and id(p) not in known]

    def _settle(self):
        """What step() does before it looks at the gradients: the side stream has landed, the flat layout holds every parameter
        that owns a gradient (laid out again, outside capture, when one got its first gradient late)."""
        _rt.join_side()              # weight gradients computed on the side stream must have landed
        self.ensure_flat()
        if self._late_params():      # first gradient arrived after the flat layout was fixed: lay it out again
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('%s: a parameter received its first gradient during graph capture; run one eager '
                                   'step with every parameter active before capturing' % type(self).__name__)
            self._flat = None
            self.ensure_flat()

    def _runs(self):
        """(flat group, lo, hi) for every contiguous run of parameters that received a gradient since zero_grad(): the ranges
        step() updates -- and the ranges a gradient norm over "what this step touches" is taken over (GradClipper)."""
        for f in self._flat:
            if f is None:
                continue
            stale = [self._stale(p) for p in f['params']]
            if not any(stale):
                yield f, 0, f['P'].numel()
                continue
            lo = None                # step the contiguous runs of parameters that did receive a gradient
            for p, st in zip(f['params'], stale):
                o, n = f['offs'][id(p)]
                if st:
                    if lo is not None:
                        yield f, lo, o
                        lo = None
                elif lo is None:
                    lo = o
            if lo is not None:
                yield f, lo, f['P'].numel()

    def _step_begin(self, runs, clip):
        """Launches of one step that span the flat groups.  runs: {id(flat record): [(lo, hi), ...]}."""

    def _step_group(self, f, group, runs, clip):
        """Launches of one step for the flat record `f` of `group`; runs: its [(lo, hi), ...]."""

    @torch.no_grad()
    def step(self, closure=None, clip=None):
        """`clip`: a mi355_clip_rec on the device (GradClipper.measure): every run is stepped on fl32(g * coef), or not at all when
        the record says skip.  The gradient buffers are only read, so ``p.grad`` keeps the unclipped values and the zeros
        nn._zero_grad_once holds in them stay zeros.  A skipped step is a skipped GradScaler step: everything below the kernel
        launches (packed copies, fp8 scales) proceeds as usual."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._settle()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        runs = {}
        for f, lo, hi in self._runs():
            runs.setdefault(id(f), []).append((lo, hi))
        self._step_begin(runs, clip)
        for f in self._flat:
            if f is None:
                continue
            self._step_group(f, self.param_groups[f['gi']], runs.get(id(f), ()), clip)
            for p in f['params']:
                if not self._stale(p):
                    p._mi_epoch = getattr(p, '_mi_epoch', 0) + 1
            repack_params(f['params'], f.setdefault('pack_cache', {}))     # packed conv copies: one launch per group
            repack_params_fp8(f['params'], f['pack_cache'])
            repack_params_mx(f['params'], f['pack_cache'])        # ('mxfp8' mode: the MX packs, so replayed graphs read fresh ones)
        if _rt.fp8_convs():
            _rt.fp8_tick()           # delayed scaling: the fp8 scales of the next pass from the amax values of this one
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._flat is None:
            return
        for f in self._flat:          # re-alias loaded state tensors onto the flat storage
            if f is None:
                continue
            for i, p in enumerate(f['params']):
                o, n = f['offs'][id(p)][0], p.numel()
                st = self.state[p]
                for sk, fk in self._BUFFERS:
                    bv = f[fk][o:o + n].as_strided(p.shape, p.stride())
                    buf = st.get(sk)
                    if buf is None:
                        bv.zero_()
                    elif buf.data_ptr() != bv.data_ptr():
                        bv.copy_(buf)
                    st[sk] = bv
                if self._COUNTER:
                    if st.get(self._COUNTER) is None:
                        f['S'][i].zero_()
                    self._alias_counter(st, f['S'][i])
        self.sync_lr(force=True)


class FusedSGD(_FlatOptimizer):
    _BUFFERS = (('momentum_buffer', 'M'),)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0, weight_decay=0.0, nesterov=False):
        if dampening != 0:
            raise NotImplementedError('dampening is not used by the reference and not built')
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)

    def _step_group(self, f, g, runs, clip):
        for lo, hi in runs:
            if clip is None:
                ops.sgd_nesterov(f['P'][lo:hi], f['G'][lo:hi], f['M'][lo:hi], f['lr_dev'], g['momentum'], g['weight_decay'],
                                 g['nesterov'])
            else:
                ops.sgd_nesterov_clipped(f['P'][lo:hi], f['G'][lo:hi], f['M'][lo:hi], f['lr_dev'], clip, g['momentum'],
                                         g['weight_decay'], g['nesterov'])


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam (``decoupled=False``: L2 weight decay) / torch.optim.AdamW (``decoupled=True``) on flat fp32 buffers:
    ``mi355_adam_step_batched`` over one table of every parameter that received a gradient since ``zero_grad()``, of every group,
    then ``mi355_adam_tick_batched`` for their step counts -- two launches per ``step()``.  Same defaults, ``param_groups`` keys and
    ``state_dict()`` layout as torch (``exp_avg``, ``exp_avg_sq`` and ``step``, an fp32 scalar, per parameter), so schedulers and
    checkpoints move between the two.  The learning rates are read from the groups' device scalars and the step counts live on
    the device (0-dim views into one array per flat group), so ``step()`` captures into a HIP graph and a replay sees the
    schedule; betas, eps and weight decay are constants of the table, rebuilt -- outside capture only -- when they or the set of
    fresh parameters change.  A parameter without a fresh gradient is not stepped and its count does not advance (torch:
    ``grad is None``).  That holds for the parameters of mi355.nn modules, which mark their gradients themselves.  Caveat for
    parameters of torch-native modules (``nn.Linear``, ``nn.Conv2d``): their flat gradient views share one version counter per group, so
    such a parameter counts as untouched since ``zero_grad()`` only if nothing else of its group was written since -- otherwise it is
    stepped on its zeroed gradient (moments decay, ``step`` advances), unlike torch.  Give a torch-native parameter that may sit out
    steps a param group of its own.  ``weight_decay=None`` is the default of the torch class it stands for: 0 (Adam), 1e-2 (``decoupled=True``,
    AdamW).  Arithmetic and its differences from torch: include/mi355pose.h."""
    _BUFFERS = (('exp_avg', 'M'), ('exp_avg_sq', 'V'))
    _COUNTER = 'step'
    _TORCH_ONLY = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, decoupled=False, **torch_only):
        for k, v in torch_only.items():
            if k not in self._TORCH_ONLY:
                raise TypeError('FusedAdam got an unexpected keyword argument %r' % k)
            if v is not self._TORCH_ONLY[k] and v != self._TORCH_ONLY[k]:
                raise NotImplementedError('FusedAdam: %s=%r is not built (only torch\'s default, %r)' % (k, v, self._TORCH_ONLY[k]))
        if weight_decay is None:
            weight_decay = 1e-2 if decoupled else 0.0       # torch.optim.AdamW's / torch.optim.Adam's default
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **self._TORCH_ONLY,
                        decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)
        self._tables = {}            # sig -> dict(sig, table, count, blocks): the few sets of fresh parameters a loop alternates between
        self._retired = []           # tables no step() will use again, kept alive for the graphs that captured them (88 bytes an item)
        self._table = None           # the one the last step() used

    def ensure_flat(self):
        if self._flat is None:
            self._retired.extend(self._tables.values())
            self._tables, self._table = {}, None         # (the tables hold addresses of the layout that is about to be replaced)
        super().ensure_flat()

    def _step_begin(self, runs, clip):
        picked, sig = [], []         # (flat record, index in it, offset, length, hyper-parameters) of every parameter to step
        for f in self._flat:
            if f is None or id(f) not in runs:
                continue
            g = self.param_groups[f['gi']]
            for k, v in self._TORCH_ONLY.items():
                if g.get(k, v) is not v and g.get(k, v) != v:
                    raise NotImplementedError('FusedAdam: %s=%r is not built' % (k, g[k]))
            hyper = (float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                     bool(g.get('decoupled_weight_decay', False)))
            for i, p in enumerate(f['params']):
                o, n = f['offs'][id(p)][0], p.numel()
                if any(lo <= o < hi for lo, hi in runs[id(f)]):
                    picked.append((f, i, o, n, hyper))
                    sig.append((f['P'].data_ptr(), o, n) + hyper)
        sig = tuple(sig)
        t = self._tables.get(sig)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FusedAdam: the set of parameters to step (or a hyper-parameter of their groups) changed during '
                                   'graph capture; run one eager step with the same parameters active before capturing')
            if len(self._tables) >= 8:           # (a loop alternates between a few sets; anything more is churn: start over --
                self._retired.extend(self._tables.values())      # but a captured graph may still read a table: none is freed)
                self._tables.clear()
            t = self._tables[sig] = dict(sig=sig)
            if picked:
                items = [(f['P'][o:o + n], f['G'][o:o + n], f['M'][o:o + n], f['V'][o:o + n], f['S'][i], f['lr_dev']) + hyper
                         for f, i, o, n, hyper in picked]
                t['table'], t['count'], t['blocks'] = ops.adam_table(items, items[0][0].device)
        self._table = t
        if picked:                   # (no fresh gradient at all: nothing to step)
            ops.adam_step_batched(t['table'], t['count'], t['blocks'], clip)
            ops.adam_tick_batched(t['table'], t['count'], clip)

    def state_dict(self):
        """torch.optim.Adam's layout: ``step`` leaves as an fp32 scalar on the host, as torch keeps it, and never as a view of the
        device array the kernels count in."""
        sd = super().state_dict()
        sd['state'] = {k: ({**st, 'step': st['step'].detach().to('cpu', copy=True)} if torch.is_tensor(st.get('step')) else st)
                       for k, st in sd['state'].items()}
        return sd


OPTIMIZERS = ('sgd', 'adam', 'adamw')


def make_optimizer(kind, params, lr, momentum=0.9, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """The training scripts' optimizer of `kind`: 'sgd' = FusedSGD with Nesterov momentum (the reference, train1.py:141-148),
    'adam' = FusedAdam with L2 weight decay, 'adamw' = FusedAdam with decoupled weight decay (`momentum` unused by both)."""
    if kind == 'sgd':
        return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True)
    if kind in ('adam', 'adamw'):
        return FusedAdam(params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled=kind == 'adamw')
    raise ValueError('optimizer must be one of %s, got %r' % (', '.join(OPTIMIZERS), kind))


def state_dict_kind(state_dict):
    """'sgd' or 'adam' -- the family of optimizer that wrote `state_dict` (AdamW is Adam with another group flag) --, told from
    the keys of its param_groups; None when neither."""
    groups = state_dict.get('param_groups') or [{}]
    if 'betas' in groups[0]:
        return 'adam'
    if 'momentum' in groups[0]:
        return 'sgd'
    return None


def check_state_dict_kind(optimizer, state_dict, what='optimizer state'):
    """Raise a ValueError that names both kinds when `state_dict` was written by the other family of optimizer than `optimizer`
    (loading it would end in a KeyError deep inside step())."""
    want = 'adam' if isinstance(optimizer, FusedAdam) else 'sgd'
    got = state_dict_kind(state_dict)
    if got is not None and got != want:
        names = {'sgd': 'SGD (--optimizer sgd)', 'adam': 'Adam / AdamW (--optimizer adam | adamw)'}
        raise ValueError('%s was written by %s but this run builds %s; resume with the optimizer the checkpoint was trained with'
                         % (what, names[got], names[want]))


class GradClipper:
    """Global gradient-norm clipping with a non-finite step guard for FusedSGD / FusedAdam optimizers, entirely on the device:
    ``torch.nn.utils.clip_grad_norm_(parameters stepped in this update, max_norm)`` in front of the optimizers' ``step()``, in two
    launches (``mi355_grad_sumsq_batched`` over every fresh run of every optimizer, ``mi355_grad_clip_coef``) that fill one
    ``mi355_clip_rec``; ``step(clip=record)`` applies the coefficient inside the SGD / Adam kernel.  Nothing is read by the
    host, so the launches sit in captured graphs beside the optimizer's.

    Differences from torch's in-place clip: the gradient buffers are never written -- ``p.grad`` keeps the unclipped values
    after the step, and the zeros ``nn._zero_grad_once`` holds in the flat buffers cannot go stale; parameters that received no
    gradient since ``zero_grad()`` are outside the norm (torch: ``grad is None``).  A non-finite sum of squares skips the update
    (parameters, momentum and low-precision copies keep their values; ``n_skipped`` counts it) while everything else of the
    iteration proceeds, like a skipped ``GradScaler`` step.  ``max_norm = inf`` measures and guards and never scales.

    One record per slot ('a', 'b', 'c': the three updates of a DAStep iteration) in one small device buffer; ``max_norm`` is a
    field of the records, written by ``sync()`` outside capture, so it may change between replays.  With several ranks call
    ``measure`` behind the gradient all-reduce: every rank then derives the same coefficient from the same bytes."""
    SLOTS = ('a', 'b', 'c')

    def ensure_slot(self, slot):
        """One more record behind the existing ones (update M of a DAStep with mixup: 'm'), outside graph capture; the records of
        the existing slots keep their values.  Nothing happens when the slot exists."""
        if slot in self.SLOTS:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('GradClipper: slot %r would be added during graph capture; run one eager iteration first' % (slot,))
        more = ops.clip_records(1, self._synced, self.device)
        self.recs = torch.cat([self.recs, more])
        self._f32 = self.recs.view(torch.float32)
        self.SLOTS = tuple(self.SLOTS) + (slot,)     # (an instance attribute from here on)

    def __init__(self, max_norm, device):
        max_norm = float(max_norm)
        if not max_norm > 0:                       # (NaN fails the comparison too)
            raise ValueError('GradClipper: max_norm must be positive (inf: measure and guard only), got %r' % (max_norm,))
        self.max_norm, self.device = max_norm, torch.device(device)
        self.recs = ops.clip_records(len(self.SLOTS), max_norm, self.device)
        self._f32 = self.recs.view(torch.float32)          # 8 floats per record; max_norm is float 2
        self._synced = max_norm
        self._tables = {}                          # slot -> dict(sig, table, count, blocks, partials)

    def record(self, slot):
        """The mi355_clip_rec of `slot` as a uint8 view of the device buffer."""
        i = self.SLOTS.index(slot)
        return self.recs[i * ops.CLIP_REC_BYTES:(i + 1) * ops.CLIP_REC_BYTES]

    def sync(self):
        """Write max_norm into the records when it changed (call outside graph capture)."""
        if self.max_norm != self._synced:
            m = float(self.max_norm)
            if not m > 0:
                raise ValueError('GradClipper: max_norm must be positive, got %r' % (m,))
            self._f32[2::8].fill_(m)
            self._synced = m

    @torch.no_grad()
    def measure(self, optimizers, slot):
        """Enqueue the norm of everything `optimizers` (FusedSGD / FusedAdam) are about to step into the record of `slot` and return that
        record, for ``step(clip=...)``.  The range table is keyed by the runs' (buffer address, lo, hi) and rebuilt -- outside
        capture only -- when that changes."""
        optimizers = list(optimizers)
        for o in optimizers:
            if not isinstance(o, (FusedSGD, FusedAdam)):
                raise TypeError('GradClipper handles FusedSGD and FusedAdam optimizers only, got %s' % type(o).__name__)
        rec = self.record(slot)
        for o in optimizers:
            o._settle()
        runs = [(f['G'], lo, hi) for o in optimizers for f, lo, hi in o._runs()]
        sig = tuple((G.data_ptr(), lo, hi) for G, lo, hi in runs)
        t = self._tables.get(slot)
        if t is None or t['sig'] != sig:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('GradClipper: the set of gradient ranges of update %r changed during graph capture; run one eager '
                                   'iteration with the clipper attached before capturing' % (slot,))
            t = dict(sig=sig)
            if runs:
                t['table'], t['count'], t['blocks'] = ops.gn_table([G[lo:hi] for G, lo, hi in runs], self.device)
                t['partials'] = torch.zeros(t['blocks'], dtype=torch.float64, device=self.device)
            self._tables[slot] = t
        if runs:                                   # (no fresh gradient at all: no optimizer launch will read the record)
            ops.grad_sumsq_batched(t['table'], t['count'], t['blocks'], t['partials'])
            ops.grad_clip_coef(t['partials'], t['blocks'], rec)
        return rec

    def read(self):
        """({slot: (norm, coef, skip)}, n_skipped over all slots): the one device read, for a progress line."""
        r = self.recs.cpu().numpy().view(ops.clip_rec_dtype())
        return ({s: (float(r['norm'][i]), float(r['coef'][i]), int(r['skip'][i])) for i, s in enumerate(self.SLOTS)},
                int(r['n_skipped'].sum()))


class EMATeacher:
    """The reference's "mean teacher" (uda/model/loss.py:252-261, the call at train1.py:461): after every training iteration

        v_ema = v_ema * m + (1. - m) * v_main     for every floating-point tensor of the two ``state_dict()``s
        v_ema = v_main                            for ``num_batches_tracked``

    in at most one launch per flat FusedSGD group plus one batched launch for everything else.  Once the optimizers are
    flat the teacher's parameters move onto flat fp32 buffers that mirror each group's parameter buffer (same offsets, same
    16-byte slots; parameter objects keep their identity), so ``mi355_ema_update`` streams group against mirror.  BatchNorm
    running statistics, parameters no optimizer laid out (the unused ``backbone.fc``) and the ``num_batches_tracked`` counters
    go through one ``mi355_ema_update_batched`` launch.  The coefficients are read from a two-float device buffer
    (``sync()``, outside capture), so ``update()`` can be captured into a HIP graph; ``mark_updated()`` is the host half of an
    update (step count, cache invalidation) for the caller that replays such a graph.

    ``warmup=True`` is ``update_ema_variables2``: m = min(1 - 1/(step + 1), decay), step counted from 0."""

    def __init__(self, model, model_ema, optimizers, decay, warmup=False):
        self.model, self.model_ema = model, model_ema
        self.optimizers = list(optimizers.values()) if isinstance(optimizers, dict) else list(optimizers)
        self.decay, self.warmup, self.step = float(decay), bool(warmup), 0
        objs = lambda m: dict(list(m.named_parameters(remove_duplicate=False)) + list(m.named_buffers(remove_duplicate=False)))
        main, ema = objs(model), objs(model_ema)
        self.pairs = []                      # (key, main tensor object, teacher tensor object, is num_batches_tracked)
        for (k_main, v_main), (k_ema, v_ema) in zip(model.state_dict().items(), model_ema.state_dict().items()):
            assert k_main == k_ema, "state_dict names are different!"
            assert v_main.shape == v_ema.shape, "state_dict shapes are different!"
            counter = 'num_batches_tracked' in k_ema
            if not counter and v_ema.dtype != torch.float32:
                raise TypeError('EMATeacher: %s is %s, only fp32 tensors and num_batches_tracked are handled' % (k_ema, v_ema.dtype))
            self.pairs.append((k_ema, main[k_main], ema[k_ema], counter))
        assert len(self.pairs) == len(model.state_dict()) == len(model_ema.state_dict()), "state_dict lengths are different!"
        self._ema_of = {id(a): b for _, a, b, _ in self.pairs}
        self._params_ema = [b for _, _, b, _ in self.pairs if isinstance(b, torch.nn.Parameter)]
        dev = self.pairs[0][2].device
        self.coef = torch.zeros(2, dtype=torch.float32, device=dev)
        self._coef_m = None
        self._layout_sig, self._flat, self._owned, self._table, self._table_sig = None, [], set(), None, None

    # ------------------------------------------------------------ coefficients
    def momentum(self):
        return min(1 - 1 / (self.step + 1), self.decay) if self.warmup else self.decay

    def sync(self):
        """Write (float32(m), float32(1.0 - m)) of the coming update to the device pair (call outside graph capture)."""
        m = self.momentum()
        if m != self._coef_m:
            self.coef[0].fill_(m)
            self.coef[1].fill_(1.0 - m)
            self._coef_m = m

    # ------------------------------------------------------------ storage
    def _groups(self):
        return [f for o in self.optimizers if getattr(o, '_flat', None) is not None for f in o._flat if f is not None]

    def _ensure_layout(self):
        """Mirror the optimizers' flat parameter buffers (again after FusedSGD laid its own out again) and rebuild the
        record table of everything else when any of those tensors moved."""
        groups = self._groups()
        sig = tuple((f['P'].data_ptr(), f['P'].numel()) for f in groups)
        capturing = torch.cuda.is_current_stream_capturing()
        if sig != self._layout_sig:
            if capturing:
                raise RuntimeError('EMATeacher: the optimizers changed their flat layout during graph capture; run one eager '
                                   'iteration with the teacher attached before capturing')
            flat, owned = [], set()
            with torch.no_grad():
                for f in groups:
                    E = torch.zeros_like(f['P'])
                    for p in f['params']:
                        pe = self._ema_of.get(id(p))
                        if pe is None:
                            raise RuntimeError('EMATeacher: an optimizer parameter is not part of model.state_dict()')
                        o, n = f['offs'][id(p)][0], p.numel()
                        ev = E[o:o + n].as_strided(p.shape, p.stride())
                        ev.copy_(pe.data)
                        pe.data = ev
                        pe._mi_epoch = getattr(pe, '_mi_epoch', 0) + 1        # packed copies must be rebuilt (storage moved)
                        owned.add(id(pe))
                    flat.append((E, f['P']))
            self._flat, self._owned, self._layout_sig, self._table_sig = flat, owned, sig, None
        rest = [(a, b, c) for _, a, b, c in self.pairs if id(b) not in self._owned]
        tsig = tuple((a.data_ptr(), b.data_ptr()) for a, b, _ in rest)
        if tsig != self._table_sig:
            if capturing:
                raise RuntimeError('EMATeacher: a tensor outside flat storage moved during graph capture')
            self._table = ops.ema_table([(a.detach(), b.detach(), ops.EMA_COPY64 if c else ops.EMA_F32) for a, b, c in rest],
                                        self.coef.device) if rest else None
            self._table_sig = tsig

    # ------------------------------------------------------------ the update
    @torch.no_grad()
    def update(self):
        """Enqueue the update on the current stream (safe during graph capture once one eager update has run).  Outside
        capture this also does the host half, mark_updated()."""
        self._ensure_layout()
        for E, P in self._flat:
            ops.ema_update(E, P, self.coef)
        if self._table is not None:
            ops.ema_update_batched(*self._table, self.coef)
        if not torch.cuda.is_current_stream_capturing():
            self.mark_updated()

    def mark_updated(self):
        """Host half of one update: count it, and make the teacher's packed weights, folded BatchNorms and captured eval graphs
        stale -- the kernels wrote behind autograd's back (as FusedSGD.step and the training BatchNorm forward do)."""
        from . import nn as _nn
        self.step += 1
        for p in self._params_ema:
            p._mi_epoch = getattr(p, '_mi_epoch', 0) + 1
        _nn._BN_GEN[0] += 1

    # ------------------------------------------------------------ state
    def state_dict(self):
        return {'step': self.step, 'decay': self.decay, 'warmup': self.warmup}

    def load_state_dict(self, state):
        self.step = int(state['step'])
