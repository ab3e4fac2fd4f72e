"""One domain-adaptation training iteration = steps A, B, C of the reference's ``train()``
(train1.py:371-458), over the MI355X kernels, optionally replayed from captured HIP graphs.

Differences from the reference loop that do not change any result (documented in DESIGN.md):
  * step B stops its backward at the neck output: the backbone/neck gradients it would produce are
    zeroed by ``optimizer_f.zero_grad()`` at the start of step C before anyone reads them (train1.py:440);
  * step C does not compute weight gradients of the adversarial heads: they are zeroed at the start of the
    next step A (train1.py:372-376) before any optimizer reads them;
  * steps B and C run the backbone, the neck and the main head ONCE on the target batch: step B only updates the
    adversarial heads (train1.py:434-436), so the second forward of the reference (train1.py:441) recomputes bit-identical
    features f_t and y_t; step C re-uses them (with their autograd graph) and the BatchNorm layers of that shared part
    apply their running-stat update twice (mi355_bn_train_fwd stat_updates=2), as two forwards would;
  * pseudo-labels, arg-max, KL and PCK stay on the device (the reference round-trips through numpy 12x / iteration).
Data parallelism: one process per GPU; the flat gradient buffers of the optimizers about to step are
all-reduced (mean) over the default process group between the backward and the optimizer kernels.
"""
import os

import torch
import torch.distributed as dist

import mi355 as _rt
from . import ops
from .nn import mark_grads_fresh


# MI355_GRAD_BUCKET_BF16=1 (opt-in): the fp32 gradient ranges travel as bf16 copies -- half the bytes on every xGMI link, one
# cast each way (read 4 + write 2 bytes per element) -- and are averaged in bf16.  Default: fp32, as the reference would.
BF16_BUCKETS = os.environ.get('MI355_GRAD_BUCKET_BF16', '0') == '1'


def _reduce_mean_(t, async_op=False):
    """In-place mean of tensor t over the ranks; returns (work or None, finish) -- finish() after the wait completes the job."""
    avg = dist.get_backend() == 'nccl'
    ws = dist.get_world_size()
    if BF16_BUCKETS and t.dtype == torch.float32:
        low = t.to(torch.bfloat16)
        w = dist.all_reduce(low, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, async_op=async_op)

        def finish():
            t.copy_(low)
            if not avg:
                t.div_(ws)
        return w, finish
    w = dist.all_reduce(t, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, async_op=async_op)
    return w, ((lambda: None) if avg else (lambda: t.div_(ws)))


# MI355_DDP_FORCE_COLLECTIVES=1: issue every collective of the multi-rank path even in a one-rank group -- the only way to run
# the RCCL calls (init, AVG all-reduce of flat gradient ranges, async work handles, broadcast of the conv-form views) on a
# one-GPU box (tests/test_gpu_ddp.py::test_rccl_single_rank_smoke); a mean over one rank is the identity.
_FORCE_COLLECTIVES = os.environ.get('MI355_DDP_FORCE_COLLECTIVES', '0') == '1'


def _distributed():
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _FORCE_COLLECTIVES)


def _allreduce_mean(bufs):
    if not _distributed():
        return
    for b in bufs:
        _, finish = _reduce_mean_(b)
        finish()


class _OverlapReducer:
    """Gradient mean of one backward pass, started piecewise while the pass is still running.

    Tensor hooks on the outputs of the neck and of the ResNet stages tell when everything *behind* that tensor has finished
    its backward: the flat gradient range of those parameters is then all-reduced asynchronously (the collective's
    stream waits for the kernels enqueued so far and runs beside the rest of the backward).  ``finish()`` reduces whatever
    no hook covered (always the stem / layer1 range, everything in the very first iteration when the optimizers are not
    flat yet) and waits for all collectives.  The result equals one all-reduce per buffer; only the timing differs."""

    def __init__(self, step, keys):
        self.step, self.keys = step, tuple(keys)
        self.works, self.covered = [], {}
        self.avg = dist.get_backend() == 'nccl'

    def _launch(self, G, lo, hi):
        t = G[lo:hi]
        w, finish = _reduce_mean_(t, async_op=True)
        self.works.append((w, finish))
        self.covered.setdefault(G.data_ptr(), []).append((lo, hi))

    def stage_done(self, stage):
        """Called from a gradient hook: the parameters of `stage` (a key of DAStep._stage_params) have their gradients."""
        for key, params in self.step._stage_params.get(stage, ()):
            if key not in self.keys:
                continue
            opt = self.step.opt[key]
            rng = opt.flat_range(params) if hasattr(opt, 'flat_range') else None
            if rng is not None:
                self._launch(*rng)

    def finish(self):
        for G in self.step._grads(self.keys):
            done = sorted(self.covered.get(G.data_ptr(), []))
            pos = 0
            for lo, hi in done + [(G.numel(), G.numel())]:
                if lo > pos:
                    self._launch(G, pos, lo)
                pos = max(pos, hi)
        for w, done in self.works:
            w.wait()
            done()
        self.works = []


def broadcast_module(module, src=0):
    """Rank `src`'s parameters and buffers to every rank.  Conv weights are strided (conv-form) views: the collective
    runs on their dense memory-order view."""
    if not _distributed():
        return
    for t in list(module.parameters()) + list(module.buffers()):
        d = t.data
        if d.dim() == 4 and not d.is_contiguous():
            d = d.permute(0, 2, 3, 1)
        if not d.is_contiguous():
            raise RuntimeError('cannot broadcast a non-dense tensor of shape %s' % (tuple(t.shape),))
        dist.broadcast(d, src)


class _Term:
    """An optional term of step C's loss, as ``DAStep`` sees it (``mi355.teacher.MeanTeacher`` is the fourth).  ``key`` names it:
    the attribute of the step that holds it, ``out['loss_<key>']`` and the meter column.  ``needs_head_graph``: step C
    differentiates the term through the main head, so step B must keep that head's autograd graph."""
    key, needs_head_graph = None, False

    def step_a(self, f_s, y_s):
        """Step A, behind the source forward: what must outlive the step, as entries of ``step.out``."""
        return {}

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        """Step C: (the term, further entries of ``step.out``).  ``y_t`` is detached; ``y_t_grad`` carries the head's graph when
        some term asked for it."""
        raise NotImplementedError


class MMDAlign(_Term):
    """What ``DAStep(mmd=...)`` takes: step C's loss gains ``weight * MMD_loss3(y_s.detach(), y_t)`` (reference
    uda/model/loss.py:1061-1104), the per-joint multi-kernel MMD between the source heat-maps of step A and the target heat-maps
    of the main head.  The weight rides inside the kernels (``scale=``); only the target side gets a gradient."""
    key, needs_head_graph = 'mmd', True

    def __init__(self, weight=0.1, kernel_mul=2.0, kernel_num=5):
        from uda.model.loss import MMD_loss3, check_positive, check_whole
        check_positive('MMDAlign: the weight', weight)
        check_positive('MMDAlign: kernel_mul', kernel_mul)
        check_whole('MMDAlign: kernel_num', kernel_num, 8)
        self.weight = float(weight)
        self.crit = MMD_loss3(kernel_mul=kernel_mul, kernel_num=kernel_num)

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        # y_s lives in step.out since step A (under capture: produced in the first graph, its storage held by that reference)
        return self.crit(step.out['y_s'].detach(), y_t_grad, scale=self.weight), {}


class JointFeatureAlign(_Term):
    """What ``DAStep(jfa=...)`` takes: step C's loss gains ``weight * loss3(f_t, <desc_s>, xy_t, .)`` (reference
    uda/model/loss.py:331-378), the KL divergence between the channel distributions of the neck output pooled around the
    predicted key points of the target batch and of the source batch.  Step A keeps only the source descriptors (B, K, C) fp32
    (the source feature map goes with its backward); the key points are the device arg-max of the detached heat-maps; only the
    target features get a gradient, through their GradFanIn beside the heads' input gradients.  The weight rides inside the
    kernels (``scale=``)."""
    key = 'jfa'

    def __init__(self, weight=1.0, radius=6, axes='xy'):
        from uda.model.loss import check_axes, check_positive, check_whole
        check_positive('JointFeatureAlign: the weight', weight)
        check_whole('JointFeatureAlign: the radius', radius, 16)
        check_axes('JointFeatureAlign: axes', axes)
        self.weight, self.radius, self.axes = float(weight), int(radius), axes

    def step_a(self, f_s, y_s):
        from uda.model.regda_4 import cached_centres
        return {'jfa_desc_s': ops.joint_pool(f_s.detach(), cached_centres(y_s), self.radius, self.axes)}

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        from uda.model.loss import loss1, joint_kl_loss
        from uda.model.regda_4 import cached_centres
        desc_t = loss1(f_t, cached_centres(y_t), self.radius, self.axes)
        return joint_kl_loss(desc_t, step.out['jfa_desc_s'], self.weight), {'jfa_desc_t': desc_t.detach()}


class PrototypeAlign(_Term):
    """What ``DAStep(proto=...)`` takes: step C's loss gains ``weight * lossx`` (``criterion='kl'``, reference
    uda/model/loss.py:381-466) or ``weight * lossx3`` (``'softkl'``, :560-652) between the per-joint class prototypes of the target
    and of the source batch: the neck output pooled around the predicted key points (each window divided by its own s1 * s2),
    averaged over the batch and blended with a running memory per domain, ``P = m * mean + (1 - m) * memory``, ``memory <- P``.
    Step A updates the source memory, once per iteration, and keeps the source prototypes (K, C); step C updates the target
    memory.  The key points are the device arg-max of the detached heat-maps; only the target features get a gradient, as the JFA
    term's.  The weight rides inside the kernels; m sits in device memory (``set_m``), and the memories live at fixed addresses, so
    captured graphs carry the state from replay to replay (``uda.model.loss.PrototypeState``).  With several ranks each rank keeps
    its own memories, as BatchNorm statistics are per GPU here."""
    key = 'proto'

    def __init__(self, weight=1.0, radius=6, axes='xy', m=0.999, criterion='kl'):
        from uda.model.loss import PrototypeState, check_positive
        check_positive('PrototypeAlign: the weight', weight)
        if criterion not in ops.PROTO_MODES:
            raise ValueError("PrototypeAlign: the criterion must be 'kl' or 'softkl', got %r" % (criterion,))
        self.weight, self.criterion = float(weight), criterion
        self.state = PrototypeState('PrototypeAlign', radius, axes, m, max_radius=16)
        self.mem_s, self.mem_t = self.state.mems
        self.set_m, self.reset = self.state.set_m, self.state.reset

    m = property(lambda self: self.state.m)

    def _proto(self, side, f, y):
        from uda.model.regda_4 import cached_centres
        return self.state.prototype(side, f, cached_centres(y))

    def step_a(self, f_s, y_s):
        return {'proto_s': self._proto(0, f_s.detach(), y_s)}

    def term(self, f_t, proto_s, y_t):
        """(the term, the target prototypes it was computed from); the target memory is updated.  A method of its own with
        plain operands: tests/test_gpu_proto.py wraps it to record what step C hands the term."""
        from uda.model.loss import prototype_kl_loss
        proto_t = self._proto(1, f_t, y_t)
        return prototype_kl_loss(proto_t, proto_s, self.criterion, self.weight), proto_t.detach()

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        loss, proto_t = self.term(f_t, step.out['proto_s'], y_t)
        return loss, {'proto_t': proto_t}

    def state_dict(self):
        """Both memories (CPU copies; None before first use) and m: what the epoch checkpoint keeps as ``proto_state``."""
        cpu = lambda mem: mem.val.detach().cpu().clone() if torch.is_tensor(mem.val) else None
        return {'memory_s': cpu(self.mem_s), 'memory_t': cpu(self.mem_t), 'm': self.m}

    def load_state_dict(self, state, device=None):
        for mem, key in ((self.mem_s, 'memory_s'), (self.mem_t, 'memory_t')):
            v = state.get(key)
            if v is None:
                mem.reset()
            else:
                mem.set(v.to(device) if (device is not None and not torch.is_tensor(mem.val)) else v)
        self.set_m(state.get('m', self.m))


class CoordRegression(_Term):
    """What ``DAStep(coord=...)`` takes: the integral-regression loss (``uda.model.loss.JointsCoordLoss``; Sun et al., ECCV 2018 --
    not in the reference) beside the heat-map losses.  Step A's loss gains ``weight * JointsCoordLoss(y_s, batch['kp_s'], w_s)``:
    the soft-arg-max of ``softmax(beta * y_s)`` against the un-quantised annotation in heat-map pixels, smooth-L1 with threshold
    ``delta``; it trains the backbone, the neck and the main head through update A.  ``target='teacher'`` also gives step C
    ``target_weight * JointsCoordLoss(y_t, soft_argmax(teacher(x_t_ema)), w_t)``, a coordinate-space consistency term against the
    EMA teacher, through the main head's graph.  The teacher's forward is the ``MeanTeacher``'s when the step has one (one forward
    per iteration), else that of an in-iteration teacher of this object's own, which step M's teacher labels reuse in turn.  Both
    weights ride inside the kernel (``scale=``)."""
    key, needs_head_graph = 'coordt', True

    def __init__(self, weight=1.0, beta=1.0, delta=1.0, target='off', target_weight=1.0, ema=None):
        from uda.model.loss import JointsCoordLoss, check_positive
        check_positive('CoordRegression: the weight', weight)
        check_positive('CoordRegression: the target weight', target_weight)
        if target not in ('off', 'teacher'):
            raise ValueError("CoordRegression: target must be 'off' or 'teacher', got %r" % (target,))
        if target == 'teacher' and ema is None:
            raise ValueError("CoordRegression: target='teacher' needs an EMATeacher (--ema-update const|warmup)")
        self.weight, self.target, self.target_weight, self.ema = float(weight), target, float(target_weight), ema
        self.crit = JointsCoordLoss(beta=beta, delta=delta)           # (checks beta and delta)
        self.crit_t = JointsCoordLoss(beta=beta, delta=delta)
        self.beta = self.crit.beta
        self._teacher = None

    def source(self, y_s, batch):
        """Step A's term; a batch without the continuous key points is an error, not a term left out."""
        if batch.get('kp_s') is None:
            raise KeyError("CoordRegression: the batch has no 'kp_s' (the continuous source key points, (B, K, 2) in heat-map pixels)")
        return self.crit(y_s, batch['kp_s'], batch['w_s'], scale=self.weight)

    def teacher(self, step):
        """The in-iteration teacher whose folded operands follow the EMA update: the MeanTeacher's when the step has one."""
        if step.mt is not None:
            return step.mt.teacher
        if self._teacher is None:
            from .teacher import InIterationTeacher
            self._teacher = InIterationTeacher(self.ema)
        return self._teacher

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        from uda.model.loss import soft_argmax
        more = {}
        y_ema = step._kept_c.get('y_t_ema') if step.mt is not None else None      # the MeanTeacher's forward of this very step C
        if y_ema is None:
            y_ema = step.teacher_forward(self.teacher(step), batch)
            more['y_t_ema'] = y_ema                                               # (kept: step M's teacher labels reuse it)
        kp_ema = soft_argmax(y_ema, self.beta)
        more['kp_t_ema'] = kp_ema
        w_t = step.teacher_weights(batch)                                         # (a geometric view: w_t * valid)
        return self.crit_t(y_t_grad, kp_ema, w_t, scale=self.target_weight), more


class KinematicPrior(_Term):
    """What ``DAStep(bone=...)`` takes: a bone-ratio skeleton prior on the target prediction (``uda.model.loss.BonePriorLoss``; in the
    family of the bone-length-ratio constraint of Zhou et al., ICCV 2017 -- not in the reference).  Step A blends the bone-length
    ratios of the source annotations (``batch['kp_s']``, ``batch['w_s']``) into running statistics (``uda.model.loss.BoneStatistics``,
    one launch; labels, not a network: they cannot drift with the student).  Step C's loss gains ``weight * BonePriorLoss(y_t,
    batch['w_t'], stats)``: the same ratios of the soft-arg-max of ``softmax(beta * y_t)``, standardised by those statistics,
    penalised beyond ``margin`` standard deviations, through the main head's graph.  No teacher, no further forward.  The weight
    rides inside the kernel (``scale=``); the statistics live at fixed addresses, so captured graphs carry them from replay to
    replay.  With several ranks each rank keeps its own statistics, as with the prototype memories."""
    key, needs_head_graph = 'bone', True

    def __init__(self, weight=1.0, margin=1.0, momentum=0.01, beta=1.0, eps=1e-4, bones=None):
        from uda.model.loss import HAND_BONES, BonePriorLoss, BoneStatistics, check_positive
        check_positive('KinematicPrior: the weight', weight)
        self.weight = float(weight)
        self.crit = BonePriorLoss(beta=beta, margin=margin, eps=eps)              # (checks beta, margin and eps)
        self.stats = BoneStatistics(HAND_BONES if bones is None else bones, momentum)

    def source(self, batch):
        """Step A's part; a batch without the continuous key points is an error, not an update left out."""
        if batch.get('kp_s') is None:
            raise KeyError("KinematicPrior: the batch has no 'kp_s' (the continuous source key points, (B, K, 2) in heat-map pixels)")
        self.stats.update(batch['kp_s'], batch['w_s'])

    def step_c(self, step, batch, f_t, y_t, y_t_grad):
        loss = self.crit(y_t_grad, batch['w_t'], self.stats, scale=self.weight)
        return loss, {'bone_uv_t': self.crit.uv}                  # (kept: the soft-arg-max the prior was taken of)

    def state_dict(self):
        return self.stats.state_dict()

    def load_state_dict(self, state):
        self.stats.load_state_dict(state)


class CrossDomainMixup:
    """What ``DAStep(mixup=...)`` takes: a fourth stage, step M, behind update C.  The reference's ``mixup`` (uda/model/loss.py:13-24,
    never called there: nothing builds heat-maps for the unlabelled target images) on the batch of the iteration: every source
    image is blended with the target image of the same index by ``lam = max(mix, 1 - mix)``, ``mix ~ Beta(beta, beta)`` per sample,
    the labels likewise, and the backbone, the neck and the main head are trained on the 2B blends with ``weight * KL``.  The
    target heat-maps are the Gaussian at the arg-max (``PseudoLabelGenerator``) of the student's prediction ``y_t`` of step C
    (``labels='student'``) or of the EMA teacher's on ``x_t_ema`` (``labels='teacher'``; with a ``MeanTeacher`` attached to the step,
    its forward of step C is reused).  One ``mi355_mixup_pairs`` launch writes the blends into buffers this object owns.

    The coefficients live in device memory at a fixed address (``lam``) and are written from the host before the iteration
    (``draw``), from an RNG state this object owns -- seeded from ``seed`` and ``rank``; the global RNG is not advanced -- with the
    reference's own expression (``uda.model.loss.draw_mixup_coefficients``).  ``state_dict()`` is what the epoch checkpoint keeps as
    ``mixup_state``."""
    key = 'mix'

    def __init__(self, beta=1.0, weight=1.0, labels='student', ema=None, seed=0, rank=0):
        from uda.model.loss import check_positive
        check_positive('CrossDomainMixup: beta', beta)
        check_positive('CrossDomainMixup: the weight', weight)
        if labels not in ('student', 'teacher'):
            raise ValueError("CrossDomainMixup: labels must be 'student' or 'teacher', got %r" % (labels,))
        if labels == 'teacher' and ema is None:
            raise ValueError("CrossDomainMixup: labels='teacher' needs an EMATeacher (--ema-update const|warmup)")
        self.beta, self.weight, self.labels, self.ema = float(beta), float(weight), labels, ema
        self.seed, self.rank = int(seed or 0), int(rank)
        self._rng = self._seeded(0)
        self.draws = 0
        self.lam = None                  # (B,) fp32 on the device, fixed address
        self.lam_host = None             # the coefficients of the last draw
        self._bufs, self._gen, self._teacher, self._w_t = None, None, None, None

    # ------------------------------------------------------------ coefficients
    def draw(self, B=None, device=None):
        """Draw the coefficients of the coming iteration and write them to the device (host work: outside graph capture)."""
        from uda.model.loss import draw_mixup_coefficients
        if self.lam is None:
            if B is None:
                raise RuntimeError('CrossDomainMixup: run one eager iteration before replaying graphs')
            self.lam = torch.zeros(int(B), dtype=torch.float32, device=device)
        with torch.random.fork_rng(devices=[]):          # the global CPU generator is put back as it was
            torch.set_rng_state(self._rng)
            lam = draw_mixup_coefficients(self.lam.numel(), self.beta)
            self._rng = torch.get_rng_state()
        self.draws += 1
        self.lam_host = lam
        self.lam.copy_(lam, non_blocking=True)
        return lam

    def _seeded(self, draws):
        """The generator state of a rank that starts (draws = 0) or joins a resumed run whose checkpoint holds another rank's state."""
        return torch.Generator().manual_seed(self.seed * 1000003 + 7919 * self.rank + 17 + 104729 * int(draws)).get_state()

    def state_dict(self):
        """The RNG state, the number of draws so far and the last coefficients (a CPU copy): what the checkpoint keeps."""
        return {'rng_state': self._rng.clone(), 'draws': self.draws, 'beta': self.beta, 'rank': self.rank,
                'lam': None if self.lam_host is None else self.lam_host.clone()}

    def load_state_dict(self, state):
        """Go on where the saved run was.  The checkpoint is rank 0's: another rank takes the number of draws and a state seeded
        from (seed, rank, draws), so that the ranks keep drawing different coefficients."""
        self.draws = int(state.get('draws', 0))
        if int(state.get('rank', 0)) == self.rank:
            self._rng = state['rng_state'].clone().to(torch.uint8).cpu()
        else:
            self._rng = self._seeded(self.draws)

    # ------------------------------------------------------------ step M
    def teacher(self, step):
        """The in-iteration teacher whose folded operands follow the EMA update: the MeanTeacher's when the step has one."""
        if step.mt is not None:
            return step.mt.teacher
        if self._teacher is None:
            from .teacher import InIterationTeacher
            self._teacher = InIterationTeacher(self.ema)
        return self._teacher

    def target_labels(self, step, batch):
        """(B, K, H, W) Gaussians at the arg-max of the student's or the teacher's prediction on the target batch."""
        from uda.model.regda_4 import PseudoLabelGenerator, cached_centres
        if self.labels == 'student':
            y = step.out['y_t']
        else:
            shared = step.mt is not None or (step.coord is not None and step.coord.target == 'teacher')
            y = step.out.get('y_t_ema') if shared else None                   # step C's teacher forward, when there was one
            if y is None:
                y = step.teacher_forward(self.teacher(step), batch)
            self._w_t = step.teacher_weights(batch)                           # (a geometric view: w_t * valid)
        K, H, W = y.shape[1:]
        if self._gen is None or (self._gen.num_keypoints, self._gen.height, self._gen.width) != (K, H, W):
            self._gen = PseudoLabelGenerator(K, H, W)
        return self._gen.labels(y, kind=0, want_gf=False, xy=cached_centres(y))[0]

    def blend(self, batch, hm_t):
        """mixup_pairs(x_s, label_s, w_s, x_t, hm_t, w_t, lam) into the buffers of this object -> (x_mix, hm_mix, w_mix)."""
        f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        w_t = batch['w_t'] if self.labels == 'student' or self._w_t is None else self._w_t
        ops_in = [f32(batch[k]) for k in ('x_s', 'label_s', 'w_s', 'x_t')] + [hm_t, f32(w_t)]
        sig = tuple(tuple(t.shape) for t in ops_in)
        if self._bufs is None or self._bufs[0] != sig:
            if torch.cuda.is_current_stream_capturing():
                raise _rt.Mi355Error('CrossDomainMixup: the blend buffers would be allocated during graph capture; run one eager iteration first')
            B, dev = ops_in[0].shape[0], ops_in[0].device
            self._bufs = (sig, tuple(torch.empty((2 * B,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in ops_in[:3]))
        if self.lam is None or self.lam.numel() != ops_in[0].shape[0]:
            raise _rt.Mi355Error('CrossDomainMixup: no coefficients for a batch of %d: draw() first' % ops_in[0].shape[0])
        return ops.mixup_pairs(*ops_in, self.lam, out=self._bufs[1])


class FourierStyle:
    """What ``DAStep(fda=...)`` takes: Fourier Domain Adaptation (Yang and Soatto, CVPR 2020; not in the reference) of the source
    batch at the head of step A.  The amplitude of the ``(2b+1)^2`` lowest frequencies of every source image, ``b = floor(min(H, W) *
    beta)``, is replaced by that of the target image of the same index and the phase is kept, so the geometry and the labels stay
    (``mi355_fda_transfer``: two launches, no FFT).  No learnable parts and no state: nothing joins the checkpoint.  This object
    owns the stylised batch and the workspace at fixed addresses, keyed by the input signature, so the launches capture."""

    def __init__(self, beta=0.01, mean=ops.MEAN, std=ops.STD):
        from uda.model.loss import check_positive
        check_positive('FourierStyle: beta', beta)
        self.beta = float(beta)
        self.mean, self.std = tuple(mean), tuple(std)
        self._bufs = None

    def band(self, H, W):
        return ops.fda_band(H, W, self.beta)

    def stylise(self, batch):
        """x_s of `batch` in the style of its x_t, in the buffer of this object; the batch's own tensors are only read."""
        f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        x_s, x_t = f32(batch['x_s']), f32(batch['x_t'])
        sig = (tuple(x_s.shape), tuple(x_t.shape), x_s.device)
        if self._bufs is None or self._bufs[0] != sig:
            if torch.cuda.is_current_stream_capturing():
                raise _rt.Mi355Error('FourierStyle: the stylised batch and the workspace would be allocated during graph capture; run one eager iteration first')
            if x_s.dim() != 4:
                raise _rt.Mi355Error('FourierStyle: x_s must be (B, C, H, W), got %s' % (tuple(x_s.shape),))
            B, C, H, W = x_s.shape
            need = _rt.load().mi355_fda_workspace_bytes(B, C, H, W, self.band(H, W))
            if need < 0:
                raise _rt.Mi355Error('FourierStyle: beta=%g on %s images: %s' % (self.beta, tuple(x_s.shape), _rt.load().mi355_last_error().decode()))
            self._bufs = (sig, torch.empty_like(x_s), torch.empty(need, dtype=torch.uint8, device=x_s.device))
        return ops.fda_transfer(x_s, x_t, self.beta, self.mean, self.std, out=self._bufs[1], ws=self._bufs[2])


class DAStep:
    """Holds the static batch buffers and runs A/B/C (and M, with ``mixup``).  ``optimizers`` = dict with keys f, h, h_adv, h_adv2,
    h_adv3 (FusedSGD or any torch optimizer), ``criteria`` = dict with keys kl, rd (x6), rd2 (x5), rd1 (x1)."""

    def __init__(self, model, optimizers, criteria, trade_off=1.0, skip_discarded=True, track_accuracy=True, ema=None, mt=None, mmd=None, jfa=None,
                 proto=None, clip=None, mixup=None, fda=None, view=None, bone=None, occlude=None, teacher_conf=0.0, conf_beta=1.0, coord=None):
        self.model, self.opt, self.crit = model, optimizers, criteria
        # optional mi355.teacher.GeometricView (may also be assigned after construction): the teacher of the iteration -- one forward,
        # shared by the MeanTeacher, CoordRegression(target='teacher') and CrossDomainMixup(labels='teacher') -- sees the target batch
        # rotated, scaled and shifted per sample, and its heat-maps are mapped back before anybody reads them; the maps whose peak it
        # did not see inside its frame drop out of the three terms.  None: nothing is launched, nothing is drawn.
        self.view, self._last_teacher = view, None
        # optional mi355.optim.GradClipper (may also be assigned after construction): each of the three updates takes the global
        # gradient norm of everything it steps (A: f and the four heads, B: the adversarial heads, C: f), behind the gradient
        # exchange, and steps on the clipped gradients -- or not at all when the norm is not finite.  None: nothing is launched.
        self.clip = clip
        self.ema = ema               # optional mi355.optim.EMATeacher: updated behind step C's optimizer (train1.py:461)
        # the optional terms of step C's loss (`_Term`; any of them may also be assigned after construction): a
        # mi355.teacher.MeanTeacher, whose folded operands are refreshed behind the EMA update, an MMDAlign, a JointFeatureAlign,
        # a PrototypeAlign
        self.mt, self.mmd, self.jfa, self.proto = mt, mmd, jfa, proto
        # optional CrossDomainMixup (may also be assigned after construction): step M behind update C -- one forward and backward
        # of the 2B blended images through the backbone, the neck and the main head, then update M of optimizer_f and optimizer_h.
        # The EMA update and the teacher's refresh then move behind update M.  None: nothing is launched, nothing moves.
        self.mixup = mixup
        # optional CoordRegression (may also be assigned after construction): step A's loss gains the coordinate loss on the source
        # batch (batch['kp_s']); with target='teacher' it is also the last of step C's terms.  None: nothing is launched.
        self.coord = coord
        # optional FourierStyle (may also be assigned after construction): step A's forward takes the source batch in the style of
        # the target batch (two launches at the head of step A) instead of batch['x_s'], which is only read; steps B, C and M, the
        # teacher views and the mixup blend keep the batch's own tensors.  None: nothing is launched.
        self.fda = fda
        # optional KinematicPrior (may also be assigned after construction): step A updates the bone-ratio statistics from
        # batch['kp_s'], and the prior on the target prediction is the last of step C's terms.  None: nothing is launched.
        self.bone = bone
        # optional mi355.teacher.KeypointOcclusion (may also be assigned after construction): the teacher's one forward of the
        # iteration moves to the head of step B, and the student's forwards of the target batch (step B's; step C's own one with
        # skip_discarded=False) read a copy of batch['x_t'] with a patch around confident teacher key points blanked.  batch['x_t']
        # is only read: the teacher, step M's blend and FDA keep the loader's images.  None: nothing is launched, nothing is drawn.
        # teacher_conf > 0 (with or without occlusion): a teacher map counts for the MeanTeacher, CoordRegression(target='teacher')
        # and CrossDomainMixup(labels='teacher') only when the peak of softmax(conf_beta * y) reaches it (the occlusion's own beta
        # when there is one) -- `conf` multiplies in wherever the view's `valid` flags do; it is also the occlusion's candidate
        # threshold.  0: no gate.
        import math
        if not (isinstance(teacher_conf, (int, float)) and math.isfinite(teacher_conf) and teacher_conf >= 0.0):
            raise ValueError('DAStep: teacher_conf must be finite and not negative, got %r' % (teacher_conf,))
        self.occlude, self.teacher_conf, self.conf_beta = occlude, float(teacher_conf), float(conf_beta)
        self._gate, self._occ_teacher, self._y_ema_iter, self._x_student = None, None, None, None
        self._kept_c = {}
        if mt is not None and self.ema is None:
            self.ema = mt.ema
        self.trade_off, self.skip, self.track_acc = trade_off, skip_discarded, track_accuracy
        self.graphs = None
        self.out = {}
        self._adv_params = [p for n in ('head_adv', 'head_adv2', 'head_adv3') for p in getattr(model, n).parameters()]
        self._reducer = None
        self._stage_params = {}
        self.overlap = os.environ.get('MI355_OVERLAP_ALLREDUCE', '1') == '1'
        self._install_stage_hooks()

    # ------------------------------------------------------------------ all-reduce overlapped with the backward
    def _install_stage_hooks(self):
        """Forward hooks that put a gradient hook on the output of the neck and of every ResNet stage.  When such a
        gradient arrives, the modules behind that tensor have finished their backward (see _OverlapReducer)."""
        m = self.model
        bb, up = getattr(m, 'backbone', None), getattr(m, 'upsampling', None)
        if bb is None or up is None or not all(hasattr(bb, n) for n in ('layer1', 'layer2', 'layer3', 'layer4', 'maxpool')):
            return
        heads = [(k, list(getattr(m, n).parameters())) for k, n in (('h', 'head'), ('h_adv', 'head_adv'), ('h_adv2', 'head_adv2'),
                                                                    ('h_adv3', 'head_adv3')) if hasattr(m, n)]
        self._stage_params = {                         # gradient of <tensor> ready  ->  these parameters are done
            'neck_out': heads,
            'layer4_out': [('f', list(up.parameters()))],
            'layer3_out': [('f', list(bb.layer4.parameters()))],
            'layer2_out': [('f', list(bb.layer3.parameters()))],
            'layer1_out': [('f', list(bb.layer2.parameters()))],
            'pool_out': [('f', list(bb.layer1.parameters()))],
        }

        def fwd_hook(stage):
            def hook(mod, inp, out):
                if torch.is_tensor(out) and out.requires_grad:
                    out.register_hook(lambda g, s=stage: self._on_stage_grad(s))
            return hook
        for stage, mod in (('neck_out', up), ('layer4_out', bb.layer4), ('layer3_out', bb.layer3), ('layer2_out', bb.layer2),
                           ('layer1_out', bb.layer1), ('pool_out', bb.maxpool)):
            mod.register_forward_hook(fwd_hook(stage))

    def _on_stage_grad(self, stage):
        _rt.flush_grouped_wgrads()       # the weight gradients of the stage just finished: one grouped launch
        if self._reducer is not None:
            self._reducer.stage_done(stage)

    def _overlap_capturable(self):
        """Can the overlapped exchange be CAPTURED into the HIP graphs?  RCCL collectives are stream work and capture like kernels
        (probed on this stack: profiles/tools/rccl_graph_probe.py -- an async all-reduce on RCCL's stream inside torch.cuda.graph, replayed);
        gloo collectives are host work and cannot.  OPT-IN (MI355_DDP_GRAPH_OVERLAP=1): the default keeps the blocking exchange
        between the graphs -- on one xGMI node the two forms are expected within a few tenths of a millisecond of each other
        (DESIGN.md section 6), the captured form has only ever run in a one-rank group (no multi-GPU box in this build's reach), and
        a capture that hangs on real ranks would cost a whole run, where an exception only costs a fallback."""
        return (self.overlap and _distributed() and dist.get_backend() == 'nccl' and
                os.environ.get('MI355_DDP_GRAPH_OVERLAP', '0') == '1')

    def _begin_reduce(self, keys):
        """Arm the overlapped reducer for the backward about to run: more than one rank, launched eagerly -- or being captured with
        a backend whose collectives capture (the all-reduces then sit in the graph on RCCL's stream, beside the rest of the backward)."""
        capturing = torch.cuda.is_current_stream_capturing()
        self._reducer = _OverlapReducer(self, keys) if (self.overlap and _distributed() and
                                                         (not capturing or self._overlap_capturable())) else None
        if self._reducer is not None:
            # collectives will run beside this backward: the one-launch BatchNorm backward needs every CU for its resident
            # blocks (mi355_bn_set_resident), so this pass takes the three-launch form
            self._bn_resident_prev = _rt.load().mi355_bn_set_resident(0)

    def _end_reduce(self, keys):
        r, self._reducer = self._reducer, None
        if r is not None:
            r.finish()
            _rt.load().mi355_bn_set_resident(self._bn_resident_prev)
        else:
            _allreduce_mean(self._grads(keys))

    # ------------------------------------------------------------------ the three steps (fwd+bwd, then update)
    def teacher_forward(self, teacher, batch):
        """The teacher's heat-maps on its view of the target batch (x_t_ema; x_t itself when the batch has none), in the loader's
        frame.  With a GeometricView the teacher also keeps the flags (`valid`) and w_t * valid (`w_out`)."""
        sel = self._selector()
        if sel is not None and self._y_ema_iter is not None:
            return self._y_ema_iter                      # this iteration's one forward: every later caller reads the same maps
        x = batch['x_t_ema'] if batch.get('x_t_ema') is not None else batch['x_t']
        teacher.view, self._last_teacher = self.view, teacher
        if self.view is None:
            y = teacher.forward(x)
        else:
            y = teacher.forward(x, w_in=batch['w_t'])
        if sel is not None:
            # the confidence of every map (of the maps as the consumers read them: mapped back under a view, whose flags enter
            # as the gate) and, with occlusion, the boxes: two launches behind the forward
            S = batch['x_t'].shape[-1]
            if sel.n > 0 and batch['x_t'].shape[-2] != S:
                raise _rt.Mi355Error('DAStep: key-point occlusion needs square target images, got %s' % (tuple(batch['x_t'].shape),))
            sel.select(y, self.teacher_conf, S, gate_in=teacher.valid if self.view is not None else None, w_in=batch['w_t'])
            self._y_ema_iter = y
            self.out.update(conf_share=sel.stats[1])
            if sel.n > 0:
                self.out.update(occ_boxes=sel.stats[0])
        return y

    def _selector(self):
        """The KeypointOcclusion whose select() follows the teacher's forward: the step's occlusion, else -- for teacher_conf > 0
        alone -- a gate of the step's own with no boxes; None when both are off."""
        if self.occlude is not None:
            return self.occlude
        if self.teacher_conf > 0.0:
            if self._gate is None:
                from .teacher import KeypointOcclusion
                self._gate = KeypointOcclusion(n=0, beta=self.conf_beta)
            return self._gate
        return None

    def _iteration_teacher(self):
        """The in-iteration teacher of the hoisted forward: the one the consumers of this step would use, else one of the step's own."""
        if self.mt is not None:
            return self.mt.teacher
        if self.coord is not None and self.coord.target == 'teacher':
            return self.coord.teacher(self)
        if self.mixup is not None and self.mixup.labels == 'teacher':
            return self.mixup.teacher(self)
        if self._occ_teacher is None:
            if self.ema is None:
                raise ValueError('key-point occlusion needs an EMATeacher (--ema-update const|warmup)')
            from .teacher import InIterationTeacher
            self._occ_teacher = InIterationTeacher(self.ema)
        return self._occ_teacher

    def _student_input(self, batch):
        """What the student's forwards of the target batch read: batch['x_t'], or -- with occlusion -- its occluded copy, behind the
        teacher's forward of the iteration at the head of step B."""
        if self.occlude is None or self.occlude.n == 0:
            return batch['x_t']
        self.teacher_forward(self._iteration_teacher(), batch)
        return self.occlude.apply(batch['x_t'])

    def teacher_weights(self, batch):
        """The joint weights a consumer of the teacher's forward uses: w_t, times the flags of the view when there is one (kept by
        the teacher that ran this iteration's forward), times the confidence flags with teacher_conf > 0."""
        if self.teacher_conf > 0.0:
            return self._selector().w_out                # w_t * conf; conf holds the view's flags
        return batch['w_t'] if self.view is None else self._last_teacher.w_out

    def teacher_map_weights(self, teacher):
        """The per-map weight of the MeanTeacher's loss: the confidence flags with teacher_conf > 0 (they hold the view's), else the
        view's flags, else None."""
        if self.teacher_conf > 0.0:
            return self._selector().conf
        return teacher.valid if teacher.view is not None else None

    def _draw_occlusion(self, batch=None):
        if self.occlude is None:
            return
        if batch is None:
            self.occlude.draw()
        else:
            self.occlude.draw(batch['x_t'].shape[0], batch['x_t'].device)

    def _draw_view(self, batch=None):
        if self.view is None:
            return
        if batch is None:
            self.view.draw()
        else:
            self.view.draw(batch['x_t'].shape[0], batch['x_t'].device, image_size=batch['x_t'].shape[-2:],
                           heatmap_size=batch['label_s'].shape[-2:])

    def terms(self):
        """The optional terms that are on, in the order in which step C adds them and issues their kernels."""
        on = [t for t in (self.mt, self.mmd, self.jfa, self.proto) if t is not None]
        if self.coord is not None and self.coord.target == 'teacher':
            on.append(self.coord)
        if self.bone is not None:
            on.append(self.bone)
        return on

    def _fwdbwd_A(self, b):
        m, c = self.model, self.crit
        for o in self.opt.values():
            o.zero_grad()
        self._y_ema_iter = None                  # (a new iteration: the teacher's forward of the last one is not this one's)
        x_s = b['x_s'] if self.fda is None else self.fda.stylise(b)
        if self.bone is not None:
            self.bone.source(b)              # the statistics step C reads: one launch, nothing of the network in it
        with _rt.grouped_wgrads():
            y_s, y_s_adv, y_s_adv2, y_s_adv3, f_s = m(x_s)
            for t in self.terms():
                self.out.update(t.step_a(f_s, y_s))
            # the coefficients of train1.py:384-387 ride inside the loss kernels (scale=), the total's gradient is the unit scalar
            loss_s = c['kl'](y_s, b['label_s'], b['w_s'], scale=2) + \
                c['rd2'](y_s, y_s_adv2, None, b['w_s'], mode='min', scale=4) + \
                c['rd'](y_s, y_s_adv, None, b['w_s'], mode='min', scale=4) + \
                c['rd1'](y_s, y_s_adv3, b['w_s'], mode='min', scale=4)
            if self.coord is None:
                loss_s.backward(_rt.unit_grad(loss_s))
            else:
                loss_coord = self.coord.source(y_s, b)
                total = loss_s + loss_coord
                total.backward(_rt.unit_grad(total))
                self.out.update(loss_coord=loss_coord.detach())
        _rt.join_side()
        self.out.update(loss_s=loss_s.detach(), y_s=y_s.detach(), y_s_adv=y_s_adv.detach())

    def _step(self, keys, slot):
        """Step the optimizers `keys` in that order; with a clipper, on the gradients clipped to one norm over all of them."""
        if self.clip is None:
            for k in keys:
                self.opt[k].step()
            return
        rec = self.clip.measure([self.opt[k] for k in keys], slot)
        self.out['gn_' + slot] = rec
        for k in keys:
            self.opt[k].step(clip=rec)

    def _update_A(self):
        self._step(('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'), 'a')

    def _fwdbwd_B(self, b):
        m, c, to = self.model, self.crit, self.trade_off
        for k in ('h_adv', 'h_adv2', 'h_adv3'):
            self.opt[k].zero_grad()
        x_t = self._x_student = self._student_input(b)
        if self.skip:
            with _rt.bn_updates(2):               # this forward also stands for step C's (identical) one
                f_t = m.features(x_t)
                y_t_grad = m.head(f_t)
                y_t = y_t_grad.detach()           # only ever used detached (pseudo-labels) in B and C ...
                if not any(t.needs_head_graph for t in self.terms()):
                    y_t_grad = None               # ... but for a term of step C that goes through the head: else its graph is freed here
            self._shared = (f_t, y_t, y_t_grad)
            y_t_adv, y_t_adv2, y_t_adv3 = m.adv_heads(f_t.detach())
        else:
            y_t, y_t_adv, y_t_adv2, y_t_adv3, _ = m(x_t)
        loss1 = c['rd1'](y_t, y_t_adv3, b['w_t'], mode='max', scale=0.3 * to)
        H = y_t.shape[-1]
        target5 = ops.bilinear_up(y_t_adv3.detach(), H, 0.5)               # 0.5 * up(y_adv3) ...
        target5 = ops.bilinear_up(y_t_adv2.detach(), H, 1.0, out=target5)   # ... + up(y_adv2)   (train1.py:410-424)
        target0 = ops.bilinear_up(y_t_adv3.detach(), H // 2)
        loss2 = c['rd'](y_t, y_t_adv, target5, b['w_t'], mode='max', scale=to)
        loss3 = c['rd2'](y_t, y_t_adv2, target0, b['w_t'], mode='max', scale=0.3 * to)
        loss_gf = loss1 + loss2 + loss3                 # = 0.3 to rd1 + to rd + 0.3 to rd2   (train1.py:426-432)
        with _rt.grouped_wgrads():
            loss_gf.backward(_rt.unit_grad(loss_gf))
        _rt.join_side()
        self.out.update(loss_gf=loss_gf.detach())

    def _update_B(self):
        self._step(('h_adv2', 'h_adv', 'h_adv3'), 'b')

    def _fwdbwd_C(self, b):
        m, c, to = self.model, self.crit, self.trade_off
        self.opt['f'].zero_grad()
        if self.skip:
            for p in self._adv_params:
                p.requires_grad_(False)
        try:
            if self.skip:
                f_t, y_t, y_t_grad = self._shared
                self._shared = None
                y_t_adv, y_t_adv2, y_t_adv3 = m.adv_heads(f_t)
            else:
                y_t, y_t_adv, y_t_adv2, y_t_adv3, f_t = m(self._x_student)
                y_t_grad = y_t
            loss1 = c['rd2'](y_t, y_t_adv2, None, b['w_t'], mode='min', scale=0.3 * to)
            loss2 = c['rd'](y_t, y_t_adv, None, b['w_t'], mode='min', scale=to)
            loss_gt = loss1 + loss2                     # = 0.3 to rd2 + to rd   (train1.py:443-448)
            # Only optimizer_f steps in C: the weight gradients this backward leaves in the main head (through a term that needs its
            # graph) are discarded by the next step A's zero_grad, like the adversarial heads'.
            total, kept = loss_gt, {}
            self._kept_c = kept                         # (a later term may reuse what an earlier one kept: the teacher's forward)
            for t in self.terms():
                loss, more = t.step_c(self, b, f_t, y_t, y_t_grad)
                total = total + loss
                kept.update(more, **{'loss_' + t.key: loss.detach()})
            with _rt.grouped_wgrads():
                total.backward(_rt.unit_grad(total))
            _rt.join_side()
        finally:
            if self.skip:
                for p in self._adv_params:
                    p.requires_grad_(True)
        self.out.update(kept, loss_gt=loss_gt.detach(), y_t=y_t.detach(), y_t_adv=y_t_adv.detach())

    def _update_C(self):
        self._step(('f',), 'c')
        if self.mixup is None:
            self._update_ema()

    def _update_ema(self):
        """Behind the last optimizer step of the iteration (update C; update M with mixup)."""
        if self.ema is not None:
            self.ema.update()
            if self.mt is not None:
                self.mt.teacher.refresh()        # the teacher's folded operands follow its weights, in place
            if self.mixup is not None and self.mixup._teacher is not None:
                self.mixup._teacher.refresh()    # (labels='teacher' without a MeanTeacher: the mixup's own in-iteration teacher)
            if self.coord is not None and self.coord._teacher is not None:
                self.coord._teacher.refresh()    # (target='teacher' without a MeanTeacher, likewise)
            if self._occ_teacher is not None:
                self._occ_teacher.refresh()      # (occlusion with no consumer of the teacher's forward: the step's own teacher)

    KM = ('f', 'h')                              # what update M steps

    def _fwdbwd_M(self, b):
        """Step M: the blends of the source and the target batch through backbone, neck and main head, weight * KL against the
        blended labels.  The adversarial heads never see the blended images."""
        m, c, mx = self.model, self.crit, self.mixup
        for k in self.KM:
            self.opt[k].zero_grad()
        x_mix, hm_mix, w_mix = mx.blend(b, mx.target_labels(self, b))
        with _rt.grouped_wgrads():
            y_mix = m.head(m.features(x_mix))
            loss_mix = c['kl'](y_mix, hm_mix, w_mix, scale=mx.weight)
            loss_mix.backward(_rt.unit_grad(loss_mix))
        _rt.join_side()
        self.out.update(loss_mix=loss_mix.detach())

    def _update_M(self):
        self._step(self.KM, 'm')
        self._update_ema()

    def _accuracy(self, b):
        """Device side of the four accuracy() calls of train1.py:464-475: arg-max coordinates + PCK distances."""
        if not self.track_acc:
            return
        o = self.out
        _, lab_s, _ = ops.argmax2d(b['label_s'])
        has_t = b.get('label_t') is not None
        lab_t = ops.argmax2d(b['label_t'])[1] if has_t else None
        H, W = o['y_s'].shape[-2:]
        from uda.model.regda_4 import cached_centres
        for name, pred, lab in (('s', o['y_s'], lab_s), ('t', o['y_t'], lab_t), ('s_adv', o['y_s_adv'], lab_s),
                                ('t_adv', o['y_t_adv'], lab_t)):
            if lab is None:
                continue
            xy = cached_centres(pred)            # (y_s / y_t: already computed for the pseudo-labels)
            o['pck_' + name] = ops.pck_dists(xy, lab, W / 10.0, H / 10.0)

    def _grads(self, keys):
        bufs = []
        for k in keys:
            o = self.opt[k]
            if hasattr(o, 'flat_grads'):
                bufs += o.flat_grads()
            else:
                bufs += [p.grad for g in o.param_groups for p in g['params'] if p.grad is not None]
        return bufs

    def check_health(self, where=''):
        """Raise if any kernel of the steps run so far reported an in-launch failure (today: a one-launch BatchNorm backward
        that gave up waiting for its blocks and poisoned its gradients).  Synchronises the device."""
        from . import ops
        ops.bn_resident_check(where)

    # ------------------------------------------------------------------ eager iteration
    def run(self, batch):
        """batch: dict x_s, label_s, w_s, x_t, w_t (+ optional label_t for the PCK bookkeeping; with `mt`: x_t_ema, the teacher's
        view of the target batch -- x_t itself when the key is absent; with `coord` or `bone`: kp_s, the continuous source key
        points (B, K, 2) in heat-map pixels)."""
        if self.graphs is not None:
            return self.replay(batch)
        from uda.model.regda_4 import _CENTRES
        _CENTRES.clear()
        self.model.train()
        if self.clip is not None:
            if self.mixup is not None:
                self.clip.ensure_slot('m')       # a fourth record for update M (the three-slot layout is untouched without mixup)
            self.clip.sync()
        if self.mixup is not None:
            self.mixup.draw(batch['x_s'].shape[0], batch['x_s'].device)
        self._draw_view(batch)
        self._draw_occlusion(batch)
        self._begin_reduce(('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'))
        self._fwdbwd_A(batch)
        self._end_reduce(('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'))
        self._update_A()
        self._fwdbwd_B(batch)                    # (heads only: nothing to overlap with)
        _allreduce_mean(self._grads(('h_adv', 'h_adv2', 'h_adv3')))
        self._update_B()
        self._begin_reduce(('f',))
        self._fwdbwd_C(batch)
        self._end_reduce(('f',))
        if self.ema is not None:
            self.ema.sync()
        self._update_C()
        if self.mixup is not None:
            self._begin_reduce(self.KM)
            self._fwdbwd_M(batch)
            self._end_reduce(self.KM)
            self._update_M()
        self._accuracy(batch)
        self.model.step()
        return self.out

    # ------------------------------------------------------------------ graph capture / replay
    def capture(self, batch, warmup=3):
        """Capture the iteration as six HIP graphs (fwd+bwd and update of A, B, C; eight with `mixup`: those of M) over static copies of
        `batch`; the gradient all-reduces run eagerly between them.  Everything that changes per iteration
        (inputs, learning rates, GL lambda, the EMA coefficients, the clipper's max_norm) is read from device memory.  With an EMA teacher attached its
        update is captured into the last update graph, behind the iteration's last optimizer step, where the eager iteration has it."""
        self.model.train()
        self.static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.run(self.static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        from uda.model.regda_4 import _CENTRES
        _CENTRES.clear()
        pool = torch.cuda.graph_pool_handle()
        KA, KB, KC = ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3'), ('h_adv', 'h_adv2', 'h_adv3'), ('f',)
        # With RCCL the gradient exchange is captured too: steps A and C with the overlapped reducer (its asynchronous all-reduces
        # become a parallel branch of the backward's graph, started where the gradient hooks fire), step B's small exchange behind
        # its backward.  Replay then issues no collective from the host.  Otherwise (one rank, gloo) the exchange stays between graphs.
        self.exchange_captured = self._overlap_capturable()
        if self.exchange_captured:
            def seg_a():
                self._begin_reduce(KA); self._fwdbwd_A(self.static); self._end_reduce(KA)

            def seg_b():
                self._fwdbwd_B(self.static); _allreduce_mean(self._grads(KB))

            def seg_c():
                self._begin_reduce(KC); self._fwdbwd_C(self.static); self._end_reduce(KC)
        else:
            seg_a, seg_b, seg_c = (lambda: self._fwdbwd_A(self.static)), (lambda: self._fwdbwd_B(self.static)), (lambda: self._fwdbwd_C(self.static))
        segs = [seg_a, self._update_A, seg_b, self._update_B, seg_c, lambda: (self._update_C(), self._accuracy(self.static))]
        if self.mixup is not None:               # two more graphs; the EMA launches sit in the last one, behind update M
            if self.exchange_captured:
                def seg_m():
                    self._begin_reduce(self.KM); self._fwdbwd_M(self.static); self._end_reduce(self.KM)
            else:
                seg_m = lambda: self._fwdbwd_M(self.static)
            segs += [seg_m, self._update_M]
        mode = _rt.graph_capture_mode()        # 'thread_local' beside an RCCL process group (its watchdog thread polls events)
        graphs = []
        with _rt.no_gc_in_capture():
            for fn in segs:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, capture_error_mode=mode):
                    fn()
                graphs.append(g)
        self.graphs = graphs          # capturing executes nothing: model / optimizer state is unchanged
        return self

    def choose_launch_mode(self, batch, after=None, threshold=0.85):
        """Multi-rank runs.  With RCCL the overlapped gradient exchange is captured into the HIP graphs, so graph replay is chosen
        outright.  With a backend whose collectives cannot be captured (gloo rehearsals): eager launches keep the exchange
        overlapped with the backward, but only pay off while the host can feed the GPU.  Times one eager iteration on the host (enqueue) and on the GPU (enqueue + drain); if enqueueing
        takes (nearly) as long as running it on ANY rank, every rank should replay graphs instead (collectives between the
        graphs).  Runs one real iteration (`after()` is called behind it: scheduler ticks) and returns 'graph' or 'eager' --
        the same answer on every rank (MAX over ranks).  MI355_DDP_GRAPH=1 / 0 forces the answer."""
        import time
        forced = os.environ.get('MI355_DDP_GRAPH')
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        self.run(batch)
        if after is not None:
            after()
        t_host = time.perf_counter() - t_a
        torch.cuda.synchronize()
        t_gpu = time.perf_counter() - t_a
        r = torch.tensor([t_host / max(t_gpu, 1e-9)], device=next(self.model.parameters()).device)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(r, op=dist.ReduceOp.MAX)
        self.host_gpu_ratio = float(r)
        if forced in ('0', '1'):
            return 'graph' if forced == '1' else 'eager'
        if self._overlap_capturable():
            return 'graph'          # RCCL: the overlapped exchange is captured into the graphs -- replay loses nothing and cannot go host-bound
        # (0.85, not ~1: one sample of the host's enqueue time on a node where eight ranks share the cores is an optimistic estimate, and
        #  an eager run that goes host-bound loses more than the blocking exchange between the graphs costs)
        return 'graph' if self.host_gpu_ratio > threshold else 'eager'

    def _host_tick(self):
        for o in self.opt.values():
            if hasattr(o, 'sync_lr'):
                o.sync_lr()
        gl = getattr(self.model, 'gl_layer', None)
        if gl is not None:
            gl.sync()
        if self.ema is not None:
            self.ema.sync()
        if self.mt is not None:
            self.mt.sync()
        if self.clip is not None:
            self.clip.sync()
        if self.mixup is not None:
            self.mixup.draw()                # the coefficients of this iteration, to their fixed device address
        self._draw_view()                    # the records of this iteration's teacher views, likewise
        self._draw_occlusion()               # the draws of this iteration's occlusion boxes, likewise

    def replay(self, batch=None):
        if batch is not None and batch is not self.static:
            for k, v in batch.items():
                if torch.is_tensor(v):
                    self.static[k].copy_(v, non_blocking=True)
        self._host_tick()
        g = self.graphs
        if getattr(self, 'exchange_captured', False):      # the collectives are nodes of the graphs
            for gr in g:
                gr.replay()
        else:
            g[0].replay()
            _allreduce_mean(self._grads(('f', 'h', 'h_adv', 'h_adv2', 'h_adv3')))
            g[1].replay()
            g[2].replay()
            _allreduce_mean(self._grads(('h_adv', 'h_adv2', 'h_adv3')))
            g[3].replay()
            g[4].replay()
            _allreduce_mean(self._grads(('f',)))
            g[5].replay()
            if len(g) > 6:                   # step M
                g[6].replay()
                _allreduce_mean(self._grads(self.KM))
                g[7].replay()
        if self.ema is not None:
            self.ema.mark_updated()          # the launches sit in the last graph (_update_C; _update_M with mixup)
        self.model.step()
        return self.out


def build_training(model, heatmap_size=64, lr=0.01, momentum=0.9, wd=1e-4, lr_gamma=1e-4, lr_decay=0.75,
                   trade_off=1.0, num_keypoints=21, skip_discarded=True, track_accuracy=True, optimizer='sgd',
                   adam_betas=(0.9, 0.999), adam_eps=1e-8, fda=None):
    """Criteria, the five SGD optimizers and their LambdaLR schedules exactly as train1.py:131-154 builds them.
    `optimizer`: 'sgd' (the reference), 'adam' (FusedAdam, L2 weight decay `wd`) or 'adamw' (decoupled weight decay `wd`) for all
    five; `momentum` is not used by the last two.  `fda`: an optional FourierStyle, handed to the DAStep.  Returns (DAStep, optimizers dict, schedulers dict)."""
    from torch.optim.lr_scheduler import LambdaLR
    from uda.model.loss import JointsKLLoss
    from uda.model.regda_4 import PseudoLabelGenerator
    from uda.model.regda_7 import (PseudoLabelGenerator01, PseudoLabelGenerator03, RegressionDisparityx1,
                                   RegressionDisparityx5, RegressionDisparityx6)
    from .optim import make_optimizer
    crit = dict(
        kl=JointsKLLoss(),
        rd=RegressionDisparityx6(PseudoLabelGenerator(num_keypoints, heatmap_size, heatmap_size), JointsKLLoss(epsilon=1e-7)),
        rd2=RegressionDisparityx5(PseudoLabelGenerator03(num_keypoints, heatmap_size // 2, heatmap_size // 2), JointsKLLoss(epsilon=1e-7)),
        rd1=RegressionDisparityx1(PseudoLabelGenerator01(num_keypoints, heatmap_size // 4, heatmap_size // 4), JointsKLLoss(epsilon=1e-7)))
    mk = lambda ps: make_optimizer(optimizer, ps, lr=0.1, momentum=momentum, weight_decay=wd, betas=adam_betas, eps=adam_eps)
    opts = dict(
        f=mk([{'params': model.backbone.parameters(), 'lr': 0.1}, {'params': model.upsampling.parameters(), 'lr': 0.1}]),
        h=mk(model.head.parameters()), h_adv=mk(model.head_adv.parameters()),
        h_adv2=mk(model.head_adv2.parameters()), h_adv3=mk(model.head_adv3.parameters()))
    fn = lambda x: lr * (1. + lr_gamma * float(x)) ** (-lr_decay)
    scheds = {k: LambdaLR(o, fn) for k, o in opts.items()}
    return DAStep(model, opts, crit, trade_off, skip_discarded, track_accuracy, fda=fda), opts, scheds
