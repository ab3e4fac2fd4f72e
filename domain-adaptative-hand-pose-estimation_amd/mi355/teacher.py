"""The mean teacher inside a training iteration (reference train1.py:351-364, uda/model/loss.py:265-297).

``EMATeacher`` moves the teacher's weights after every iteration, so the BatchNorm-folded operands of its one-launch eval
convs go stale every iteration.  The host fold of ``mi355.nn._FoldedBn`` is several ATen launches per layer and allocates: it
cannot sit in a replayed graph.  ``InIterationTeacher`` owns fixed-address storage for every (conv, BatchNorm) pair the
teacher's eval forward folds -- fp32 scratch, packed operand, bias -- pins it into the layers' ``_FoldedBn`` and refreshes all
of it with ``refresh()``: one ``mi355_bn_fold_batched`` launch, one ``mi355_pack_weights_batched`` launch, the stem's pack, and
the ``repack_params`` / cast route for the convs with no BatchNorm behind them.  The packed operands are made from the folded
fp32 weights by the packers the host path uses, so they are that path's bits.  A grouped conv is folded in the dense
block-diagonal form the host path packs: its master is copied onto the diagonal of a zeroed fixed-address buffer first.

``GeometricView`` is what ``DAStep(view=...)`` takes: per sample another rotation, scale and shift of what the teacher sees, and the
way back for its heat-maps (``csrc/warp.hip``; Kim et al., ECCV 2022 -- not in the reference).

``MeanTeacher`` is what ``DAStep(mt=...)`` takes: the teacher, the device-resident loss and the per-epoch schedule of its weight
``m`` and of the joint curriculum ``k``.
"""
import torch

import mi355 as _rt
from . import Mi355Error, ops
from . import nn as _nn


def _pair(size):
    if isinstance(size, int):
        return size, size
    h, w = size
    return int(h), int(w)


class GeometricView:
    """Another view of the target batch for the teacher: per sample a rotation ``a ~ U(-rot_deg, rot_deg)`` degrees, a scale
    ``s ~ U(lo, hi)`` and a shift ``t ~ U(-shift, shift) * side`` about the image centre (Kim et al., ECCV 2022).  ``apply(x)`` is the
    teacher's input (``mi355_affine_warp_images``), ``undo(y, w_in)`` maps its heat-maps back to the loader's frame and flags the
    maps whose peak the teacher saw at least ``margin`` heat-map pixels inside its frame (``mi355_affine_unwarp_heatmaps``).
    Forward only: the teacher is detached, nothing is differentiated through either warp; a differentiable warp for a view on the
    student's side is out of scope.

    The record table lives in device memory at a fixed address and is written from the host before the iteration (``draw``), from
    an RNG state this object owns -- seeded from ``seed`` and ``rank``; the global RNG is not advanced.  The warped batch, the
    back-mapped maps, the flags and the masked weights live at fixed addresses too, keyed by the signature of the operands.
    ``state_dict()`` is what the epoch checkpoint keeps as ``view_state``.  The default ranges are placeholders: their effect on
    convergence has not been measured."""

    def __init__(self, rot_deg=30.0, scale=(0.75, 1.25), shift=0.1, margin=2.0, seed=0, rank=0, image_size=None, heatmap_size=None):
        import math
        lo, hi = (float(v) for v in scale)
        if not (math.isfinite(rot_deg) and 0.0 <= rot_deg <= 180.0):
            raise ValueError('GeometricView: rot_deg must lie in 0 .. 180 degrees, got %r' % (rot_deg,))
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError('GeometricView: the scale range must be finite with 0 < lo <= hi, got %r' % (scale,))
        if not (math.isfinite(shift) and 0.0 <= shift <= 1.0):
            raise ValueError('GeometricView: shift is a fraction of the image side in 0 .. 1, got %r' % (shift,))
        if not (math.isfinite(margin) and margin >= 0.0):
            raise ValueError('GeometricView: margin must be finite and not negative, got %r' % (margin,))
        self.rot_deg, self.scale, self.shift, self.margin = float(rot_deg), (lo, hi), float(shift), float(margin)
        self.seed, self.rank = int(seed or 0), int(rank)
        self._rng = self._seeded(0)
        self.draws = 0
        self.image_size = None if image_size is None else _pair(image_size)
        self.heatmap_size = None if heatmap_size is None else _pair(heatmap_size)
        self.recs = None                 # (B * 18,) fp32 on the device, fixed address
        self.recs_host = None            # the records of the last draw, (B, 18) fp32
        self.params_host = None          # the last draw: (B, 4) float64 angle (degrees), scale, tx, ty (image pixels)
        self._bufs = {}

    # ------------------------------------------------------------ draws
    def draw(self, B=None, device=None, image_size=None, heatmap_size=None):
        """Draw the views of the coming iteration and write their records to the device (host work: outside graph capture).
        Returns the (B, 4) draws: angle in degrees, scale, shift in image pixels."""
        if image_size is not None:
            self.image_size = _pair(image_size)
        if heatmap_size is not None:
            self.heatmap_size = _pair(heatmap_size)
        if self.recs is None or (B is not None and self.recs.numel() != int(B) * ops.VIEW_REC_FLOATS):
            if B is None:
                raise RuntimeError('GeometricView: run one eager iteration before replaying graphs')
            if torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise Mi355Error('GeometricView: the record table would be allocated during graph capture; run one eager iteration first')
            self.recs = torch.zeros(int(B) * ops.VIEW_REC_FLOATS, dtype=torch.float32, device=device)
        if self.image_size is None or self.heatmap_size is None:
            raise RuntimeError('GeometricView: draw() needs image_size and heatmap_size the first time')
        n = self.recs.numel() // ops.VIEW_REC_FLOATS
        with torch.random.fork_rng(devices=[]):          # the global CPU generator is put back as it was
            torch.set_rng_state(self._rng)
            u = torch.rand(n, 4, dtype=torch.float64).numpy()
            self._rng = torch.get_rng_state()
        self.draws += 1
        H, W = self.image_size
        lo, hi = self.scale
        p = u.copy()
        p[:, 0] = (2.0 * u[:, 0] - 1.0) * self.rot_deg
        p[:, 1] = lo + (hi - lo) * u[:, 1]
        p[:, 2] = (2.0 * u[:, 2] - 1.0) * self.shift * W
        p[:, 3] = (2.0 * u[:, 3] - 1.0) * self.shift * H
        self.params_host = p
        self.recs_host = ops.view_records(p[:, 0], p[:, 1], p[:, 2:], self.image_size, self.heatmap_size)   # (refuses non-finite, s <= 0)
        self.recs.copy_(torch.from_numpy(self.recs_host).view(-1), non_blocking=True)
        return p

    def _seeded(self, draws):
        """The generator state of a rank that starts (draws = 0) or joins a resumed run whose checkpoint holds another rank's state."""
        return torch.Generator().manual_seed(self.seed * 1000003 + 7907 * self.rank + 29 + 104723 * int(draws)).get_state()

    def state_dict(self):
        """The RNG state, the number of draws so far and the last draws (a CPU copy): what the checkpoint keeps."""
        return {'rng_state': self._rng.clone(), 'draws': self.draws, 'rank': self.rank,
                'ranges': (self.rot_deg, self.scale, self.shift, self.margin),
                'params': None if self.params_host is None else torch.from_numpy(self.params_host.copy())}

    def load_state_dict(self, state):
        """Go on where the saved run was.  The checkpoint is rank 0's: another rank takes the number of draws and a state seeded
        from (seed, rank, draws), so that the ranks keep drawing different views."""
        self.draws = int(state.get('draws', 0))
        if int(state.get('rank', 0)) == self.rank:
            self._rng = state['rng_state'].clone().to(torch.uint8).cpu()
        else:
            self._rng = self._seeded(self.draws)

    # ------------------------------------------------------------ the two warps
    def _buffers(self, key, shapes, device):
        got = self._bufs.get(key[0])
        if got is None or got[0] != key:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise Mi355Error('GeometricView: the %s buffers would be allocated during graph capture; run one eager iteration first' % key[0])
            got = self._bufs[key[0]] = (key, tuple(None if s is None else torch.empty(s, dtype=torch.float32, device=device) for s in shapes))
        return got[1]

    def _check(self, what, t, size, which):
        if self.recs is None:
            raise Mi355Error('GeometricView: no records: draw() first')
        if t.dim() != 4 or t.shape[0] * ops.VIEW_REC_FLOATS != self.recs.numel() or tuple(t.shape[-2:]) != size:
            raise Mi355Error('GeometricView: %s of shape %s, the records were drawn for %d samples and a %s of %s'
                             % (what, tuple(t.shape), self.recs.numel() // ops.VIEW_REC_FLOATS, which, size))

    def apply(self, x):
        """The teacher's input: x (B, C, H, W) under the views of the last draw, in a buffer of this object."""
        x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
        self._check('a batch', x, self.image_size, 'image size')
        out, = self._buffers(('apply', tuple(x.shape)), (tuple(x.shape),), x.device)
        return ops.affine_warp_images(x, self.recs, out=out)

    def undo(self, y, w_in=None):
        """(y_hat, valid, w_out): the teacher's heat-maps y (B, K, h, w) mapped back to the loader's frame, the per-map flags (B, K)
        and w_in * valid in w_in's shape (None without w_in), in buffers of this object."""
        f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        y = f32(y.detach())
        self._check('heat-maps', y, self.heatmap_size, 'heat-map size')
        if w_in is not None:
            w_in = f32(w_in)
        B, K = y.shape[:2]
        key = ('undo', tuple(y.shape), None if w_in is None else tuple(w_in.shape))
        out = self._buffers(key, (tuple(y.shape), (B, K), None if w_in is None else tuple(w_in.shape)), y.device)
        return ops.affine_unwarp_heatmaps(y, self.recs, self.margin, w_in=w_in, out=out)


class KeypointOcclusion:
    """What ``DAStep(occlude=...)`` takes: the student's view of the target batch with a square patch around up to ``n`` of the key
    points the teacher is sure of set to the data-set mean (0 in normalised space), with probability ``prob`` per sample (the
    adaptive occlusion of Kim et al., ECCV 2022; the patch rule is this project's -- PAPERS.md).  ``size`` = (lo, hi) are the
    smallest and the largest side of a patch as fractions of the image side.  A joint is a candidate when the peak of
    ``softmax(beta * y)`` of the teacher's map reaches the step's ``teacher_conf`` (and, under a geometric view, the map is valid,
    and its weight is positive).  ``select(y, ...)`` is ``mi355_peak_prob`` + ``mi355_teacher_select``, ``apply(x)``
    ``mi355_occlude_images``; with ``n = 0`` it only gates (``DAStep(teacher_conf=...)`` without occlusion).

    The draw table lives in device memory at a fixed address and is written from the host before the iteration (``draw``), from an
    RNG state this object owns -- seeded from ``seed`` and ``rank``; the global RNG is not advanced.  The peaks, the flags, the
    boxes, the counts and the occluded batch live at fixed addresses too, keyed by the signature of the operands.
    ``state_dict()`` is what the epoch checkpoint keeps as ``occlude_state``.  Every default is a placeholder: its effect on
    convergence has not been measured."""

    def __init__(self, prob=0.5, n=1, size=(0.08, 0.16), beta=1.0, seed=0, rank=0):
        import math
        lo, hi = (float(v) for v in size)
        if not (isinstance(prob, (int, float)) and 0.0 <= prob <= 1.0):
            raise ValueError('KeypointOcclusion: prob must lie in 0 .. 1, got %r' % (prob,))
        if isinstance(n, bool) or int(n) != n or not 0 <= n <= ops.OCC_MAX_BOXES:
            raise ValueError('KeypointOcclusion: n must be a whole number in 0 .. %d, got %r' % (ops.OCC_MAX_BOXES, n))
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi <= 1.0):
            raise ValueError('KeypointOcclusion: the size range is given as fractions of the image side, 0 < lo <= hi <= 1, got %r' % (size,))
        if not (math.isfinite(beta) and beta > 0.0):
            raise ValueError('KeypointOcclusion: beta must be finite and positive, got %r' % (beta,))
        self.prob, self.n, self.size, self.beta = float(prob), int(n), (lo, hi), float(beta)
        self.seed, self.rank = int(seed or 0), int(rank)
        self._rng = self._seeded(0)
        self.draws = 0
        self.u = None                    # (B, 1 + 2n) fp32 on the device, fixed address
        self.u_host = None               # the table of the last draw
        self.stats = None                # two fp32 on the device: mean boxes per sample, mean of conf
        self.p = self.xy = self.conf = self.w_out = self.boxes = self.count = self.x_occ = None
        self._bufs = {}

    def sides(self, S):
        """(lo, hi) in pixels of an image of side S: the fractions rounded to whole pixels, at least one pixel."""
        lo, hi = (max(1, min(int(S), int(round(f * S)))) for f in self.size)
        return lo, max(lo, hi)

    # ------------------------------------------------------------ draws
    def draw(self, B=None, device=None):
        """Draw the table of the coming iteration and write it to the device (host work: outside graph capture).  Returns the
        (B, 1 + 2n) float32 draws; nothing is drawn with n = 0."""
        if self.n == 0:
            return None
        if self.u is None or (B is not None and self.u.shape[0] != int(B)):
            if B is None:
                raise RuntimeError('KeypointOcclusion: run one eager iteration before replaying graphs')
            if torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise Mi355Error('KeypointOcclusion: the draw table would be allocated during graph capture; run one eager iteration first')
            self.u = torch.zeros(int(B), 1 + 2 * self.n, dtype=torch.float32, device=device)
        with torch.random.fork_rng(devices=[]):          # the global CPU generator is put back as it was
            torch.set_rng_state(self._rng)
            u = torch.rand(tuple(self.u.shape), dtype=torch.float32)      # in [0, 1): at most 1 - 2^-24
            self._rng = torch.get_rng_state()
        self.draws += 1
        self.u_host = u
        self.u.copy_(u, non_blocking=True)
        return u

    def _seeded(self, draws):
        """The generator state of a rank that starts (draws = 0) or joins a resumed run whose checkpoint holds another rank's state."""
        return torch.Generator().manual_seed(self.seed * 1000003 + 7927 * self.rank + 41 + 104743 * int(draws)).get_state()

    def state_dict(self):
        """The RNG state and the number of draws so far, what the run goes on from; `ranges` = (prob, n, size, beta), which
        load_state_dict compares with this object's; `u`, the last table (a CPU copy), is a record for whoever reads the checkpoint
        and is not read back: the next draw replaces it."""
        return {'rng_state': self._rng.clone(), 'draws': self.draws, 'rank': self.rank,
                'ranges': (self.prob, self.n, self.size, self.beta),
                'u': None if self.u_host is None else self.u_host.clone()}

    def load_state_dict(self, state):
        """Go on where the saved run was.  The checkpoint is rank 0's: another rank takes the number of draws and a state seeded
        from (seed, rank, draws), so that the ranks keep drawing different boxes.  A checkpoint written with another prob, n, size
        or beta is loaded with a warning: the run goes on, but not as the saved one would have (another n is another table shape,
        so other draws from the same RNG state)."""
        saved, mine = state.get('ranges'), (self.prob, self.n, self.size, self.beta)
        if saved is not None and (float(saved[0]), int(saved[1]), tuple(float(v) for v in saved[2]), float(saved[3])) != mine:
            import warnings
            warnings.warn('KeypointOcclusion: the checkpoint was written with (prob, n, size, beta) = %r, this run has %r: the resumed '
                          'run will not draw the boxes the saved run would have' % (tuple(saved), mine))
        self.draws = int(state.get('draws', 0))
        if int(state.get('rank', 0)) == self.rank:
            self._rng = state['rng_state'].clone().to(torch.uint8).cpu()
        else:
            self._rng = self._seeded(self.draws)

    # ------------------------------------------------------------ the three launches
    def _buffers(self, key, specs, device):
        got = self._bufs.get(key[0])
        if got is None or got[0] != key:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise Mi355Error('KeypointOcclusion: the %s buffers would be allocated during graph capture; run one eager iteration first' % key[0])
            got = self._bufs[key[0]] = (key, tuple(None if s is None else torch.empty(s[0], dtype=s[1], device=device) for s in specs))
        return got[1]

    def select(self, y, tau, image_side, gate_in=None, w_in=None):
        """The gate and the boxes from the teacher's heat-maps y (B, K, H, W): sets and returns (conf, w_out); `boxes` and `count`
        are kept for apply().  tau: the confidence threshold; gate_in: the flags of a geometric view; w_in: the joint weights."""
        f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        y = f32(y.detach())
        B, K = y.shape[:2]
        if w_in is not None:
            w_in = f32(w_in)
        if gate_in is not None:
            gate_in = f32(gate_in)
        n = self.n
        if n > 0 and (self.u is None or self.u.shape[0] != B):
            raise Mi355Error('KeypointOcclusion: no draws for a batch of %d: draw() first' % B)
        i32 = torch.int32
        key = ('select', tuple(y.shape), None if w_in is None else tuple(w_in.shape), n)
        bufs = self._buffers(key, (((B, K), i32), ((B, K, 2), torch.float32), ((B, K), torch.float32), ((B, K), torch.float32),
                                   None if w_in is None else (tuple(w_in.shape), torch.float32),
                                   None if n == 0 else ((B, n, 4), i32), None if n == 0 else ((B,), i32), ((2,), torch.float32)), y.device)
        idx, self.xy, self.p, conf, w_out, boxes, count, self.stats = bufs
        ops.peak_prob(y, self.beta, out=(idx, self.xy, self.p))
        lo, hi = self.sides(image_side) if n > 0 else (1, 1)
        self.conf, self.w_out, self.boxes, self.count = ops.teacher_select(
            self.p, self.xy, self.u if n > 0 else None, tau, self.prob, n, lo, hi, int(image_side) if n > 0 else 1, tuple(y.shape[-2:]),
            gate_in=gate_in, w_in=w_in, out=(conf, w_out, boxes, count), stats=self.stats)
        return self.conf, self.w_out

    def apply(self, x):
        """The student's input: x (B, C, S, S) with the boxes of the last select() blanked, in a buffer of this object."""
        if self.boxes is None:
            raise Mi355Error('KeypointOcclusion: no boxes: select() first (n = %d)' % self.n)
        x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
        out, = self._buffers(('apply', tuple(x.shape)), ((tuple(x.shape), torch.float32),), x.device)
        self.x_occ = ops.occlude_images(x, self.boxes, out=out)
        return self.x_occ


class InIterationTeacher:
    def __init__(self, ema, view=None):
        self.ema, self.model = ema, ema.model_ema
        # optional GeometricView (may also be assigned later): the teacher runs on view.apply(x) and forward() returns its
        # heat-maps mapped back (view.undo), keeping the flags in `valid` and the masked weights in `w_out`.  None: x as it is.
        self.view, self.valid, self.w_out = view, None, None
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

    def forward(self, x, w_in=None):
        """y_t_ema = model_ema(x)[0]: eval mode, running statistics, no_grad (train1.py:364).  With a view: the teacher runs on
        view.apply(x) and its heat-maps come back mapped to x's frame; `valid` and `w_out` (= w_in * valid) are kept."""
        if self.view is not None:
            x = self.view.apply(x)
        if self._pairs is None:
            self._build(x)
            self.refresh()
        y = self._run(x)
        if self.view is None:
            return y
        y, self.valid, self.w_out = self.view.undo(y, w_in)
        return y

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
        y_ema = step.teacher_forward(self.teacher, batch)
        if not torch.cuda.is_current_stream_capturing():
            self.sync(y_t_grad.shape)
        # with a geometric view the maps whose peak the teacher did not see inside its frame are left out (weight 0), with
        # teacher_conf > 0 those the teacher is not sure of; weight_t stays ignored, as in the reference's mt_loss
        return self.loss(y_t_grad, y_ema, wmap=step.teacher_map_weights(self.teacher)), \
            {'y_t_ema': y_ema}                                   # (kept: step M's teacher labels reuse this forward)
