"""Forward-only path (``test.py`` / ``validate()``, reference train1.py:495-536): ``model(x)`` of a fixed input shape replayed
from a HIP graph.  Eager, one forward of the pose network is ~120 launches that the host needs longer to enqueue than the GPU
needs to run; replayed it is one graph launch.  ``FlipForward`` is the flip test's forward (the batch and its mirror images in one
graph) and ``PosePredictor`` the one-call interface on top: normalised images in, key points in image pixels out."""
import torch

from . import compute_dtype, fp8_convs, graph_capture_mode, mx_eval, nn as _nn, no_gc_in_capture


class GraphedForward:
    """``y = GraphedForward(model)(x)``: eval-mode, no-grad forwards are captured per input shape after ``warmup`` eager calls
    (they allocate the workspaces and fold the BatchNorms into the convs) and replayed from then on; anything else (training
    mode, gradients enabled) goes to ``model(x)``.  The graphs are dropped when a parameter, a buffer or a running statistic
    changes (training resumed, ``load_state_dict``) or the compute dtype or the MX inference switch does
    (``mi355.set_compute_dtype``, ``mi355.set_mx_eval``: the graphs hold the packed weights and kernels of the setting they were
    captured under).  The returned tensor is a copy: it stays valid across calls."""

    def __init__(self, model, warmup=2):
        self.model, self.warmup = model, warmup
        self._graphs, self._seen, self._stamp = {}, {}, None

    def _state_stamp(self):
        v = _nn._BN_GEN[0]
        for t in self.model.parameters():
            v = v * 1000003 + t._version + getattr(t, '_mi_epoch', 0)
        for t in self.model.buffers():
            v = v * 1000003 + t._version
        return v & ((1 << 62) - 1), compute_dtype(), fp8_convs(), mx_eval()

    def __call__(self, x):
        if self.model.training or torch.is_grad_enabled() or not x.is_cuda:
            return self.model(x)
        stamp = self._state_stamp()
        if stamp != self._stamp:
            self._graphs.clear(); self._seen.clear(); self._stamp = stamp
        key = (tuple(x.shape), x.dtype, x.device)
        ent = self._graphs.get(key)
        if ent is None:
            n = self._seen[key] = self._seen.get(key, 0) + 1
            if n <= self.warmup:
                return self.model(x)
            sx = x.clone()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with no_gc_in_capture(), torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
                sy = self.model(sx)
            ent = self._graphs[key] = (g, sx, sy)
        g, sx, sy = ent
        sx.copy_(x, non_blocking=True)
        g.replay()
        return sy.clone()


class FlipForward:
    """``y, y_flip = FlipForward(model)(x)``: the flip test's forward -- the heat-maps of x (B,C,H,W) and of its images mirrored
    along W, from ONE forward of the 2B batch that ``ops.mirror_batch`` builds, through a ``GraphedForward`` (one graph per
    input shape; the ragged last batch of a data set runs eagerly, as without the flip).  ``y_flip`` is NOT mirrored back:
    ``ops.flip_decode`` / ``decode_keypoints(..., y_flip=)`` do that while they average."""

    def __init__(self, model, warmup=2):
        self.forward = GraphedForward(model, warmup)

    def __call__(self, x):
        from . import ops
        y2 = self.forward(ops.mirror_batch(x))
        B = x.shape[0]
        return y2[:B], y2[B:]


class PosePredictor:
    """``xy, maxval = PosePredictor(model, image_size)(x)``: key points (B,K,2) fp32 [x, y] in pixels of the image_size x
    image_size network input and their heat-map maxima (B,K,1), on the device, for a batch x (B,3,image_size,image_size) of
    normalised images.  ``decode``: 'argmax' | 'upsample' | 'quarter' | 'taylor' (``utils.keypoint_detection.decode_keypoints``);
    ``flip_test``: average with the heat-maps of the mirrored images (``flip_shift``: see there); ``sigma``: the Gaussian of the
    training labels, used by 'taylor'.  The model is put in eval mode; forwards of a repeated batch shape replay a HIP graph.
    No joint pairs are swapped on the flip: a single hand has none."""

    def __init__(self, model, image_size, decode='taylor', flip_test=True, flip_shift=1, sigma=2.0):
        if decode not in ('argmax', 'upsample', 'quarter', 'taylor'):
            raise ValueError("decode must be 'argmax', 'upsample', 'quarter' or 'taylor', got %r" % (decode,))
        if flip_shift not in (0, 1):
            raise ValueError('flip_shift must be 0 or 1, got %r' % (flip_shift,))
        self.model, self.image_size, self.decode = model.eval(), int(image_size), decode
        self.flip_test, self.flip_shift, self.sigma = bool(flip_test), int(flip_shift), float(sigma)
        self.forward = FlipForward(model) if self.flip_test else GraphedForward(model)

    def __call__(self, x):
        from utils.keypoint_detection import decode_keypoints
        with torch.no_grad():
            y, y_flip = self.forward(x) if self.flip_test else (self.forward(x), None)
            return decode_keypoints(y, self.image_size, self.decode, with_maxval=True, y_flip=y_flip, flip_shift=self.flip_shift,
                                    sigma=self.sigma)


class HandTracker:
    """From camera frames and rough hand boxes to key points in the frame, following each hand from frame to frame without the
    host: ``tracker.reset(boxes)`` once, then ``kp, vis, score, live, boxes = tracker.step(frames)`` per frame.

    The boxes live in device memory as ``max_hands`` records (``ops.TRACK_REC_DTYPE``, ``tracker.recs``) at a fixed address.  One
    step is the chain ``ops.roi_crop_normalize`` (crop, resize, mirror, normalise from the uint8 frame) -> ``ops.mirror_batch``
    (with ``flip_test``) -> ``model`` -> the sub-pixel decode (``decode_keypoints``, ``PosePredictor``'s: the key points in crop
    pixels are its, bit for bit) -> ``ops.peak_prob`` on the decoded (averaged) maps, the confidence being the peak of
    softmax(conf_beta * y) as ``--teacher-conf`` defines it -> ``ops.track_update`` in place: key points mapped back to the frame,
    and the next box.  After ``warmup`` eager calls the chain is captured once per frame-batch shape -- a single-stream chain, no
    parallel branches -- and replayed: the host copies the frames in and launches one graph.  The graphs are dropped by the state
    stamp of ``GraphedForward``.

    ``model``: any callable that maps (B, 3, S, S) normalised fp32 images to (B, K, h, w) fp32 heat-maps (a module is put in eval
    mode).  ``frame_shape``: (Hf, Wf).  ``frames``: a uint8 (F, Hf, Wf, 3) RGB device tensor; a record's ``frame`` says which of
    the F frames its hand is in.  Track parameters (``ops.TRACK_DEFAULTS``): scale = 1.5 is the data sets' crop; tau, min_joints,
    alpha, grow, max_lost and min_side are PLACEHOLDERS whose effect has not been measured.

    ``step`` does not synchronise.  kp (N, K, 2) are frame pixels, vis (N, K) and score (N,) as ``ops.track_update`` writes them;
    live (N,) bool and boxes (N, 4) = (x0, y0, x1, y1) are the records AFTER the update: the squares the next frame is cropped by.
    Under replay the five tensors are the graph's own: valid until the next ``step``, clone what must be kept."""

    def __init__(self, model, image_size, frame_shape, max_hands, decode='taylor', flip_test=True, conf_beta=1.0, flip_shift=1, sigma=2.0,
                 warmup=2, graph=True, **track_params):
        from . import ops
        if decode not in ('argmax', 'upsample', 'quarter', 'taylor'):
            raise ValueError("decode must be 'argmax', 'upsample', 'quarter' or 'taylor', got %r" % (decode,))
        if int(max_hands) < 1:
            raise ValueError('max_hands must be at least 1, got %r' % (max_hands,))
        if not float(conf_beta) > 0:
            raise ValueError('conf_beta must be positive, got %r' % (conf_beta,))
        self.model = model.eval() if hasattr(model, 'eval') else model
        self.image_size, self.max_hands = int(image_size), int(max_hands)
        self.frame_shape = tuple(int(v) for v in frame_shape)
        self.decode, self.flip_test, self.flip_shift, self.sigma = decode, bool(flip_test), int(flip_shift), float(sigma)
        self.conf_beta, self.warmup, self.graph = float(conf_beta), int(warmup), bool(graph)
        self.track = dict(ops.TRACK_DEFAULTS, **track_params)
        self.params = ops.track_params(self.frame_shape, self.image_size, **track_params)
        self.recs = None                       # int32 (max_hands, 8) on the device, made by reset()
        self._bufs, self._graphs, self._seen, self._stamp = {}, {}, {}, None
        self._stamper = GraphedForward(model) if isinstance(model, torch.nn.Module) else None

    # ---- records
    def _records(self, boxes, mirror, frame_index):
        """TRACK_REC_DTYPE records of (x0, y0, x1, y1) boxes: squared and scaled by `scale` the way scale_box does (without its
        rounding to whole pixels), capped by the frame and 4 S, shifted inside the frame.  Unused slots get live = 0."""
        import numpy as np
        from . import ops
        boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        n, N = len(boxes), self.max_hands
        if n > N:
            raise ValueError('%d boxes for max_hands=%d' % (n, N))
        if n and (not np.isfinite(boxes).all() or (boxes[:, 2] <= boxes[:, 0]).any() or (boxes[:, 3] <= boxes[:, 1]).any()):
            raise ValueError('boxes must be finite (x0, y0, x1, y1) with x1 > x0 and y1 > y0, got %s' % (boxes.tolist(),))
        Hf, Wf = self.frame_shape
        cap = float(min(Wf, Hf, 4 * self.image_size))
        rec = ops.track_records(N)
        side = np.minimum(np.maximum(self.track['scale'] * np.maximum(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]), min(self.track['min_side'], cap)), cap)
        cx, cy = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
        rec['x0'][:n] = np.minimum(np.maximum(cx - side / 2, 0.0), Wf - side)
        rec['y0'][:n] = np.minimum(np.maximum(cy - side / 2, 0.0), Hf - side)
        rec['side'][:n], rec['live'][:n] = side, 1
        rec['mirror'][:n] = 0 if mirror is None else np.asarray(mirror).astype(bool).astype(np.int32).reshape(-1)[:n]
        rec['frame'][:n] = 0 if frame_index is None else np.asarray(frame_index, dtype=np.int32).reshape(-1)[:n]
        return rec

    def reset(self, boxes, mirror=None, frame_index=None, device=None):
        """Start tracking the hands inside `boxes` ((n, 4) as (x0, y0, x1, y1) in frame pixels, n <= max_hands); mirror: per box,
        true for a hand the network must see flipped (a left hand); frame_index: per box, the frame of the batch it is in."""
        from . import ops
        rec = self._records(boxes, mirror, frame_index)
        if self.recs is None:
            self.recs = ops.pack_track_records(rec, device if device is not None else torch.device('cuda', torch.cuda.current_device()))
        else:
            ops.pack_track_records(rec, out=self.recs)
        return self

    # ---- the chain
    def _state_stamp(self):
        return self._stamper._state_stamp() if self._stamper is not None else (0, compute_dtype(), fp8_convs(), mx_eval())

    def _buffers(self, dev, K):
        b = self._bufs.get((dev, K))
        if b is None:
            N, S = self.max_hands, self.image_size
            mk = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
            b = self._bufs[(dev, K)] = dict(idx=mk((N, K), torch.int32), pxy=mk((N, K, 2)), p=mk((N, K)), kp=mk((N, K, 2)), vis=mk((N, K)),
                                            score=mk((N,)), scratch=mk((N, 8), torch.int32))
        return b

    def _chain(self, frames, recs, rec_out):
        from . import ops
        from utils.keypoint_detection import decode_keypoints
        N, S = self.max_hands, self.image_size
        xb = self._bufs.get(('x', frames.device))
        if xb is None:
            xb = self._bufs[('x', frames.device)] = torch.empty((N, 3, S, S), dtype=torch.float32, device=frames.device)
        x = ops.roi_crop_normalize(frames, recs, S, out=xb)
        if self.flip_test:
            y2 = self.model(ops.mirror_batch(x))
            y, y_flip = y2[:N], y2[N:]
        else:
            y, y_flip = self.model(x), None
        xy, _, avg = decode_keypoints(y, S, self.decode, with_maxval=True, y_flip=y_flip, flip_shift=self.flip_shift, sigma=self.sigma,
                                      return_avg=True)
        K = int(xy.shape[1])
        b = self._buffers(frames.device, K)
        ops.peak_prob(avg.float().contiguous(), self.conf_beta, out=(b['idx'], b['pxy'], b['p']))
        kp, vis, score, _ = ops.track_update(recs, xy, b['p'], self.params, out=(b['kp'], b['vis'], b['score']),
                                             rec_out=b['scratch'] if rec_out is None else rec_out)
        shown = recs                                           # step(): updated in place by now; predict(): the boxes given
        f = shown[:, 1:4].view(torch.float32)
        boxes = torch.stack((f[:, 0], f[:, 1], f[:, 0] + f[:, 2], f[:, 1] + f[:, 2]), dim=1)
        self.crop_xy = xy                                      # key points in crop pixels (PosePredictor's), for inspection
        return kp, vis, score, shown[:, 5] != 0, boxes

    def _run(self, mode, frames, recs, rec_out):
        if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4
                and tuple(frames.shape[1:]) == self.frame_shape + (3,)):
            got = '%s %s' % (frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__
            raise ValueError('frames must be a uint8 (F, %d, %d, 3) device tensor, got %s' % (self.frame_shape + (got,)))
        frames = frames.contiguous()
        stamp = self._state_stamp()
        if stamp != self._stamp:
            self._graphs.clear(); self._seen.clear(); self._stamp = stamp
        key = (mode, tuple(frames.shape), frames.device)
        ent = self._graphs.get(key)
        if ent is None:
            n = self._seen[key] = self._seen.get(key, 0) + 1
            if not self.graph or n <= self.warmup:
                with torch.no_grad():
                    return self._chain(frames, recs, rec_out)
            sf = frames.clone()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with no_gc_in_capture(), torch.no_grad(), torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
                outs = self._chain(sf, recs, rec_out)          # (a capture launches nothing: the records are as they were)
            ent = self._graphs[key] = (g, sf, outs, self.crop_xy)
        g, sf, outs, self.crop_xy = ent
        sf.copy_(frames, non_blocking=True)
        g.replay()
        return outs

    def step(self, frames):
        """One frame (batch): (kp, vis, score, live, boxes) on the device, and the records moved to the next boxes."""
        if self.recs is None:
            raise RuntimeError('HandTracker.step before reset(boxes)')
        return self._run('step', frames, self.recs, self.recs)

    def predict(self, frames, boxes, mirror=None, frame_index=None):
        """The one-shot form for still images: key points of the hands inside `boxes`, as fresh tensors.  The tracker's own
        records, and so a sequence it is following, are left as they are; `boxes` in the result are the squares that were cropped."""
        from . import ops
        rec = self._records(boxes, mirror, frame_index)
        prec = self._bufs.get(('predict', frames.device))
        if prec is None:
            prec = self._bufs[('predict', frames.device)] = ops.pack_track_records(rec, frames.device)
        else:
            ops.pack_track_records(rec, out=prec)
        return tuple(t.clone() for t in self._run('predict', frames, prec, None))
