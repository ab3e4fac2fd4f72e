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
