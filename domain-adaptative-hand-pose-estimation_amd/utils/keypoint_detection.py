"""Key-point decode and PCK (reference ``utils/keypoint_detection.py``): ``get_max_preds`` (:7-35),
``calc_dists`` / ``dist_acc`` / ``accuracy`` (:38-92), ``compute_uv_from_heatmaps3`` (:209-239).

The reference works on numpy arrays after a device->host copy of whole heat-maps.  Here the arg-max runs
on the GPU (bit-exact with numpy's first-max rule) and only the (B,K,2) coordinates travel:
numpy inputs are accepted for API parity (uploaded once), torch CUDA tensors avoid the copy."""
import numpy as np
import torch

from mi355 import ops


def _to_dev(hm):
    if isinstance(hm, np.ndarray):
        assert hm.ndim == 4, 'batch_images should be 4-ndim'
        return torch.from_numpy(np.ascontiguousarray(hm, dtype=np.float32)).cuda()
    assert torch.is_tensor(hm) and hm.dim() == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    return hm.detach()


def get_max_preds_device(batch_heatmaps):
    """(preds (B,K,2) fp32 [x,y], maxvals (B,K,1)) as device tensors; no synchronisation."""
    _, xy, mv = ops.argmax2d(_to_dev(batch_heatmaps))
    return xy, mv


def get_max_preds(batch_heatmaps):
    """get predictions from score maps; returns numpy (preds, maxvals) like the reference."""
    xy, mv = get_max_preds_device(batch_heatmaps)
    return xy.cpu().numpy(), mv.cpu().numpy()


def calc_dists(preds, target, normalize):
    preds = preds.astype(np.float32)
    target = target.astype(np.float32)
    dists = np.zeros((preds.shape[1], preds.shape[0]))
    ok = (target[:, :, 0] > 1) & (target[:, :, 1] > 1)
    d = np.linalg.norm(preds / normalize[:, None, :] - target / normalize[:, None, :], axis=2)
    dists[:] = np.where(ok, d, -1).T
    return dists


def dist_acc(dists, thr=0.5):
    """Return percentage below threshold while ignoring values with a -1"""
    dist_cal = np.not_equal(dists, -1)
    num_dist_cal = dist_cal.sum()
    if num_dist_cal > 0:
        return np.less(dists[dist_cal], thr).sum() * 1.0 / num_dist_cal
    return -1


def accuracy_from_preds(pred, target_pred, h, w, thr=0.5):
    """PCK from decoded coordinates: pred / target_pred (B,K,2) numpy arg-max positions of the h x w heat-maps.
    Returns (per-keypoint acc, average acc, count, pred) -- the arithmetic of ``accuracy`` after its two decodes."""
    norm = np.ones((pred.shape[0], 2)) * np.array([h, w]) / 10
    dists = calc_dists(pred, target_pred, norm)
    K = pred.shape[1]
    acc = np.zeros(K)
    avg_acc, cnt = 0, 0
    for i in range(K):
        acc[i] = dist_acc(dists[i], thr)
        if acc[i] >= 0:
            avg_acc += acc[i]
            cnt += 1
    avg_acc = avg_acc / cnt if cnt != 0 else 0
    return acc, avg_acc, cnt, pred


def accuracy(output, target, hm_type='gaussian', thr=0.5):
    """PCK on heat-maps (ground-truth heat-map arg-max as the label), reference :63-92.
    Returns (per-keypoint acc, average acc, count, pred (B,K,2))."""
    pred, _ = get_max_preds(output)
    tgt, _ = get_max_preds(target)
    return accuracy_from_preds(pred, tgt, output.shape[2], output.shape[3], thr)


def compute_uv_from_heatmaps3(heatmap: torch.Tensor) -> torch.Tensor:
    """Soft-arg-max: softmax(100*hm) expectation of (column, row), times 4 (reference :209-239)."""
    return ops.softargmax(heatmap.detach(), beta=100.0, out_scale=4.0)


# ---------------------------------------------------------------- evaluation at image resolution
def compute_uv_from_heatmaps2(hm, resize_dim):
    """Arg-max of the heat-maps up-sampled bilinearly to ``resize_dim`` (reference :172-205): (B,K,2) fp32 [x,y] in pixels of
    that size on the device, zero where the maximum is not positive.  One launch, no up-sampled maps in memory, no
    synchronisation."""
    return ops.upsample_argmax(_to_dev(hm), resize_dim)[1]


def decode_keypoints(y, image_size, mode='argmax', with_maxval=False, y_flip=None, flip_shift=1, sigma=2.0, return_avg=False):
    """Key points in image pixels from heat-maps y (B,K,h,w), on the device.  ``argmax``: the heat-map arg-max times
    image_size / heatmap_size (the scaling the reference's ``visualize`` uses); ``upsample``: compute_uv_from_heatmaps2 at
    size = image_size; ``quarter``: the arg-max moved a quarter heat-map pixel towards its higher neighbour (Simple Baselines /
    HRNet ``get_final_preds``); ``taylor``: DARK's second-order step on the log of the map smoothed by a Gaussian of ``sigma``
    (exact for the Gaussian labels the network is trained on), both times the same scaling.

    ``y_flip``: the heat-maps of the mirrored images (flip test).  They are mirrored back, moved ``flip_shift`` columns to the
    right (1: Simple Baselines' SHIFT_HEATMAP, which puts the two peaks a quarter heat-map pixel either side of the truth
    instead of three quarters to one side) and averaged with ``y`` in the decode's own launch; ``upsample`` averages first and
    decodes the average.  No joint pairs are swapped: a single hand has no left / right pairs.  ``return_avg`` appends the
    map that was decoded (``y`` itself without ``y_flip``).  Without ``y_flip``, ``argmax`` and ``upsample`` launch what they
    always did."""
    y = _to_dev(y)
    if mode not in ('argmax', 'upsample', 'quarter', 'taylor'):
        raise ValueError("decode mode must be 'argmax', 'upsample', 'quarter' or 'taylor', got %r" % (mode,))
    if y_flip is not None:
        y_flip = _to_dev(y_flip)
    scale = (float(image_size) / float(y.shape[3]), float(image_size) / float(y.shape[2]))
    avg = y
    if mode == 'upsample':
        if y_flip is not None:
            avg = ops.flip_decode(y, y_flip, flip_shift, 'argmax', want_avg=True)[3]
        _, xy, mv = ops.upsample_argmax(avg, image_size)
    elif mode == 'argmax' and y_flip is None:
        _, xy, mv = ops.argmax2d(y)
        xy = xy * (float(image_size) / float(y.shape[3]))
    else:
        _, xy, mv, a = ops.flip_decode(y, y_flip, flip_shift, mode, sigma, scale, want_avg=return_avg and y_flip is not None)
        avg = a if a is not None else y
    out = (xy, mv) if with_maxval else (xy,)
    if return_avg:
        out = out + (avg,)
    return out if len(out) > 1 else out[0]


def _trapz(y, x):
    """np.trapz's arithmetic (numpy 2 renamed the function)."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


class PoseMetrics:
    """End-point error in pixels and the PCK curve with its AUC over ``linspace(0, max_px, steps)`` (the RHD / STB 2-D
    protocol: 0 - 30 px), accumulated on the device: mean joint distance as the reference's ``accuracy_2d`` (:128-136) over the
    visible joints, thresholded curve and trapezoid AUC as its ``accuracy_3d`` (:95-126).  ``update`` launches one kernel and
    does not synchronise; ``result`` reads the device once."""

    def __init__(self, num_keypoints, max_px=30.0, steps=31, device='cuda'):
        self.K, self.max_px = int(num_keypoints), float(max_px)
        self.thresholds = np.linspace(0.0, self.max_px, int(steps)).astype(np.float32)
        self.device = torch.device(device)
        self._state = None
        if self.device.type == 'cuda':
            self.thr_dev = torch.from_numpy(self.thresholds).to(self.device)
            self._state = ops.pose_metrics_state(self.K, len(self.thresholds), self.device)

    def update(self, pred, gt, vis):
        """pred, gt (B,K,2) in pixels, vis (B,K) or (B,K,1): a joint counts where vis > 0."""
        ops.pose_metrics(pred, gt, vis, self.thr_dev, self._state)

    def state(self, reduce=None):
        """(sum_err float64 [K], count int64 [K], hits int64 [K,T]) as numpy: one device read.  ``reduce``: called with the three
        device accumulators packed into one float64 tensor before the read (the all-reduce over ranks; every value is an integer
        or a float64 sum, so the packing is exact)."""
        s, c, h = self._state
        flat = torch.cat([s, c.double(), h.double().reshape(-1)])
        if reduce is not None:
            reduce(flat)
        flat = flat.cpu().numpy()
        K, T = self.K, len(self.thresholds)
        return flat[:K].copy(), flat[K:2 * K].astype(np.int64), flat[2 * K:].astype(np.int64).reshape(K, T)

    def result(self, groups=None, reduce=None, state=None):
        """{'epe', 'epe_<group>' per entry of ``groups`` (name -> joint indices), 'pck_curve', 'auc', 'thresholds'}.  A data set
        with no visible joint gives nan.  ``state``: accumulators to evaluate instead of the device's."""
        sum_err, count, hits = self.state(reduce) if state is None else state
        sum_err, count, hits = np.asarray(sum_err, np.float64), np.asarray(count, np.int64), np.asarray(hits, np.int64)
        with np.errstate(divide='ignore', invalid='ignore'):
            n = np.float64(count.sum())
            out = {'epe': float(sum_err.sum() / n)}
            for name, ks in (groups or {}).items():
                ks = list(ks)
                out['epe_' + name] = float(sum_err[ks].sum() / np.float64(count[ks].sum()))
            out['pck_curve'] = hits.sum(0) / n
        thr = self.thresholds.astype(np.float64)
        out['auc'] = _trapz(out['pck_curve'], thr) / self.max_px
        out['thresholds'] = self.thresholds
        return out
