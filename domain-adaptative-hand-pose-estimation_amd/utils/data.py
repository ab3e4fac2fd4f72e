"""Endless batch source over a finite loader (API of the reference's ``utils/data.py``:
``ForeverDataIterator(loader)`` with ``next()`` and ``len()``)."""
import itertools

import torch


def _cycle_fresh(loader):
    # itertools.cycle would replay the cached first epoch; a shuffling loader must be re-iterated instead
    passes = 0
    while True:
        empty = True
        sampler = getattr(loader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):        # DistributedSampler: a new permutation for every pass over the shard
            sampler.set_epoch(passes)
        passes += 1
        for batch in loader:
            empty = False
            yield batch
        if empty:
            raise ValueError('data loader yields no batches')


class ForeverDataIterator:
    """Restarts the wrapped loader whenever it is exhausted, so training loops can draw a fixed number of
    iterations per epoch regardless of the dataset size."""

    def __init__(self, data_loader):
        self.data_loader = data_loader
        self._stream = _cycle_fresh(data_loader)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._stream)

    def __len__(self):
        return len(self.data_loader)

    def take(self, n):
        """The next n batches as a list (convenience for warm-up / tests)."""
        return list(itertools.islice(self._stream, n))


class DevicePrefetcher:
    """Host -> HBM staging off the critical path (replaces the blocking ``.to(device)`` calls of the
    reference's loop, train1.py:359-366): while the training step consumes batch i, batch i+1 is copied on a side stream
    from pinned host memory.  Tensors the loader did not pin go through persistent pinned staging buffers (two slots,
    double-buffered), so no pinned allocation happens per batch.  Non-tensor items (the ``meta`` dicts) pass through, except
    for the tensors under ``meta_keys`` (``('image_ema',)`` for the mean-teacher's view of the target batch), which are staged
    like the batch's own tensors.

    ``next()`` returns the batch with every tensor on ``device``; the consumer's stream waits on the copy event and the
    tensors are recorded on it, so the caching allocator does not recycle them early."""

    def __init__(self, iterator, device, slots=2, meta_keys=()):
        self.meta_keys = tuple(meta_keys)
        self.it = iter(iterator)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('DevicePrefetcher stages to a GPU; there is no CPU path')
        self.stream = torch.cuda.Stream(self.device)
        self.slots, self._slot = int(slots), 0
        self._staging = [dict() for _ in range(self.slots)]      # slot -> {(index, shape, dtype): pinned buffer}
        self._slot_free = [None] * self.slots                   # event: the slot's last copies have left host memory
        self._ready = None
        self._preload()

    def _to_device(self, slot, idx, t):
        if not t.is_pinned():
            key = (idx, tuple(t.shape), t.dtype)
            buf = self._staging[slot].get(key)
            if buf is None:
                buf = self._staging[slot][key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            buf.copy_(t)
            t = buf
        return t.to(self.device, non_blocking=True)

    def _stage_meta(self, slot, idx, x):
        if not self.meta_keys or not isinstance(x, dict):
            return x
        x = dict(x)
        for k in self.meta_keys:
            if torch.is_tensor(x.get(k)):
                x[k] = self._to_device(slot, (idx, k), x[k])
        return x

    def _preload(self):
        try:
            host = next(self.it)
        except StopIteration:
            self._ready = None
            return
        slot = self._slot
        self._slot = (slot + 1) % self.slots
        if self._slot_free[slot] is not None:
            self._slot_free[slot].synchronize()                 # the staging buffers of this slot are about to be rewritten
        seq = isinstance(host, (tuple, list))
        items = list(host) if seq else [host]
        with torch.cuda.stream(self.stream):
            out = [self._to_device(slot, i, x) if torch.is_tensor(x) else self._stage_meta(slot, i, x) for i, x in enumerate(items)]
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._slot_free[slot] = ev
        self._ready = (type(host)(out) if seq else out[0], ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._ready is None:
            raise StopIteration
        batch, ev = self._ready
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for x in (batch if isinstance(batch, (tuple, list)) else [batch]):
            if torch.is_tensor(x):
                x.record_stream(cur)
            elif self.meta_keys and isinstance(x, dict):
                for k in self.meta_keys:
                    if torch.is_tensor(x.get(k)) and x[k].is_cuda:
                        x[k].record_stream(cur)
        self._preload()
        return batch


# ---------------------------------------------------------------- device augmentation (train1.py --device-augment)
def ragged_collate(samples):
    """Collate of the ``DeviceAugment`` / ``DeviceResize`` data sets: (AugmentSample, key points, visibility, meta) per sample ->
    (packed uint8 (sum of h*w*3,), table int64 (B, 3) of (offset, h, w), params float64 (B, 11), key points float64 (B, K, 2),
    visibility float32 (B, K, 1), meta).  Ragged sources travel as one flat buffer, so the loader's ``pin_memory`` pins a
    single tensor per batch; ``image_ema`` (made on the GPU) is dropped from the meta dicts."""
    from torch.utils.data import default_collate
    import numpy as np
    images = [s[0] for s in samples]
    sizes = [im.pixels.size for im in images]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate([im.pixels.reshape(-1) for im in images]))
    table = torch.tensor([[int(o), im.pixels.shape[0], im.pixels.shape[1]] for o, im in zip(offsets, images)], dtype=torch.int64)
    params = torch.from_numpy(np.stack([im.params for im in images]))
    keypoints = torch.stack([s[1] for s in samples])
    visible = torch.stack([s[2] for s in samples])
    meta = default_collate([{k: v for k, v in s[3].items() if k != 'image_ema'} for s in samples])
    return packed, table, params, keypoints, visible, meta


def snap_keypoints(keypoints, heatmap_size, image_size):
    """Key points (B, K, 2) float64 -> float32 positions that generate_target_device maps to exactly the heat-map centre the
    CPU labels use (``int(kp / stride + 0.5)`` in float64, uda/dataset/util.py): the centre times the stride, or far
    outside when the CPU rule drops the joint."""
    kp = torch.as_tensor(keypoints, dtype=torch.float64)
    stride = float(image_size) / float(heatmap_size)
    v = kp / stride + 0.5
    centre = torch.trunc(v)
    snapped = centre * stride
    return torch.where(v > -1, snapped, torch.full_like(snapped, -1.0e4)).float()


class DeviceAugmentIterator:
    """Batches of ``ragged_collate`` -> the ``(x, target, weight, meta)`` batches the training loops consume, on the GPU:
    the packed sources are copied to HBM, ``mi355.augment`` produces x (and ``meta['image_ema']`` with want_ema) and
    ``utils.labels.generate_target_device`` the heat-maps from the key points.  Everything is enqueued on the current
    stream.  ``out=`` buffers: pass ``out`` (B, 3, S, S) to have x written into a preallocated tensor.

    ``geometry_only`` (validation, ``DeviceResize`` data sets): x is ``mi355.augment.resize_normalize`` of the batch -- rotate /
    crop / resize / normalise in one launch, no jitter, no blur, no ``image_ema``."""

    def __init__(self, iterator, device, image_size=256, heatmap_size=64, sigma=2, want_ema=False, out=None, geometry_only=False):
        self.it = iter(iterator)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('DeviceAugmentIterator runs the augmentation on a GPU; there is no CPU path')
        if geometry_only and want_ema:
            raise ValueError('DeviceAugmentIterator: the geometry-only mode has no image_ema (x is that image)')
        self.image_size, self.heatmap_size, self.sigma, self.want_ema, self.out = image_size, heatmap_size, sigma, want_ema, out
        self.geometry_only = geometry_only

    def __iter__(self):
        return self

    def __len__(self):
        return len(self.it)

    def __next__(self):
        from mi355.augment import augment, resize_normalize
        from utils.labels import generate_target_device
        packed, table, params, keypoints, visible, meta = next(self.it)
        packed = packed.to(self.device, non_blocking=True)
        if self.geometry_only:
            res = resize_normalize(packed, table, params, out=self.out, size=self.image_size)
        else:
            res = augment(packed, table, params, out=self.out, want_ema=self.want_ema, size=self.image_size)
        x = res[0] if self.want_ema else res
        if self.want_ema:
            meta = dict(meta, image_ema=res[1])
        kp = snap_keypoints(keypoints, self.heatmap_size, self.image_size).to(self.device, non_blocking=True)
        target, weight = generate_target_device(kp, visible.to(self.device, non_blocking=True), self.heatmap_size, self.sigma,
                                                self.image_size)
        return x, target, weight, meta


# ---------------------------------------------------------------- rendered hands (train1.py --synthetic-hands)
HAND_KEYPOINTS = 21


def record_collate(samples):
    """Collate of ``RenderedHand21``: (record, key points (21, 2) float32, visibility (21, 1) float32) per sample -> ONE uint8 tensor
    [B records | B x 21 x 2 key points | B x 21 visibilities], so that a batch is a single pinned buffer and a single copy (the
    default collate does not take numpy structured scalars).  A record is 480 bytes, so all three parts start 8-byte aligned."""
    import numpy as np
    recs = np.stack([s[0] for s in samples])
    kp = np.stack([s[1] for s in samples]).astype(np.float32, copy=False)
    vis = np.stack([s[2] for s in samples]).astype(np.float32, copy=False)
    return torch.from_numpy(np.concatenate([recs.view(np.uint8).reshape(-1), kp.view(np.uint8).reshape(-1), vis.view(np.uint8).reshape(-1)]))


class RenderedHandIterator:
    """Batches of ``record_collate`` -> the ``(x, target, weight, meta)`` batches the training and validation loops consume, on the
    GPU: the packed batch is copied from pinned host memory on a side stream while the previous one is consumed (two staging slots,
    as ``DevicePrefetcher``), ``mi355.ops.render_hands`` draws x -- and, with want_ema, ``meta['image_ema']``, the same scene without
    gain, bias and sensor noise, in the same launch -- and ``utils.labels.generate_target_device`` makes the heat-maps from the key
    points: two launches of the library per batch.  With want_keypoints ``meta['keypoint2d']`` holds the un-quantised key points
    (B, 21, 2), image pixels, on the device."""

    def __init__(self, iterator, device, image_size=256, heatmap_size=64, sigma=2, want_ema=False, want_keypoints=False):
        from mi355.ops import HAND_REC_DTYPE
        self.source = iterator
        self.it = iter(iterator)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('RenderedHandIterator renders on a GPU; there is no CPU path')
        self.image_size, self.heatmap_size, self.sigma = int(image_size), int(heatmap_size), sigma
        self.want_ema, self.want_keypoints = bool(want_ema), bool(want_keypoints)
        self.rec_bytes = HAND_REC_DTYPE.itemsize
        self.sample_bytes = self.rec_bytes + HAND_KEYPOINTS * 12
        self.stream = torch.cuda.Stream(self.device)
        self._staging, self._slot_free, self._slot = [dict(), dict()], [None, None], 0
        self._ready = None
        self._preload()

    def __iter__(self):
        return self

    def __len__(self):
        return len(self.source)

    def _preload(self):
        try:
            host = next(self.it)
        except StopIteration:
            self._ready = None
            return
        if host.dtype != torch.uint8 or host.dim() != 1 or host.numel() == 0 or host.numel() % self.sample_bytes:
            raise ValueError('RenderedHandIterator: a batch must be the flat uint8 tensor of record_collate, got %s %s' % (host.dtype, tuple(host.shape)))
        slot = self._slot
        self._slot = 1 - slot
        if self._slot_free[slot] is not None:
            self._slot_free[slot].synchronize()                 # the staging buffer of this slot is about to be rewritten
        if not host.is_pinned():
            buf = self._staging[slot].get(host.numel())
            if buf is None:
                buf = self._staging[slot][host.numel()] = torch.empty(host.numel(), dtype=torch.uint8, pin_memory=True)
            buf.copy_(host)
            host = buf
        with torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._slot_free[slot] = ev
        self._ready = (dev, ev)

    def __next__(self):
        from mi355 import ops
        from utils.labels import generate_target_device
        if self._ready is None:
            raise StopIteration
        dev, ev = self._ready
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        dev.record_stream(cur)
        self._preload()
        B, S = dev.numel() // self.sample_bytes, self.image_size
        recs = dev[:B * self.rec_bytes]
        kp = dev[B * self.rec_bytes:B * (self.rec_bytes + HAND_KEYPOINTS * 8)].view(torch.float32).view(B, HAND_KEYPOINTS, 2)
        vis = dev[B * (self.rec_bytes + HAND_KEYPOINTS * 8):].view(torch.float32).view(B, HAND_KEYPOINTS, 1)
        x = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        ema = torch.empty_like(x) if self.want_ema else None
        ops.render_hands(recs, S, out=x, out_ema=ema)
        target, weight = generate_target_device(kp, vis, self.heatmap_size, self.sigma, S)
        meta = {}
        if self.want_keypoints:
            meta['keypoint2d'] = kp
        if self.want_ema:
            meta['image_ema'] = ema
        return x, target, weight, meta
