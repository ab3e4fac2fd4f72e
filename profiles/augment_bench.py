"""Device augmentation measurements (train1.py --device-augment).

  python profiles/augment_bench.py loader [--workers 4 15] [--out FILE]
      host-side loader throughput, images/s, on a fabricated H3D_crop tree of 2048 320 x 320 JPEGs (32 batches of 64 per
      pass, so that every worker has work): the CPU chain (decode +
      Pillow augmentation + labels in the workers) against the device-augment loader (decode + parameter draw + ragged
      collate in the workers; the pixel work is left to the GPU).  No GPU needed.
  python profiles/augment_bench.py kernels
      two 64-image batches through mi355.augment (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd')]

import numpy as np
import torch


def fabricate(root, n=2048, side=320, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'H3D_crop')
    os.makedirs(os.path.join(d, 'p'), exist_ok=True)
    K = [[900.0, 0, side / 2], [0, 900.0, side / 2], [0, 0, 1.0]]
    samples = []
    yy, xx = np.mgrid[0:side, 0:side]
    for i in range(n):
        base = np.stack([128 + 100 * np.sin(xx / rng.uniform(5, 40)), 128 + 100 * np.cos(yy / rng.uniform(5, 40)), (xx + yy) % 256], 2)
        arr = np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(d, 'p/%d.jpg' % i), quality=92)
        kp = rng.uniform(side * 0.3, side * 0.7, (21, 2))
        samples.append({'name': 'p/%d.jpg' % i, 'keypoint2d': kp.tolist(), 'keypoint3d': np.hstack([kp / 900, np.ones((21, 1))]).tolist(),
                        'intrinsic_matrix': K, 'without_object': 1})
    json.dump(samples, open(os.path.join(d, 'annotation.json'), 'w'))


def loader_rate(ds, workers, collate, batch=64, batches=24):
    from torch.utils.data import DataLoader
    ld = DataLoader(ds, batch_size=batch, shuffle=True, num_workers=workers, collate_fn=collate, drop_last=True,
                    persistent_workers=workers > 0)
    it = iter(ld)
    for _ in range(max(workers, 1)):                   # worker start-up and the first round of prefetched batches
        next(it)
    n, t0 = 0, time.perf_counter()
    while n < batches:
        try:
            next(it)
        except StopIteration:
            it = iter(ld)
            continue
        n += 1
    return n * batch / (time.perf_counter() - t0)


def loader(workers, out):
    import uda.dataset.keypoint_detection as T
    from uda.dataset import Hand3DStudio
    from utils.data import ragged_collate
    torch.set_num_threads(1)
    with tempfile.TemporaryDirectory() as tmp:
        fabricate(tmp)
        cpu_tf = T.Compose([T.RandomRotation(180), T.RandomResizedCrop(size=256, scale=(0.6, 1.3)),
                            T.ColorJitter(brightness=0.25, contrast=0.25, saturation=0.25), T.GaussianBlur(), T.ToTensor(),
                            T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
        res = {'images': '320x320 JPEG, batch 64', 'cpus': os.cpu_count(), 'affinity': len(os.sched_getaffinity(0))}
        for name, tf, collate in (('cpu_chain', cpu_tf, None), ('device_augment', T.DeviceAugment(180, 256), ragged_collate)):
            ds = Hand3DStudio(tmp, split='all', transforms=tf, download=False)
            for j in workers:
                res['%s_j%d_images_per_s' % (name, j)] = round(loader_rate(ds, j, collate), 1)
                print(name, j, res['%s_j%d_images_per_s' % (name, j)], flush=True)
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, 'w'), indent=1)


def kernels():
    import uda.dataset.keypoint_detection as T
    from PIL import Image
    from mi355.augment import augment
    from utils.data import ragged_collate
    rng = np.random.default_rng(1)
    items = []
    for i in range(64):
        side = int(rng.integers(200, 480))
        im = Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8))
        s, e = T.DeviceAugment(180, 256)(im, keypoint2d=rng.uniform(0, side, (21, 2)), intrinsic_matrix=np.eye(3))
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {}))
    packed, table, params, _, _, _ = ragged_collate(items)
    packed = packed.cuda()
    for _ in range(2):
        x, ema = augment(packed, table, params, want_ema=True)
    torch.cuda.synchronize()
    print('augmented 2 x 64 images; x', tuple(x.shape), 'finite', bool(torch.isfinite(x).all()))


if __name__ == '__main__':
    a = sys.argv[1:]
    if a and a[0] == 'loader':
        w = [int(v) for v in a[a.index('--workers') + 1:] if v.isdigit()] if '--workers' in a else [4, 15]
        loader(w, a[a.index('--out') + 1] if '--out' in a else None)
    elif a and a[0] == 'kernels':
        kernels()
    else:
        print(__doc__)
