"""Device augmentation measurements (train1.py --device-augment).

  python profiles/augment_bench.py loader [--workers 4 15] [--out FILE]
      host-side loader throughput, images/s, on a fabricated H3D_crop tree of 2048 320 x 320 JPEGs (32 batches of 64 per
      pass, so that every worker has work): the CPU chain (decode +
      Pillow augmentation + labels in the workers) against the device-augment loader (decode + parameter draw + ragged
      collate in the workers; the pixel work is left to the GPU).  No GPU needed.
  python profiles/augment_bench.py kernels
      two 64-image batches through mi355.augment (for `rocprofv3 --kernel-trace --stats -- python ...`).
  python profiles/augment_bench.py val [--out profiles/val_loader.json]
      validation on the same tree (needs the GPU): (1) loader rate of the CPU validation chain (Resize, ToTensor, Normalize,
      labels) at 0 / 4 / 15 workers against the DeviceResize loader at 4 / 15; (2) kernel times of mi355.augment.resize_normalize
      at S = 256, B = 64 and S = 512, B = 32 and of both mi355.augment launches at S = 512, from a `rocprofv3 --kernel-trace
      --stats` run of `val-kernels` in a child process; (3) wall time of train1.validate over the tree, ResNet-50 at 256 x 256,
      through the CPU loader (0 workers, as without --device-augment) and the device loader (4 workers), alternated A B A B."""
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


def _device_batch(tf, sides, rng):
    from PIL import Image
    from utils.data import ragged_collate
    items = []
    for side in sides:
        im = Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8))
        s, e = tf(im, keypoint2d=rng.uniform(0, side, (21, 2)), intrinsic_matrix=np.eye(3))
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {}))
    packed, table, params, _, _, _ = ragged_collate(items)
    return packed.cuda(), table, params


VAL_KERNEL_RUNS = 3


def val_kernels():
    """The launches `val` reads from the kernel trace, told apart by kernel name and grid (S / 8 or S / 16 row bands x B)."""
    import uda.dataset.keypoint_detection as T
    from mi355.augment import augment, resize_normalize
    rng = np.random.default_rng(2)
    b256 = _device_batch(T.DeviceResize(256), [int(v) for v in rng.integers(200, 480, 64)], rng)
    b512 = _device_batch(T.DeviceResize(512), [int(v) for v in rng.integers(300, 1000, 32)], rng)
    a512 = _device_batch(T.DeviceAugment(180, 512), [int(v) for v in rng.integers(300, 1000, 32)], rng)
    for _ in range(VAL_KERNEL_RUNS):
        x256 = resize_normalize(*b256, size=256)
        x512 = resize_normalize(*b512, size=512)
        y512, ema = augment(*a512, want_ema=True, size=512)
        torch.cuda.synchronize()
    print('val-kernels:', tuple(x256.shape), tuple(x512.shape), tuple(y512.shape), 'finite',
          bool(torch.isfinite(x256).all() and torch.isfinite(x512).all() and torch.isfinite(y512).all() and torch.isfinite(ema).all()))


def _kernel_times(tmp):
    """us per launch, by (kernel, blocks in x, blocks in y), from a rocprofv3 run of `val-kernels` in a child process."""
    import csv
    import glob
    import subprocess
    d = os.path.join(tmp, 'prof')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--', sys.executable,
           os.path.abspath(__file__), 'val-kernels']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit('rocprofv3 run failed:\n' + r.stdout[-2000:] + r.stderr[-2000:])
    traces = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if len(traces) != 1:
        raise SystemExit('expected one kernel trace under %s, found %s' % (d, traces))
    out = {}
    for row in csv.DictReader(open(traces[0])):
        name = row['Kernel_Name']
        if 'aug_' not in name:
            continue
        kind = 'aug_photometric' if 'aug_photometric' in name else ('resize_normalize' if 'aug_geometry<false>' in name or 'aug_geometryILb0E' in name else 'aug_geometry')
        grid = (int(row['Grid_Size_X']) // int(row['Workgroup_Size_X']), int(row['Grid_Size_Y']) // int(row['Workgroup_Size_Y']))
        out.setdefault((kind,) + grid, []).append(round((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3, 1))
    want = {'resize_normalize S=256 B=64': ('resize_normalize', 32, 64), 'resize_normalize S=512 B=32': ('resize_normalize', 64, 32),
            'aug_geometry (with image_ema) S=512 B=32': ('aug_geometry', 64, 32), 'aug_photometric S=512 B=32': ('aug_photometric', 32, 32)}
    res = {}
    for label, key in want.items():
        if len(out.get(key, [])) != VAL_KERNEL_RUNS:
            raise SystemExit('kernel trace: %s launches of %s, expected %d (have %s)' % (len(out.get(key, [])), key, VAL_KERNEL_RUNS, sorted(out)))
        res[label + ' us'] = out[key]
    return res


def val(out):
    import argparse
    import uda.dataset.keypoint_detection as T
    from uda.dataset import Hand3DStudio
    from utils.data import ragged_collate
    torch.set_num_threads(1)
    res = {'what': 'validation data path on a fabricated H3D_crop tree of 2048 320x320 JPEGs, batch 64 (profiles/augment_bench.py val)',
           'cpus': os.cpu_count(), 'affinity': len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        fabricate(tmp)
        cpu_tf = lambda: T.Compose([T.Resize(256), T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
        mk = lambda tf: Hand3DStudio(tmp, split='all', transforms=tf, download=False)
        # (1) loaders, before this process touches the GPU
        rates = res['loader_images_per_s'] = {}
        for name, tf, collate, workers in (('cpu_validation_chain', cpu_tf(), None, (0, 4, 15)),
                                           ('device_resize', T.DeviceResize(256), ragged_collate, (4, 15))):
            for j in workers:
                rates['%s_j%d' % (name, j)] = round(loader_rate(mk(tf), j, collate), 1)
                print(name, j, rates['%s_j%d' % (name, j)], flush=True)
        res['device_j4_out_delivers_cpu_j15'] = rates['device_resize_j4'] > rates['cpu_validation_chain_j15']
        # (2) kernels, in a child process under rocprofv3
        res['kernels'] = dict(_kernel_times(tmp), source='rocprofv3 --kernel-trace --stats --output-format csv, %d launches each' % VAL_KERNEL_RUNS)
        print(res['kernels'], flush=True)
        # (3) validate(), CPU loader as without --device-augment against the device loader, A B A B
        import mi355
        import train1
        import uda.model as models
        from uda.model.loss import JointsKLLoss
        from uda.model.pose_resnet2 import Upsampling, PoseResNet
        mi355.load()
        torch.manual_seed(0)
        bb = models.resnet50(pretrained=False)
        model = PoseResNet(bb, Upsampling(bb.out_features), 256, 21, finetune=True).to('cuda').eval()
        criterion = JointsKLLoss()
        passes = res['validate_pass_s'] = {'cpu_loader_j0': [], 'device_loader_j4': []}
        accs = []
        for _ in range(2):
            for name, flag, tf in (('cpu_loader_j0', False, cpu_tf()), ('device_loader_j4', True, T.DeviceResize(256))):
                args = argparse.Namespace(batch_size=64, workers=4, device_augment=flag, synthetic=False, print_freq=100)
                loader_ = train1.make_loader(mk(tf), args, train=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc = train1.validate(loader_, model, criterion, args)
                torch.cuda.synchronize()
                passes[name].append(round(time.perf_counter() - t0, 3))
                accs.append(acc)
                print(name, passes[name][-1], flush=True)
        res['validate_results_equal'] = all(a == accs[0] for a in accs)
        res['model'] = ('PoseResNet(resnet50) at 256x256, bf16, 2048 images per pass; validate() captures its forward graph in every pass, '
                        'the first pass of each kind also carries the one-off allocations and weight packing')
        res['second_pass_device_shorter'] = passes['device_loader_j4'][1] < passes['cpu_loader_j0'][1]
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, 'w'), indent=1)


if __name__ == '__main__':
    a = sys.argv[1:]
    if a and a[0] == 'loader':
        w = [int(v) for v in a[a.index('--workers') + 1:] if v.isdigit()] if '--workers' in a else [4, 15]
        loader(w, a[a.index('--out') + 1] if '--out' in a else None)
    elif a and a[0] == 'kernels':
        kernels()
    elif a and a[0] == 'val-kernels':
        val_kernels()
    elif a and a[0] == 'val':
        val(a[a.index('--out') + 1] if '--out' in a else None)
    else:
        print(__doc__)
