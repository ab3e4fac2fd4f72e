"""The training augmentation on the MI355X (mi355.augment, csrc/augment.hip) against the CPU chain train1.py builds:
one ragged batch of 64 sources (64..512 px, some non-square, angles over +-180 degrees) seeded like the CPU chain gives
torch.equal network inputs, image_ema, labels and weights, into fresh or preallocated buffers, run after run; the rotation
shortcuts and the crop-only / up- / down-scaling cases against the numpy restatement; and a train1.py run with
--device-augment on a fabricated Hand-3D-Studio tree."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from augment_cases import K0, cpu_chain, labels, ref_from_params, seeded, sources
from conftest import PKG


def _batch(n=64, seed=11):
    import uda.dataset.keypoint_detection as T
    from utils.data import ragged_collate
    chain, dev_tf = cpu_chain(), T.DeviceAugment(180, 256, (0.6, 1.3))
    xs, emas, ts, ws, items = [], [], [], [], []
    for i, (im, kp) in enumerate(sources(n, seed=seed)):
        x, d = seeded(lambda: chain(im, keypoint2d=kp, intrinsic_matrix=K0), 1000 + i)
        t, w = labels(d['keypoint2d'])
        xs.append(x); emas.append(d['image_ema']); ts.append(t); ws.append(w)
        s, e = seeded(lambda: dev_tf(im, keypoint2d=kp, intrinsic_matrix=K0), 1000 + i)
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {'index': i}))
    want = tuple(torch.stack(v) for v in (xs, emas, ts, ws))
    return ragged_collate(items), want


@pytest.mark.gpu
def test_device_augment_matches_cpu_chain(gpu):
    from utils.data import DeviceAugmentIterator
    batch, (x_cpu, ema_cpu, t_cpu, w_cpu) = _batch()
    angles = batch[2][:, 0]
    assert float(angles.min()) < -90 and float(angles.max()) > 90
    assert (batch[1][:, 1] != batch[1][:, 2]).any() and int(batch[1][:, 1:].min()) >= 64 and int(batch[1][:, 1:].max()) <= 512
    runs = []
    for _ in range(2):
        x, t, w, meta = next(DeviceAugmentIterator(iter([batch]), gpu, want_ema=True))
        torch.cuda.synchronize()
        runs.append((x.cpu(), meta['image_ema'].cpu(), t.cpu(), w.cpu()))
    for got in runs:
        for name, a, b in zip(('x', 'image_ema', 'target', 'weight'), got, (x_cpu, ema_cpu, t_cpu, w_cpu)):
            assert a.dtype == b.dtype and a.shape == b.shape, name
            bad = (a != b).nonzero()
            assert torch.equal(a, b), '%s: %d mismatches, first at %s' % (name, len(bad), bad[:4].tolist())
    # out=: straight into a preallocated buffer, twice
    buf = torch.full((64, 3, 256, 256), float('nan'), device=gpu)
    for _ in range(2):
        x, t, w, meta = next(DeviceAugmentIterator(iter([batch]), gpu, out=buf))
        assert x.data_ptr() == buf.data_ptr() and 'image_ema' not in meta
        assert torch.equal(buf.cpu(), x_cpu) and torch.equal(t.cpu(), t_cpu) and torch.equal(w.cpu(), w_cpu)


@pytest.mark.gpu
def test_device_augment_shortcuts_and_scales(gpu):
    """Rotation shortcuts (0 / 90 / 180 / 270 on square sources, the affine path at 90 on non-square ones), crop sides
    below, at and above the output size, all jitter orders, blur on and off: against the numpy restatement."""
    from mi355.augment import augment
    rng = np.random.default_rng(5)
    shapes = [(300, 300), (300, 300), (300, 300), (300, 300), (200, 260), (512, 512), (64, 64), (400, 380)]
    angles = [0.0, 90.0, 180.0, -90.0, 90.0, 450.0, 33.5, -179.0]
    sides = [256, 300, 120, 256, 200, 512, 64, 380]
    orders = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0), (1, -1, -1), (-1, -1, -1)]
    arrs, rows = [], []
    for (h, w), a, side, o in zip(shapes, angles, sides, orders):
        arrs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        top, left = int(rng.integers(0, h - side + 1)), int(rng.integers(0, w - side + 1))
        f = list(rng.uniform(0.75, 1.25, 3))
        rows.append([a, top, left, side] + f + list(o) + [float(rng.uniform(0, 0.8)) if len(rows) % 2 else 0.0])
    offsets = np.cumsum([0] + [x.size for x in arrs])[:-1]
    table = torch.tensor([[int(o), x.shape[0], x.shape[1]] for o, x in zip(offsets, arrs)], dtype=torch.int64)
    params = torch.tensor(rows, dtype=torch.float64)
    packed = torch.from_numpy(np.concatenate([x.reshape(-1) for x in arrs])).to(gpu)
    x, ema = augment(packed, table, params, want_ema=True)
    torch.cuda.synchronize()
    for i, arr in enumerate(arrs):
        rx, rema = ref_from_params(arr, params[i].numpy())
        assert torch.equal(x[i].cpu(), rx), i
        assert torch.equal(ema[i].cpu(), rema), i


@pytest.mark.gpu
def test_train_cli_with_device_augment(gpu, tmp_path):
    """train1.py's parser and main() with --device-augment on a fabricated H3D_crop tree (16 Pillow-written images):
    source-only pre-training (the path a missing --pretrain file takes) and one adaptation epoch through the device
    augmentation, finite losses, the reference's checkpoint layout."""
    from PIL import Image
    root = tmp_path / 'H3D_crop'
    os.makedirs(root / 'p')
    samples = []
    for i, (im, kp) in enumerate(sources(16, seed=21, lo=180, hi=320)):
        side = min(im.size)                               # H3D crops are square (validation's Resize expects them)
        im = im.crop((0, 0, side, side))
        kp = side * (0.45 + 0.1 * np.random.default_rng(i).random((21, 2)))     # near the centre: every joint stays
        im.save(root / ('p/%d.jpg' % i), quality=92)                               # inside the crops (no 0/0 label maps)
        samples.append({'name': 'p/%d.jpg' % i, 'keypoint2d': kp.tolist(), 'keypoint3d': np.hstack([kp / 900, np.ones((21, 1))]).tolist(),
                        'intrinsic_matrix': K0.tolist(), 'without_object': 1})
    json.dump(samples, open(root / 'annotation.json', 'w'))
    log = tmp_path / 'run'
    argv = [str(tmp_path), '--source_root', str(tmp_path), '-s', 'Hand3DStudio', '-t', 'Hand3DStudio', '--device-augment',
            '-a', 'resnet18', '-b', '4', '-i', '3', '-j', '0', '-p', '1', '--pretrain_epochs', '1', '--epochs', '1', '--log', str(log)]
    code = ('import sys, train1; a = train1.build_parser().parse_args(sys.argv[1:]); '
            'a.pretrain = None; train1.main(a)')     # no pre-training checkpoint: train1 pre-trains first
    r = subprocess.run([sys.executable, '-c', code] + argv, cwd=PKG, env=dict(os.environ, PYTHONPATH=PKG), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert 'Pretraining the model on source domain.' in out and 'Target(best)' in out
    losses = [float(v) for v in re.findall(r'Loss \((?:s|t, false|t, truth)\) ([-+0-9.eainf]+)', out)]
    assert losses and all(np.isfinite(losses)), out[-3000:]
    for name in ('pretrain.pth', '0.pth', 'model_ema.pth'):
        assert os.path.exists(log / 'checkpoints' / name), name
