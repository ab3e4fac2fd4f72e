"""--synthetic-hands end to end on the GPU: utils.data.RenderedHandIterator (records -> images, teacher images, labels), a tiny
train1.py run with --metrics full and --debug in a child process, the same with a teacher that reads the rendered image_ema, and
--synthetic, whose first-iteration losses must still be the parent commit's."""
import glob
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

SIZES = ['--image-size', '64', '--heatmap-size', '16']           # the smallest pair the model accepts (a 2 x 2 map after layer4)
TINY = ['data/none', '-t', 'Hand3DStudio', '-a', 'resnet18', '-b', '4', '-i', '4', '-p', '2', '-j', '0', '--epochs', '1',
        '--pretrain_epochs', '1'] + SIZES


def _run(extra, log, limit=300):
    r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.join(PKG, 'train1.py')] + TINY + ['--log', log] + extra,
                       env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _loader(domain, batch, n, S=64, workers=0):
    from torch.utils.data import DataLoader
    from utils.data import record_collate
    from utils.rendered_dataset import RenderedHand21
    ds = RenderedHand21(length=n, image_size=S, heatmap_size=S // 4, seed=31, domain=domain)
    return ds, DataLoader(ds, batch_size=batch, shuffle=False, num_workers=workers, pin_memory=True, collate_fn=record_collate)


@pytest.mark.parametrize('domain', ['cg', 'photo'])
def test_iterator_yields_rendered_images_their_teacher_view_and_the_labels_of_their_key_points(gpu, domain):
    from mi355 import ops
    from utils.data import RenderedHandIterator
    from utils.labels import generate_target_device
    S, B, n = 64, 4, 10                                            # two full batches and a ragged one
    ds, loader = _loader(domain, B, n)
    seen = 0
    for x, target, weight, meta in RenderedHandIterator(loader, gpu, S, S // 4, ds.sigma, want_ema=True, want_keypoints=True):
        b = x.shape[0]
        items = [ds[seen + i] for i in range(b)]
        kp = meta['keypoint2d']
        assert tuple(x.shape) == (b, 3, S, S) and tuple(target.shape) == (b, 21, S // 4, S // 4) and tuple(weight.shape) == (b, 21, 1)
        assert np.array_equal(kp.cpu().numpy(), np.stack([it[1] for it in items]))
        vis = torch.from_numpy(np.stack([it[2] for it in items])).to(gpu)
        want_t, want_w = generate_target_device(kp, vis, S // 4, ds.sigma, S)
        assert torch.equal(target, want_t) and torch.equal(weight, want_w)
        recs = torch.from_numpy(np.stack([it[0] for it in items]).view(np.uint8).reshape(b, -1).copy()).to(gpu)
        ema = torch.empty_like(x)
        assert torch.equal(x, ops.render_hands(recs, S, out_ema=ema)) and torch.equal(meta['image_ema'], ema)
        assert bool(torch.isfinite(x).all())
        if domain == 'cg':
            assert torch.equal(meta['image_ema'], x)               # gain 1, bias 0, no sensor noise: nowhere
        else:
            assert not torch.equal(meta['image_ema'], x)
            r = np.stack([it[0] for it in items])                  # what gain / bias / sensor noise allow, in normalised units
            std = np.array([0.229, 0.224, 0.225], np.float32)
            raw = (meta['image_ema'].cpu().numpy() * std[None, :, None, None] + np.array([0.485, 0.456, 0.406], np.float32)[None, :, None, None])
            bound = (np.abs(r['gain'] - 1)[:, :, None, None] * np.abs(raw) + np.abs(r['bias'])[:, :, None, None]
                     + 2 * r['sensor_sigma'][:, None, None, None]) / std[None, :, None, None]
            assert (np.abs((x - meta['image_ema']).cpu().numpy()) <= bound + 1e-4).all()
        seen += b
    assert seen == n
    plain = next(iter(RenderedHandIterator(loader, gpu, S, S // 4, ds.sigma)))
    assert plain[3] == {}                                          # nothing asked for, nothing made


def _finite_losses(out):
    """Every loss a progress line prints is a number: a NaN would mean that a label of a joint outside the frame reached the KL loss
    un-guarded (train1.py RENDERED_LABEL_EPSILON).  Returns how many were read."""
    vals = re.findall(r'Loss(?: \([^)]*\))? (\S+) \((\S+)\)', out)
    assert vals and all(math.isfinite(float(v)) for pair in vals for v in pair), [p for p in vals if not all(math.isfinite(float(v)) for v in p)][:5]
    return len(vals)


def _epe_lines(out):
    return [float(m) for m in re.findall(r'^EPE: ([^ ]+) px', out, flags=re.M)]


def test_train1_synthetic_hands_with_metrics_full_and_debug(gpu, tmp_path):
    log = str(tmp_path / 'run')
    out = _run(['--synthetic-hands', '--render-train-size', '64', '--render-val-size', '8', '--metrics', 'full', '--debug',
                '--pretrain', str(tmp_path / 'none.pth')], log)
    assert 'Start regression domain adaptation.' in out and 'Target(best)' in out
    assert _finite_losses(out) >= 8                                  # pre-training, adaptation and validation lines
    epe = _epe_lines(out)
    assert len(epe) >= 3 and all(math.isfinite(v) and v >= 0 for v in epe), out[-2000:]     # pre-training source, then source and target
    images = glob.glob(os.path.join(log, 'visualize', '0', '*.jpg'))
    assert {os.path.basename(p) for p in images} >= {'source_0.jpg', 'target_0.jpg', 'source_2.jpg', 'target_2.jpg'}
    from PIL import Image
    assert Image.open(images[0]).size == (64, 64)
    assert os.path.exists(os.path.join(log, 'checkpoints', '0.pth'))


def test_train1_synthetic_hands_teacher_reads_the_rendered_image_ema(gpu, tmp_path):
    log = str(tmp_path / 'run')
    out = _run(['--synthetic-hands', '--render-train-size', '64', '--render-val-size', '8', '--metrics', 'full', '--debug',
                '--ema-update', 'const', '--mt-loss', 'on', '--occlude', 'keypoint', '--pretrain', str(tmp_path / 'none.pth')], log)
    assert 'Target(best)' in out and 'ema:' in out and 'Loss (mt)' in out
    assert all(math.isfinite(v) for v in _epe_lines(out))
    assert _finite_losses(out) >= 8
    assert glob.glob(os.path.join(log, 'visualize', '0', 'target_*.jpg')) and os.path.exists(os.path.join(log, 'checkpoints', '0.pth'))


# `train1.py data/none -t Hand3DStudio -a resnet18 -b 4 -i 4 -p 2 -j 0 --epochs 1 --pretrain_epochs 1 --image-size 64 --heatmap-size 16
# --synthetic --seed 1` on the parent commit (1629051), MI355X: the first line of the adaptation epoch
PARENT_FIRST_ITERATION = ('1.05e+01', '1.33e+00', '1.53e+00')


def test_synthetic_alone_prints_the_parent_commits_first_iteration_losses(gpu, tmp_path):
    """--synthetic is untouched by --synthetic-hands: the same noise data set, the same iterators, the same losses.  The parent
    commit printed, for the command above, ``Loss (s) 1.05e+01  Loss (t, false) 1.33e+00  Loss (t, truth) 1.53e+00`` on its first
    adaptation iteration (recorded from a run of the parent's tree on the same MI355X box, beside this tree's)."""
    out = _run(['--synthetic', '--seed', '1', '--pretrain', str(tmp_path / 'none.pth')], str(tmp_path / 'run'))
    line = next(l for l in out.splitlines() if l.startswith('Epoch: [0][0/4]') and 'Loss (t, false)' in l)
    got = tuple(re.search(re.escape(name) + r' (\S+)', line).group(1) for name in ('Loss (s)', 'Loss (t, false)', 'Loss (t, truth)'))
    print('first adaptation iteration:', got)
    assert got == PARENT_FIRST_ITERATION, line
