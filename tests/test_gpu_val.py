"""Validation on the device data path, on the MI355X: mi355.augment.resize_normalize (one launch of the geometry kernel)
against the Pillow validation chain and the numpy restatement, both augmentation kernels at output side 512, the
geometry-only contract with mi355.augment's image_ema, writes confined to `out`, and train1.validate through the CPU loader
and the device loader -- equal results, no host synchronisation per batch, equal command-line output."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import augment_ref as R
from augment_cases import K0, MEAN, STD, cpu_chain, labels, seeded, sources
from conftest import PKG

pytestmark = pytest.mark.gpu


def _image(rng, side):
    yy, xx = np.mgrid[0:side, 0:side]
    base = np.stack([128 + 100 * np.sin(xx / rng.uniform(5, 40)), 128 + 100 * np.cos(yy / rng.uniform(5, 40)), (xx + yy) % 256], 2)
    return np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)


def _pack(arrs, rows):
    offsets = np.cumsum([0] + [x.size for x in arrs])[:-1]
    table = torch.tensor([[int(o), x.shape[0], x.shape[1]] for o, x in zip(offsets, arrs)], dtype=torch.int64)
    return torch.from_numpy(np.concatenate([x.reshape(-1) for x in arrs])), table, torch.tensor(rows, dtype=torch.float64)


def _identity_rows(arrs):
    return [[0.0, 0, 0, a.shape[0], 0.0, 0.0, 0.0, -1, -1, -1, 0.0] for a in arrs]


# ------------------------------------------------------------------ the validation chain: one ragged batch at 256 / 64
def test_device_resize_matches_cpu_validation_chain(gpu):
    import uda.dataset.keypoint_detection as T
    from uda.dataset.util import generate_target
    from utils.data import DeviceAugmentIterator, ragged_collate
    rng = np.random.default_rng(7)
    sides = [256, 255, 257, 17, 128, 515, 773, 1024] + [int(v) for v in rng.integers(64, 641, 16)]
    assert len(sides) == 24
    chain, dev_tf = T.Compose([T.Resize(256), T.ToTensor(), T.Normalize(MEAN, STD)]), T.DeviceResize(256)
    xs, ts, ws, items = [], [], [], []
    for i, side in enumerate(sides):
        im = Image.fromarray(_image(rng, side))
        kp = rng.uniform(0.05 * side, 0.95 * side, (21, 2))
        vis = np.ones((21, 1), np.float32)
        if i < 3:
            kp[2] = (-0.3 * side, 0.5 * side)                 # far outside: the CPU rule drops the joint
            kp[5] = (-3.0 * side / 256, 0.4 * side)           # outside, yet int(-0.75 + 0.5) = 0: kept, Gaussian clipped at the border
            kp[9] = (255.9 * side / 256, 0.3 * side)          # inside, yet int(63.975 + 0.5) = 64: dropped
            vis[7] = 0                                        # invisible
        x, d = chain(im, keypoint2d=kp, intrinsic_matrix=K0)
        t, w = generate_target(d['keypoint2d'], vis, (64, 64), 2, (256, 256))
        xs.append(x); ts.append(torch.from_numpy(t)); ws.append(torch.from_numpy(w))
        s, e = dev_tf(im, keypoint2d=kp, intrinsic_matrix=K0)
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.from_numpy(vis), {'index': i}))
    want = dict(x=torch.stack(xs), target=torch.stack(ts), weight=torch.stack(ws))
    assert want['weight'][:3, [2, 5, 7, 9], 0].tolist() == [[0, 1, 0, 0]] * 3 and float(want['weight'][3:].min()) == 1
    assert float(want['target'][:3, 5].amax()) > 0.3 and float(want['target'][:3, [2, 7, 9]].amax()) == 0
    batch = ragged_collate(items)

    def check(x, t, w):
        for name, a in (('x', x), ('target', t), ('weight', w)):
            a, b = a.cpu(), want[name]
            assert a.dtype == b.dtype and a.shape == b.shape, name
            bad = (a != b).nonzero()
            assert torch.equal(a, b), '%s: %d mismatches, first at %s' % (name, len(bad), bad[:4].tolist())

    for _ in range(2):
        x, t, w, meta = next(DeviceAugmentIterator(iter([batch]), gpu, 256, 64, geometry_only=True))
        assert 'image_ema' not in meta
        check(x, t, w)
    buf = torch.full((24, 3, 256, 256), float('nan'), device=gpu)
    for _ in range(2):
        x, t, w, meta = next(DeviceAugmentIterator(iter([batch]), gpu, 256, 64, out=buf, geometry_only=True))
        assert x.data_ptr() == buf.data_ptr()
        check(buf, t, w)
    with pytest.raises(ValueError):
        DeviceAugmentIterator(iter([batch]), gpu, want_ema=True, geometry_only=True)


# ------------------------------------------------------------------ output sides 16 and 512
@pytest.mark.parametrize('S,sides', [(512, (512, 511, 700, 1500, 2048)), (16, (16, 17, 64))])
def test_resize_normalize_at_the_size_limits(gpu, S, sides):
    from mi355.augment import resize_normalize
    rng = np.random.default_rng(S)
    arrs = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8) for s in sides]
    packed, table, params = _pack(arrs, _identity_rows(arrs))
    x = resize_normalize(packed.to(gpu), table, params, size=S).cpu()
    assert tuple(x.shape) == (len(sides), 3, S, S) and x.dtype == torch.float32
    for i, arr in enumerate(arrs):
        ref = torch.from_numpy(R.normalise(R.resize(arr, S)))
        assert torch.equal(x[i], ref), (sides[i], int((x[i] != ref).sum()))


def test_training_chain_at_512(gpu):
    """Both launches of mi355.augment at S = 512 (dynamic LDS above the 64 KB default) against the Pillow chain, labels at 128."""
    import uda.dataset.keypoint_detection as T
    from utils.data import DeviceAugmentIterator, ragged_collate
    chain, dev_tf = cpu_chain(size=512), T.DeviceAugment(180, 512, (0.6, 1.3))
    xs, emas, ts, ws, items = [], [], [], [], []
    for i, (im, kp) in enumerate(sources(6, seed=31, lo=300, hi=1400)):
        x, d = seeded(lambda: chain(im, keypoint2d=kp, intrinsic_matrix=K0), 1000 + i)
        t, w = labels(d['keypoint2d'], size=512, hm=128)
        xs.append(x); emas.append(d['image_ema']); ts.append(t); ws.append(w)
        s, e = seeded(lambda: dev_tf(im, keypoint2d=kp, intrinsic_matrix=K0), 1000 + i)
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {'index': i}))
    batch = ragged_collate(items)
    crop = batch[2][:, 3]
    assert float(crop.max()) <= 4 * 512                      # a property of the sources (at most 1400 px), not a case left out
    assert float(crop.min()) < 512 < float(crop.max())       # the crops are scaled up and down
    assert tuple(xs[0].shape) == (3, 512, 512) and tuple(ts[0].shape) == (21, 128, 128)
    x, t, w, meta = next(DeviceAugmentIterator(iter([batch]), gpu, 512, 128, want_ema=True))
    for name, a, b in (('x', x, xs), ('image_ema', meta['image_ema'], emas), ('target', t, ts), ('weight', w, ws)):
        a, b = a.cpu(), torch.stack(b)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = (a != b).nonzero()
        assert torch.equal(a, b), '%s: %d mismatches, first at %s' % (name, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------ the geometry stage alone
def _shortcut_batch():
    """The eight records of test_gpu_augment.test_device_augment_shortcuts_and_scales."""
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
    return _pack(arrs, rows)


def test_resize_normalize_is_the_geometry_stage_of_augment(gpu):
    from mi355.augment import augment, records, resize_normalize
    packed, table, params = _shortcut_batch()
    assert sorted(set(records(table, params)['rot'].tolist())) == [0, 1, 2, 3, 4]
    packed = packed.to(gpu)
    _, ema = augment(packed, table, params, want_ema=True)
    x = resize_normalize(packed, table, params)
    assert x.dtype == ema.dtype and x.shape == ema.shape and torch.equal(x, ema)
    out = torch.full_like(ema, float('nan'))
    assert resize_normalize(packed, table, params, out=out) is out and torch.equal(out, ema)
    # the argument contract of augment()
    from mi355 import Mi355Error
    for bad in (lambda: resize_normalize(packed.cpu(), table, params), lambda: resize_normalize(packed, table, params, out=out[:4]),
                lambda: resize_normalize(packed, table, params, out=out.double()), lambda: resize_normalize(packed, table[:7], params),
                lambda: resize_normalize(packed, table, params, size=520)):
        with pytest.raises(Mi355Error):
            bad()


@pytest.mark.parametrize('S,sides', [(16, (16, 17, 64)), (512, (512, 700))])
def test_resize_normalize_writes_inside_out_only(gpu, S, sides):
    from mi355.augment import resize_normalize
    rng = np.random.default_rng(S + 1)
    arrs = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8) for s in sides]
    packed, table, params = _pack(arrs, _identity_rows(arrs))
    n = len(sides) * 3 * S * S
    buf = torch.full((64 + n + 64,), float('nan'), device=gpu)
    out = buf[64:64 + n].view(len(sides), 3, S, S)
    assert resize_normalize(packed.to(gpu), table, params, out=out, size=S).data_ptr() == buf.data_ptr() + 256
    host = buf.cpu()
    assert bool(torch.isnan(host[:64]).all()) and bool(torch.isnan(host[-64:]).all())
    assert not bool(torch.isnan(host[64:64 + n]).any())       # and every word of `out` was written


# ------------------------------------------------------------------ train1.validate
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """A fabricated H3D_crop tree: 22 Pillow-written square JPEGs of 180..320 px (batch 8: the last batch holds 6)."""
    root = tmp_path_factory.mktemp('val')
    os.makedirs(root / 'H3D_crop' / 'p')
    rng = np.random.default_rng(41)
    samples = []
    for i in range(22):
        side = int(rng.integers(180, 321))
        Image.fromarray(_image(rng, side)).save(root / 'H3D_crop' / ('p/%d.jpg' % i), quality=92)
        kp = side * (0.2 + 0.6 * rng.random((21, 2)))
        samples.append({'name': 'p/%d.jpg' % i, 'keypoint2d': kp.tolist(), 'keypoint3d': np.hstack([kp / 900, np.ones((21, 1))]).tolist(),
                        'intrinsic_matrix': K0.tolist(), 'without_object': 1})
    json.dump(samples, open(root / 'H3D_crop' / 'annotation.json', 'w'))
    return str(root)


@pytest.fixture(scope='module')
def model(gpu):
    import mi355
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling, PoseResNet
    mi355.load()
    torch.manual_seed(3)
    bb = models.resnet18(pretrained=False)
    return PoseResNet(bb, Upsampling(bb.out_features), 256, 21, finetune=True).to(gpu).eval()


def _args(device_augment, print_freq=1, workers=0):
    return argparse.Namespace(batch_size=8, workers=workers, device_augment=device_augment, synthetic=False, print_freq=print_freq,
                              image_size=256, heatmap_size=64)


def _loader(tree, args):
    import train1
    import uda.dataset.keypoint_detection as T
    from uda.dataset import Hand3DStudio
    tf = T.DeviceResize(256) if args.device_augment else T.Compose([T.Resize(256), T.ToTensor(), T.Normalize(MEAN, STD)])
    ds = Hand3DStudio(tree, split='all', transforms=tf, image_size=(256, 256), heatmap_size=(64, 64))
    assert len(ds) == 22
    return train1.make_loader(ds, args, train=False)


def _validate_as_before(val_loader, model, criterion, gpu):
    """validate() of the parent commit: a host read of the loss and two coordinate copies per batch."""
    from mi355.infer import GraphedForward
    from utils.keypoint_detection import accuracy
    from utils.meter import AverageMeter, AverageMeterDict
    losses, acc = AverageMeter('Loss', ':.2e'), AverageMeterDict(val_loader.dataset.keypoints_group.keys(), ":3.2f")
    forward = GraphedForward(model)
    with torch.no_grad():
        for x, label, weight, meta in val_loader:
            x, label, weight = x.to(gpu), label.to(gpu), weight.to(gpu)
            y = forward(x)
            losses.update(criterion(y, label, weight).item(), x.size(0))
            acc.update(val_loader.dataset.group_accuracy(accuracy(y, label)[0]), x.size(0))
    return acc.average(), losses.avg


@pytest.fixture(scope='module')
def before(tree, model, gpu):
    from uda.model.loss import JointsKLLoss
    return _validate_as_before(_loader(tree, _args(False)), model, JointsKLLoss(), gpu)


def test_validation_loaders(tree, gpu):
    from utils.data import ragged_collate
    cpu, dev = _loader(tree, _args(False, workers=3)), _loader(tree, _args(True, workers=3))
    assert cpu.num_workers == 0 and cpu.collate_fn is not ragged_collate and len(cpu) == 3
    assert dev.num_workers == 3 and dev.collate_fn is ragged_collate and len(dev) == 3
    assert not cpu.drop_last and not dev.drop_last


@pytest.mark.parametrize('print_freq', [1, 100])
def test_validate_device_loader_equals_cpu_loader(tree, model, gpu, before, print_freq, capsys, monkeypatch):
    import train1
    from uda.model.loss import JointsKLLoss
    from utils import meter
    got = {}
    for flag in (False, True):
        seen = []
        monkeypatch.setattr(train1, 'AverageMeter', lambda *a, **k: seen.append(meter.AverageMeter(*a, **k)) or seen[-1])
        capsys.readouterr()
        res = train1.validate(_loader(tree, _args(flag, print_freq)), model, JointsKLLoss(), _args(flag, print_freq))
        lines = [l.split('\t') for l in capsys.readouterr().out.splitlines() if l.startswith('Test: ')]
        loss_meter = [m for m in seen if m.name == 'Loss'][0]
        assert loss_meter.count == 22
        assert [l[0] for l in lines] == (['Test: [0/3]', 'Test: [1/3]', 'Test: [2/3]'] if print_freq == 1 else ['Test: [0/3]'])
        got[flag] = (res, loss_meter.avg, [l[2:] for l in lines])          # (field 1 is the time meter)
    assert sorted(got[True][0]) == ['DIP', 'MCP', 'PIP', 'all', 'fingertip']
    for k, v in got[False][0].items():
        assert got[True][0][k] == v, k
    assert got[True][1] == got[False][1] and np.isfinite(got[True][1])
    assert got[True][2] == got[False][2]
    # and both equal the per-batch host arithmetic validate() replaced
    assert got[False][0] == before[0] and got[False][1] == before[1]


def test_validate_metric_step_does_not_synchronise(gpu, monkeypatch):
    import train1
    from uda.model.loss import JointsKLLoss
    from seeded import rand, randn, weights_bk
    y, label = randn(202, 4, 21, 64, 64).to(gpu), rand(205, 4, 21, 64, 64) * (rand(206, 4, 21, 64, 64) > 0.9)
    label[..., 0, 0] += 0.5                                   # (no all-zero map: the loss is finite)
    label, weight, criterion = label.to(gpu), weights_bk(207, 4, 21).to(gpu), JointsKLLoss()
    with torch.no_grad():
        ref = train1.validate_batch_metrics(y, label, weight, criterion)      # (first call: allocations, lazy initialisation)
        probe = torch.zeros((), device=gpu)
        torch.cuda.synchronize()
        old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode('error')
        try:
            try:
                probe.item()
                honoured = False
            except RuntimeError:
                honoured = True
            if honoured:
                with pytest.raises(RuntimeError):
                    probe.item()
                out = train1.validate_batch_metrics(y, label, weight, criterion)
            else:
                torch.cuda.set_sync_debug_mode(old)
                calls = []
                for name in ('item', 'cpu', 'tolist'):
                    monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _n=name, **k: calls.append(_n))
                out = train1.validate_batch_metrics(y, label, weight, criterion)
                monkeypatch.undo()
                assert calls == []
        finally:
            torch.cuda.set_sync_debug_mode(old)
    loss, pred, tgt = out
    assert loss.is_cuda and loss.dim() == 0 and bool(torch.isfinite(loss)) and tuple(pred.shape) == tuple(tgt.shape) == (4, 21, 2)
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    from utils.keypoint_detection import accuracy, accuracy_from_preds
    want = accuracy(y, label)
    have = accuracy_from_preds(pred.cpu().numpy(), tgt.cpu().numpy(), 64, 64)
    assert np.array_equal(have[0], want[0]) and have[1:3] == want[1:3] and np.array_equal(have[3], want[3])


def test_test_phase_cli_with_and_without_device_augment(tree, gpu, tmp_path):
    """train1.py --phase test on the fabricated tree, CPU validation loader against --device-augment (with loader workers).
    The --pretrain file holds every tensor of the network train1 builds, so that no weight is left to the random initialisation
    (whose draws depend on how many loader iterators were started before it)."""
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    torch.manual_seed(5)
    bb = models.resnet18(pretrained=False)
    ck = tmp_path / 'pretrain.pth'
    torch.save({'model': PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).state_dict()}, ck)
    outs = []
    for extra in ([], ['--device-augment', '-j', '2']):
        argv = [tree, '--source_root', tree, '-s', 'Hand3DStudio', '-t', 'Hand3DStudio', '-a', 'resnet18', '-b', '3', '-j', '0', '-p', '1',
                '--phase', 'test', '--pretrain', str(ck), '--log', str(tmp_path / ('run%d' % len(outs)))] + extra
        r = subprocess.run([sys.executable, 'train1.py'] + argv, cwd=PKG, env=dict(os.environ, PYTHONPATH=PKG), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs.append(r.stdout.splitlines())
    pick = lambda lines: [l for l in lines if re.match(r'(Source: \S+ Target: \S+|(MCP|PIP|DIP|fingertip|all): \S+)$', l)]
    progress = lambda lines: [l.split('\t')[:1] + l.split('\t')[2:] for l in lines if l.startswith('Test: ')]
    assert len(pick(outs[0])) == 6 and pick(outs[0])[0].startswith('Source: ')
    assert pick(outs[0]) == pick(outs[1])
    assert len(progress(outs[0])) == 4 and progress(outs[0]) == progress(outs[1])       # 4 test images, batch 3: 2 batches per set
