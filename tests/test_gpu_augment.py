"""The training augmentation on the MI355X (mi355.augment, csrc/augment.hip) against the CPU chain train1.py builds:
one ragged batch of 64 sources (64..512 px, some non-square, angles over +-180 degrees) seeded like the CPU chain gives
torch.equal network inputs, image_ema, labels and weights, into fresh or preallocated buffers, run after run; the rotation
shortcuts and the crop-only / up- / down-scaling cases against the numpy restatement; and a train1.py run with
--device-augment on a fabricated Hand-3D-Studio tree.

Guards (tests/guarded.py).  test_device_augment_shortcuts_and_scales and the edge cases of augment_cases (output sides 16 and
48, crop sides 1 .. 4 S at the corners of the first and last image under every rotation mode, jitter factors 0 .. 3.5 in every
order, the contrast tie, blur radii up to the last one the host accepts, one mixed batch) run through _guarded: the packed
sources are a G.place() copy, so the byte after the last image and the byte before the first are 0xFF; x, image_ema and the
workspace are allocated inside the window -- the wrapper's workspace cache (mi355.augment._ws) is emptied for the test, so the
buffer has exactly mi355_augment_workspace(B, S) bytes -- and the geometry image and the luminance sums the first launch
leaves in it are compared with the reference as well.  The device copy of the records is made by Tensor.to inside the wrapper
and is not guarded there; the mixed batch runs a second time through the ABI with a placed copy of the records."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_cases as A
import guarded as G
from augment_cases import K0, cpu_chain, labels, ref_from_params, seeded, sources
from conftest import PKG


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guarded(gpu, monkeypatch, case, S, label, direct=False):
    """One batch through mi355.augment.augment (direct: through mi355_augment with a placed copy of the records) inside guard
    buffers: x and image_ema equal the reference, every output element is written, the workspace has exactly the size the library
    reports and holds the reference's geometry image and luminance sums, no flank byte changes, the sources are only read."""
    import mi355
    import mi355.augment as M
    from mi355 import ops
    packed, table, params = A.pack(case)
    B = len(case)
    need = int(mi355.load().mi355_augment_workspace(B, S))
    assert need == (B * 8 + 255) // 256 * 256 + B * S * S * 3
    monkeypatch.setattr(M, '_ws', {})                    # the old cache comes back after the test
    G.row_pitch(max(max(a.shape[1] for a, _ in case) * 3, S * 4))
    src = G.place(packed.to(gpu), 'packed sources')
    if direct:
        rec = M.records(table.numpy(), params.numpy())
        rec_dev = G.place(torch.from_numpy(rec.view(np.uint8).copy()).to(gpu), 'records')
        norm = np.array(list(M.MEAN) + list(M.STD), dtype=np.float32)
        with G.window(ops, label):
            x, ema = torch.empty(B, 3, S, S, device=gpu), torch.empty(B, 3, S, S, device=gpu)
            ws = M._workspace(gpu, B, S)
            mi355.call('mi355_augment', src.data_ptr(), src.numel(), rec.ctypes.data, rec_dev.data_ptr(), B, S, norm.ctypes.data,
                       x.data_ptr(), ema.data_ptr(), ws.data_ptr(), ws.numel(), mi355.stream_ptr())
    else:
        with G.window(ops, label):
            x, ema = M.augment(src, table, params, want_ema=True, size=S)
        ws = M._ws[gpu]
    assert ws.numel() == need and G._buf_of(ws) is not None and G._buf_of(ws).n == need      # a guarded buffer of exactly that size
    torch.cuda.synchronize()
    G.check(label)
    assert G.unwritten(x) == 0 and G.unwritten(ema) == 0
    assert torch.equal(src.cpu(), packed)
    lsum = ws[:B * 8].view(torch.int64).cpu()
    geo = ws[need - B * S * S * 3:].view(B, S, S, 3).cpu()
    for i, (arr, row) in enumerate(case):
        p = np.array(row)
        rx, rema = ref_from_params(arr, p, S)
        assert torch.equal(x[i].cpu(), rx), (label, i, row)
        assert torch.equal(ema[i].cpu(), rema), (label, i, row)
        assert np.array_equal(geo[i].numpy(), A.ref_stages(arr, p, S)[0]), (label, i, row)      # a byte output: equality is the check
        assert int(lsum[i]) == A.ref_lsum(arr, p, S), (label, i, row)
    return x.cpu(), ema.cpu()


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
def test_device_augment_shortcuts_and_scales(gpu, monkeypatch):
    """Rotation shortcuts (0 / 90 / 180 / 270 on square sources, the affine path at 90 on non-square ones), crop sides
    below, at and above the output size, all jitter orders, blur on and off: against the numpy restatement."""
    import mi355
    from mi355.augment import augment
    mi355_ws = lambda B, S: int(mi355.load().mi355_augment_workspace(B, S))
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
    import mi355.augment as M
    from mi355 import ops
    monkeypatch.setattr(M, '_ws', {})
    G.row_pitch(512 * 3)
    packed = G.place(packed, 'packed sources')
    with G.window(ops, 'shortcuts and scales'):
        x, ema = augment(packed, table, params, want_ema=True)
    torch.cuda.synchronize()
    G.check('shortcuts and scales')
    assert G.unwritten(x) == 0 and G.unwritten(ema) == 0
    assert M._ws[gpu].numel() == mi355_ws(8, 256)
    for i, arr in enumerate(arrs):
        rx, rema = ref_from_params(arr, params[i].numpy())
        assert torch.equal(x[i].cpu(), rx), i
        assert torch.equal(ema[i].cpu(), rema), i


# ------------------------------------------------------------------ the photometric launch at its edges, inside guards
@pytest.mark.gpu
@pytest.mark.parametrize('S,side', [(S, side) for S in A.EDGE_SIDES for side in A.crop_sides(S)])
def test_edge_crop_sides_at_the_corners_of_the_first_and_last_image(gpu, monkeypatch, S, side):
    case = A.geometry_case(S, side)
    assert int(A.pack(case)[0].max()) < 255              # ... so a geometry byte read from a flank cannot pass
    _guarded(gpu, monkeypatch, case, S, 'crop side %d -> %d' % (side, S))


@pytest.mark.gpu
def test_edge_jitter_factors_and_orders(gpu, monkeypatch):
    _guarded(gpu, monkeypatch, A.jitter_case(), 16, 'jitter factors')


@pytest.mark.gpu
def test_contrast_tie_rounds_to_11(gpu, monkeypatch):
    case = A.tie_case()
    x, _ = _guarded(gpu, monkeypatch, case, 16, 'contrast tie')
    assert not torch.equal(x[0, :, :8], x[0, :, 8:])     # mean 11 keeps the halves apart at factor 0.5; a mean of 10 merges them


@pytest.mark.gpu
@pytest.mark.parametrize('S', A.EDGE_SIDES)
def test_edge_blur_radii(gpu, monkeypatch, S):
    from mi355 import Mi355Error
    from mi355.augment import blur_record
    with pytest.raises(Mi355Error):
        blur_record(A.largest_blur_radius()[1])
    _guarded(gpu, monkeypatch, A.blur_case(S), S, 'blur radii at %d' % S)


@pytest.mark.gpu
def test_mixed_batch_twice_same_bits(gpu, monkeypatch):
    case = A.mixed_case(48)
    a = _guarded(gpu, monkeypatch, case, 48, 'mixed batch, wrapper')
    b = _guarded(gpu, monkeypatch, case, 48, 'mixed batch, ABI with placed records', direct=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_workspace_one_byte_short_launches_nothing(gpu):
    import mi355
    import mi355.augment as M
    from mi355 import ops
    case = A.blur_case(16)
    packed, table, params = A.pack(case)
    B, S = len(case), 16
    need = int(mi355.load().mi355_augment_workspace(B, S))
    src = G.place(packed.to(gpu), 'packed sources')
    rec = M.records(table.numpy(), params.numpy())
    rec_dev = G.place(torch.from_numpy(rec.view(np.uint8).copy()).to(gpu), 'records')
    norm = np.array(list(M.MEAN) + list(M.STD), dtype=np.float32)
    with G.window(ops, 'workspace one byte short'):
        x, ema = torch.empty(B, 3, S, S, device=gpu), torch.empty(B, 3, S, S, device=gpu)
        ws = ops.workspace(need, gpu)
    ops.prof_reset(); ops.prof_enable(2)
    try:
        rc = mi355.load().mi355_augment(src.data_ptr(), src.numel(), rec.ctypes.data, rec_dev.data_ptr(), B, S, norm.ctypes.data,
                                        x.data_ptr(), ema.data_ptr(), ws.data_ptr(), need - 1, mi355.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -3 and b'workspace' in mi355.load().mi355_last_error()          # MI355_EWORKSPACE
        assert ops.prof_launches() == []
    finally:
        ops.prof_enable(0); ops.prof_reset()
    G.check('workspace one byte short')
    assert G.unwritten(x) == x.numel() * 4 and G.unwritten(ema) == ema.numel() * 4 and bool((ws == 0xFF).all())     # not even the memset


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
