"""The device augmentation's contract, checked without a GPU: the numpy restatement of every Pillow stage (augment_ref)
is bit-exact against Pillow, the host records mi355.augment builds reproduce Pillow's rotation / blur arithmetic, the
DeviceAugment transform draws the CPU chain's parameters with the CPU chain's RNG calls (identical key points, camera
matrix, labels and RNG state afterwards, and the parameters reproduce the chain's tensors bit for bit), the ragged
collate, and the C ABI's host-side argument checks."""
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter

import augment_ref as R
import augment_cases as A
from augment_cases import K0, cpu_chain, labels, ref_from_params, seeded, sources


def _img(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------ stage by stage against Pillow
@pytest.mark.parametrize('shape', [(96, 96), (64, 130), (257, 200), (512, 511)])
def test_rotate_matches_pillow(shape):
    rng = np.random.default_rng(shape[0])
    arr = _img(rng, *shape)
    angles = [0, 90, 180, 270, -90, -180, 360, 450, 179.99999, 90.0000001] + list(rng.uniform(-180, 180, 12))
    for a in angles:
        assert np.array_equal(R.rotate(arr, a), np.asarray(Image.fromarray(arr).rotate(a))), (shape, a)


@pytest.mark.parametrize('side', [64, 100, 255, 256, 257, 300, 384, 511, 512])
def test_resized_crop_matches_pillow(side):
    rng = np.random.default_rng(side)
    arr = _img(rng, 600, 620)
    top, left = int(rng.integers(0, 600 - side)), int(rng.integers(0, 620 - side))
    crop = arr[top:top + side, left:left + side]
    want = Image.fromarray(arr).crop((left, top, left + side, top + side)).resize((256, 256), Image.BILINEAR)
    assert np.array_equal(R.resize(crop, 256), np.asarray(want))


@pytest.mark.parametrize('order', [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)])
def test_jitter_matches_pillow(order):
    rng = np.random.default_rng(sum(o * 3 ** i for i, o in enumerate(order)))
    enh = [ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color]
    for factors in ([0.75, 0.75, 0.75], [1.25, 1.25, 1.25], [0.75, 1.25, 1.0], list(rng.uniform(0.75, 1.25, 3))):
        arr = _img(rng, 80, 96)
        im = Image.fromarray(arr)
        for k in order:
            im = enh[k](im).enhance(factors[k])
        assert np.array_equal(R.jitter(arr, factors, order), np.asarray(im)), (order, factors)


@pytest.mark.parametrize('radius', [0.0, 1e-6, 0.05, 0.3, 0.55, 0.7999, 0.8])
def test_blur_matches_pillow(radius):
    arr = _img(np.random.default_rng(7), 70, 90)
    assert np.array_equal(R.blur(arr, radius), np.asarray(Image.fromarray(arr).filter(ImageFilter.GaussianBlur(radius))))


# ------------------------------------------------------------------ the edge cases the GPU suite runs (augment_cases), against Pillow
def _pillow_stages(arr, p, size):
    """The chain of augment_cases.ref_stages done by Pillow itself."""
    enh = [ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color]
    top, left, side = int(p[1]), int(p[2]), int(p[3])
    im = Image.fromarray(arr).rotate(p[0]).crop((left, top, left + side, top + side)).resize((size, size), Image.BILINEAR)
    g = np.asarray(im)
    for k in [int(o) for o in p[7:10] if o >= 0]:
        im = enh[k](im).enhance(p[4 + k])
    j = np.asarray(im)
    return g, j, np.asarray(im.filter(ImageFilter.GaussianBlur(p[10])))


def _agrees_with_pillow(case, size):
    for i, (arr, row) in enumerate(case):
        p = np.array(row)
        for name, a, b in zip(('geometry', 'jitter', 'blur'), A.ref_stages(arr, p, size), _pillow_stages(arr, p, size)):
            assert np.array_equal(a, b), (name, i, row)


@pytest.mark.parametrize('S', A.EDGE_SIDES)
def test_edge_crop_sides_match_pillow(S):
    """Output sides 16 and 48, crop sides 1, 2, S - 1, S, S + 1, 2 S + 1, 4 S - 1 and 4 S at both corners under every rotation
    mode."""
    from mi355.augment import records
    assert A.crop_sides(S) == [1, 2, S - 1, S, S + 1, 2 * S + 1, 4 * S - 1, 4 * S]
    for side in A.crop_sides(S):
        case = A.geometry_case(S, side)
        packed, table, params = A.pack(case)
        rec = records(table, params)
        assert sorted(rec['rot'].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and rec['rot'][0] == rec['rot'][-1] == 1
        assert int(rec['top'][0]) == int(rec['left'][0]) == 0                        # the first image from its first byte ...
        assert int(rec['top'][-1] + side) == int(rec['h'][-1]) and int(rec['left'][-1] + side) == int(rec['w'][-1])
        assert int(rec['offset'][-1]) + int(rec['h'][-1]) * int(rec['w'][-1]) * 3 == packed.numel()    # ... the last to the last byte
        assert int(packed.max()) < 255
        _agrees_with_pillow(case, S)


def test_the_affine_case_leaves_the_source_on_all_four_sides():
    from mi355.augment import rotation_record
    arr, row = A.geometry_case(16, 16)[1]
    h, w = arr.shape[:2]
    assert h != w
    mode, c = rotation_record(row[0], w, h)
    assert mode == 0
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xs, ys = (c[2] + y * c[1] + x * c[0]) >> 16, (c[5] + y * c[4] + x * c[3]) >> 16
    assert (xs < 0).any() and (xs >= w).any() and (ys < 0).any() and (ys >= h).any()


def test_edge_jitter_factors_match_pillow():
    case = A.jitter_case()
    rows = np.array([r for _, r in case])
    assert A.ABOVE_ONE > 1 and np.float32(A.ABOVE_ONE) == np.nextafter(np.float32(1), np.float32(2))
    for op in range(3):                                   # every factor for each op alone
        alone = rows[7 * op:7 * op + 7]
        assert ((alone[:, 7:10] >= 0).sum(1) == 1).all() and (alone[:, 7 + op] == op).all()
        assert alone[:, 4 + op].tolist() == A.FACTORS
    for order in A.ORDERS + A.PARTIAL_ORDERS:             # and every order, with every factor in every slot
        sel = rows[(rows[:, 7:10] == np.array(order)).all(1)]
        assert len(sel) == len(A.FACTORS) and all(set(sel[:, 4 + k].tolist()) == set(A.FACTORS) for k in range(3))
    assert all((a == 0).all(2).any() and (a == 255).all(2).any() for a, _ in case)      # rows of 0 and of 255
    clipped = [A.ref_stages(a, np.array(r), 16)[1] for a, r in case]
    assert any((j == 0).any() for j in clipped) and any((j == 255).any() for j in clipped)
    _agrees_with_pillow(case, 16)


def test_contrast_tie_rounds_up_and_matches_pillow():
    case = A.tie_case()
    L = R.luminance(case[0][0])
    assert sorted(np.unique(L).tolist()) == [10, 11] and float(L.astype(np.int64).sum()) / L.size == 10.5
    assert sorted({r[5] for _, r in case}) == [0.5, 1.5]
    assert A.ref_lsum(case[0][0], np.array(case[0][1]), 16) == 10 * 128 + 11 * 128
    want = R.blend(np.full_like(case[0][0], 11), case[0][0], 0.5)                   # mean 11, not 10
    assert np.array_equal(A.ref_stages(case[0][0], np.array(case[0][1]), 16)[1], want) and (want[:8] == 10).all()
    assert not np.array_equal(want, R.blend(np.full_like(case[0][0], 10), case[0][0], 0.5))      # a mean of 10 would show
    _agrees_with_pillow(case, 16)


@pytest.mark.parametrize('S', A.EDGE_SIDES)
def test_edge_blur_radii_match_pillow(S):
    from mi355 import Mi355Error
    from mi355.augment import blur_record
    radii = A.blur_radii()
    lo, hi = A.largest_blur_radius()
    assert radii[:6] == [0.0, 1e-6, 1e-3, 0.05, 0.8, 1.0] and radii[6] == lo and abs(lo - 1.41421347) < 1e-8
    assert hi == np.nextafter(lo, 2.0) and int(R.box_radius(lo)) == 0 and int(R.box_radius(hi)) == 1
    assert blur_record(1e-6) == (1, 1 << 24, 0)            # 255 * 2^24 + 2^23: the largest sum the kernel forms in 32 bits
    assert 255 * (1 << 24) + (1 << 23) < 1 << 32
    for r in radii:
        on, ww, fw = blur_record(r)
        assert (on, ww, fw) == ((0, 0, 0) if r == 0 else (1,) + R.box_weights(R.box_radius(r))[1:]) and ww + 2 * fw <= 1 << 24
    with pytest.raises(Mi355Error):
        blur_record(hi)
    _agrees_with_pillow(A.blur_case(S), S)


def test_mixed_batch_matches_pillow():
    case = A.mixed_case(48)
    assert 20 <= len(case) <= 28 and len({a.shape for a, _ in case}) > 8
    _agrees_with_pillow(case, 48)


# ------------------------------------------------------------------ host records of mi355.augment
def test_rotation_records_reproduce_pillow():
    from mi355.augment import rotation_record
    rng = np.random.default_rng(3)
    for (h, w) in [(100, 100), (90, 130), (211, 200)]:
        arr = _img(rng, h, w)
        for a in [0, 90, 180, 270, -90, 33.3] + list(rng.uniform(-180, 180, 6)):
            mode, c = rotation_record(a, w, h)
            if mode == 0:
                y, x = np.mgrid[0:h, 0:w].astype(np.int64)
                xs, ys = (c[2] + y * c[1] + x * c[0]) >> 16, (c[5] + y * c[4] + x * c[3]) >> 16
                ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
                got = np.zeros_like(arr)
                got[ok] = arr[ys[ok], xs[ok]]
                assert np.all(np.abs(c[:2] + c[3:5]) <= 2 * 65536)
            else:
                got = {1: arr, 2: arr[::-1, ::-1], 3: np.rot90(arr, 1), 4: np.rot90(arr, 3)}[mode]
                assert w == h or mode in (1, 2)
            assert np.array_equal(got, np.asarray(Image.fromarray(arr).rotate(a))), (h, w, a)


def test_blur_records_match_pillow_weights():
    from mi355 import Mi355Error
    from mi355.augment import blur_record
    for r in np.linspace(0, 0.8, 41):
        on, ww, fw = blur_record(float(r))
        fr = R.box_radius(r) if r else 0
        if not fr:
            assert on == 0
            continue
        assert on == 1 and (0, ww, fw) == R.box_weights(fr) and ww + 2 * fw <= 1 << 24
    with pytest.raises(Mi355Error):
        blur_record(2.5)                 # box radius 1: not on the device path


# ------------------------------------------------------------------ the transform: RNG calls, labels, parameters
def test_device_transform_draws_the_cpu_chains_parameters():
    import uda.dataset.keypoint_detection as T
    dev_tf = T.DeviceAugment(180, 256, (0.6, 1.3))
    chain = cpu_chain()
    for i, (im, kp) in enumerate(sources(24, seed=5)):
        x, d = seeded(lambda: chain(im, keypoint2d=kp, intrinsic_matrix=K0), 100 + i)
        st_cpu = (random.getstate(), np.random.get_state())
        s, e = seeded(lambda: dev_tf(im, keypoint2d=kp, intrinsic_matrix=K0), 100 + i)
        st_dev = (random.getstate(), np.random.get_state())
        assert st_cpu[0] == st_dev[0]
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(st_cpu[1], st_dev[1]))
        assert isinstance(s, T.AugmentSample) and s.pixels.dtype == np.uint8 and s.pixels.shape == (im.size[1], im.size[0], 3)
        assert np.array_equal(d['keypoint2d'], e['keypoint2d']) and np.array_equal(d['intrinsic_matrix'], e['intrinsic_matrix'])
        t0, w0 = labels(d['keypoint2d'])
        t1, w1 = labels(e['keypoint2d'])
        assert torch.equal(t0, t1) and torch.equal(w0, w1)
        rx, rema = ref_from_params(s.pixels, s.params)
        assert torch.equal(rx, x) and torch.equal(rema, d['image_ema']), i


def test_snapped_keypoints_keep_the_cpu_labels():
    """utils.data.snap_keypoints: float32 positions whose heat-map centre under the label rule is the CPU chain's."""
    from utils.data import snap_keypoints
    rng = np.random.default_rng(9)
    kp = np.concatenate([rng.uniform(-20, 280, (400, 21, 2)), (np.arange(-8, 264, 0.5)[:, None, None] + np.zeros((1, 21, 2)))[:400]])
    kp[:50] = np.round(kp[:50] * 8) / 8 + 2.0                   # exact half-way points of the 0.5 rounding
    snapped = snap_keypoints(torch.from_numpy(kp), 64, 256).double().numpy()
    for a, b in zip(kp, snapped):
        ta, wa = labels(a)
        tb, wb = labels(b)
        assert torch.equal(ta, tb) and torch.equal(wa, wb)


def test_ragged_collate():
    import uda.dataset.keypoint_detection as T
    from utils.data import ragged_collate
    samples = []
    for i, (im, kp) in enumerate(sources(5, seed=2)):
        s, e = seeded(lambda: T.DeviceAugment(180, 256)(im, keypoint2d=kp, intrinsic_matrix=K0), i)
        samples.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {'image': 'x%d' % i, 'image_ema': s}))
    packed, table, params, kp, vis, meta = ragged_collate(samples)
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and table.dtype == torch.int64 and tuple(table.shape) == (5, 3)
    assert int(table[-1, 0] + table[-1, 1] * table[-1, 2] * 3) == packed.numel()
    for (s, *_), (off, h, w) in zip(samples, table.tolist()):
        assert np.array_equal(packed[off:off + h * w * 3].numpy().reshape(h, w, 3), s.pixels)
    assert params.dtype == torch.float64 and tuple(params.shape) == (5, 11) and tuple(kp.shape) == (5, 21, 2)
    assert tuple(vis.shape) == (5, 21, 1) and meta['image'] == ['x%d' % i for i in range(5)] and 'image_ema' not in meta


def test_h3d_reader_with_device_transform(tmp_path):
    """A data set built with DeviceAugment hands out the raw sample and key points + visibility instead of heat-maps."""
    import json
    import os
    import uda.dataset.keypoint_detection as T
    from uda.dataset import Hand3DStudio
    from utils.data import ragged_collate
    root = tmp_path / 'H3D_crop'
    os.makedirs(root)
    samples = []
    for i, (im, kp) in enumerate(sources(6, seed=4, lo=120, hi=200)):
        im.convert('L').save(root / ('%d.png' % i)) if i == 0 else im.save(root / ('%d.jpg' % i), quality=95)
        samples.append({'name': '%d.png' % i if i == 0 else '%d.jpg' % i, 'keypoint2d': kp.tolist(),
                        'keypoint3d': np.hstack([kp / 900, np.ones((21, 1))]).tolist(), 'intrinsic_matrix': K0.tolist(),
                        'without_object': 1})
    json.dump(samples, open(root / 'annotation.json', 'w'))
    ds = Hand3DStudio(str(tmp_path), split='all', transforms=T.DeviceAugment(180, 256), download=False)
    items = [ds[i] for i in range(len(ds))]
    for s, kp, vis, meta in items:
        assert isinstance(s, T.AugmentSample) and s.pixels.ndim == 3 and s.pixels.shape[2] == 3     # grey sources -> RGB
        assert kp.dtype == torch.float64 and tuple(kp.shape) == (21, 2) and torch.equal(vis, torch.ones(21, 1))
        assert np.array_equal(kp.numpy(), meta['keypoint2d'])
    batch = ragged_collate(items)
    assert tuple(batch[2].shape) == (6, 11)


# ------------------------------------------------------------------ C ABI: host-side checks before any launch
def test_augment_argument_validation_without_gpu():
    import mi355
    from mi355.augment import records, REC
    lib = mi355.load()
    table = np.array([[0, 100, 120], [36000, 64, 64]], np.int64)
    params = np.array([[30.0, 5, 7, 90, 1.1, 0.9, 1.2, 2, 0, 1, 0.4], [90.0, 0, 0, 64, 1, 1, 1, 0, 1, 2, 0.0]])
    good = records(table, params)
    src_bytes = 36000 + 64 * 64 * 3
    norm = np.array(MEANSTD, np.float32)
    ws = lib.mi355_augment_workspace(2, 256)
    assert ws >= 2 * 256 * 256 * 3
    FAKE = 1 << 40                                        # device pointers are never touched when a check fails

    def run(rec, B=2, S=256, nbytes=src_bytes, wsb=ws, out=FAKE):
        rec = np.ascontiguousarray(rec, REC)
        return lib.mi355_augment(FAKE, nbytes, rec.ctypes.data, FAKE, B, S, norm.ctypes.data, out, 0, FAKE, wsb, 0)

    def bad(msg, **kw):
        rec = good.copy()
        for k, v in kw.pop('set', {}).items():
            rec[k[0]][k[1]] = v
        assert run(rec, **kw) < 0
        assert msg in lib.mi355_last_error(), (msg, lib.mi355_last_error())

    bad(b'output side', S=200)
    bad(b'output side', S=512)
    bad(b'batch', B=0)
    bad(b'null', out=0)
    bad(b'workspace', wsb=ws - 1)
    bad(b'packed buffer', nbytes=src_bytes - 1)
    bad(b'packed buffer', set={('offset', 1): -3})
    bad(b'size', set={('h', 0): 5000})
    bad(b'rotation mode', set={('rot', 0): 7})
    bad(b'90 / 270', set={('rot', 0): 3})
    bad(b'rotation coefficient', set={('a', 0): np.array([70000, 0, 0, 0, 0, 0])})
    bad(b'out of range', set={('a', 0): np.array([0, 0, 1 << 30, 0, 0, 0])})
    bad(b'crop', set={('top', 0): 20})
    bad(b'crop', set={('side', 1): 0})
    bad(b'op order', set={('order', 0): np.array([1, 1, 0])})
    bad(b'factor', set={('factor', 0): np.array([-1.0, 1, 1])})
    bad(b'box weights', set={('ww', 0): 1 << 25})
    assert lib.mi355_augment(FAKE, src_bytes, good.ctypes.data, FAKE, 65535, 256, norm.ctypes.data, FAKE, 0, FAKE, ws, 0) < 0
    assert b'32-bit index range' in lib.mi355_last_error()


MEANSTD = [0.485, 0.456, 0.406, 0.229, 0.224, 0.225]
