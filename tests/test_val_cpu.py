"""Validation on the device data path, the parts a machine without a GPU can check: the numpy restatement of Image.resize
against the Pillow validation chain at 64 / 256 / 512, the host side of DeviceResize (identity parameter row, labels of
Resize, no random draw), the records mi355.augment builds from such rows, accuracy_from_preds on the G4 fixture, and the
argument checks of mi355_resize_normalize before any launch."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import augment_ref as R
from augment_cases import K0, MEAN, STD
from conftest import golden

MEANSTD = MEAN + STD


def _val_chain(size):
    import uda.dataset.keypoint_detection as T
    return T.Compose([T.Resize(size), T.ToTensor(), T.Normalize(MEAN, STD)])


def _pin_cases():
    cases = []
    for S in (64, 256, 512):
        for side in (S, S - 1, S + 1, 17, S // 2, 2 * S + 3, 3 * S + 5, 4 * S, 300, 480, 640):
            if side <= 4 * S:
                cases.append((S, side))
    return cases


def test_the_pin_has_thirty_cases():
    assert len(_pin_cases()) == 30


@pytest.mark.parametrize('S,side', _pin_cases())
def test_resize_restatement_equals_pillow_validation_chain(S, side):
    rng = np.random.default_rng(S * 10007 + side)
    arr = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    want, _ = _val_chain(S)(Image.fromarray(arr), keypoint2d=np.zeros((21, 2)), intrinsic_matrix=K0)
    got = torch.from_numpy(R.normalise(R.resize(arr, S)))
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), '%d mismatches' % int((got != want).sum())


# ------------------------------------------------------------------ DeviceResize, host side
@pytest.mark.parametrize('mode', ['RGB', 'L', 'RGBA'])
def test_device_resize_host_side(mode):
    import uda.dataset.keypoint_detection as T
    rng = np.random.default_rng(3)
    side = 300
    arr = rng.integers(0, 256, (side, side, 4), dtype=np.uint8)
    im = Image.fromarray({'RGB': arr[:, :, :3], 'L': arr[:, :, 0], 'RGBA': arr}[mode], mode)
    kp = rng.uniform(-20, side + 20, (21, 2))
    tf = T.DeviceResize(256)
    assert tf.labels_on_device is True
    random.seed(9); np.random.seed(9)
    s0, n0 = random.getstate(), np.random.get_state()
    sample, d = tf(im, keypoint2d=kp, intrinsic_matrix=K0, extra='kept')
    assert random.getstate() == s0
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    assert isinstance(sample, T.AugmentSample)
    assert sample.pixels.dtype == np.uint8 and np.array_equal(sample.pixels, np.asarray(im.convert('RGB')))
    assert sample.params.dtype == np.float64
    assert sample.params.tolist() == [0.0, 0.0, 0.0, float(side), 0.0, 0.0, 0.0, -1.0, -1.0, -1.0, 0.0]
    _, want = T.Resize(256)(im, keypoint2d=kp, intrinsic_matrix=K0)
    for k in ('keypoint2d', 'intrinsic_matrix'):
        assert d[k].dtype == want[k].dtype and np.array_equal(d[k], want[k]), k
    assert d['extra'] == 'kept'
    assert np.array_equal(kp, np.asarray(kp)) and K0[0, 0] == 900.0           # the inputs are not modified


def test_device_resize_refuses_non_square_sources_like_resize():
    import uda.dataset.keypoint_detection as T
    im = Image.new('RGB', (300, 301))
    msgs = []
    for fn in (lambda: T.DeviceResize(256)(im, keypoint2d=np.zeros((21, 2)), intrinsic_matrix=K0),
               lambda: T.resize(im, 256, keypoint2d=np.zeros((21, 2)), intrinsic_matrix=K0)):
        with pytest.raises(AssertionError) as e:
            fn()
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and 'square' in msgs[0]


def test_device_resize_samples_collate_and_give_identity_records():
    import uda.dataset.keypoint_detection as T
    from mi355.augment import records
    from utils.data import ragged_collate
    rng = np.random.default_rng(4)
    items, sides = [], (64, 300, 17, 1024)
    for i, side in enumerate(sides):
        im = Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8))
        s, d = T.DeviceResize(256)(im, keypoint2d=rng.uniform(0, side, (21, 2)), intrinsic_matrix=K0)
        items.append((s, torch.from_numpy(d['keypoint2d']), torch.ones(21, 1), {'index': i, 'image_ema': s}))
    packed, table, params, kp, vis, meta = ragged_collate(items)
    assert packed.dtype == torch.uint8 and packed.numel() == sum(3 * s * s for s in sides)
    assert tuple(params.shape) == (4, 11) and 'image_ema' not in meta
    rec = records(table, params)
    assert rec['rot'].tolist() == [1] * 4                                  # Image.rotate(0): Pillow's copy shortcut
    assert not rec['a'].any()
    assert rec['blur'].tolist() == [0] * 4 and rec['ww'].tolist() == [0] * 4 and rec['fw'].tolist() == [0] * 4
    assert rec['top'].tolist() == [0] * 4 and rec['left'].tolist() == [0] * 4
    assert rec['side'].tolist() == list(sides) == rec['h'].tolist() == rec['w'].tolist()          # the whole image
    assert (rec['order'] == -1).all() and not rec['factor'].any()
    assert rec['offset'].tolist() == np.concatenate([[0], np.cumsum([3 * s * s for s in sides])[:-1]]).tolist()


# ------------------------------------------------------------------ accuracy_from_preds
def _np_max_preds(hm):
    """The reference's get_max_preds in numpy: first maximum of the flattened map, (x, y), zeroed where the maximum is <= 0."""
    B, K, H, W = hm.shape
    flat = hm.reshape(B, K, -1)
    idx, mv = np.argmax(flat, 2), np.amax(flat, 2)
    preds = np.stack([idx % W, idx // W], axis=2).astype(np.float32)
    return preds * (mv > 0)[:, :, None].astype(np.float32)


def test_accuracy_from_preds_on_the_g4_fixture():
    from seeded import peaky_heatmaps
    from utils.keypoint_detection import accuracy_from_preds
    g = golden('g4_argmax_accuracy')
    hm = peaky_heatmaps(401, 3, 21, 64, 64).numpy()
    hm[1, 0] = 0.5
    hm[1, 1, 10, 7] = hm[1, 1, 40, 3] = 9.0
    hm[2, 2, 63, 63] = 11.0
    lab = np.maximum(peaky_heatmaps(402, 3, 21, 64, 64).numpy(), 0)
    pred, tgt = _np_max_preds(hm), _np_max_preds(lab)
    assert np.array_equal(pred, g['preds'])
    acc, avg, cnt, out = accuracy_from_preds(pred, tgt, 64, 64)
    assert np.array_equal(acc, g['acc']) and avg == float(g['avg']) and cnt == int(g['cnt']) and np.array_equal(out, g['pred'])
    # the threshold is a parameter: nothing lies below 0
    acc0, avg0, cnt0, _ = accuracy_from_preds(pred, tgt, 64, 64, thr=0.0)
    assert cnt0 == cnt and avg0 == 0 and not acc0[acc0 >= 0].any()


# ------------------------------------------------------------------ C ABI: host-side checks before any launch
def test_resize_normalize_argument_validation_without_gpu():
    import mi355
    from mi355.augment import records, REC
    lib = mi355.load()
    table = np.array([[0, 100, 100], [30000, 64, 64]], np.int64)
    params = np.array([[0.0, 0, 0, 100, 0, 0, 0, -1, -1, -1, 0.0], [0.0, 0, 0, 64, 0, 0, 0, -1, -1, -1, 0.0]])
    good = records(table, params)
    src_bytes = 30000 + 64 * 64 * 3
    FAKE = 1 << 40                                        # device pointers are never touched when a check fails

    def run(rec, B=2, S=256, nbytes=src_bytes, out=FAKE, norm=MEANSTD):
        rec = np.ascontiguousarray(rec, REC)
        norm = np.array(norm, np.float32)
        return lib.mi355_resize_normalize(FAKE, nbytes, rec.ctypes.data, FAKE, B, S, norm.ctypes.data, out, 0)

    def bad(msg, **kw):
        rec = good.copy()
        for k, v in kw.pop('set', {}).items():
            rec[k[0]][k[1]] = v
        assert run(rec, **kw) == -1, kw                   # MI355_EINVAL
        assert msg in lib.mi355_last_error(), (msg, lib.mi355_last_error())

    bad(b'output side', S=8)
    bad(b'output side', S=520)
    bad(b'output side', S=528)
    bad(b'null', out=0)
    bad(b'std[1] = 0', norm=MEAN + [0.229, 0.0, 0.225])
    bad(b'> 4 x 256', set={('side', 1): 1025, ('h', 1): 1025, ('w', 1): 1025}, nbytes=30000 + 1025 * 1025 * 3)
    bad(b'> 4 x 16', S=16, set={('side', 1): 65, ('h', 1): 65, ('w', 1): 65}, nbytes=30000 + 65 * 65 * 3)
    bad(b'packed buffer', set={('offset', 1): src_bytes})
    bad(b'packed buffer', set={('offset', 1): 30001})
    bad(b'batch', B=0)
    bad(b'rotation mode', set={('rot', 0): 7})
    # mi355_augment takes S = 512 through the same checks: with a workspace sized for it, the first refusal is the null record copy
    ws = lib.mi355_augment_workspace(2, 512)
    assert ws >= 2 * 512 * 512 * 3
    norm = np.array(MEANSTD, np.float32)
    rec = np.ascontiguousarray(good, REC)
    assert lib.mi355_augment(FAKE, src_bytes, rec.ctypes.data, 0, 2, 512, norm.ctypes.data, FAKE, 0, FAKE, ws, 0) == -1
    assert b'null' in lib.mi355_last_error()
    assert lib.mi355_augment(FAKE, src_bytes, rec.ctypes.data, FAKE, 2, 528, norm.ctypes.data, FAKE, 0, FAKE, ws, 0) == -1
    assert b'output side' in lib.mi355_last_error()
