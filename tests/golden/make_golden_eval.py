"""Generate the image-resolution evaluation golden vectors by calling the reference's live functions
(utils/keypoint_detection.py: compute_uv_from_heatmaps2 :172-205, accuracy_2d :128-136, accuracy_3d :95-126; run where the
reference tree is present).  Writes tests/golden/g13_eval.npz.  Import recipe as make_golden_mt.py: namespace stubs for the
reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_eval.py

Stored:
  uv/hm (2,21,16,16) integer-valued fp32 maps in [-512, 512], uv/size = 64, uv/out (2,21,2) int64 = compute_uv_from_heatmaps2;
  m/pred, m/gt (4,21,2) fp32 pixel coordinates, m/epe = accuracy_2d(pred, gt) (float64 of its fp32 scalar);
  m/pred3, m/gt3 (4,21,3) fp32 = the same points / 1000 with z = 0, m/thr = accuracy_3d's thresholds 20, 23 .. 50 and
  m/auc = the AUC accuracy_3d(pred3, gt3) returns (its curve / 30), m/epe3 its mean error.

The offsets pred - gt are Pythagorean pairs, so every distance is an integer (5 .. 50, several of them ON a threshold: the
strict `<`), the sum of each sample's 21 distances is a multiple of 21 and accuracy_3d's `* 1000` gives back the integer
pixel coordinates (asserted below): the reference's fp32 arithmetic is then exact, and a float64 restatement must reproduce
its EPE and AUC to the last bit.  About 25 KB."""
import os
import sys
import types
import numpy as np
import torch

REF = os.environ.get('REFERENCE_ROOT', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
np.int = int
np.float = float
if not hasattr(np, 'trapz'):
    np.trapz = np.trapezoid


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub('utils', f'{REF}/utils')

import utils.keypoint_detection as ref_kd  # noqa: E402

PAIRS = [(3, 4), (6, 8), (9, 12), (12, 16), (15, 20), (18, 24), (21, 28), (24, 32), (27, 36), (30, 40), (5, 12), (10, 24),
         (15, 36), (8, 15), (16, 30), (7, 24), (20, 21), (9, 40), (12, 35), (0, 0), (0, 20), (29, 0)]


def _points(rng):
    """(pred, gt) (4,21,2) integer pixel coordinates: Pythagorean offsets, per-sample distance sums divisible by 21, and
    coordinates that survive `/ 1000` then accuracy_3d's `* 1000` in fp32."""
    ok = np.array([np.float32(np.float32(n) / np.float32(1000)) * np.float32(1000) == np.float32(n) for n in range(256)])
    pred, gt = np.zeros((4, 21, 2)), np.zeros((4, 21, 2))
    for b in range(4):
        while True:
            g = rng.integers(60, 190, size=(21, 2))
            off = np.array([PAIRS[i] for i in rng.integers(0, len(PAIRS), 21)])
            off = np.where(rng.integers(0, 2, (21, 1)) == 1, off[:, ::-1], off) * rng.choice([-1, 1], size=(21, 2))
            p = g + off
            d = np.sqrt((off ** 2).sum(1))
            if d.sum() % 21 == 0 and ok[g].all() and ok[p].all():
                break
        pred[b], gt[b] = p, g
    return pred.astype(np.float32), gt.astype(np.float32)


def main():
    rng = np.random.default_rng(1301)
    out = {}
    hm = torch.from_numpy(rng.integers(-512, 513, size=(2, 21, 16, 16)).astype(np.float32))
    out['uv/hm'] = hm.numpy()
    out['uv/size'] = np.int64(64)
    out['uv/out'] = ref_kd.compute_uv_from_heatmaps2(hm.clone(), 64).numpy()

    pred, gt = _points(rng)
    out['m/pred'], out['m/gt'] = pred, gt
    out['m/epe'] = np.float64(float(ref_kd.accuracy_2d(torch.from_numpy(pred), torch.from_numpy(gt))))
    z = np.zeros((4, 21, 1), np.float32)
    pred3 = np.concatenate([pred / np.float32(1000), z], 2)
    gt3 = np.concatenate([gt / np.float32(1000), z], 2)
    assert np.array_equal((torch.from_numpy(pred3) * 1000).numpy()[..., :2], pred)
    assert np.array_equal((torch.from_numpy(gt3) * 1000).numpy()[..., :2], gt)
    epe3, auc = ref_kd.accuracy_3d(torch.from_numpy(pred3), torch.from_numpy(gt3))
    out['m/pred3'], out['m/gt3'] = pred3, gt3
    out['m/thr'] = np.array(range(20, 51, 3), dtype=np.float32)
    out['m/auc'], out['m/epe3'] = np.float64(auc), np.float64(float(epe3))
    np.savez_compressed(os.path.join(HERE, 'g13_eval.npz'), **out)
    print('g13_eval', len(out), 'arrays; epe', out['m/epe'], 'auc', out['m/auc'])


if __name__ == '__main__':
    main()
