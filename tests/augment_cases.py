"""Shared cases of the augmentation tests: ragged RGB sources with key points, the CPU chain train1.py builds (Pillow) and
the DeviceAugment host side, both run from the same random / np.random seeds."""
import random

import numpy as np
import torch
from PIL import Image

K0 = np.array([[900.0, 0, 100.0], [0, 900.0, 100.0], [0, 0, 1.0]])
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def sources(n, seed=0, lo=64, hi=512):
    """n (PIL RGB image, key points (21, 2)) pairs of sides lo..hi; every third one non-square (aspect <= 1.1, so that
    RandomResizedCrop always finds a square crop), smooth content plus noise so that blur and jitter change pixels."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h = int(rng.integers(lo, hi + 1))
        w = h if i % 3 else int(np.clip(h * rng.uniform(0.91, 1.1), lo, hi))
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 100 * np.sin(xx / rng.uniform(5, 40)), 128 + 100 * np.cos(yy / rng.uniform(5, 40)),
                         (xx + yy) % 256], axis=2)
        arr = np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
        kp = np.stack([rng.uniform(0, w, 21), rng.uniform(0, h, 21)], axis=1)
        out.append((Image.fromarray(arr), kp))
    return out


def cpu_chain(size=256, rotation=180, scale=(0.6, 1.3)):
    import uda.dataset.keypoint_detection as T
    return T.Compose([T.RandomRotation(rotation), T.RandomResizedCrop(size=size, scale=scale),
                      T.ColorJitter(brightness=0.25, contrast=0.25, saturation=0.25), T.GaussianBlur(), T.ToTensor(),
                      T.Normalize(MEAN, STD)])


def seeded(fn, seed):
    random.seed(seed)
    np.random.seed(seed)
    return fn()


def labels(kp, size=256, hm=64):
    from uda.dataset.util import generate_target
    t, w = generate_target(kp, np.ones((21, 1), np.float32), (hm, hm), 2, (size, size))
    return torch.from_numpy(t), torch.from_numpy(w)


def ref_from_params(arr, p, size=256):
    """The CPU chain restated (augment_ref) from a DeviceAugment parameter row: (x, image_ema) as torch tensors."""
    import augment_ref as R
    angle, top, left, side = p[0], int(p[1]), int(p[2]), int(p[3])
    g = R.resize(R.rotate(arr, angle)[top:top + side, left:left + side], size)
    j = R.jitter(g, p[4:7], [int(o) for o in p[7:10] if o >= 0])
    return torch.from_numpy(R.normalise(R.blur(j, p[10]))), torch.from_numpy(R.normalise(g))
