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


def ref_stages(arr, p, size=256):
    """The CPU chain restated (augment_ref) from a DeviceAugment parameter row, as uint8 images: the geometry image (rotate,
    crop, resize), the jittered one and the blurred one."""
    import augment_ref as R
    angle, top, left, side = p[0], int(p[1]), int(p[2]), int(p[3])
    g = R.resize(R.rotate(arr, angle)[top:top + side, left:left + side], size)
    j = R.jitter(g, p[4:7], [int(o) for o in p[7:10] if o >= 0])
    return g, j, R.blur(j, p[10])


def ref_from_params(arr, p, size=256):
    """... as (x, image_ema) torch tensors."""
    import augment_ref as R
    g, j, b = ref_stages(arr, p, size)
    return torch.from_numpy(R.normalise(b)), torch.from_numpy(R.normalise(g))


def ref_lsum(arr, p, size=256):
    """The integer luminance sum the contrast op takes its mean from: of the geometry image after the ops drawn ahead of the
    contrast; 0 when the row has no contrast op."""
    import augment_ref as R
    order = [int(o) for o in p[7:10] if o >= 0]
    if 1 not in order:
        return 0
    g = ref_stages(arr, p, size)[0]
    return int(R.luminance(R.jitter(g, p[4:7], order[:order.index(1)])).astype(np.int64).sum())


# ------------------------------------------------------------------ the photometric launch at its edges
# One case is a list of (source HWC uint8, parameter row) pairs: one batch of a given output side.  tests/test_augment_cpu.py
# runs every pair through Pillow itself, tests/test_gpu_augment.py through the kernels inside guard buffers.
EDGE_SIDES = (16, 48)         # one photometric tile and two geometry bands; three tiles: first and last clamp, the middle has both halos
ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))
FACTORS = [0.0, 0.5, 1.0, ABOVE_ONE, 1.25, 2.0, 3.5]
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
PARTIAL_ORDERS = [(-1, 1, 0), (2, -1, 0), (-1, -1, 1), (-1, 2, -1), (0, -1, 1), (-1, 0, 2)]       # -1 in the first or middle slot


def crop_sides(S):
    return [1, 2, S - 1, S, S + 1, 2 * S + 1, 4 * S - 1, 4 * S]


def largest_blur_radius():
    """The largest (float64) blur radius whose box radius (augment_ref.box_radius) is still below 1, and the float64 after it:
    bisection over the float64 values between 1 and 2 (1.41421347...: the host rounds the radius to float32 first, so this is the
    last value that rounds to the float32 below sqrt(2))."""
    import augment_ref as R
    bits = lambda v: int(np.float64(v).view(np.uint64))
    val = lambda b: float(np.uint64(b).view(np.float64))
    lo, hi = bits(1.0), bits(2.0)
    assert int(R.box_radius(val(lo))) == 0 and int(R.box_radius(val(hi))) >= 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if int(R.box_radius(val(mid))) == 0 else (lo, mid)
    return val(lo), val(hi)


def blur_radii():
    return [0.0, 1e-6, 1e-3, 0.05, 0.8, 1.0, largest_blur_radius()[0]]


def edge_source(h, w, seed, top=254):
    """Values 0..top with a sharp edge on the first and last row and column (0 against top)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, top + 1, (h, w, 3), dtype=np.uint8)
    a[0], a[-1] = 0, top
    a[1:-1, 0], a[1:-1, -1] = top, 0
    return a


def _row(angle, top, left, side, factors=(1, 1, 1), order=(-1, -1, -1), blur=0.0):
    return [float(angle), top, left, side] + [float(f) for f in factors] + [int(o) for o in order] + [float(blur)]


def geometry_case(S, side):
    """Ten images for one crop side: every rotation mode (0: the affine path at 33.5 degrees on a non-square source, where source
    coordinates leave the image on all four sides; 1, 2: copy and 180 degrees, non-square; 3, 4: 90 and 270 degrees, square) with
    the crop at the top-left and at the bottom-right corner.  The first image is a copy cropped at its first byte, the last one
    a copy cropped at its last byte: the last byte of the packed buffer.  No source byte is 0xFF."""
    modes = {0: 33.5, 1: 0.0, 2: 180.0, 3: 90.0, 4: -90.0}
    plan = [(1, 'tl'), (0, 'tl'), (0, 'br'), (2, 'tl'), (2, 'br'), (3, 'tl'), (3, 'br'), (4, 'tl'), (4, 'br'), (1, 'br')]
    radii = blur_radii()
    out = []
    for i, (mode, corner) in enumerate(plan):
        h = max(side, 3) + (i % 3) * 2
        w = h if mode >= 3 else h + 5 + i
        arr = edge_source(h, w, 1000 * S + 10 * side + i)
        top, left = (0, 0) if corner == 'tl' else (h - side, w - side)
        k = i + side
        out.append((arr, _row(modes[mode], top, left, side, [FACTORS[(k + j) % len(FACTORS)] for j in range(3)],
                              (ORDERS + PARTIAL_ORDERS)[k % 12], radii[k % len(radii)])))
    return out


def jitter_case(S=16):
    """Every factor for each op alone, for all six orders and for the orders with holes, on sources with rows of 0 and rows of 255
    (both clips of Blend.c); the crop is the whole source, larger than S, so the rows survive the resize."""
    out = []
    def src(i):
        a = np.random.default_rng(77 + i).integers(0, 256, (S + 4, S + 4, 3), dtype=np.uint8)
        a[2:5], a[-5:-2] = 0, 255
        return a
    for op in range(3):
        for f in FACTORS:
            fac = [1.0, 1.0, 1.0]
            fac[op] = f
            order = [-1, -1, -1]
            order[op % 3] = op                         # alone, in the first, middle and last slot
            out.append((src(len(out)), _row(0.0, 0, 0, S + 4, fac, order)))
    for i, order in enumerate(ORDERS + PARTIAL_ORDERS):
        for j in range(len(FACTORS)):
            fac = [FACTORS[(j + 2 * k + i) % len(FACTORS)] for k in range(3)]
            out.append((src(len(out)), _row(0.0, 0, 0, S + 4, fac, order)))
    return out


def tie_case():
    """16 x 16, half at luminance 10 and half at 11: the mean 10.5 rounds to 11 (int(mean + 0.5))."""
    a = np.full((16, 16, 3), 10, np.uint8)
    a[8:] = 11
    return [(a.copy(), _row(0.0, 0, 0, 16, (1.0, f, 1.0), order)) for f in (0.5, 1.5) for order in ((1, -1, -1), (-1, 1, -1), (0, 1, 2))]


def blur_case(S):
    """Every radius on a sharp-edged source: crop only (side S) and a down-scaling crop, so the edges reach the first and last
    row and column of the blurred image."""
    out = []
    for i, r in enumerate(blur_radii()):
        out.append((edge_source(S, S, 500 + i, top=255), _row(0.0, 0, 0, S, blur=r)))
        out.append((edge_source(S + 7, S + 9, 600 + i), _row(180.0, 7, 9, S, (1.0, 1.25, 0.5), (2, 1, -1), r)))
    return out


def mixed_case(S=48):
    """About 24 ragged images of all kinds in one batch: the records differ block to block."""
    out = []
    for i, side in enumerate(crop_sides(S)):
        out.append(geometry_case(S, side)[(3 * i + 1) % 10])
    out += jitter_case(16)[5::9][:8]
    out += blur_case(16)[1::2][:7]
    out += tie_case()[:1]
    return out


def pack(case):
    """(packed uint8 sources, (B, 3) offset / h / w table, (B, 11) parameter rows) of one case."""
    arrs = [a for a, _ in case]
    offsets = np.cumsum([0] + [a.size for a in arrs])[:-1]
    table = torch.tensor([[int(o), a.shape[0], a.shape[1]] for o, a in zip(offsets, arrs)], dtype=torch.int64)
    params = torch.tensor([r for _, r in case], dtype=torch.float64)
    return torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])), table, params
